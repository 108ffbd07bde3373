"""N-channel feature render (gsr_render_features / gsr_render_features_backward, `render_features`, `GaussianRasterizer.features`) through the shipped
package on the CPU: the SIMT build of the whole library behind the package's own loader, as in tests/test_contrib_cpu.py, whose scenes these are.
Reference and bars: tests/feature_reference.py.

Scenes: the dense 100 x 70 frame (partial tiles and partial 8x8 blocks on both axes, 3000 Gaussians, opacity logits raised by 3: terminating pixels, lists
over 128 entries), the sparse 96 x 80 frame (most pixels without a contributor; the group-edge sweep runs there to keep SIMT time down) and the two
hand-computable frames of tests/probe_reference.py.

G = 16 channels per forward walk and 16 / 8 / 4 per backward walk (16 while more than 8 remain, then 8, then 4) are the kernels' compile-time constants
(csrc/features.hip); the LDS bounds of tests/test_features_isa_cpu.py fail if they change without these tests.

Test infrastructure: the product never loads the SIMT library."""
import ctypes as C
import functools

import pytest
import torch

from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import feature_reference as R
import probe_reference as PR
import test_composite_cpu as T
import test_contrib_cpu as TC

W, H = TC.W, TC.H
G = 16
# the issue's set for G, and for the backward's three group widths: 8 / 9 (one group of 8 / of 16), 11, 21 (16 + 8), 24 (16 + 8), 20 (16 + 4)
EDGE_CHANNELS = sorted({1, 3, 4, 5, G - 1, G, G + 1, 2 * G + 3} | {7, 8, 9, 11, 20, 21, 24})


@functools.lru_cache(maxsize=None)
def inputs(P, h, w, channels, seed=31):
    """(features [P,C] in [-1,1], upstream gradient [C,h,w] in [-0.5,0.5]): computed once per shape, shared, never modified."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(P, channels, generator=g) * 2.0 - 1.0, torch.rand(channels, h, w, generator=g) - 0.5


def geometry(lv, form):
    return dict(cov3D_precomp=lv["cov"]) if form == "precomp" else dict(scales=lv["scales"], rotations=lv["rot"])


def feature_pass(pkg, rendered, f, grad_out):
    """-> (F, dL/df) of one call of render_features on a fresh leaf."""
    leaf = f.clone().requires_grad_(True)
    out = pkg.render_features(rendered, leaf)
    out.backward(grad_out)
    return out.detach(), leaf.grad


def view_depth(S, means):
    vm = S.viewmatrix
    return means[:, 0] * vm[0, 2] + means[:, 1] * vm[1, 2] + means[:, 2] * vm[2, 2] + vm[3, 2]


def test_the_gradient_reference_is_the_contribution_reference_per_channel():
    """Reference alone: the all-channel form of tests/feature_reference.py against its definition, and the input condition of the scenes."""
    for which, h, w in (("dense", H, W), ("sparse", 80, 96)):
        aux, s0 = TC.oracle_aux(which)
        assert R.check_input(aux) < 0.01
        _, g_up = inputs(aux["means2D"].shape[0], h, w, 3)
        g_up = torch.stack([R.mask_fragile(g_up[c], aux) for c in range(3)])
        a, b = R.gradient(aux, s0, g_up), R.gradient_per_channel(aux, s0, g_up)
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) and float(b.abs().max()) > 0.0


@pytest.mark.parametrize("form", ["fused", "precomp"])
def test_dense_frame_against_the_reference(simt_lib, form):
    aux, s0 = TC.oracle_aux("dense", form)
    f, g_up = inputs(3000, H, W, 5)
    g_up = torch.stack([R.mask_fragile(g_up[c], aux) for c in range(5)])
    ref_F, ref_g = R.forward(aux, s0, f), R.gradient(aux, s0, g_up)
    stats = TC.R.reference(aux, s0)
    # termination and several batches of 64 are exercised, as in the probe's test
    assert float(stats["terminated"].float().mean()) > 0.02 and stats["longest"] > 128
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", form)
        got_F, got_g = feature_pass(pkg, out[0].clamp(0.0, 1.0), f, g_up)
    R.check_image(f"features_cpu_dense_{form}_image", got_F, ref_F, aux, float(f.abs().max()))
    R.check_gradient(f"features_cpu_dense_{form}_grad", got_g, ref_g, aux)


def test_identities_against_the_product_itself(simt_lib):
    """Colour, alpha and expected depth are feature renders of particular columns; the gradient of a channel is contribution_stats' weight_sum; and the
    forward and the backward are adjoint.  On all pixels, at the bars of tests/feature_reference.py."""
    f, g_up = inputs(3000, H, W, 3)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", "precomp", return_alpha=True)
        colors = lv["colors"].detach()
        z = view_depth(S, lv["means"].detach())
        as_colour = pkg.render_features(out[0], colors)
        as_alpha = pkg.render_features(out[0], torch.ones(3000, 1))
        as_depth = pkg.render_features(out[0], torch.stack([colors[:, 0], z], dim=1))
        probe = pkg.pixel_probe(out[0])
        got_F, got_g = feature_pass(pkg, out[0], f, g_up)
        sums = [pkg.contribution_stats(out[0], g_up[c]).weight_sum for c in range(3)]
    d_colour = float((as_colour - out[0].detach()).abs().max())
    d_alpha = float((as_alpha - out[3].detach()).abs().max())
    z_max = float(z.abs().max())
    d_depth = float((as_depth[1] - probe.expected_depth).abs().max()) / z_max
    d_sum = max(float((got_g[:, c].double() - sums[c].double()).abs().max()) / float(sums[c].abs().max()) for c in range(3))
    lhs = float((g_up.double() * got_F.double()).sum())
    rhs = float((got_g.double() * f.double()).sum())
    d_adj = abs(lhs - rhs) / abs(lhs)
    R.parity_report("features_cpu_identities", colour_abs_max=d_colour, alpha_abs_max=d_alpha, depth_rel_zmax=d_depth, grad_vs_weight_sum_rel_max=d_sum,
                    adjoint_rel=d_adj, grad_equals_weight_sum_bits=all(torch.equal(got_g[:, c], sums[c]) for c in range(3)))
    assert d_colour <= 1e-5 * float(colors.abs().max()) and d_alpha <= 1e-5
    assert torch.equal(as_depth[0], as_colour[0])
    assert d_depth <= 1e-5
    assert d_sum < 1e-5
    assert abs(lhs) > 1.0 and d_adj <= 1e-5


def test_group_edges_every_channel_has_the_bits_of_a_call_on_its_column_alone(simt_lib):
    aux, _ = TC.oracle_aux("sparse")
    P = aux["means2D"].shape[0]
    c_max = max(EDGE_CHANNELS)
    f, g_up = inputs(P, 80, 96, c_max)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "sparse")
        alone = [feature_pass(pkg, out[0], f[:, c:c + 1].contiguous(), g_up[c:c + 1]) for c in range(c_max)]
        for channels in EDGE_CHANNELS:
            got_F, got_g = feature_pass(pkg, out[0], f[:, :channels].contiguous(), g_up[:channels])
            assert got_F.shape == (channels, 80, 96) and got_g.shape == (P, channels)
            for c in range(channels):
                assert torch.equal(got_F[c], alone[c][0][0]), (channels, c)
                assert torch.equal(got_g[:, c], alone[c][1][:, 0]), (channels, c)
    assert float(alone[0][0].abs().max()) > 0.0 and float(alone[0][1].abs().max()) > 0.0


def test_two_calls_and_the_standalone_form_give_equal_bits(simt_lib):
    f, g_up = inputs(3000, H, W, 5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        a = feature_pass(pkg, out[0], f, g_up)
        b = feature_pass(pkg, out[0] * 2.0, f, g_up)
        leaf = f.clone().requires_grad_(True)
        alone, radii = pkg.GaussianRasterizer(S).features(lv["means"], lv["opac"], leaf, **geometry(lv, "fused"))
        alone.backward(g_up)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], alone.detach()) and torch.equal(a[1], leaf.grad) and torch.equal(radii, out[1])


def test_only_contributors_count(simt_lib):
    """Rows of Gaussians that contribute nowhere (culled, hidden) never reach the image, whatever they hold, and get exact zero gradients."""
    f, g_up = inputs(3000, H, W, 5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        nowhere = pkg.contribution_stats(out[0]).pixel_count == 0
        clean = feature_pass(pkg, out[0], f, g_up)
        poisoned = f.clone()
        poisoned[nowhere] = float("nan")
        got = feature_pass(pkg, out[0], poisoned, g_up)
    assert int(nowhere.sum()) > 100 and int((nowhere & (out[1] > 0)).sum()) > 20      # culled and hidden ones
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1])
    assert float(clean[1][nowhere].abs().max()) == 0.0 and float(clean[1][~nowhere].abs().max()) > 0.0


def through_the_c_abi(pkg, rendered, S, f, prefill=7.5, tile_rows=None):
    """gsr_render_features on the state behind `rendered`, onto an array prefilled with garbage."""
    from diff_gaussian_rasterization import _lib
    st = pkg._saved_state(rendered, "render_features", "features")
    keep = []
    s = pkg._make_settings(S, keep, tile_rows, bg_image=True)
    raw = torch.full((f.shape[1], int(S.image_height), int(S.image_width)), prefill)
    f = f.contiguous()
    assert _lib.load().gsr_render_features(C.byref(s), st.P, st.fwd.num_rendered, pkg._ptr(st.fwd.geom), pkg._ptr(st.fwd.binning), pkg._ptr(st.fwd.img),
                                           pkg._ptr(f), f.shape[1], pkg._ptr(raw), None) == 0
    return raw


def test_every_pixel_is_written(simt_lib):
    """Through the C ABI onto arrays prefilled with garbage: pixels nobody contributes to come out exactly 0 in every channel -- 8x8 blocks without a
    contributor (the walk is skipped) and, on the isolated Gaussian of the hand-computable frames, tiles with an empty range included."""
    aux, s0 = TC.oracle_aux("sparse")
    P = aux["means2D"].shape[0]
    f, _ = inputs(P, 80, 96, G + 1)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "sparse")
        raw = through_the_c_abi(pkg, out[0], S, f)
        got = pkg.render_features(out[0], f)
        count = pkg.pixel_probe(out[0]).count
        R.check_image("features_cpu_sparse_image", got, R.forward(aux, s0, f), aux, float(f.abs().max()))
        assert torch.equal(raw, got)
        empty = count == 0
        assert float(empty.float().mean()) > 0.3 and int((count.reshape(10, 8, 12, 8).amax(dim=(1, 3)) == 0).sum()) >= 1
        assert float(raw[:, empty].abs().max()) == 0.0 and bool((raw[:, ~empty] != 7.5).all())

        cam, hl = PR.hand_frame("isolated")
        S2 = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        out2 = pkg.GaussianRasterizer(S2)(means3D=hl["means"].clone().requires_grad_(True), means2D=None, opacities=hl["opac"],
                                          colors_precomp=torch.zeros(2, 3), scales=hl["scales"], rotations=hl["rot"])
        f2 = torch.tensor([[float("nan")] * 5, [1.0, -2.0, 3.0, 0.5, -0.25]])
        raw2 = through_the_c_abi(pkg, out2[0], S2, f2)
        count2 = pkg.pixel_probe(out2[0]).count
    empty2 = count2 == 0
    tiles_without = count2.reshape(3, 16, 4, 16).amax(dim=(1, 3)) == 0
    assert 0 < int(tiles_without.sum()) < 12 and int(((count2.reshape(6, 8, 8, 8).amax(dim=(1, 3)) == 0)
                                                       & ~tiles_without.repeat_interleave(2, 0).repeat_interleave(2, 1)).sum()) > 0
    assert float(raw2[:, empty2].abs().max()) == 0.0 and bool((raw2[:, ~empty2] != 7.5).all()) and not bool(raw2.isnan().any())


def test_hand_computable_frames(simt_lib):
    """The weights tests/probe_reference.py derives by hand: the isolated Gaussian blends with w = 0.95 at the centre pixel and nothing from 12 px on; of
    the two layers the front one (index 1) blends with w = 0.3 and the back one (index 0) with 0.7 * 0.9 = 0.63."""
    ys, xs = torch.meshgrid(torch.arange(PR.HAND_H), torch.arange(PR.HAND_W), indexing="ij")
    far = ((xs - PR.HAND_PX) ** 2 + (ys - PR.HAND_PY) ** 2).double().sqrt() >= 12.0
    with package_on_the_cpu(simt_lib) as pkg:
        for which, f, want in (("isolated", [[float("nan")] * 3, [2.0, -3.0, 0.5]], [0.95 * 2.0, 0.95 * -3.0, 0.95 * 0.5]),
                               ("layers", [[1.0, -2.0, 4.0], [3.0, 0.5, -1.0]], [0.3 * 3.0 + 0.63 * 1.0, 0.3 * 0.5 + 0.63 * -2.0, 0.3 * -1.0 + 0.63 * 4.0])):
            cam, lv = PR.hand_frame(which)
            rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3)))
            leaf = torch.tensor(f).requires_grad_(True)
            F, radii = rast.features(lv["means"], lv["opac"], leaf, scales=lv["scales"], rotations=lv["rot"])
            at = F.detach()[:, PR.HAND_PY, PR.HAND_PX]
            assert float((at - torch.tensor(want)).abs().max()) <= 1e-5 * 4.0, (which, at)
            # one pixel's upstream gradient: the gradient of a row is that pixel's weight
            up = torch.zeros_like(F)
            up[:, PR.HAND_PY, PR.HAND_PX] = torch.tensor([1.0, 2.0, -1.0])
            F.backward(up)
            w = (0.0, 0.95) if which == "isolated" else (0.63, 0.3)
            for i in range(2):
                assert float((leaf.grad[i] - w[i] * torch.tensor([1.0, 2.0, -1.0])).abs().max()) <= 2e-5, (which, i, leaf.grad)
            if which == "isolated":
                assert float(F.detach()[:, far].abs().max()) == 0.0 and radii.tolist()[0] == 0


def test_band(simt_lib):
    band = (1, 3)
    f, g_up = inputs(3000, H, W, 5)
    r0, r1 = band[0] * 16, band[1] * 16
    with package_on_the_cpu(simt_lib) as pkg:
        full_out, lv, S = TC.render(pkg, "dense")
        full = feature_pass(pkg, full_out[0], f, g_up)
        parts = {}
        for b in ((0, 1), band, (3, 5)):      # the band and the two bands that complete the frame
            out, _, Sb = TC.render(pkg, "dense", tile_rows=b)
            parts[b] = feature_pass(pkg, out[0], f, g_up)
            if b == band:
                raw = through_the_c_abi(pkg, out[0], Sb, f, prefill=-3.25, tile_rows=band)
                rast = pkg.GaussianRasterizer(Sb)
                rast.tile_rows = band
                alone, _ = rast.features(lv["means"], lv["opac"], f, **geometry(lv, "fused"))
    got_F, got_g = parts[band]
    assert torch.equal(got_F[:, r0:r1], full[0][:, r0:r1]) and torch.equal(alone, got_F)
    assert float(got_F[:, :r0].abs().max()) == 0.0 and float(got_F[:, r1:].abs().max()) == 0.0      # through Python: zeros outside the band
    assert torch.equal(raw[:, r0:r1], got_F[:, r0:r1]) and bool((raw[:, :r0] == -3.25).all()) and bool((raw[:, r1:] == -3.25).all())
    assert float(full[0][:, :r0].abs().max()) > 0.0 and float(full[0][:, r1:].abs().max()) > 0.0
    total = sum(p[1].double() for p in parts.values())
    d = float((total - full[1].double()).abs().max()) / float(full[1].abs().max())
    R.parity_report("features_cpu_band", bands_sum_vs_full_rel_max=d)
    assert d <= 1e-6 and not torch.equal(got_g, full[1])


def test_edge_and_error_cases(simt_lib):
    z3 = torch.zeros(0, 3)
    f, g_up = inputs(3000, H, W, 5)
    with package_on_the_cpu(simt_lib) as pkg:
        cam, sc = TC.scene("dense")
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        rast = pkg.GaussianRasterizer(S)
        # no Gaussian at all, and a frame without a single instance (every Gaussian behind the camera)
        leaf0 = torch.zeros(0, 5, requires_grad=True)
        F0, radii0 = rast.features(z3, torch.zeros(0, 1), leaf0, scales=z3, rotations=torch.zeros(0, 4))
        F0.backward(g_up)
        assert F0.shape == (5, H, W) and float(F0.detach().abs().max()) == 0.0 and radii0.shape == (0,) and leaf0.grad.shape == (0, 5)
        out, lv, _ = TC.render(pkg, "dense")
        behind = lv["means"].detach() * torch.tensor([1.0, 1.0, -1.0])
        leaf = f.clone().requires_grad_(True)
        F1, _ = rast.features(behind, lv["opac"], leaf, scales=lv["scales"], rotations=lv["rot"])
        F1.backward(g_up)
        assert F1.shape == (5, H, W) and float(F1.detach().abs().max()) == 0.0 and leaf.grad.shape == (3000, 5) and float(leaf.grad.abs().max()) == 0.0
        # refused inputs
        for bad, what in ((torch.zeros(3000, 0), "channels"), (torch.zeros(3000, 1025), "channels"), (torch.zeros(2999, 5), "rows"),
                          (torch.zeros(3000), r"shape \[P, C\]"), (torch.zeros(3000, 5, device="meta"), "lives on")):
            with pytest.raises(pkg.GsrError, match=what):
                pkg.render_features(out[0], bad)
            with pytest.raises(pkg.GsrError, match=what):
                rast.features(lv["means"], lv["opac"], bad, scales=lv["scales"], rotations=lv["rot"])
        with pytest.raises(pkg.GsrError, match="no rasterizer call found"):
            pkg.render_features(out[0].detach(), f)
        out2, _, _ = TC.render(pkg, "dense")
        with pytest.raises(pkg.GsrError, match="2 rasterizer calls"):
            pkg.render_features(out[0] + out2[0], f)
        # without a gradient to compute nothing is kept; the result does not require grad
        plain = pkg.render_features(out[0], f)
        assert not plain.requires_grad and plain.grad_fn is None
        # the backward works after the frame's own backward() has run, and no gradient reaches the geometry through F
        leaf = f.clone().requires_grad_(True)
        F = pkg.render_features(out[0], leaf)
        before = feature_pass(pkg, out2[0], f, g_up)
        out[0].sum().backward()
        with pytest.raises(pkg.GsrError, match="call render_features before backward"):
            pkg.render_features(out[0], f)
        F.backward(g_up)
        assert torch.equal(F.detach(), before[0]) and torch.equal(leaf.grad, before[1])
        out3, lv3, _ = TC.render(pkg, "dense")
        leaf3 = f.clone().requires_grad_(True)
        (pkg.render_features(out3[0], leaf3) * g_up).sum().backward()
        assert lv3["means"].grad is None and lv3["opac"].grad is None and torch.equal(leaf3.grad, before[1])
        assert "render_features" in pkg.__all__ and callable(pkg.GaussianRasterizer.features)


def test_c_level_argument_checks(simt_lib):
    with package_on_the_cpu(simt_lib):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = _lib.GsrRasterSettings()
        s.image_width, s.image_height = 40, 40
        s.bg = s.viewmatrix = s.projmatrix = s.campos = 0x1000
        s.tanfovx = s.tanfovy = 0.5
        fwd, bwd = lib.gsr_render_features, lib.gsr_render_features_backward
        assert fwd(C.byref(s), 10, 0, None, None, None, None, 3, None, None) == -1 and b"features / out" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 0, None, None, None, None, 3, None, None, None) == -1 and b"dL_dout / dL_dfeatures" in lib.gsr_last_error()
        assert fwd(C.byref(s), 10, 5, None, 0x1000, 0x1000, 0x1000, 3, 0x1000, None) == -1 and b"state buffers" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 5, None, 0x1000, 0x1000, 0x1000, 3, 0x1000, 0x1000, None) == -1 and b"state buffers" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 5, 0x1000, 0x1000, 0x1000, 0x1000, 3, None, 0x1000, None) == -1 and b"scratch" in lib.gsr_last_error()
        for P, R_ in ((-1, 0), (10, -1)):
            assert fwd(C.byref(s), P, R_, None, None, None, 0x1000, 3, 0x1000, None) == -1
            assert bwd(C.byref(s), P, R_, None, None, None, 0x1000, 3, None, 0x1000, None) == -1
        assert fwd(None, 10, 0, None, None, None, 0x1000, 3, 0x1000, None) == -1
        assert bwd(None, 10, 0, None, None, None, 0x1000, 3, None, 0x1000, None) == -1
        for bad in (0, -1, 1025):
            assert fwd(C.byref(s), 0, 0, None, None, None, None, bad, None, None) == -1 and b"[1, 1024]" in lib.gsr_last_error()
            assert bwd(C.byref(s), 0, 0, None, None, None, None, bad, None, None, None) == -1 and b"[1, 1024]" in lib.gsr_last_error()
        # contrib.hip's layout with a record of 16, 32 or 64 bytes (C <= 4, <= 8, more): four slots and a flag word per instance, sized in 64 bits,
        # and no larger for 1024 channels than for 9
        size = lib.gsr_feature_grad_scratch_bytes
        assert size(1_000_000, 0, 64) == 0 and size(10, 1000, 3) % 128 == 0
        assert size(1_000_000, 8_000_000, 3) == lib.gsr_contribution_scratch_bytes(1_000_000, 8_000_000)
        assert 8_000_000 * 132 <= size(1_000_000, 8_000_000, 8) < size(1_000_000, 8_000_000, 9) == size(1_000_000, 8_000_000, 1024) < 8_000_000 * 261
        assert size(1_000_000, 40_000_000, 64) >= 40_000_000 * 260 > 2 ** 31
        # P == 0 / no instance: no state is needed, zeros are written over the band and nowhere else, every gradient row is zero
        for P, R_, band in ((0, 0, (0, 0)), (10, 0, (0, 0)), (0, 0, (1, 2)), (10, 0, (1, 2))):
            out = torch.full((3, 40, 40), 7.5)
            f = torch.ones(max(P, 1), 3)
            grad = torch.full((max(P, 1), 3), 7.5)
            s.tile_y0, s.tile_y1 = band
            assert fwd(C.byref(s), P, R_, None, None, None, f.data_ptr(), 3, out.data_ptr(), None) == 0
            assert bwd(C.byref(s), P, R_, None, None, None, out.data_ptr(), 3, None, grad.data_ptr(), None) == 0
            r0, r1 = (0, 40) if band == (0, 0) else (16, 32)
            assert bool((out[:, r0:r1] == 0.0).all()) and bool((out[:, :r0] == 7.5).all()) and bool((out[:, r1:] == 7.5).all())
            assert bool((grad == (0.0 if P else 7.5)).all())
