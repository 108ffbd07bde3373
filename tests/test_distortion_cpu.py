"""The distortion loss on a rendered frame (gsr_distortion / gsr_distortion_backward, `distortion_map`, `GaussianRasterizer.distortion`) through the
shipped package on the CPU: the SIMT build of the whole library behind the package's own loader, on tests/test_contrib_cpu.py's dense frame (100 x 70,
3000 Gaussians: a missing right quadrant, a partial tile row, lists over 128 entries, more than 2 % of the pixels terminate) and the two hand-computable
frames of tests/probe_reference.py.  Reference and bars: tests/distortion_reference.py.

Test infrastructure: the product never loads the SIMT library."""
import ctypes as C
import functools

import pytest
import torch

from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import distortion_reference as R
import probe_reference as PR
import test_composite_cpu as T
import test_contrib_cpu as TC

W, H = TC.W, TC.H
GEOMETRY = {"fused": ("means", "opac", "scales", "rot"), "precomp": ("means", "opac", "cov")}


@functools.lru_cache(maxsize=None)
def upstream(form="fused", aa=False, seed=41):
    """dL/dD [H,W] in [-0.3, 0.7] with the fragile pixels zeroed: computed once, never modified."""
    aux, _ = TC.oracle_aux("dense", form, aa)
    g = torch.Generator().manual_seed(seed)
    return R.mask_fragile(torch.rand(H, W, generator=g) - 0.3, aux)


@functools.lru_cache(maxsize=None)
def reference(form, depth_mode, dtype=torch.float64):
    aux, s0 = TC.oracle_aux("dense", form)
    return R.reference(aux, s0, upstream(form), depth_mode, dtype)


def through_the_c_abi(pkg, rendered, S, g, depth_mode, tile_rows=None):
    """gsr_distortion and gsr_distortion_backward on the state behind `rendered` -> (D [H,W], saved [2,H,W], a copy of the [P,12] records)."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    st = pkg._saved_state(rendered, "distortion_map", "distortion")
    keep = []
    s = pkg._make_settings(S, keep, tile_rows, bg_image=True)
    h, w = int(S.image_height), int(S.image_width)
    D, saved = torch.zeros(h, w), torch.zeros(2, h, w)
    out = _lib.DistortionOut(D.data_ptr(), saved.data_ptr(), depth_mode, 0)
    state = (pkg._ptr(st.fwd.geom), pkg._ptr(st.fwd.binning), pkg._ptr(st.fwd.img))
    assert lib.gsr_distortion(C.byref(s), st.P, st.fwd.num_rendered, *state, C.byref(out), None) == 0, lib.gsr_last_error()
    scratch = torch.full((int(lib.gsr_backward_scratch_bytes(st.P, st.fwd.num_rendered)),), 0xA5, dtype=torch.uint8)      # garbage, not zeros
    rec = C.c_void_p(0)
    g = g.contiguous()
    assert lib.gsr_distortion_backward(C.byref(s), st.P, st.fwd.num_rendered, *state, pkg._ptr(g), pkg._ptr(saved), depth_mode, pkg._ptr(scratch),
                                       C.byref(rec), None) == 0, lib.gsr_last_error()
    off = int(rec.value) - scratch.data_ptr()
    return D, saved, scratch[off:off + st.P * 48].view(torch.float32).view(st.P, 12).clone()


@pytest.mark.parametrize("depth_mode", [0, 1])
def test_the_reference_is_the_oracles_autograd_of_the_pairwise_sum(depth_mode):
    aux, s0 = TC.oracle_aux("dense")
    cam, sc = TC.scene("dense")
    ora = R.autograd_oracle(cam, T.make_leaves(sc, "fused", grad=False), "fused", upstream(), depth_mode)
    R.check_reference(f"distortion_reference_dense_mode{depth_mode}", reference("fused", depth_mode), ora, aux, s0)


@pytest.mark.parametrize("form", ["fused", "precomp"])
def test_map_saved_and_records_against_the_reference_through_the_c_abi(simt_lib, form):
    aux, _ = TC.oracle_aux("dense", form)
    stats = TC.R.reference(*TC.oracle_aux("dense", form))
    assert float(stats["terminated"].float().mean()) > 0.02 and stats["longest"] > 128
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", form)
        for depth_mode in (0, 1):
            ref, ref32 = reference(form, depth_mode), reference(form, depth_mode, torch.float32)
            assert ref["multi"] > 0.25 * W * H, ref["multi"]
            D, saved, rec = through_the_c_abi(pkg, out[0], S, upstream(form), depth_mode)
            R.check_map(f"distortion_cpu_dense_{form}_mode{depth_mode}_map", D, saved, ref, ref32, aux)
            R.check_records(f"distortion_cpu_dense_{form}_mode{depth_mode}", rec, ref, ref32, aux)


@pytest.mark.parametrize("aa", [False, True])
def test_end_to_end_against_the_autograd_oracle(simt_lib, aa):
    cam, sc = TC.scene("dense")
    g = upstream("fused", aa)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", "fused", aa)
        for depth_mode in (0, 1):
            ora = R.autograd_oracle(cam, T.make_leaves(sc, "fused", grad=False), "fused", g, depth_mode, aa)
            D = pkg.distortion_map(out[0], inverse_depth=bool(depth_mode))
            grads = torch.autograd.grad((D * g).sum(), [lv[k] for k in GEOMETRY["fused"]], retain_graph=True)
            T.grad_bars(dict(zip(GEOMETRY["fused"], grads)), {k: ora[k] for k in GEOMETRY["fused"]}, f"distortion_cpu_e2e_aa{int(aa)}_mode{depth_mode}")


def test_two_runs_the_standalone_form_and_no_grad(simt_lib):
    g = upstream()
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        a, b = through_the_c_abi(pkg, out[0], S, g, 1), through_the_c_abi(pkg, out[0], S, g, 1)
        D = pkg.distortion_map(out[0], inverse_depth=True)
        (D * g).sum().backward()
        mine = {k: lv[k].grad for k in GEOMETRY["fused"]}
        lv2 = T.make_leaves(TC.scene("dense")[1], "fused")
        D2, radii = pkg.GaussianRasterizer(S).distortion(lv2["means"], lv2["opac"], scales=lv2["scales"], rotations=lv2["rot"], inverse_depth=True)
        (D2 * g).sum().backward()
        # nothing to differentiate: nothing kept, no graph, the same bits
        with torch.no_grad():
            plain, _ = pkg.GaussianRasterizer(S).distortion(lv2["means"], lv2["opac"], scales=lv2["scales"], rotations=lv2["rot"], inverse_depth=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[2].abs().max()) > 0.0
    assert torch.equal(D.detach(), a[0]) and torch.equal(D2.detach(), a[0]) and torch.equal(radii, out[1])
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, a[0])
    for k in GEOMETRY["fused"]:
        assert torch.equal(mine[k], lv2[k].grad) and float(mine[k].abs().max()) > 0.0, k


def test_means2D_receives_the_screen_space_gradient(simt_lib):
    """means2D, if it was passed to the rasterizer call, gets words 0, 1 of the records in its own units (0.5 W, 0.5 H per pixel), third column zero."""
    g = upstream()
    ref = reference("fused", 0)["records"]
    cam, sc = TC.scene("dense")
    with package_on_the_cpu(simt_lib) as pkg:
        lv = T.make_leaves(sc, "fused")
        m2 = torch.zeros(lv["means"].shape[0], 3, requires_grad=True)
        rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3)))
        out = rast(**{**T.call_kwargs(lv, "fused"), "means2D": m2})
        (pkg.distortion_map(out[0]) * g).sum().backward()
    want = ref[:, :2] * torch.tensor([0.5 * W, 0.5 * H], dtype=ref.dtype)
    d = float((m2.grad[:, :2].double() - want).abs().max()) / float(want.abs().max())
    R.parity_report("distortion_cpu_means2D", means2D_rel_max=d)
    assert d <= 1e-5 and float(m2.grad[:, 2].abs().max()) == 0.0 and lv["means"].grad is not None


def test_band(simt_lib):
    g = upstream()
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        D, _, full = through_the_c_abi(pkg, out[0], S, g, 0)
        parts, maps = [], []
        for b in ((0, 1), (1, 3), (3, 5)):
            outb, _, Sb = TC.render(pkg, "dense", tile_rows=b)
            Db, _, rb = through_the_c_abi(pkg, outb[0], Sb, g, 0, tile_rows=b)
            parts.append(rb)
            maps.append(Db)
            rows = slice(16 * b[0], min(16 * b[1], H))
            outside = torch.ones(H, dtype=torch.bool)
            outside[rows] = False
            assert torch.equal(Db[rows], D[rows]) and float(Db[rows].abs().max()) > 0.0 and float(Db.cpu()[outside].abs().sum()) == 0.0      # zeros outside the band
    total = sum(p.double() for p in parts)
    words = (0, 1, 2, 3, 4, 5, 9)
    d = [float((total[:, k] - full[:, k].double()).abs().max()) / float(full[:, k].abs().max()) for k in words]
    R.parity_report("distortion_cpu_band", **{f"word{k}_bands_sum_vs_full_rel_max": v for k, v in zip(words, d)})
    assert max(d) <= 1e-6 and not torch.equal(parts[1], full) and float(parts[1].abs().max()) > 0.0


def hand(pkg, which, inverse_depth):
    """hand_frame(which) through GaussianRasterizer.distortion with an upstream gradient of 1 at pixel (32, 24) alone -> (D, leaves with gradients)."""
    cam, lv = PR.hand_frame(which)
    lv = {k: v.clone().requires_grad_(True) for k, v in lv.items()}
    rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3)))
    D, _ = rast.distortion(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], inverse_depth=inverse_depth)
    up = torch.zeros_like(D)
    up[PR.HAND_PY, PR.HAND_PX] = 1.0
    D.backward(up)
    return D.detach(), lv


def check_hand_frames(run):
    """run(which, inverse_depth) -> (D on the CPU, leaves with gradients on the CPU).  Isolated: one contributor per pixel, D = 0 exactly, the culled row's
    gradients are exact zeros and the Gaussian's own at most 1e-6.  Layers, at pixel (32, 24): the front weight is 0.3 at depth 4, the back weight
    w_b = (1 - o_f) o_b = 0.63 at depth 6, so D = 2 w_f w_b |dt| = 2 |dt| o_f (1 - o_f) o_b with the derivatives worked out beside the asserts."""
    for inverse in (False, True):
        D, lv = run("isolated", inverse)
        assert float(D.abs().max()) == 0.0
        for k in ("means", "opac", "scales", "rot"):
            assert not bool(lv[k].grad.isnan().any()), k
            assert float(lv[k].grad[0].abs().max()) == 0.0 and float(lv[k].grad[1].abs().max()) <= 1e-6, (k, lv[k].grad)
    # z mode: dt = 2.  D = 2 * 0.3 * 0.63 * 2; dD/do_f = 2 dt o_b (1 - 2 o_f) = 2 * 2 * 0.9 * 0.4; dD/do_b = 2 dt o_f (1 - o_f) = 2 * 2 * 0.21
    D, lv = run("layers", False)
    got = lv["opac"].grad.reshape(-1)
    assert abs(float(D[PR.HAND_PY, PR.HAND_PX]) - 0.756) <= 1e-5 * 0.756
    assert abs(float(got[1]) - 1.44) <= 1e-5 * 1.44 and abs(float(got[0]) - 0.84) <= 1e-5 * 1.44, got
    # dD/dz_back = 2 w_f w_b = 0.378 = -dD/dz_front; the centre offsets are about 1e-6 px, so the covariance and mean paths vanish there
    gz = lv["means"].grad[:, 2]
    assert abs(float(gz[0]) - 0.378) <= 1e-4 * 0.378 and abs(float(gz[1]) + 0.378) <= 1e-4 * 0.378, gz
    # 1/z mode: dt = 1/4 - 1/6 = 1/12
    D, lv = run("layers", True)
    got = lv["opac"].grad.reshape(-1)
    assert abs(float(D[PR.HAND_PY, PR.HAND_PX]) - 0.0315) <= 1e-5 * 0.0315
    assert abs(float(got[1]) - 0.06) <= 1e-5 * 0.06 and abs(float(got[0]) - 0.035) <= 1e-5 * 0.035, got
    assert not bool(lv["means"].grad.isnan().any()) and not bool(lv["scales"].grad.isnan().any())


def test_hand_computable_frames(simt_lib):
    with package_on_the_cpu(simt_lib) as pkg:
        check_hand_frames(lambda which, inverse: hand(pkg, which, inverse))


def test_edge_cases(simt_lib):
    z3 = torch.zeros(0, 3)
    g = upstream()
    with package_on_the_cpu(simt_lib) as pkg:
        cam, sc = TC.scene("dense")
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        rast = pkg.GaussianRasterizer(S)
        # no Gaussian at all
        m0, o0 = z3.clone().requires_grad_(True), torch.zeros(0, 1, requires_grad=True)
        D0, _ = rast.distortion(m0, o0, scales=z3, rotations=torch.zeros(0, 4))
        (D0 * g).sum().backward()
        assert D0.shape == (H, W) and float(D0.detach().abs().max()) == 0.0 and m0.grad.shape == (0, 3) and o0.grad.shape == (0, 1)
        # a frame without a single instance (every Gaussian behind the camera): zero map, zero rows
        lv = T.make_leaves(sc, "fused")
        behind = (lv["means"].detach() * torch.tensor([1.0, 1.0, -1.0])).requires_grad_(True)
        D1, _ = rast.distortion(behind, lv["opac"], scales=lv["scales"], rotations=lv["rot"])
        (D1 * g).sum().backward()
        assert float(D1.detach().abs().max()) == 0.0
        for t in (behind, lv["opac"], lv["scales"], lv["rot"]):
            assert t.grad is not None and float(t.grad.abs().max()) == 0.0
        # the multi-GPU renderers stay refused; freed state raises the existing message
        lv = T.make_leaves(sc, "fused")
        kw = T.call_kwargs(lv, "fused")
        synced = pkg.rasterize_gaussians(kw["means3D"], None, kw["shs"], None, kw["opacities"], kw["scales"], kw["rotations"], None, S,
                                         grad_sync=lambda records: None)
        with pytest.raises(pkg.GsrError, match="multi-GPU"):
            pkg.distortion_map(synced[0])
        out, lv, _ = TC.render(pkg, "dense")
        out[0].sum().backward()
        with pytest.raises(pkg.GsrError, match="call distortion_map before backward"):
            pkg.distortion_map(out[0])


def test_c_level_argument_checks(simt_lib):
    with package_on_the_cpu(simt_lib):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = _lib.GsrRasterSettings()
        s.image_width, s.image_height = 40, 40
        s.bg = s.viewmatrix = s.projmatrix = s.campos = 0x1000
        s.tanfovx = s.tanfovy = 0.5
        ok = 0x1000
        fwd, bwd = lib.gsr_distortion, lib.gsr_distortion_backward
        out = _lib.DistortionOut(ok, None, 0, 0)
        assert fwd(C.byref(s), 10, 0, None, None, None, None, None) == -1 and b"GsrDistortionOut" in lib.gsr_last_error()
        assert fwd(C.byref(s), 10, 0, None, None, None, C.byref(_lib.DistortionOut(None, None, 0, 0)), None) == -1 and b"distortion is NULL" in lib.gsr_last_error()
        for bad in (-1, 2):
            assert fwd(C.byref(s), 10, 0, None, None, None, C.byref(_lib.DistortionOut(ok, None, bad, 0)), None) == -1 and b"depth_mode" in lib.gsr_last_error()
        assert fwd(C.byref(s), 10, 5, None, ok, ok, C.byref(out), None) == -1 and b"state buffers" in lib.gsr_last_error()
        assert fwd(None, 10, 0, None, None, None, C.byref(out), None) == -1
        for P, R_ in ((-1, 0), (10, -1)):
            assert fwd(C.byref(s), P, R_, None, None, None, C.byref(out), None) == -1
        rec = C.c_void_p(0)
        assert bwd(C.byref(s), 10, 0, None, None, None, ok, ok, 0, None, C.byref(rec), None) == -1 and b"bwd_scratch" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 0, None, None, None, ok, ok, 0, ok, None, None) == -1 and b"splat_grads_out" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 5, None, ok, ok, ok, ok, 0, ok, C.byref(rec), None) == -1 and b"state buffers" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 5, ok, ok, ok, None, ok, 0, ok, C.byref(rec), None) == -1 and b"dL_ddistortion / saved" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 5, ok, ok, ok, ok, None, 0, ok, C.byref(rec), None) == -1 and b"dL_ddistortion / saved" in lib.gsr_last_error()
        assert bwd(C.byref(s), 10, 0, None, None, None, ok, ok, 0, 0x1008, C.byref(rec), None) == -1 and b"16-byte" in lib.gsr_last_error()
        for bad in (-1, 2):
            assert bwd(C.byref(s), 10, 0, None, None, None, ok, ok, bad, ok, C.byref(rec), None) == -1 and b"depth_mode" in lib.gsr_last_error()
        for P, R_ in ((-1, 0), (10, -1)):
            assert bwd(C.byref(s), P, R_, None, None, None, ok, ok, 0, ok, C.byref(rec), None) == -1
        assert bwd(None, 10, 0, None, None, None, ok, ok, 0, ok, C.byref(rec), None) == -1
        # P == 0: nothing to write; no instance: zeros over the band / zero rows, and no state, gradient or saved planes are needed
        assert bwd(C.byref(s), 0, 0, None, None, None, None, None, 0, None, C.byref(rec), None) == 0 and rec.value is None
        for band in ((0, 0), (1, 2)):
            s.tile_y0, s.tile_y1 = band
            scratch = torch.full((int(lib.gsr_backward_scratch_bytes(10, 0)),), 0xA5, dtype=torch.uint8)
            assert bwd(C.byref(s), 10, 0, None, None, None, None, None, 1, scratch.data_ptr(), C.byref(rec), None) == 0
            off = int(rec.value) - scratch.data_ptr()
            assert 0 <= off and bool((scratch[off:off + 480].view(torch.float32) == 0.0).all())
            D, saved = torch.full((40, 40), 7.0), torch.full((2, 40, 40), 7.0)
            assert fwd(C.byref(s), 10, 0, None, None, None, C.byref(_lib.DistortionOut(D.data_ptr(), saved.data_ptr(), 1, 0)), None) == 0
            rows = slice(16 * band[0], 16 * band[1]) if band != (0, 0) else slice(0, 40)      # (0, 0): the whole frame
            inside = torch.zeros(40, dtype=torch.bool)
            inside[rows] = True
            assert float(D[inside].abs().max()) == 0.0 and float(saved[:, inside].abs().max()) == 0.0
            assert bool((D[~inside] == 7.0).all()) and bool((saved[:, ~inside] == 7.0).all())
