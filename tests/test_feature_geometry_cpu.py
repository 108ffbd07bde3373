"""Geometry and opacity gradients through the N-channel feature render (gsr_render_features_backward_geometry, `render_features(..., geometry=True)`,
`GaussianRasterizer.features(..., geometry=True)`) through the shipped package on the CPU: the SIMT build of the whole library behind the package's own
loader, on the scenes of tests/test_features_cpu.py.  Reference and bars: tests/feature_geometry_reference.py.

16 / 8 / 4 channels per walk (16 while more than 8 remain, then 8, then 4) are the kernel's compile-time groups (csrc/feature_geom.hip):
C = 1 and 5 fill a group partly, 16 exactly, 17 = 16 + 1 and 35 = 16 + 16 + 3 accumulate two and three groups into one record.

Test infrastructure: the product never loads the SIMT library."""
import ctypes as C
import functools
import os
import subprocess
import sys
from unittest import mock

import pytest
import torch

from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import feature_geometry_reference as R
import probe_reference as PR
import test_composite_cpu as T
import test_contrib_cpu as TC
import test_features_cpu as TF

W, H = TC.W, TC.H
ROOT = T.ROOT
GEOMETRY = {"fused": ("means", "opac", "scales", "rot"), "precomp": ("means", "opac", "cov")}


def inputs(which, channels, form="fused", h=H, w=W):
    """(features, upstream gradient with the fragile pixels zeroed) of tests/test_features_cpu.inputs: shared, never modified."""
    aux, _ = TC.oracle_aux(which, form)
    f, up = TF.inputs(aux["means2D"].shape[0], h, w, channels)
    return f, R.mask_fragile(up, aux)


@functools.lru_cache(maxsize=None)
def reference(which, channels, form="fused", h=H, w=W):
    aux, s0 = TC.oracle_aux(which, form)
    return R.reference(aux, s0, *inputs(which, channels, form, h, w))


def records_through_the_c_abi(pkg, rendered, S, f, g, tile_rows=None):
    """gsr_render_features_backward_geometry on the state behind `rendered` -> a copy of the [P,12] records."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    st = pkg._saved_state(rendered, "render_features", "features")
    keep = []
    s = pkg._make_settings(S, keep, tile_rows, bg_image=True)
    scratch = torch.full((int(lib.gsr_backward_scratch_bytes(st.P, st.fwd.num_rendered)),), 0xA5, dtype=torch.uint8)      # garbage, not zeros
    rec = C.c_void_p(0)
    f, g = f.contiguous(), g.contiguous()
    assert lib.gsr_render_features_backward_geometry(C.byref(s), st.P, st.fwd.num_rendered, pkg._ptr(st.fwd.geom), pkg._ptr(st.fwd.binning),
                                                     pkg._ptr(st.fwd.img), pkg._ptr(f), pkg._ptr(g), f.shape[1], pkg._ptr(scratch), C.byref(rec),
                                                     None) == 0, lib.gsr_last_error()
    off = int(rec.value) - scratch.data_ptr()
    return scratch[off:off + st.P * 48].view(torch.float32).view(st.P, 12).clone()


def geometry_pass(pkg, which, f, g, form="fused", aa=False, geometry=True, feature_grad=True):
    """One frame, one feature render, one backward of (F * g).sum() -> (F, dict of the leaves' gradients, incl. `features` unless feature_grad is off:
    the feature gradient's own walks are tests/test_features_cpu.py's business and take SIMT time)."""
    out, lv, S = TC.render(pkg, which, form, aa)
    leaf = f.clone().requires_grad_(feature_grad)
    F = pkg.render_features(out[0], leaf, geometry=geometry)
    (F * g).sum().backward()
    got = {k: lv[k].grad for k in GEOMETRY[form]}
    if feature_grad:
        got["features"] = leaf.grad
    return F.detach(), got


def rel(a, b, scale):
    return float((a.detach().double() - b.detach().double()).abs().max()) / float(scale.detach().double().abs().max())


def test_the_reference_is_the_composed_oracles_autograd():
    """Reference alone, before it judges anything: words 0, 1 and 5 against the oracle's autograd through colors_precomp triples (2e-5 of max |grad|)."""
    aux, s0 = TC.oracle_aux("dense")
    cam, sc = TC.scene("dense")
    f, g = inputs("dense", 5)
    ora = R.composed_oracle(cam, T.make_leaves(sc, "fused", grad=False), "fused", f, g)
    R.check_reference("feature_geometry_reference_dense", reference("dense", 5), ora, aux, s0)


@pytest.mark.parametrize("form", ["fused", "precomp"])
def test_records_against_the_reference_through_the_c_abi(simt_lib, form):
    aux, _ = TC.oracle_aux("dense", form)
    stats = TC.R.reference(*TC.oracle_aux("dense", form))
    assert float(stats["terminated"].float().mean()) > 0.02 and stats["longest"] > 128
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", form)
        for channels in (1, 5, 16, 17, 35):
            f, g = inputs("dense", channels, form)
            got = records_through_the_c_abi(pkg, out[0], S, f, g)
            R.check_records(f"feature_geometry_cpu_dense_{form}_c{channels}", got, reference("dense", channels, form), aux)


@pytest.mark.parametrize("aa", [False, True])
def test_end_to_end_against_the_composed_oracle(simt_lib, aa):
    cam, sc = TC.scene("dense")
    aux, _ = TC.oracle_aux("dense", "fused", aa)
    f, up = TF.inputs(3000, H, W, 5)
    g = R.mask_fragile(up, aux)
    ora = R.composed_oracle(cam, T.make_leaves(sc, "fused", grad=False), "fused", f, g, aa)
    with package_on_the_cpu(simt_lib) as pkg:
        _, got = geometry_pass(pkg, "dense", f, g, "fused", aa)
    T.grad_bars(got, {k: ora[k] for k in got}, f"feature_geometry_cpu_e2e_aa{int(aa)}")


def test_identity_against_the_colour_render_itself(simt_lib):
    """features = colors_precomp, C = 3, bg = 0: the feature path's geometry gradients are the colour render's own, both fp32 evaluations of the same sums
    in different orders.  Per tensor: distance to the composed fp64 oracle <= max(1e-5, 2 x the colour path's distance on this frame)."""
    cam, sc = TC.scene("dense")
    aux, _ = TC.oracle_aux("dense", "precomp")
    _, up = TF.inputs(3000, H, W, 3)
    g = R.mask_fragile(up, aux)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", "precomp")
        (out[0] * g).sum().backward()
        colour = {k: lv[k].grad for k in GEOMETRY["precomp"]}
        colors = lv["colors"].detach()
        _, feature = geometry_pass(pkg, "dense", colors, g, "precomp")
    ora = R.composed_oracle(cam, lv, "precomp", colors, g)
    nums = {}
    for k in GEOMETRY["precomp"]:
        nums[f"{k}_colour"], nums[f"{k}_feature"] = rel(colour[k], ora[k], ora[k]), rel(feature[k], ora[k], ora[k])
    R.parity_report("feature_geometry_cpu_colour_identity", **nums)
    for k in GEOMETRY["precomp"]:
        assert nums[f"{k}_feature"] <= max(1e-5, 2.0 * nums[f"{k}_colour"]), nums


@pytest.mark.parametrize("leaves", ["plain", "non_leaf_fp64"])
def test_a_colour_loss_and_a_feature_loss_on_one_frame(simt_lib, leaves):
    """One backward of both losses gives every leaf the sum of the two separate backwards (fp32 addition); also when opacities / scales are non-leaves and
    means3D arrives as fp64 -- the case where the tensors the rasterizer saved are converted copies."""
    cam, sc = TC.scene("sparse")
    f, g = inputs("sparse", 5, h=80, w=96)
    wc = T.weights(80, 96)[0]
    with package_on_the_cpu(simt_lib) as pkg:
        lv = T.make_leaves(sc, "fused")
        leaf = f.clone().requires_grad_(True)
        if leaves == "plain":
            roots = dict(lv, features=leaf)
            call = lv
        else:
            raw_op = torch.logit(lv["opac"].detach().clamp(1e-4, 1 - 1e-4)).requires_grad_(True)
            raw_sc = lv["scales"].detach().log().requires_grad_(True)
            means64 = lv["means"].detach().double().requires_grad_(True)
            roots = dict(means=means64, opac=raw_op, scales=raw_sc, rot=lv["rot"], shs=lv["shs"], features=leaf)
            call = dict(lv, means=means64, opac=torch.sigmoid(raw_op), scales=torch.exp(raw_sc))
        out, S = T.render_pkg(pkg, cam, call, "fused", torch.zeros(3), return_alpha=False)
        F = pkg.render_features(out[0], leaf, geometry=True)
        loss_c, loss_f = (out[0] * wc).sum(), (F * g).sum()
        keys = list(roots)
        gc = torch.autograd.grad(loss_c, [roots[k] for k in keys], retain_graph=True, allow_unused=True)
        gf = torch.autograd.grad(loss_f, [roots[k] for k in keys], retain_graph=True, allow_unused=True)
        both = torch.autograd.grad(loss_c + loss_f, [roots[k] for k in keys], allow_unused=True)
    nums = {}
    for k, a, b, ab in zip(keys, gc, gf, both):
        if k == "shs":
            assert b is None and torch.equal(a, ab)
            continue
        if k == "features":
            assert a is None and torch.equal(b, ab)
            continue
        assert a is not None and b is not None and float(b.abs().max()) > 0.0, k
        assert ab.dtype == roots[k].dtype and ab.shape == roots[k].shape
        nums[k] = rel(ab, a.double() + b.double(), ab)
    R.parity_report(f"feature_geometry_cpu_two_losses_{leaves}", **nums)
    assert max(nums.values()) <= 1e-6, nums


def test_geometry_false_is_todays_path(simt_lib):
    f, g = inputs("sparse", 5, h=80, w=96)
    with package_on_the_cpu(simt_lib) as pkg:
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        calls = []
        real = lib.gsr_render_features_backward_geometry
        with mock.patch.object(lib, "gsr_render_features_backward_geometry", lambda *a: (calls.append("g"), real(*a))[1]):
            out, lv, S = TC.render(pkg, "sparse")
            leaf = f.clone().requires_grad_(True)
            F0 = pkg.render_features(out[0], leaf)
            (F0 * g).sum().backward()
            assert calls == [] and all(lv[k].grad is None for k in GEOMETRY["fused"])
            # nothing to differentiate: nothing kept, no graph
            with torch.no_grad():
                plain = pkg.render_features(out[0], f, geometry=True)
            assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, F0.detach())
            with torch.no_grad():
                alone, _ = pkg.GaussianRasterizer(S).features(lv["means"], lv["opac"], f, scales=lv["scales"], rotations=lv["rot"], geometry=True)
            assert alone.grad_fn is None and torch.equal(alone, F0.detach())
            F1, got = geometry_pass(pkg, "sparse", f, g)
            assert calls == ["g"]
            # geometry=True with no geometry tensor that requires grad: the feature gradient alone, the geometry walk does not run
            leaf2 = f.clone().requires_grad_(True)
            F2, _ = pkg.GaussianRasterizer(S).features(lv["means"].detach(), lv["opac"].detach(), leaf2, scales=lv["scales"].detach(),
                                                       rotations=lv["rot"].detach(), geometry=True)
            (grad2,) = torch.autograd.grad((F2 * g).sum(), [leaf2])
            assert calls == ["g"]
    assert torch.equal(F0.detach(), F1) and torch.equal(leaf.grad, got["features"]) and torch.equal(grad2, leaf.grad)
    assert all(float(got[k].abs().max()) > 0.0 for k in GEOMETRY["fused"])


def test_only_contributors_count(simt_lib):
    """Rows of Gaussians that contribute nowhere may hold NaN: no output bit changes; their records and parameter gradients are exact zeros."""
    f, g = inputs("dense", 5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        nowhere = pkg.contribution_stats(out[0]).pixel_count == 0
        poisoned = f.clone()
        poisoned[nowhere] = float("nan")
        clean_rec = records_through_the_c_abi(pkg, out[0], S, f, g)
        got_rec = records_through_the_c_abi(pkg, out[0], S, poisoned, g)
        F_clean, clean = geometry_pass(pkg, "dense", f, g, feature_grad=False)
        F_got, got = geometry_pass(pkg, "dense", poisoned, g, feature_grad=False)
    assert int(nowhere.sum()) > 100 and int((nowhere & (out[1] > 0)).sum()) > 20      # culled and hidden ones
    assert torch.equal(got_rec, clean_rec) and not bool(got_rec.isnan().any()) and torch.equal(F_got, F_clean)
    assert float(clean_rec[nowhere].abs().max()) == 0.0 and float(clean_rec[~nowhere].abs().max()) > 0.0
    for k in clean:
        assert torch.equal(got[k], clean[k]), k
        assert float(clean[k][nowhere].abs().max()) == 0.0 and float(clean[k][~nowhere].abs().max()) > 0.0, k


def test_two_runs_and_the_standalone_form_give_equal_bits(simt_lib):
    f, g = inputs("dense", 5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, _, S0 = TC.render(pkg, "dense")
        ra, rb = records_through_the_c_abi(pkg, out[0], S0, f, g), records_through_the_c_abi(pkg, out[0], S0, f, g)
        Fa, a = geometry_pass(pkg, "dense", f, g, feature_grad=False)
        cam, sc = TC.scene("dense")
        lv = T.make_leaves(sc, "fused")
        leaf = f.clone()
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        F, radii = pkg.GaussianRasterizer(S).features(lv["means"], lv["opac"], leaf, scales=lv["scales"], rotations=lv["rot"], geometry=True)
        (F * g).sum().backward()
    alone = {k: lv[k].grad for k in GEOMETRY["fused"]}
    assert torch.equal(ra, rb) and float(ra.abs().max()) > 0.0 and torch.equal(Fa, F.detach())
    for k in a:
        assert torch.equal(a[k], alone[k]) and float(a[k].abs().max()) > 0.0, k


def test_the_launch_order_does_not_show_in_the_bits(simt_lib):
    """The walks start in the blend backward's planned order (option bwd_heavy_first: tiles by their heaviest half by default): every wave owns its
    slots, so index order and half tiles on their own give the same records."""
    f, g = inputs("sparse", 17, h=80, w=96)
    with package_on_the_cpu(simt_lib) as pkg:
        from diff_gaussian_rasterization import _lib
        out, lv, S = TC.render(pkg, "sparse")
        got = []
        try:
            for order in (2, 0, 3):
                _lib.set_option("bwd_heavy_first", order)
                got.append(records_through_the_c_abi(pkg, out[0], S, f, g))
        finally:
            _lib.set_option("bwd_heavy_first", 2)
    assert float(got[0].abs().max()) > 0.0 and torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def test_records_are_independent_of_the_lane_schedule(simt_lib, tmp_path):
    """SIMT_SCHEDULE shuffles wave interleaving and workgroup order: the records (two channel groups accumulate) are the same bits."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, torch\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {os.path.join(ROOT, 'gaussian-splatting_amd')!r}]\n"
        "import test_feature_geometry_cpu as G\n"
        "f, g = G.inputs('sparse', 17, h=80, w=96)\n"
        "with G.package_on_the_cpu(sys.argv[1]) as pkg:\n"
        "    out, lv, S = G.TC.render(pkg, 'sparse')\n"
        "    torch.save(G.records_through_the_c_abi(pkg, out[0], S, f, g), sys.argv[2])\n")
    outs = []
    for k, sched in enumerate([None, "5", "11"]):
        env = dict(os.environ)
        env.pop("SIMT_SCHEDULE", None)
        if sched is not None:
            env["SIMT_SCHEDULE"] = sched
        out = tmp_path / f"r{k}.pt"
        subprocess.run([sys.executable, str(script), simt_lib, str(out)], check=True, env=env, cwd=ROOT, timeout=900)
        outs.append(torch.load(out))
    assert float(outs[0].abs().max()) > 0.0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_band(simt_lib):
    f, g = inputs("dense", 5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        full = records_through_the_c_abi(pkg, out[0], S, f, g)
        parts = []
        for b in ((0, 1), (1, 3), (3, 5)):
            outb, _, Sb = TC.render(pkg, "dense", tile_rows=b)
            parts.append(records_through_the_c_abi(pkg, outb[0], Sb, f, g, tile_rows=b))
    total = sum(p.double() for p in parts)
    d = [float((total[:, k] - full[:, k].double()).abs().max()) / float(full[:, k].abs().max()) for k in range(6)]
    R.parity_report("feature_geometry_cpu_band", **{f"word{k}_bands_sum_vs_full_rel_max": v for k, v in enumerate(d)})
    assert max(d) <= 1e-6 and not torch.equal(parts[1], full) and float(parts[1].abs().max()) > 0.0


def test_hand_computable_frames(simt_lib):
    """An upstream gradient at pixel (32, 24) alone, s_k = <f_k, g>, G = 1 at the centre.  Isolated: dL/dopacity[1] = s_1 (T = 1, nothing behind), row 0
    zero.  Layers (front id 1, alpha 0.3; back id 0, alpha 0.9): dL/dopacity[1] = s_1 - 0.9 s_0 (T = 1; the suffix w_0 s_0 = 0.7 0.9 s_0 over 1 - 0.3),
    dL/dopacity[0] = 0.7 s_0."""
    gvec = torch.tensor([1.0, 2.0, -1.0])
    with package_on_the_cpu(simt_lib) as pkg:
        for which, f in (("isolated", [[float("nan")] * 3, [2.0, -3.0, 0.5]]), ("layers", [[1.0, -2.0, 4.0], [3.0, 0.5, -1.0]])):
            cam, lv = PR.hand_frame(which)
            lv = {k: v.clone().requires_grad_(True) for k, v in lv.items()}
            rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3)))
            F, _ = rast.features(lv["means"], lv["opac"], torch.tensor(f), scales=lv["scales"], rotations=lv["rot"], geometry=True)
            up = torch.zeros_like(F)
            up[:, PR.HAND_PY, PR.HAND_PX] = gvec
            F.backward(up)
            got = lv["opac"].grad.reshape(-1)
            s = [float((torch.tensor(row) * gvec).sum()) for row in f]
            if which == "isolated":
                want, smax = [0.0, s[1]], abs(s[1])
                assert float(got[0]) == 0.0 and float(lv["means"].grad[0].abs().max()) == 0.0
            else:
                want, smax = [0.7 * s[0], s[1] - 0.9 * s[0]], max(abs(s[0]), abs(s[1]))
            assert float((got - torch.tensor(want)).abs().max()) <= 1e-5 * smax, (which, got, want)
            assert not bool(lv["means"].grad.isnan().any()) and not bool(lv["scales"].grad.isnan().any())


def test_edge_and_error_cases(simt_lib):
    z3 = torch.zeros(0, 3)
    f, g = inputs("dense", 5)
    with package_on_the_cpu(simt_lib) as pkg:
        cam, sc = TC.scene("dense")
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        rast = pkg.GaussianRasterizer(S)
        # no Gaussian at all
        m0, o0 = z3.clone().requires_grad_(True), torch.zeros(0, 1, requires_grad=True)
        F0, _ = rast.features(m0, o0, torch.zeros(0, 5, requires_grad=True), scales=z3, rotations=torch.zeros(0, 4), geometry=True)
        (F0 * g).sum().backward()
        assert F0.shape == (5, H, W) and m0.grad.shape == (0, 3) and o0.grad.shape == (0, 1)
        # a frame without a single instance (every Gaussian behind the camera): zero rows
        lv = T.make_leaves(sc, "fused")
        behind = (lv["means"].detach() * torch.tensor([1.0, 1.0, -1.0])).requires_grad_(True)
        F1, _ = rast.features(behind, lv["opac"], f, scales=lv["scales"], rotations=lv["rot"], geometry=True)
        (F1 * g).sum().backward()
        assert float(F1.detach().abs().max()) == 0.0
        for t in (behind, lv["opac"], lv["scales"], lv["rot"]):
            assert t.grad is not None and float(t.grad.abs().max()) == 0.0
        # the multi-GPU renderers stay refused; freed state raises the existing message
        lv = T.make_leaves(sc, "fused")
        kw = T.call_kwargs(lv, "fused")
        synced = pkg.rasterize_gaussians(kw["means3D"], None, kw["shs"], None, kw["opacities"], kw["scales"], kw["rotations"], None, S,
                                         grad_sync=lambda records: None)
        with pytest.raises(pkg.GsrError, match="multi-GPU"):
            pkg.render_features(synced[0], f, geometry=True)
        out, lv, _ = TC.render(pkg, "dense")
        out[0].sum().backward()
        with pytest.raises(pkg.GsrError, match="call render_features before backward"):
            pkg.render_features(out[0], f, geometry=True)


def test_c_level_argument_checks(simt_lib):
    with package_on_the_cpu(simt_lib):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = _lib.GsrRasterSettings()
        s.image_width, s.image_height = 40, 40
        s.bg = s.viewmatrix = s.projmatrix = s.campos = 0x1000
        s.tanfovx = s.tanfovy = 0.5
        fn = lib.gsr_render_features_backward_geometry
        rec = C.c_void_p(0)
        ok = 0x1000
        assert fn(C.byref(s), 10, 0, None, None, None, None, None, 3, ok, C.byref(rec), None) == -1 and b"features / dL_dout" in lib.gsr_last_error()
        assert fn(C.byref(s), 10, 0, None, None, None, ok, ok, 3, None, C.byref(rec), None) == -1 and b"bwd_scratch" in lib.gsr_last_error()
        assert fn(C.byref(s), 10, 0, None, None, None, ok, ok, 3, ok, None, None) == -1 and b"splat_grads_out" in lib.gsr_last_error()
        assert fn(C.byref(s), 10, 5, None, ok, ok, ok, ok, 3, ok, C.byref(rec), None) == -1 and b"state buffers" in lib.gsr_last_error()
        assert fn(C.byref(s), 10, 0, None, None, None, ok, ok, 3, 0x1008, C.byref(rec), None) == -1 and b"16-byte" in lib.gsr_last_error()
        for P, R_ in ((-1, 0), (10, -1)):
            assert fn(C.byref(s), P, R_, None, None, None, ok, ok, 3, ok, C.byref(rec), None) == -1
        assert fn(None, 10, 0, None, None, None, ok, ok, 3, ok, C.byref(rec), None) == -1
        for bad in (0, -1, 1025):
            assert fn(C.byref(s), 0, 0, None, None, None, None, None, bad, None, C.byref(rec), None) == -1 and b"[1, 1024]" in lib.gsr_last_error()
        # P == 0: nothing to write; no instance: zero rows, and no state is needed
        assert fn(C.byref(s), 0, 0, None, None, None, None, None, 3, None, C.byref(rec), None) == 0 and rec.value is None
        for band in ((0, 0), (1, 2)):
            s.tile_y0, s.tile_y1 = band
            scratch = torch.full((int(lib.gsr_backward_scratch_bytes(10, 0)),), 0xA5, dtype=torch.uint8)
            x = torch.ones(10, 3)
            assert fn(C.byref(s), 10, 0, None, None, None, x.data_ptr(), x.data_ptr(), 3, scratch.data_ptr(), C.byref(rec), None) == 0
            off = int(rec.value) - scratch.data_ptr()
            assert 0 <= off and bool((scratch[off:off + 480].view(torch.float32) == 0.0).all())


def test_the_colors_precomp_form_of_the_per_gaussian_call_equals_the_sh_form(simt_lib):
    """The geometry path runs gsr_backward_preprocess with a zero colors_precomp instead of the frame's SH tensor (no [P,M,3] gradient allocated): on the
    same records every geometry gradient has the SH-form call's bits."""
    f, g = inputs("dense", 5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense")
        st = pkg._saved_state(out[0], "render_features", "features")
        frame, _ = pkg._geometry_frame(st)
        records = records_through_the_c_abi(pkg, out[0], S, f, g)
        a = pkg._geometry_from_records(frame, records, records.device)
        saved = st.node.saved_tensors
        P, M = st.P, st.node.M
        b, _ = pkg._gradients(P, records.device, False, False, M, False, True, True)
        keep = []
        s = pkg._make_settings(S, keep, None, bg_image=True)
        pkg._backward_preprocess(s, P, M, (saved[0], saved[1], None, saved[3], saved[4], saved[5], None), saved[7], st.fwd.geom, records, b, records.device)
    assert M == 16 and b[5].shape == (P, 16, 3) and float(b[5].abs().max()) == 0.0 and float(a[1].abs().max()) == 0.0
    for k in (0, 2, 3, 6, 7):      # dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dscales, dL_drotations
        assert torch.equal(a[k], b[k]) and float(a[k].abs().max()) > 0.0, k
