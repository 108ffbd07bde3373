"""Geometry and opacity gradients through the N-channel feature render on the MI355X (gsr_render_features_backward_geometry): the checks of
tests/test_feature_geometry_cpu.py on tests/test_gpu_contrib.py's frame (20 K Gaussians, 256 x 256, the one shared oracle frame, lists over 128 entries,
more than 1 % of the pixels terminate) and on the dense 100 x 70 / 3000 frame (a right quadrant missing at the image border, a partial tile row, several
batches per list) against the fp64 reference of tests/feature_geometry_reference.py with the same bars, the colour identity, the bit contracts, a band
and the two hand-computable frames.  The bench-frame size is covered by tools/gpu_feature_geometry_time.py."""
import functools

import pytest
import torch

import contrib_reference as CR
import feature_geometry_reference as R
import probe_reference as PR
import test_composite_cpu as T
import test_contrib_cpu as TC
import test_gpu_contrib as GC

pytestmark = pytest.mark.gpu

W = H = GC.W
P = 20_000
GEOMETRY = {"fused": ("means", "opac", "scales", "rot"), "precomp": ("means", "opac", "cov")}


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


@functools.lru_cache(maxsize=None)
def inputs(channels, seed=31):
    """(features [P,C] in [-1,1], upstream gradient [C,H,W] in [-0.5,0.5] with the fragile pixels zeroed), on the CPU: computed once, never modified."""
    aux, _ = GC.oracle_aux()
    g = torch.Generator().manual_seed(seed)
    f, up = torch.rand(P, channels, generator=g) * 2.0 - 1.0, torch.rand(channels, H, W, generator=g) - 0.5
    return f, R.mask_fragile(up, aux)


@functools.lru_cache(maxsize=None)
def dense_inputs(channels, form="fused", seed=31):
    aux, _ = TC.oracle_aux("dense", form)
    g = torch.Generator().manual_seed(seed)
    f, up = torch.rand(3000, channels, generator=g) * 2.0 - 1.0, torch.rand(channels, TC.H, TC.W, generator=g) - 0.5
    return f, R.mask_fragile(up, aux)


@functools.lru_cache(maxsize=None)
def reference_20k(channels):
    """The fp64 reference on the shared frame: computed once per channel count, never modified."""
    aux, s0 = GC.oracle_aux()
    return R.reference(aux, s0, *inputs(channels))


def records(pkg, rendered, f, g):
    """The [P,12] records of gsr_render_features_backward_geometry on the state behind `rendered` (a copy)."""
    st = pkg._saved_state(rendered, "render_features", "features")
    frame, _ = pkg._geometry_frame(st)
    with torch.cuda.device(st.device):
        rec, _scratch = pkg._feature_geometry_records(frame, f.cuda().contiguous(), g.cuda().contiguous())
    return rec.clone()


def geometry_pass(pkg, out, lv, f, g, keys):
    leaf = f.cuda().requires_grad_(True)
    F = pkg.render_features(out[0], leaf, geometry=True)
    (F * g.cuda()).sum().backward()
    got = {k: lv[k].grad for k in keys}
    got["features"] = leaf.grad
    return F.detach(), got


def dense_render(pkg, form="fused", tile_rows=None):
    cam, sc = TC.scene("dense")
    lv = T.make_leaves(sc, form, "cuda")
    out, S = T.render_pkg(pkg, cam, lv, form, torch.zeros(3, device="cuda"), return_alpha=False, tile_rows=tile_rows, device="cuda")
    return out, lv, S


def rel(a, b, scale):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max()) / float(scale.detach().double().abs().max())


@pytest.mark.parametrize("channels", [5, 35])
def test_gpu_records_match_the_reference_20k(channels):
    pkg = _pkg()
    aux, s0 = GC.oracle_aux()
    f, g = inputs(channels)
    stats = CR.reference(aux, s0)
    assert float(stats["terminated"].float().mean()) > 0.01 and stats["longest"] > 128
    out, lv, S = GC.render(pkg)
    R.check_records(f"feature_geometry_gpu_20k_c{channels}", records(pkg, out[0], f, g), reference_20k(channels), aux)


def test_gpu_end_to_end_against_the_composed_oracle_20k():
    pkg = _pkg()
    aux, s0 = GC.oracle_aux()
    cam, sc = GC.scene()
    f, g = inputs(5)
    ora = R.composed_oracle(cam, T.make_leaves(sc, "fused", grad=False), "fused", f, g)
    R.check_reference("feature_geometry_reference_20k", reference_20k(5), ora, aux, s0)
    out, lv, S = GC.render(pkg)
    _, got = geometry_pass(pkg, out, lv, f, g, GEOMETRY["fused"])
    T.grad_bars(got, {k: ora[k] for k in got}, "feature_geometry_gpu_e2e_20k")


def test_gpu_dense_frame_two_channel_groups():
    pkg = _pkg()
    aux, s0 = TC.oracle_aux("dense")
    f, g = dense_inputs(17)
    out, lv, S = dense_render(pkg)
    R.check_records("feature_geometry_gpu_dense_c17", records(pkg, out[0], f, g), R.reference(aux, s0, f, g), aux)


def test_gpu_identity_against_the_colour_render_itself():
    """features = colors_precomp, C = 3, bg = 0: per tensor the feature path's distance to the composed fp64 oracle is <= max(1e-5, 2 x the colour
    path's distance on this frame)."""
    pkg = _pkg()
    cam, sc = TC.scene("dense")
    _, g = dense_inputs(3, "precomp")
    out, lv, S = dense_render(pkg, "precomp")
    (out[0] * g.cuda()).sum().backward()
    colour = {k: lv[k].grad for k in GEOMETRY["precomp"]}
    colors = lv["colors"].detach().cpu()
    out2, lv2, _ = dense_render(pkg, "precomp")
    _, feature = geometry_pass(pkg, out2, lv2, colors, g, GEOMETRY["precomp"])
    ora = R.composed_oracle(cam, {k: v.detach().cpu() for k, v in lv.items()}, "precomp", colors, g)
    nums = {}
    for k in GEOMETRY["precomp"]:
        nums[f"{k}_colour"], nums[f"{k}_feature"] = rel(colour[k], ora[k], ora[k]), rel(feature[k], ora[k], ora[k])
    R.parity_report("feature_geometry_gpu_colour_identity", **nums)
    for k in GEOMETRY["precomp"]:
        assert nums[f"{k}_feature"] <= max(1e-5, 2.0 * nums[f"{k}_colour"]), nums


def test_gpu_two_runs_and_nan_rows():
    pkg = _pkg()
    f, g = inputs(17)
    out, lv, S = GC.render(pkg)
    a = records(pkg, out[0], f, g)
    out_b, lv_b, _ = GC.render(pkg)
    b = records(pkg, out_b[0], f, g)
    assert torch.equal(a, b) and float(a.abs().max()) > 0.0
    Fa, ga = geometry_pass(pkg, out, lv, f, g, GEOMETRY["fused"])
    Fb, gb = geometry_pass(pkg, out_b, lv_b, f, g, GEOMETRY["fused"])
    assert torch.equal(Fa, Fb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    # rows of Gaussians that contribute nowhere may hold NaN: no output bit changes, and their rows are exact zeros
    nowhere = pkg.contribution_stats(out[0]).pixel_count == 0
    poisoned = f.clone()
    poisoned[nowhere.cpu()] = float("nan")
    c = records(pkg, out[0], poisoned, g)
    assert int(nowhere.sum()) > 1000 and int((nowhere & (out[1] > 0)).sum()) > 100
    assert torch.equal(c, a) and float(a[nowhere].abs().max()) == 0.0 and float(a[:, 6:].abs().max()) == 0.0
    for k in GEOMETRY["fused"]:
        assert float(ga[k][nowhere].abs().max()) == 0.0 and float(ga[k][~nowhere].abs().max()) > 0.0, k


def test_gpu_band():
    pkg = _pkg()
    f, g = dense_inputs(5)
    out, lv, S = dense_render(pkg)
    full = records(pkg, out[0], f, g)
    parts = []
    for b in ((0, 1), (1, 3), (3, 5)):
        outb, _, _ = dense_render(pkg, tile_rows=b)
        parts.append(records(pkg, outb[0], f, g))
    total = sum(p.double() for p in parts)
    d = [float((total[:, k] - full[:, k].double()).abs().max()) / float(full[:, k].abs().max()) for k in range(6)]
    R.parity_report("feature_geometry_gpu_band", **{f"word{k}_bands_sum_vs_full_rel_max": v for k, v in enumerate(d)})
    assert max(d) <= 1e-6 and not torch.equal(parts[1], full) and float(parts[1].abs().max()) > 0.0


def test_gpu_hand_computable_frames():
    """tests/test_feature_geometry_cpu.py test_hand_computable_frames on the GPU."""
    pkg = _pkg()
    gvec = torch.tensor([1.0, 2.0, -1.0])
    for which, f in (("isolated", [[float("nan")] * 3, [2.0, -3.0, 0.5]]), ("layers", [[1.0, -2.0, 4.0], [3.0, 0.5, -1.0]])):
        cam, lv = PR.hand_frame(which)
        lv = {k: v.cuda().requires_grad_(True) for k, v in lv.items()}
        rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device="cuda"), device="cuda"))
        F, _ = rast.features(lv["means"], lv["opac"], torch.tensor(f, device="cuda"), scales=lv["scales"], rotations=lv["rot"], geometry=True)
        up = torch.zeros_like(F)
        up[:, PR.HAND_PY, PR.HAND_PX] = gvec.cuda()
        F.backward(up)
        got = lv["opac"].grad.reshape(-1).cpu()
        s = [float((torch.tensor(row) * gvec).sum()) for row in f]
        if which == "isolated":
            want, smax = [0.0, s[1]], abs(s[1])
            assert float(got[0]) == 0.0 and float(lv["means"].grad[0].abs().max()) == 0.0
        else:
            want, smax = [0.7 * s[0], s[1] - 0.9 * s[0]], max(abs(s[0]), abs(s[1]))
        assert float((got - torch.tensor(want)).abs().max()) <= 1e-5 * smax, (which, got, want)
        assert not bool(lv["means"].grad.isnan().any()) and not bool(lv["scales"].grad.isnan().any())
