"""The distortion loss on a rendered frame on the MI355X (gsr_distortion / gsr_distortion_backward): the checks of tests/test_distortion_cpu.py on
tests/test_gpu_contrib.py's frame (20 K Gaussians, 256 x 256, the one shared oracle frame, lists over 128 entries, more than 1 % of the pixels terminate)
and on the dense 100 x 70 / 3000 frame (a right quadrant missing at the image border, a partial tile row, several batches per list) against the fp64
reference of tests/distortion_reference.py with the same bars, the bit contracts, a band and the two hand-computable frames.  The bench-frame size is
covered by tools/gpu_distortion_time.py."""
import functools
from types import SimpleNamespace

import pytest
import torch

import contrib_reference as CR
import distortion_reference as R
import test_composite_cpu as T
import test_contrib_cpu as TC
import test_distortion_cpu as TD
import test_gpu_contrib as GC

pytestmark = pytest.mark.gpu

W = H = GC.W
GEOMETRY = TD.GEOMETRY


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


@functools.lru_cache(maxsize=None)
def upstream_20k(seed=41):
    """dL/dD [H,W] in [-0.3, 0.7] with the fragile pixels zeroed, on the CPU: computed once, never modified."""
    aux, _ = GC.oracle_aux()
    g = torch.Generator().manual_seed(seed)
    return R.mask_fragile(torch.rand(H, W, generator=g) - 0.3, aux)


@functools.lru_cache(maxsize=None)
def reference_20k(depth_mode, dtype=torch.float64):
    """The reference on the shared frame: computed once per mode and precision, never modified."""
    aux, s0 = GC.oracle_aux()
    return R.reference(aux, s0, upstream_20k(), depth_mode, dtype)


def run(pkg, rendered, g, depth_mode):
    """(D, saved, a copy of the [P,12] records) of the two entry points on the state behind `rendered`."""
    st = pkg._saved_state(rendered, "distortion_map", "distortion")
    frame, _ = pkg._geometry_frame(st)
    D, saved = pkg._distortion_forward(frame, depth_mode, True, st.device)
    with torch.cuda.device(st.device):
        rec, _scratch = pkg._distortion_records(frame, g.cuda().contiguous(), saved, depth_mode)
    return D, saved, rec.clone()


def dense_render(pkg, form="fused", tile_rows=None):
    cam, sc = TC.scene("dense")
    lv = T.make_leaves(sc, form, "cuda")
    out, S = T.render_pkg(pkg, cam, lv, form, torch.zeros(3, device="cuda"), return_alpha=False, tile_rows=tile_rows, device="cuda")
    return out, lv, S


@pytest.mark.parametrize("depth_mode", [0, 1])
def test_gpu_map_and_records_match_the_reference_20k(depth_mode):
    pkg = _pkg()
    aux, s0 = GC.oracle_aux()
    stats = CR.reference(aux, s0)
    assert float(stats["terminated"].float().mean()) > 0.01 and stats["longest"] > 128
    ref, ref32 = reference_20k(depth_mode), reference_20k(depth_mode, torch.float32)
    assert ref["multi"] > 0.25 * W * H
    out, lv, S = GC.render(pkg)
    D, saved, rec = run(pkg, out[0], upstream_20k(), depth_mode)
    R.check_map(f"distortion_gpu_20k_mode{depth_mode}_map", D, saved, ref, ref32, aux)
    R.check_records(f"distortion_gpu_20k_mode{depth_mode}", rec, ref, ref32, aux)


@pytest.mark.parametrize("depth_mode", [0, 1])
def test_gpu_dense_frame(depth_mode):
    pkg = _pkg()
    aux, _ = TC.oracle_aux("dense")
    out, lv, S = dense_render(pkg)
    D, saved, rec = run(pkg, out[0], TD.upstream(), depth_mode)
    ref, ref32 = TD.reference("fused", depth_mode), TD.reference("fused", depth_mode, torch.float32)
    R.check_map(f"distortion_gpu_dense_mode{depth_mode}_map", D, saved, ref, ref32, aux)
    R.check_records(f"distortion_gpu_dense_mode{depth_mode}", rec, ref, ref32, aux)


def test_gpu_end_to_end_against_the_autograd_oracle_20k():
    """The product's gradients against the oracle's autograd of the pairwise sum (T.grad_bars).  The reference's own distance to that autograd is the
    business of tests/test_distortion_cpu.py on the dense frame; on this frame it measures 2.8e-5 (means2D), 2.4e-6 (opacity), 6.3e-7 (depth) of
    max |grad|, above the 2e-5 that check_reference holds the dense frame to (the distance is between the fp32 frame inside `aux` and the fp64 frame of
    the autograd; why it is larger on this frame was not looked into)."""
    pkg = _pkg()
    cam, sc = GC.scene()
    g = upstream_20k()
    ora = R.autograd_oracle(cam, T.make_leaves(sc, "fused", grad=False), "fused", g, 1)
    out, lv, S = GC.render(pkg)
    D = pkg.distortion_map(out[0], inverse_depth=True)
    (D * g.cuda()).sum().backward()
    T.grad_bars({k: lv[k].grad for k in GEOMETRY["fused"]}, {k: ora[k] for k in GEOMETRY["fused"]}, "distortion_gpu_e2e_20k_mode1")


def test_gpu_two_runs_give_equal_bits():
    pkg = _pkg()
    g = upstream_20k()
    out, lv, S = GC.render(pkg)
    out_b, lv_b, _ = GC.render(pkg)
    a, b = run(pkg, out[0], g, 0), run(pkg, out_b[0], g, 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[2].abs().max()) > 0.0
    assert float(a[2][:, [6, 7, 8, 10, 11]].abs().max()) == 0.0
    grads = []
    for o, l in ((out, lv), (out_b, lv_b)):
        D = pkg.distortion_map(o[0])
        (D * g.cuda()).sum().backward()
        assert torch.equal(D.detach(), a[0])
        grads.append({k: l[k].grad for k in GEOMETRY["fused"]})
    assert all(torch.equal(grads[0][k], grads[1][k]) and float(grads[0][k].abs().max()) > 0.0 for k in grads[0])
    with torch.no_grad():
        plain, radii = pkg.GaussianRasterizer(S).distortion(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"])
    assert plain.grad_fn is None and torch.equal(plain, a[0]) and torch.equal(radii, out[1])


def test_gpu_band():
    pkg = _pkg()
    g = TD.upstream()
    out, lv, S = dense_render(pkg)
    D, _, full = run(pkg, out[0], g, 0)
    parts = []
    for b in ((0, 1), (1, 3), (3, 5)):
        outb, _, _ = dense_render(pkg, tile_rows=b)
        Db, _, rb = run(pkg, outb[0], g, 0)
        parts.append(rb)
        rows = slice(16 * b[0], min(16 * b[1], TC.H))
        outside = torch.ones(TC.H, dtype=torch.bool)
        outside[rows] = False
        assert torch.equal(Db[rows], D[rows]) and float(Db[rows].abs().max()) > 0.0 and float(Db.cpu()[outside].abs().sum()) == 0.0      # zeros outside the band
    total = sum(p.double() for p in parts)
    words = (0, 1, 2, 3, 4, 5, 9)
    d = [float((total[:, k] - full[:, k].double()).abs().max()) / float(full[:, k].abs().max()) for k in words]
    R.parity_report("distortion_gpu_band", **{f"word{k}_bands_sum_vs_full_rel_max": v for k, v in zip(words, d)})
    assert max(d) <= 1e-6 and not torch.equal(parts[1], full) and float(parts[1].abs().max()) > 0.0


def test_gpu_hand_computable_frames():
    """tests/test_distortion_cpu.py test_hand_computable_frames on the GPU."""
    import probe_reference as PR
    pkg = _pkg()

    def hand(which, inverse_depth):
        cam, lv = PR.hand_frame(which)
        lv = {k: v.cuda().requires_grad_(True) for k, v in lv.items()}
        rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device="cuda"), device="cuda"))
        D, _ = rast.distortion(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], inverse_depth=inverse_depth)
        up = torch.zeros_like(D)
        up[PR.HAND_PY, PR.HAND_PX] = 1.0
        D.backward(up)
        return D.detach().cpu(), {k: SimpleNamespace(grad=v.grad.cpu()) for k, v in lv.items()}

    TD.check_hand_frames(hand)
