"""Absolute screen-space gradients on the MI355X (gsr_backward_blend_abs, `GaussianRasterizer(..., absgrad=True)`): the checks of
tests/test_absgrad_cpu.py at 20 K Gaussians / 256 x 256 (the scene of tests/test_gpu_contrib.py) against the fp64 reference of tests/absgrad_reference.py
with the same bars (one oracle frame, shared), the bit identities at the same size, the single-pixel and cancellation cases, and band additivity."""
import functools

import pytest
import torch

from helpers import O, make_camera, make_scene
import absgrad_reference as R
import contrib_reference as CR
import test_composite_cpu as T

pytestmark = pytest.mark.gpu

W = H = 256
DEV = "cuda"


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


@functools.lru_cache(maxsize=None)
def scene(which="frame"):
    if which == "corner":      # one isotropic Gaussian on the optical axis of a 32 x 32 frame: centre (15.5, 15.5), a pixel corner
        cam = make_camera(32, 32)
        sc = make_scene(1, cam, seed=1)
        sc.means3D = torch.tensor([[0.0, 0.0, 4.0]])
        sc.scales = torch.full((1, 3), 0.3)
        sc.rotations = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
        sc.opacities = torch.tensor([[0.8]])
        return cam, sc
    cam = make_camera(W, H)
    sc = make_scene(20_000, cam, seed=3, s_med=0.02)
    sc.opacities = CR.raise_opacity(sc.opacities)
    return cam, sc


@functools.lru_cache(maxsize=None)
def oracle_aux(which="frame", form="fused"):
    """The oracle's frame: computed once, shared by the tests, never modified."""
    cam, sc = scene(which)
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, False)
    with torch.no_grad():
        aux = O.rasterize(s=s0, want_fragile=True, return_aux=True, **T.call_kwargs(T.make_leaves(sc, form, grad=False), form, oracle=True))[3]
    return aux, s0


@functools.lru_cache(maxsize=None)
def loss_weights(which="frame", form="fused", seed=7):
    """(dL/dC [3,H,W], dL/dD [1,H,W]) on the CPU, zero at the fragile pixels."""
    aux, _ = oracle_aux(which, form)
    cam, _ = scene(which)
    g = torch.Generator().manual_seed(seed)
    return [R.mask_fragile(torch.rand(n, cam.image_height, cam.image_width, generator=g) - 0.3, aux) for n in (3, 1)]


def run(pkg, which="frame", form="fused", absgrad=True, wC=None, wD=None, tile_rows=None, backward=True):
    cam, sc = scene(which)
    lv = T.make_leaves(sc, form, DEV)
    lv["m2d"] = torch.zeros(sc.P, 3, device=DEV, requires_grad=True)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device=DEV), device=DEV)
    rast = pkg.GaussianRasterizer(S, absgrad=absgrad)
    if tile_rows is not None:
        rast.tile_rows = tile_rows
    out = rast(**dict(T.call_kwargs(lv, form), means2D=lv["m2d"]))
    if backward:
        loss = (out[0] * wC.to(DEV)).sum()
        if wD is not None:
            loss = loss + (out[2] * wD.to(DEV)).sum()
        loss.backward()
    return out, lv, S


def records(pkg, out, S, wC, wD, absgrad, tile_rows=None):
    """The [P,12] records of gsr_backward_blend / gsr_backward_blend_abs on the state the render's autograd node keeps (call before backward())."""
    fn = out[0].grad_fn
    saved = fn.saved_tensors
    geom, binning, img = saved[8:11]
    keep = []
    with torch.cuda.device(geom.device):
        s = pkg._make_settings(S, keep, tile_rows, bg_image=True)
        rec = pkg._backward_blend(s, int(saved[0].shape[0]), pkg._Forward(geom, binning, img, fn.num_rendered), wC.to(DEV).contiguous(),
                                  None if wD is None else wD.to(DEV).contiguous(), geom.device, None, absgrad)
        return rec.clone()


@pytest.mark.parametrize("depth", [False, True])
def test_gpu_absgrad_matches_the_reference_20k(depth):
    pkg = _pkg()
    aux, s0 = oracle_aux()
    wC, wD = loss_weights()
    wD = wD if depth else None
    ref = R.reference(aux, s0, wC, wD)
    _, lv, _ = run(pkg, wC=wC, wD=wD)
    m2d = lv["m2d"]
    # the reference's signed sums against the product's own means2D.grad are reported; tests/test_absgrad_cpu.py validates the reference against the
    # oracle's autograd at the project's bar on the small frames
    nums = R.check(f"absgrad_gpu_20k_d{int(depth)}", m2d.absgrad, m2d.grad, ref, aux)
    a, g = m2d.absgrad[:, :2].double(), m2d.grad[:, :2].double().abs()
    assert bool((a + R.BAR * float(a.max()) >= g).all()) and nums["cancellation"] < 0.9
    silent = (ref["abs"].sum(1) == 0).to(DEV)
    assert int(silent.sum()) > 100 and float(m2d.absgrad[silent].abs().max()) == 0.0


@pytest.mark.parametrize("depth", [False, True])
def test_gpu_on_off_and_two_runs_agree_bit_for_bit_20k(depth):
    pkg = _pkg()
    wC, wD = loss_weights()
    wD = wD if depth else None
    out, lv_on, S = run(pkg, wC=wC, wD=wD, backward=False)
    rec_on, rec_off = records(pkg, out, S, wC, wD, True), records(pkg, out, S, wC, wD, False)
    loss = (out[0] * wC.to(DEV)).sum()
    (loss if wD is None else loss + (out[2] * wD.to(DEV)).sum()).backward()
    _, lv_off, _ = run(pkg, absgrad=False, wC=wC, wD=wD)
    _, lv_again, _ = run(pkg, wC=wC, wD=wD)
    for k in lv_on:
        assert lv_on[k].grad is not None and torch.equal(lv_on[k].grad, lv_off[k].grad), k
        assert torch.equal(lv_on[k].grad, lv_again[k].grad), k
    assert torch.equal(rec_on[:, :10], rec_off[:, :10]) and float(rec_on[:, :10].abs().max()) > 0
    assert float(rec_off[:, 10:].abs().max()) == 0.0 and float(rec_on[:, 10:].min()) >= 0.0 and int((rec_on[:, 10] > 0).sum()) > 5000
    assert torch.equal(lv_on["m2d"].absgrad, lv_again["m2d"].absgrad) and not hasattr(lv_off["m2d"], "absgrad")
    assert torch.equal(lv_on["m2d"].absgrad[:, 0], rec_on[:, 10] * (0.5 * W)) and torch.equal(lv_on["m2d"].absgrad[:, 1], rec_on[:, 11] * (0.5 * H))


def test_gpu_single_pixel_loss_20k():
    pkg = _pkg()
    aux, _ = oracle_aux()
    ok = (~aux["fragile"]) & (aux["n_contrib"] > 20)
    ok[:, :10] = False
    y, x = [int(v) for v in ok.nonzero()[0]]
    wC = torch.zeros(3, H, W)
    wC[:, y, x] = torch.tensor([0.7, -0.4, 0.5])
    _, lv, _ = run(pkg, wC=wC)
    a, g = lv["m2d"].absgrad[:, :2].double(), lv["m2d"].grad[:, :2].double().abs()
    assert int((g.sum(1) > 0).sum()) > 10
    d = float((a - g).abs().max()) / float(g.max())
    R.parity_report("absgrad_gpu_single_pixel", abs_vs_grad_rel_max=d, gaussians=int((g.sum(1) > 0).sum()))
    assert d < R.BAR


def test_gpu_cancellation_under_one_gaussian():
    """One isotropic Gaussian on a pixel corner, dL/dC symmetric about its centre -- the per-pixel gradient terms are then antisymmetric, see
    tests/test_absgrad_cpu.py --: |grad| < 1e-3 absgrad, and absgrad is the reference's."""
    pkg = _pkg()
    aux, s0 = oracle_aux("corner", "precomp")
    frag = aux["fragile"] | aux["fragile"].flip(0, 1)
    w = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(3)) - 0.3
    wC = w + w.flip(1, 2)
    wC[:, frag] = 0.0
    ref = R.reference(aux, s0, wC)
    _, lv, _ = run(pkg, "corner", "precomp", wC=wC)
    a, g = lv["m2d"].absgrad[0, :2].double().cpu(), lv["m2d"].grad[0, :2].double().abs().cpu()
    R.parity_report("absgrad_gpu_cancellation", grad_over_absgrad_x=float(g[0] / a[0]), grad_over_absgrad_y=float(g[1] / a[1]))
    assert bool((g < 1e-3 * a).all()) and float(a.min()) > 0
    R.check("absgrad_gpu_corner", lv["m2d"].absgrad, None, ref, aux)


def test_gpu_bands_add_up_20k():
    pkg = _pkg()
    wC, wD = loss_weights()
    k, gy = 7, H // 16
    recs = []
    for band in (None, (0, k), (k, gy)):
        out, _, S = run(pkg, wC=wC, wD=wD, tile_rows=band, backward=False)
        recs.append(records(pkg, out, S, wC, wD, True, band)[:, 10:].double())
    full, lo, hi = recs
    d = float((lo + hi - full).abs().max()) / float(full.max())
    R.parity_report("absgrad_gpu_bands", sum_vs_full_rel_max=d)
    assert d < 1e-6 and float(lo.max()) > 0 and float(hi.max()) > 0 and int(((lo.sum(1) > 0) & (hi.sum(1) > 0)).sum()) > 100
