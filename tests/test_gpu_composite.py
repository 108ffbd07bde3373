"""The differentiable alpha image and the per-pixel / learnable background on the MI355X (gsr_rasterize_forward_composite,
gsr_backward_blend_composite): the checks of tests/test_composite_cpu.py at 20 K Gaussians / 256 x 256 against the composed oracle with the
bars of tests/test_gpu_reference_glue.py, bit-reproducibility at the bench frame's size (1 M Gaussians, 1920 x 1080), and a pose fitted on a
silhouette alone."""
import math

import pytest
import torch

from helpers import make_camera, make_scene
import test_camera_grad_cpu as CG
import test_composite_cpu as T

pytestmark = pytest.mark.gpu

W = H = 256


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


def _scene(which, P=20_000):
    """The two kinds of scene of the CPU tests at 20 K Gaussians: coverage scales with P * s_med^2 (dense: mean alpha 0.76, 1.8 % of the pixels
    above 0.99; sparse: 11 % of the pixels, 7 K of them, have no contributor -- at 20 K Gaussians on 65 K pixels the 0.3-pixel low-pass filter keeps
    every footprint a few pixels wide, so the share does not grow with a smaller s_med; the tests ask for 5 %)."""
    cam = make_camera(W, H)
    return cam, make_scene(P, cam, seed=3, s_med=0.02 if which == "dense" else 0.001)


def _run(pkg, cam, sc, form, aa, bg, parts, return_alpha=True):
    w = T.weights(H, W, "cuda")
    lv = T.make_leaves(sc, form, "cuda")
    out, _ = T.render_pkg(pkg, cam, lv, form, bg, aa, return_alpha=return_alpha, device="cuda")
    Tf = T.final_T_of(pkg, out[0], sc.P, H, W)      # (before backward frees the node's state)
    T.loss_of(out[0], out[3] if return_alpha else None, out[2], w, parts).backward()
    return out, lv, Tf


def _oracle(cam, sc, form, aa, bg, parts):
    w = T.weights(H, W)
    lo = T.make_leaves(sc, form)
    co, ao, do, aux = T.render_oracle(cam, lo, form, bg, aa)
    T.loss_of(co, ao, do, w, parts).backward()
    return (co, ao, do), lo, aux


@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_gpu_alpha_image_20k(which):
    """alpha against 1 - final_T of the oracle; color and invdepth the same bits as the plain call; alpha = 1 - final_T of the kept state bit for bit;
    an alpha-only loss against the composed oracle."""
    pkg = _pkg()
    cam, sc = _scene(which)
    bg = torch.tensor(T.BG, device="cuda")
    (color, radii, invd, alpha), lv, Tf = _run(pkg, cam, sc, "fused", False, bg, "a")
    (color3, radii3, invd3), _, _ = _run(pkg, cam, sc, "fused", False, bg, "cd", return_alpha=False)
    assert torch.equal(color, color3) and torch.equal(invd, invd3) and torch.equal(radii, radii3)
    assert torch.equal(alpha[0], 1.0 - Tf)
    (co, ao, do), lo, aux = _oracle(cam, sc, "fused", False, torch.tensor(T.BG), "a")
    T.image_bars(alpha, 1.0 - aux["final_T"][None], f"gpu alpha ({which})")
    T.image_bars(color, co, f"gpu color ({which})")
    empty = aux["n_contrib"] == 0
    print(f"[composite] {which}: mean alpha {float(alpha.detach().mean()):.3f}, empty pixels {float(empty.float().mean()):.3f}")
    if which == "sparse":
        assert float(empty.float().mean()) > 0.05
    assert float(alpha.detach()[0].cpu()[empty].abs().max() if bool(empty.any()) else 0.0) == 0.0
    T.grad_bars({k: v.grad for k, v in lv.items()}, {k: v.grad for k, v in lo.items()}, f"gpu alpha only ({which})")


@pytest.mark.parametrize("form,aa", [("fused", False), ("fused", True), ("split", False), ("split", True), ("precomp", False), ("precomp", True)])
def test_gpu_gradients_match_the_composed_oracle_20k(form, aa):
    """A loss on (color, alpha, invdepth) over a constant background that requires grad; the colour-only loss with return_alpha=True gives the plain
    call's gradients bit for bit."""
    pkg = _pkg()
    cam, sc = _scene("dense")
    bgp = torch.tensor(T.BG, device="cuda", requires_grad=True)
    (color, radii, invd, alpha), lv, Tf = _run(pkg, cam, sc, form, aa, bgp, "cad")
    bgo = torch.tensor(T.BG, requires_grad=True)
    (co, ao, do), lo, aux = _oracle(cam, sc, form, aa, bgo, "cad")
    assert int((radii > 0).sum()) > 10_000
    T.image_bars(color, co, "gpu color"), T.image_bars(alpha, ao, "gpu alpha")
    T.grad_bars({k: v.grad for k, v in lv.items()}, {k: v.grad for k, v in lo.items()}, f"gpu {form} aa={aa}")
    T.bg_sum_bound(Tf, T.weights(H, W)[0], bgp.grad)
    T.grad_bars({"bg": bgp.grad}, {"bg": bgo.grad}, "gpu dL/dbg")
    bg = torch.tensor(T.BG, device="cuda")
    _, l1, _ = _run(pkg, cam, sc, form, aa, bg, "cd")
    _, l0, _ = _run(pkg, cam, sc, form, aa, bg, "cd", return_alpha=False)
    for k in l0:
        assert torch.equal(l0[k].grad, l1[k].grad), k


@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_gpu_per_pixel_background_20k(which):
    pkg = _pkg()
    cam, sc = _scene(which)
    B = T._bg_image(H, W)
    w = T.weights(H, W)
    bgp = B.clone().cuda().requires_grad_(True)
    (color, radii, invd, alpha), lv, Tf = _run(pkg, cam, sc, "fused", False, bgp, "cad")
    with torch.no_grad():
        (c0, _, _), _ = T.render_pkg(pkg, cam, T.make_leaves(sc, "fused", "cuda", grad=False), "fused", torch.zeros(3, device="cuda"), return_alpha=False,
                                     device="cuda")
    T.image_bars(color, (c0 + Tf[None] * B.cuda()).cpu(), "gpu color over bg_image vs color(bg=0) + T bg_image")
    assert torch.equal(bgp.grad, Tf[None] * w[0].cuda())      # the fp32 product, bit for bit
    bgo = B.clone().requires_grad_(True)
    (co, ao, do), lo, aux = _oracle(cam, sc, "fused", False, bgo, "cad")
    T.image_bars(color, co, "gpu color over bg_image vs the composed oracle")
    empty = aux["n_contrib"] == 0
    if which == "sparse":
        assert float(empty.float().mean()) > 0.05 and torch.equal(bgp.grad.cpu()[:, empty], w[0][:, empty])
    T.grad_bars({k: v.grad for k, v in lv.items()}, {k: v.grad for k, v in lo.items()}, f"gpu bg_image ({which})")
    T.grad_bars({"bg": bgp.grad}, {"bg": bgo.grad}, f"gpu dL/dbg_image ({which})")


def test_gpu_bit_reproducible_at_the_bench_frame():
    """1 M Gaussians at 1920 x 1080: two runs give the same bits for alpha, every gradient, dL/dbg and dL/dbg_image; alpha is 1 - final_T of the kept
    state bit for bit; dL/dbg is inside its bound."""
    pkg = _pkg()
    Wb, Hb = 1920, 1080
    sc = CG.prep(CG.scene(1_000_000, 23), "precomp")
    fovx = 1.0
    fovy = 2 * math.atan(math.tan(fovx / 2) * Hb / Wb)
    vm, pm, cp = [t.float().cuda() for t in CG.camera_from_pose(torch.tensor(CG.POSE0, dtype=torch.float64), fovx, fovy)]
    w = T.weights(Hb, Wb, "cuda")
    for image in (False, True):
        runs = []
        for _ in range(2):
            bg = (T._bg_image(Hb, Wb) if image else torch.tensor(T.BG)).cuda().requires_grad_(True)
            lv = {k: v.cuda().requires_grad_(True) for k, v in sc.items()}
            S = pkg.GaussianRasterizationSettings(Hb, Wb, math.tan(fovx / 2), math.tan(fovy / 2), bg, 1.0, vm, pm, 0, cp, False, False, False)
            color, radii, invd, alpha = pkg.GaussianRasterizer(S, return_alpha=True)(means3D=lv["means"], means2D=None, opacities=lv["opac"],
                                                                                     colors_precomp=lv["colors"], cov3D_precomp=lv["cov"])
            Tf = T.final_T_of(pkg, color, 1_000_000, Hb, Wb)
            T.loss_of(color, alpha, invd, w).backward()
            runs.append((alpha.detach(), bg.grad, {k: v.grad for k, v in lv.items()}, Tf))
        assert int((radii > 0).sum()) > 500_000
        (a1, g1, l1, T1), (a2, g2, l2, T2) = runs
        assert torch.equal(a1, a2) and torch.equal(g1, g2) and torch.equal(a1[0], 1.0 - T1)
        for k in l1:
            assert torch.equal(l1[k], l2[k]), k
        if image:
            assert torch.equal(g1, T1[None] * w[0])
        else:
            T.bg_sum_bound(T1, w[0], g1)
        print(f"[composite] bench frame (bg image: {image}): mean alpha {float(a1.mean()):.3f}")


def test_gpu_pose_fitting_on_a_silhouette():
    """Frozen Gaussians, a perturbed pose (about 3 degrees, 5 % of the scene's depth), Adam on abs(alpha - alpha_target) alone: the loss and the pose
    error must both end lower than they started.  The ratios are printed (DESIGN.md records them): results, not bars."""
    pkg = _pkg()
    sc = {k: v.cuda() for k, v in CG.prep(CG.scene(20_000, 24), "precomp").items()}
    Hs = Ws = 128
    fovx = fovy = 1.0

    def silhouette(pose):
        vm, pm, cp = CG.camera_from_pose(pose.cpu(), fovx, fovy)
        S = pkg.GaussianRasterizationSettings(Hs, Ws, math.tan(fovx / 2), math.tan(fovy / 2), torch.zeros(3, device="cuda"), 1.0, vm.float().cuda(),
                                              pm.float().cuda(), 0, cp.float().cuda(), False, False, False)
        return pkg.GaussianRasterizer(S, return_alpha=True)(means3D=sc["means"], means2D=None, opacities=sc["opac"], colors_precomp=sc["colors"],
                                                            cov3D_precomp=sc["cov"])[3]

    true = torch.tensor(CG.POSE0, dtype=torch.float64)
    with torch.no_grad():
        target = silhouette(true)
    start = true + torch.tensor([0.04, -0.03, 0.02, 0.15, -0.1, 0.2], dtype=torch.float64)
    pose = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([pose], lr=3e-3)
    losses = []
    for _ in range(150):
        opt.zero_grad()
        loss = (silhouette(pose) - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        last = float((silhouette(pose.detach()) - target).abs().mean())
    e0, e1 = float((start - true).norm()), float((pose.detach() - true).norm())
    print(f"[composite] silhouette fit: loss {losses[0]:.5f} -> {last:.5f} (ratio {last / losses[0]:.3f}), pose error {e0:.4f} -> {e1:.4f} "
          f"(ratio {e1 / e0:.3f})")
    assert last < losses[0] and e1 < e0, (losses[0], last, e0, e1)
