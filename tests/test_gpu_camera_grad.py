"""Camera gradients on the MI355X (gsr_backward_preprocess_camera): the affine identity of tests/test_camera_grad_cpu.py on the operator's own
outputs, at 20 K Gaussians / 256 x 256 for every input form and at the bench frame's size (1 M Gaussians, 1920 x 1080); bit-reproducibility;
Gaussian gradients bit-identical with and without the camera gradient; pose recovery with frozen Gaussians."""
import math

import pytest
import torch

import test_camera_grad_cpu as T

pytestmark = pytest.mark.gpu


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


@pytest.mark.parametrize("form,aa,depth_loss", T.CASES + [("fused", True, True), ("split", False, True)])
def test_gpu_camera_gradient_identity_20k(form, aa, depth_loss):
    sc = T.prep(T.scene(20_000, 21), form)
    pkg = _pkg()
    runs = []
    for cam_grad in (True, True, False):
        cam, leaves, loss, radii = T.render(pkg, sc, W=256, H=256, form=form, aa=aa, depth_loss=depth_loss, device="cuda", cam_grad=cam_grad)
        loss.backward()
        runs.append((cam, leaves))
    assert int((radii > 0).sum()) > 10_000
    (c1, l1), (c2, l2), (_, l3) = runs
    if form in ("precomp", "sh_cov"):
        T.identity_check(c1, l1, form)
    for k in l1:
        assert torch.equal(l1[k].grad, l3[k].grad) and torch.equal(l1[k].grad, l2[k].grad), k
    for a, b in zip(c1, c2):
        assert a.grad is not None and torch.equal(a.grad, b.grad)


def test_gpu_camera_only_fitting_20k():
    sc = T.prep(T.scene(20_000, 22), "precomp")
    pkg = _pkg()
    cam, _, loss, _ = T.render(pkg, sc, W=256, H=256, device="cuda", gauss_grad=False)
    loss.backward()
    cam2, _, loss2, _ = T.render(pkg, sc, W=256, H=256, device="cuda")
    loss2.backward()
    for a, b in zip(cam, cam2):
        assert a.grad is not None and torch.equal(a.grad, b.grad)


def test_gpu_camera_gradient_identity_at_the_bench_frame():
    """1 M Gaussians at 1920 x 1080 with colors_precomp + cov3D_precomp: the identity in fp64 on the operator's outputs, twice, same bits."""
    sc = T.prep(T.scene(1_000_000, 23), "precomp")
    pkg = _pkg()
    grads = []
    for _ in range(2):
        cam, leaves, loss, radii = T.render(pkg, sc, W=1920, H=1080, device="cuda")
        loss.backward()
        grads.append([t.grad.clone() for t in cam])
    assert int((radii > 0).sum()) > 500_000
    err = T.identity_check(cam, leaves, "precomp")
    print(f"bench-frame identity: max error {err:.2e} of the absolute sum")
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_gpu_pose_recovery_with_frozen_gaussians():
    """Render a target from a pose, perturb the pose (about 3 degrees, 5 % of the scene's depth), freeze the Gaussians and fit the pose with
    Adam through the operator: the pose error must drop at least 5-fold (a factor fixed before the first GPU run)."""
    pkg = _pkg()
    sc = {k: v.cuda() for k, v in T.prep(T.scene(20_000, 24), "precomp").items()}
    H, W, fovx = 128, 128, 1.0
    fovy = fovx

    def image(pose):
        vm, pm, cp = T.camera_from_pose(pose.cpu(), fovx, fovy)
        S = pkg.GaussianRasterizationSettings(H, W, math.tan(fovx / 2), math.tan(fovy / 2), torch.zeros(3, device="cuda"), 1.0, vm.float().cuda(),
                                              pm.float().cuda(), 0, cp.float().cuda(), False, False, False)
        return pkg.GaussianRasterizer(S)(means3D=sc["means"], means2D=None, opacities=sc["opac"], colors_precomp=sc["colors"],
                                         cov3D_precomp=sc["cov"])[0]

    true = torch.tensor(T.POSE0, dtype=torch.float64)
    with torch.no_grad():
        target = image(true)
    start = true + torch.tensor([0.04, -0.03, 0.02, 0.15, -0.1, 0.2], dtype=torch.float64)
    pose = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([pose], lr=3e-3)
    for _ in range(150):
        opt.zero_grad()
        loss = (image(pose) - target).abs().mean()
        loss.backward()
        opt.step()
    e0 = float((start - true).norm())
    e1 = float((pose.detach() - true).norm())
    print(f"pose error {e0:.4f} -> {e1:.4f}")
    assert e1 * 5 < e0, (e0, e1)
