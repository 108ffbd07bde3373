"""Camera gradients (gsr_backward_preprocess_camera, include/gsr.h) through the shipped package on the CPU: the SIMT build of the whole library
(tests/simt_build.py) behind the package's own loader, as in tests/test_simt_package_cpu.py.

The reference's camera is built from a pose with its own formulas (scene/cameras.py: world_view_transform, full_proj_transform =
world_view_transform @ projection_matrix, camera_center = world_view_transform.inverse()[3, :3]).  The bars check the camera gradient against the
Gaussian gradients the operator returns, which the rest of the suite holds against the oracle:

  moving the world by an affine map A~ = [[A, a], [0, 1]] (means m -> A m + a, covariances S -> A S A^T) is the same as V -> V A~ and P -> P A~,
  so  V^T dL/dV + P^T dL/dP  (math matrices, rows 0-2)  =  sum_i dL/dm_i (m_i, 1)^T  +  sum_i 2 G_i S_i  (3 x 3 block),
  G_i = dL/dS_i as a symmetric matrix.  With SH colours the translation column also carries the view direction: the translation column equals
  sum_i dL/dm_i + dL/dcampos.

Test infrastructure: the product never loads the SIMT library."""
import math
import os
import subprocess
import sys

import pytest
import torch

from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference's camera formulas (utils/graphics_utils.py getWorld2View2 / getProjectionMatrix, scene/cameras.py:80-89) ----
def rodrigues(w):
    th = torch.sqrt((w * w).sum() + 1e-30)
    k = w / th
    K = torch.zeros(3, 3, dtype=w.dtype)
    K = K + torch.stack([torch.stack([0 * th, -k[2], k[1]]), torch.stack([k[2], 0 * th, -k[0]]), torch.stack([-k[1], k[0], 0 * th])])
    return torch.eye(3, dtype=w.dtype) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


def projection_matrix(znear, zfar, fovx, fovy, dtype=torch.float32):
    tanx, tany = math.tan(fovx / 2), math.tan(fovy / 2)
    top, right = tany * znear, tanx * znear
    P = torch.zeros(4, 4, dtype=dtype)
    P[0, 0] = 2.0 * znear / (2 * right)
    P[1, 1] = 2.0 * znear / (2 * top)
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def camera_from_pose(pose, fovx, fovy):
    """pose = (rotation vector, translation) of world -> view; returns the three tensors the reference passes, differentiable in pose."""
    R = rodrigues(pose[:3])
    Rt = torch.cat([torch.cat([R, pose[3:6, None]], 1), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=pose.dtype)], 0)
    world_view = Rt.transpose(0, 1)
    full_proj = world_view @ projection_matrix(0.01, 100.0, fovx, fovy, pose.dtype).transpose(0, 1)
    campos = world_view.inverse()[3, :3]
    return world_view, full_proj, campos


def scene(P, seed, depth=4.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    means = torch.cat([(r(P, 2) - 0.5) * 2.4, depth + (r(P, 1) - 0.5) * 2.0], 1)
    scales = 0.03 + 0.12 * r(P, 3)
    q = torch.randn(P, 4, generator=g)
    rot = q / q.norm(dim=1, keepdim=True)
    opac = 0.3 + 0.6 * r(P, 1)
    shs = torch.randn(P, 16, 3, generator=g) * 0.3
    colors = r(P, 3)
    return dict(means=means, scales=scales, rot=rot, opac=opac, shs=shs, colors=colors)


def cov3d(scales, rot):
    r, x, y, z = rot.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    Mx = R * scales[:, None, :]
    S = Mx @ Mx.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()


POSE0 = [0.02, -0.03, 0.01, 0.05, -0.04, 0.1]


def render(pkg, sc, W=96, H=64, form="precomp", aa=False, depth_loss=True, pose=None, cam_grad=True, gauss_grad=True, deg=3, device="cpu",
           wts=None):
    """One frame + a fixed loss; returns (pose-or-camera leaves, Gaussian leaves, loss)."""
    fovx = 1.0
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    if pose is None:
        pose = torch.tensor(POSE0, dtype=torch.float64)
    vm, pm, cp = camera_from_pose(pose, fovx, fovy)
    vm, pm, cp = [t.float().detach().to(device) for t in (vm, pm, cp)]
    cam = [t.clone().requires_grad_(cam_grad) for t in (vm, pm, cp)]
    leaves = {k: v.to(device).clone().requires_grad_(gauss_grad) for k, v in sc.items()}
    S = pkg.GaussianRasterizationSettings(H, W, math.tan(fovx / 2), math.tan(fovy / 2), torch.zeros(3, device=device), 1.0, cam[0], cam[1],
                                          deg, cam[2], False, False, aa)
    rast = pkg.GaussianRasterizer(S)
    kw = dict(means3D=leaves["means"], means2D=None, opacities=leaves["opac"])
    if form in ("precomp", "sh_cov"):
        kw["cov3D_precomp"] = leaves["cov"] if "cov" in leaves else None
    if form == "precomp":
        kw["colors_precomp"] = leaves["colors"]
    elif form == "sh_cov":
        kw["shs"] = leaves["shs"]
    elif form == "split":
        kw.update(dc=leaves["shs"][:, :1].contiguous(), shs=leaves["shs"][:, 1:].contiguous(), scales=leaves["scales"], rotations=leaves["rot"])
    else:      # fused SH with scales / rotations
        kw.update(shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rot"])
    color, radii, invd = rast(**kw)
    g = torch.Generator().manual_seed(7)
    w1 = torch.rand(color.shape, generator=g).to(device) if wts is None else wts[0]
    loss = (color * w1).sum()
    if depth_loss:
        w2 = torch.rand(invd.shape, generator=g).to(device) if wts is None else wts[1]
        loss = loss + (invd * w2).sum()
    return cam, leaves, loss, radii


def prep(sc, form):
    sc = dict(sc)
    if form in ("precomp", "sh_cov"):
        sc["cov"] = cov3d(sc["scales"], sc["rot"])
        for k in ("scales", "rot"):
            sc.pop(k)
    if form != "precomp":
        sc.pop("colors")
    if form == "precomp":
        sc.pop("shs")
    return sc


def identity_check(cam, leaves, form, bar=1e-5):
    """The affine identity of the module docstring, in fp64 from the operator's own fp32 gradients."""
    vm, pm, cp = cam
    gV = vm.grad.double().cpu()
    gP = pm.grad.double().cpu()
    lhs = vm.detach().double().cpu() @ gV.t() + pm.detach().double().cpu() @ gP.t()      # V^T dL/dV + P^T dL/dP, math layout
    m = leaves["means"].detach().double().cpu()
    dm = leaves["means"].grad.double().cpu()
    ph = torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64)], 1)
    terms = dm[:, :, None] * ph[:, None, :]                                              # [P, 3, 4]
    if "cov" in leaves:
        c = leaves["cov"].detach().double().cpu()
        gc = leaves["cov"].grad.double().cpu()
        Sg = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).view(-1, 3, 3)
        G = torch.stack([gc[:, 0], gc[:, 1] / 2, gc[:, 2] / 2, gc[:, 1] / 2, gc[:, 3], gc[:, 4] / 2, gc[:, 2] / 2, gc[:, 4] / 2, gc[:, 5]], 1).view(-1, 3, 3)
        terms[:, :, :3] += 2 * (G @ Sg)
    rhs = terms.sum(0)
    scale = terms.abs().sum(0)
    if form == "precomp":
        err = (lhs[:3] - rhs).abs() / scale.clamp_min(1e-30)
        assert float(cp.grad.abs().max()) == 0.0, "colors_precomp: dL/dcampos must be exactly zero"
    else:      # view-direction term: only the translation column is an identity here
        rhs_t = rhs[:, 3] + cp.grad.double().cpu()
        err = (lhs[:3, 3] - rhs_t).abs() / scale[:, 3].clamp_min(1e-30)
    # structural zeros: view row 3 and projection row 2 (tensor layout: column 3 / column 2)
    assert torch.equal(vm.grad[:, 3], torch.zeros_like(vm.grad[:, 3])) and torch.equal(pm.grad[:, 2], torch.zeros_like(pm.grad[:, 2]))
    assert float(err.max()) <= bar, (float(err.max()), err)
    return float(err.max())


CASES = [("precomp", False, True), ("precomp", True, False), ("sh_cov", False, True), ("sh_cov", True, True)]


@pytest.mark.parametrize("form,aa,depth_loss", CASES)
def test_camera_gradient_matches_the_gaussian_gradients(simt_lib, form, aa, depth_loss):  # noqa: F811
    sc = prep(scene(300, 11), form)
    with package_on_the_cpu(simt_lib) as pkg:
        cam, leaves, loss, radii = render(pkg, sc, form=form, aa=aa, depth_loss=depth_loss)
        loss.backward()
    assert int((radii > 0).sum()) > 100
    assert all(t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype for t in cam)
    assert float(cam[0].grad.abs().max()) > 0 and float(cam[1].grad.abs().max()) > 0
    identity_check(cam, leaves, form)


@pytest.mark.parametrize("form", ["fused", "split"])
def test_camera_gradient_is_the_same_bits_for_every_sh_form_and_leaves_the_gaussian_gradients_alone(simt_lib, form):  # noqa: F811
    """fused [P,16,3] SH and the split dc / rest form give the same camera gradient; every Gaussian gradient is bit-identical with and without
    the camera gradient requested; two runs give the same camera bits."""
    sc = prep(scene(300, 12), form)
    with package_on_the_cpu(simt_lib) as pkg:
        runs = []
        for cam_grad in (True, True, False):
            cam, leaves, loss, _ = render(pkg, sc, form=form, cam_grad=cam_grad)
            loss.backward()
            runs.append((cam, leaves))
    (c1, l1), (c2, l2), (c3, l3) = runs
    for k in l1:
        assert torch.equal(l1[k].grad, l3[k].grad), k
        assert torch.equal(l1[k].grad, l2[k].grad), k
    for a, b in zip(c1, c2):
        assert torch.equal(a.grad, b.grad)
    assert all(t.grad is None for t in c3)
    assert float(c1[2].grad.abs().max()) > 0      # the SH view-direction term reaches campos


def test_fused_and_split_sh_agree(simt_lib):  # noqa: F811
    sc = prep(scene(300, 13), "fused")
    out = {}
    with package_on_the_cpu(simt_lib) as pkg:
        for form in ("fused", "split"):
            cam, leaves, loss, _ = render(pkg, sc, form=form)
            loss.backward()
            out[form] = [t.grad for t in cam]
    for a, b in zip(out["fused"], out["split"]):
        assert torch.equal(a, b)


def test_camera_only_fitting_with_frozen_gaussians(simt_lib):  # noqa: F811
    """No Gaussian input requires grad: the forward still keeps its backward state and the camera gradients arrive -- the same bits as
    when the Gaussians require grad too."""
    sc = prep(scene(300, 14), "precomp")
    with package_on_the_cpu(simt_lib) as pkg:
        cam, leaves, loss, _ = render(pkg, sc, gauss_grad=False)
        loss.backward()
        cam2, _, loss2, _ = render(pkg, sc, gauss_grad=True)
        loss2.backward()
    assert all(t.grad is not None for t in cam)
    for a, b in zip(cam, cam2):
        assert torch.equal(a.grad, b.grad)


def test_gradient_through_a_pose_matches_the_identity_route(simt_lib):  # noqa: F811
    """pose (6-vector) -> the reference's formulas -> GaussianRasterizer -> loss: the pose gradient autograd returns is the chain rule through
    the three camera gradients of a render with leaf camera tensors (which the identity test pins) -- no layout convention in between."""
    sc = prep(scene(300, 15), "sh_cov")
    H, W, fovx = 64, 96, 1.0
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    pose = torch.tensor(POSE0, dtype=torch.float64, requires_grad=True)
    with package_on_the_cpu(simt_lib) as pkg:
        vm, pm, cp = camera_from_pose(pose, fovx, fovy)
        S = pkg.GaussianRasterizationSettings(H, W, math.tan(fovx / 2), math.tan(fovy / 2), torch.zeros(3), 1.0, vm.float(), pm.float(), 3,
                                              cp.float(), False, False, False)
        color, _, invd = pkg.GaussianRasterizer(S)(means3D=sc["means"], means2D=None, opacities=sc["opac"], shs=sc["shs"], cov3D_precomp=sc["cov"])
        g = torch.Generator().manual_seed(7)
        loss = (color * torch.rand(color.shape, generator=g)).sum() + (invd * torch.rand(invd.shape, generator=g)).sum()
        loss.backward()
        cam, _, loss2, _ = render(pkg, sc, form="sh_cov", gauss_grad=False)
        loss2.backward()
    vm, pm, cp = camera_from_pose(pose, fovx, fovy)
    want = torch.autograd.grad((vm, pm, cp), pose, tuple(t.grad.double() for t in cam))[0]
    assert float(pose.grad.abs().max()) > 0
    assert torch.allclose(pose.grad, want, rtol=1e-6, atol=1e-9 * float(want.abs().max())), (pose.grad, want)


def test_camera_grad_entry_point_is_not_called_without_camera_grad(simt_lib):  # noqa: F811
    from unittest import mock
    sc = prep(scene(200, 16), "precomp")
    with package_on_the_cpu(simt_lib) as pkg:
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        real = lib.gsr_backward_preprocess_camera
        calls = []
        with mock.patch.object(lib, "gsr_backward_preprocess_camera", lambda *a: (calls.append(1), real(*a))[1]):
            _, leaves, loss, _ = render(pkg, sc, cam_grad=False)
            loss.backward()
            assert calls == []
            cam, leaves, loss, _ = render(pkg, sc, cam_grad=True)
            loss.backward()
            assert calls == [1]


def test_fused_sh_adam_and_camera_grad_raise(simt_lib):  # noqa: F811
    sc = prep(scene(200, 17), "split")
    with package_on_the_cpu(simt_lib) as pkg:
        dc = torch.nn.Parameter(sc["shs"][:, :1].contiguous())
        rest = torch.nn.Parameter(sc["shs"][:, 1:].contiguous())
        opt = torch.optim.Adam([{"params": [dc], "lr": 1e-3}, {"params": [rest], "lr": 1e-3}], eps=1e-15)
        handle = pkg.fuse_sh_adam_into_backward(opt, dc, rest)
        try:
            fovx, H, W = 1.0, 64, 96
            fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
            vm, pm, cp = [t.float().detach().requires_grad_(True) for t in camera_from_pose(torch.tensor(POSE0, dtype=torch.float64), fovx, fovy)]
            S = pkg.GaussianRasterizationSettings(H, W, math.tan(fovx / 2), math.tan(fovy / 2), torch.zeros(3), 1.0, vm, pm, 3, cp, False, False, False)
            with pytest.raises(pkg.GsrError, match="camera gradients"):
                pkg.GaussianRasterizer(S)(means3D=sc["means"], means2D=None, opacities=sc["opac"], dc=dc, shs=rest, scales=sc["scales"],
                                          rotations=sc["rot"])
        finally:
            handle.remove()


def test_camera_gradient_is_independent_of_the_lane_schedule(simt_lib, tmp_path):  # noqa: F811
    """SIMT_SCHEDULE shuffles wave interleaving and workgroup order: the camera gradient is the same bits (no float atomics, fixed order)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, torch\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {os.path.join(ROOT, 'gaussian-splatting_amd')!r}]\n"
        "import test_camera_grad_cpu as T\n"
        "sc = T.prep(T.scene(300, 18), 'fused')\n"
        "with T.package_on_the_cpu(sys.argv[1]) as pkg:\n"
        "    cam, leaves, loss, _ = T.render(pkg, sc, form='fused', aa=True)\n"
        "    loss.backward()\n"
        "torch.save([t.grad for t in cam], sys.argv[2])\n")
    outs = []
    for k, sched in enumerate([None, "5", "11"]):
        env = dict(os.environ)
        env.pop("SIMT_SCHEDULE", None)
        if sched is not None:
            env["SIMT_SCHEDULE"] = sched
        out = tmp_path / f"g{k}.pt"
        subprocess.run([sys.executable, str(script), simt_lib, str(out)], check=True, env=env, cwd=ROOT, timeout=600)
        outs.append(torch.load(out))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def test_parallel_band_renderer_passes_the_camera_detached():
    from diff_gaussian_rasterization import parallel
    t = torch.eye(4, requires_grad=True)
    import diff_gaussian_rasterization as pkg
    rs = pkg.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, t, t * 2, 0, torch.zeros(3, requires_grad=True), False, False)
    d = parallel._camera_detached(rs)
    assert not d.viewmatrix.requires_grad and not d.projmatrix.requires_grad and not d.campos.requires_grad
    assert torch.equal(d.viewmatrix, rs.viewmatrix) and torch.equal(d.projmatrix, rs.projmatrix)


@pytest.mark.parametrize("M", [1, 4, 9])
def test_camera_gradient_for_smaller_sh_records(simt_lib, M):  # noqa: F811
    """Fused [P,M,3] SH records below degree 3 (the kernel's unstaged path): the translation identity holds, campos gets the SH term."""
    sc = prep(scene(300, 19), "sh_cov")
    sc["shs"] = sc["shs"][:, :M].contiguous()
    with package_on_the_cpu(simt_lib) as pkg:
        cam, leaves, loss, _ = render(pkg, sc, form="sh_cov", deg=int(round(math.sqrt(M))) - 1)
        loss.backward()
    identity_check(cam, leaves, "sh_cov")
    assert (float(cam[2].grad.abs().max()) > 0) == (M > 1)      # degree 0: the colour does not depend on the view direction


def test_camera_gradient_of_an_empty_scene_is_zero(simt_lib):  # noqa: F811
    sc = {k: v[:0] for k, v in prep(scene(10, 20), "precomp").items()}
    with package_on_the_cpu(simt_lib) as pkg:
        cam, _, loss, _ = render(pkg, sc)
        loss.backward()
    for t in cam:
        assert t.grad is not None and torch.equal(t.grad, torch.zeros_like(t))
