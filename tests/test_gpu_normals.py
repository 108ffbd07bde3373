"""The normal-consistency regulariser on the MI355X: the gsr_normals package on the device against tests/normals_reference.py (fp64 on the CPU)
with the bars of tests/test_normals_cpu.py, which runs the same kernel source on the host -- the same small shapes plus one 270 x 480 frame,
run-to-run bits, a non-default stream, the non-finite contract, and the recipe end to end on one rasterizer call against the same chain with
the three new calls written in fp32 torch."""
import math

import pytest
import torch

import normals_reference as NR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IMAGE_SHAPES = [(1, 1), (2, 5), (3, 3), (5, 9), (37, 53), (70, 150), (270, 480)]
TX, TY = NR.TANFOV


def bits(t):
    return t.view(torch.int32)


def run_map(depth, dL):
    """depth_to_normal on the device -> Nd, dL/ddepth on the host."""
    import gsr_normals as GN
    z = depth.to(DEV).requires_grad_(True)
    nd = GN.depth_to_normal(z, TX, TY)
    nd.backward(dL.to(DEV))
    return nd.detach().cpu(), z.grad.cpu()


def run_loss(depth, normals, weight, want="nd"):
    """normal_consistency_loss on the device, 1.75 loss backpropagated -> loss, dL/dnormals, dL/ddepth on the host (None where not in `want`)."""
    import gsr_normals as GN
    z, n = depth.to(DEV).requires_grad_("d" in want), normals.to(DEV).requires_grad_("n" in want)
    loss = GN.normal_consistency_loss(z, n, TX, TY, None if weight is None else weight.to(DEV))
    if want:
        (1.75 * loss).backward()
    return loss.detach().cpu(), (n.grad.cpu() if "n" in want else None), (z.grad.cpu() if "d" in want else None)


def compare_image(what, nd, dmap, loss, gn, gz, H, W, seed, weighted):
    r_nd, r_dmap, r_loss, r_gz, r_gn = NR.image_reference(H, W, seed, weighted)
    NR.check(what, {"Nd": (NR.rel_max(nd, r_nd), "depth_normals"), "ddepth(map)": (NR.rel_max(dmap, r_dmap), "depth_grad"),
                    "loss": (abs(float(loss) - r_loss) / r_loss, "loss"), "ddepth(loss)": (NR.rel_max(gz, r_gz), "depth_grad"),
                    "dnormals": (NR.rel_max(gn, r_gn), "normal_grad")})


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", IMAGE_SHAPES)
def test_image_kernels_on_the_device_are_the_reference(shape, weighted):
    H, W = shape
    seed = H + W
    depth, normals, weight, dL = NR.image_case(H, W, seed, weighted)
    nd, dmap = run_map(depth, dL)
    loss, gn, gz = run_loss(depth, normals, weight)
    compare_image(f"gpu {shape} weight {weighted}", nd, dmap, loss, gn, gz, H, W, seed, weighted)
    if H < 3 or W < 3:
        assert float(loss) == 1.0 and float(nd.abs().max()) == 0.0 and float(gn.abs().max()) == 0.0 and float(gz.abs().max()) == 0.0
    # a second run: the same bits of every output; one gradient alone: the same bits of that gradient
    nd2, dmap2 = run_map(depth, dL)
    loss2, gn2, gz2 = run_loss(depth, normals, weight)
    assert torch.equal(bits(nd2), bits(nd)) and torch.equal(bits(dmap2), bits(dmap)) and torch.equal(bits(loss2), bits(loss))
    assert torch.equal(bits(gn2), bits(gn)) and torch.equal(bits(gz2), bits(gz))
    _, gn3, none = run_loss(depth, normals, weight, want="n")
    assert none is None and torch.equal(bits(gn3), bits(gn))
    _, none, gz3 = run_loss(depth, normals, weight, want="d")
    assert none is None and torch.equal(bits(gz3), bits(gz))


def run_gaussians(s, q, m, vm, dL):
    import gsr_normals as GN
    qd = q.to(DEV).requires_grad_(True)
    n = GN.gaussian_normals(s.to(DEV), qd, m.to(DEV), vm.to(DEV))
    n.backward(dL.to(DEV))
    return n.detach().cpu(), qd.grad.cpu()


def test_gaussian_kernels_on_the_device_are_the_reference():
    P = 5000
    s, q, m, vm, dL = NR.make_gaussians(P)
    n, drot = run_gaussians(s, q, m, vm, dL)
    r_n, r_dq, compared = NR.gaussian_reference(P)
    assert int((~compared).sum()) <= NR.SIGN_EXEMPT_MAX * P
    NR.check(f"gpu P {P}", {"n": (float((n.double() - r_n)[compared].abs().max()), "gaussian_normals"),
                            "drot": (float((drot.double() - r_dq)[compared].abs().max() / r_dq.abs().max()), "rotation_grad")})
    assert float(n[6:15].abs().max()) == 0.0 and float(drot[6:15].abs().max()) == 0.0      # the rows with NaN / inf in an input
    n2, drot2 = run_gaussians(s, q, m, vm, dL)
    assert torch.equal(bits(n2), bits(n)) and torch.equal(bits(drot2), bits(drot))
    import gsr_normals as GN
    assert GN.gaussian_normals(s[:0].to(DEV), q[:0].to(DEV), m[:0].to(DEV), vm.to(DEV)).shape == (0, 3)


def test_side_stream_and_an_image_base_off_16_byte_alignment():
    import gsr_normals as GN
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    want_nd, want_dmap = run_map(depth, dL)
    want_loss, want_gn, want_gz = run_loss(depth, normals, weight)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        def shifted(t):      # a copy whose base sits 4 bytes past a 16-byte boundary
            buf = torch.empty(t.numel() + 4, device=DEV)
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t.to(DEV))
            assert v.data_ptr() % 16 == 4
            return v
        z = shifted(depth).requires_grad_(True)
        nd = GN.depth_to_normal(z, TX, TY)
        nd.backward(shifted(dL))
        z2, n2 = shifted(depth).requires_grad_(True), shifted(normals).requires_grad_(True)
        loss = GN.normal_consistency_loss(z2, n2, TX, TY, shifted(weight))
        (1.75 * loss).backward()
    stream.synchronize()
    assert torch.equal(bits(nd.detach().cpu()), bits(want_nd)) and torch.equal(bits(z.grad.cpu()), bits(want_dmap))
    assert torch.equal(bits(loss.detach().cpu()), bits(want_loss))
    assert torch.equal(bits(n2.grad.cpu()), bits(want_gn)) and torch.equal(bits(z2.grad.cpu()), bits(want_gz))


@pytest.mark.parametrize("poison", [math.nan, math.inf, 0.0, -1.0])
def test_poisoned_depths_on_the_device(poison):
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    nd, dmap = run_map(depth, dL)
    loss, gn, gz = run_loss(depth, normals, weight)
    spots = [(0, 0), (0, 20), (17, 29), (H - 1, W - 2), (16, 51)]
    bad = depth.clone()
    for y, x in spots:
        bad[y, x] = poison
    nd_b, dmap_b = run_map(bad, dL)
    loss_b, gn_b, gz_b = run_loss(bad, normals, weight)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    dist = torch.stack([(yy - y).abs() + (xx - x).abs() for y, x in spots]).amin(0)
    near1, near2 = dist <= 1, dist <= 2
    assert torch.equal(bits(nd_b)[:, ~near1], bits(nd)[:, ~near1]) and float(nd_b[:, near1].abs().max()) == 0.0
    assert torch.equal(bits(gn_b)[:, ~near1], bits(gn)[:, ~near1]) and float(gn_b[:, near1].abs().max()) == 0.0
    assert torch.equal(bits(dmap_b)[~near2], bits(dmap)[~near2]) and torch.equal(bits(gz_b)[~near2], bits(gz)[~near2])
    for t in (nd_b, dmap_b, gn_b, gz_b, loss_b):
        assert bool(torch.isfinite(t).all())


def test_nan_normals_where_nothing_is_compared_on_the_device():
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    depth = depth.clone()
    depth[20, 30] = math.nan
    nd, _ = run_map(depth, dL)
    off = (nd == 0).all(0) | (weight == 0)
    zeros, nans = normals.clone(), normals.clone()
    zeros[:, off] = 0.0
    nans[:, off] = math.nan
    a, b = run_loss(depth, zeros, weight), run_loss(depth, nans, weight)
    for x, y in zip(a, b):
        assert bool(torch.isfinite(y).all()) and torch.equal(bits(x), bits(y))
    assert float(b[1][:, off].abs().max()) == 0.0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------
def e2e_scene(P=300, seed=11):
    """About 300 flat Gaussians around the plane z = 5 + 0.3 x in front of helpers.make_camera(64, 48): the flat axis is the plane's normal,
    tilted by a few degrees per Gaussian."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(P, generator=g) * 2 - 1) * 3.0
    y = (torch.rand(P, generator=g) * 2 - 1) * 2.3
    means = torch.stack([x, y, 5.0 + 0.3 * x + 0.02 * torch.randn(P, generator=g)], dim=1)
    scales = torch.stack([0.25 * torch.exp(0.2 * torch.randn(P, generator=g)), 0.22 * torch.exp(0.2 * torch.randn(P, generator=g)),
                          0.02 * torch.exp(0.2 * torch.randn(P, generator=g))], dim=1)
    ang = math.atan(0.3)      # rotate z towards -x by the plane's slope, about the y axis, then perturb
    q = torch.tensor([math.cos(-ang / 2), 0.0, math.sin(-ang / 2), 0.0]).expand(P, 4) + 0.05 * torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    opac = 0.5 + 0.45 * torch.rand(P, 1, generator=g)
    colors = torch.rand(P, 3, generator=g)
    return means.contiguous(), scales.contiguous(), q.contiguous(), opac.contiguous(), colors.contiguous()


def e2e_chain(kernels: bool):
    """The recipe of the gsr_normals docstring on one rasterizer call -> loss, the four parameter gradients.  kernels = False: the three new
    calls are the reference's expressions in fp32 torch on the device; everything else is the same code."""
    import diff_gaussian_rasterization as pkg
    import gsr_normals as GN
    import test_composite_cpu as T
    from helpers import make_camera
    cam = make_camera(64, 48)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device=DEV), False, DEV)
    means, scales, q, opac, colors = (t.to(DEV) for t in e2e_scene())
    leaves = [t.clone().requires_grad_(True) for t in (means, scales, q, opac)]
    xyz, s, rot, o = leaves
    color, radii, invd, alpha = pkg.GaussianRasterizer(S, return_alpha=True)(means3D=xyz, means2D=None, opacities=o, colors_precomp=colors,
                                                                               scales=s, rotations=rot)
    vm = S.viewmatrix
    n = GN.gaussian_normals(s, rot, xyz, vm) if kernels else NR.gaussian_normals(s, rot, xyz, vm)
    z = xyz @ vm[:3, 2] + vm[3, 2]
    F = pkg.render_features(color, torch.cat([n, z[:, None]], dim=1), geometry=True)
    depth = F[3] / alpha[0].clamp_min(1e-6)
    w = alpha[0].detach()
    if kernels:
        loss = GN.normal_consistency_loss(depth, F[:3], S.tanfovx, S.tanfovy, weight=w)
    else:
        loss = NR.normal_consistency_loss(depth, F[:3], S.tanfovx, S.tanfovy, weight=w)
    loss.backward()
    return float(loss.detach()), [t.grad.detach().cpu() for t in leaves], float((alpha[0] > 0.5).float().mean())


def test_recipe_end_to_end_moves_every_parameter():
    loss_k, grads_k, covered = e2e_chain(True)
    loss_t, grads_t, _ = e2e_chain(False)
    print(f"[normals] gpu end to end: loss {loss_k:.6f} (torch chain {loss_t:.6f}), {covered * 100:.0f} % of the pixels with alpha > 0.5", flush=True)
    assert covered >= 0.5 and 0.0 < loss_k < 1.0
    assert abs(loss_k - loss_t) <= 1e-5 * abs(loss_t)
    for name, a, b in zip(("means3D", "scales", "rotations", "opacities"), grads_k, grads_t):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"[normals] gpu end to end: dL/d{name} differs by {err:.2e} of its maximum {float(b.abs().max()):.3e} (bar 1e-05)", flush=True)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0, name
        assert err <= 1e-5, (name, err)
