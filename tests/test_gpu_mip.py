"""The 3D smoothing filter of Mip-Splatting on the MI355X: gsr_scene.mip on the device against tests/mip_reference.py (fp64 on the CPU) with the
bars of tests/test_mip_cpu.py, which runs the same kernel source on the host -- the sweep off the fragile set, the activations forward and
backward, run-to-run bits, a non-default stream, and one antialiased rasterizer call fed by filtered_activations whose raw-parameter gradients
are held against the same chain with upstream's torch expressions in place of the kernel."""
import math

import pytest
import torch

import mip_reference as MR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def bits(t):
    return t.view(torch.int32)


def run_sweep(P, C):
    from gsr_scene import mip
    means, cams = MR.scene_reference(P, C)[:2]
    filt, seen = mip.compute_3d_filter(means.to(DEV), cams.to(DEV), return_seen=True)
    assert filt.shape == (P, 1) and seen.shape == (P,) and seen.dtype == torch.bool
    return filt.reshape(-1).cpu(), seen.cpu()


@pytest.mark.parametrize("P,C", [(1027, 2), (1027, 65), (100003, 33)])
def test_sweep_on_the_device_is_upstreams_loop(P, C):
    from gsr_scene import mip
    got, seen = run_sweep(P, C)
    MR.check_sweep("gpu", got, seen, P, C)
    got2, seen2 = run_sweep(P, C)      # a second run: the same bits (the maximum is an integer maximum)
    assert torch.equal(bits(got2), bits(got)) and torch.equal(seen2, seen)
    means, cams = MR.scene_reference(P, C)[:2]
    alone = mip.compute_3d_filter(means.to(DEV), cams.to(DEV))      # seen = NULL
    assert torch.equal(bits(alone.reshape(-1).cpu()), bits(got))


def run_activations(P, seed, want="so"):
    """filtered_activations on the device, both outputs (or one) backpropagated -> scales', opacity', dL/draw_scales, dL/draw_opacity on the host."""
    from gsr_scene import mip
    rs, ro, f, gs, go = (t.to(DEV) for t in MR.activation_case(P, seed))
    a, b = rs.clone().requires_grad_(True), ro.clone().requires_grad_(True)
    s, o = mip.filtered_activations(a, b, f)
    loss = 0.0
    if "s" in want:
        loss = loss + (s * gs).sum()
    if "o" in want:
        loss = loss + (o * go).sum()
    loss.backward()
    return s.detach().cpu(), o.detach().cpu(), a.grad.cpu(), b.grad.cpu()


@pytest.mark.parametrize("P", [1027, 100003])
def test_activations_on_the_device_are_upstreams_expression(P):
    seed = 40 + P
    got = run_activations(P, seed)
    MR.check_activations("gpu", got, P, seed)
    again = run_activations(P, seed)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got, again))
    only_o = run_activations(P, seed, want="o")      # dL/draw_opacity depends on dL/dopacity alone: the bits of the pair
    assert torch.equal(bits(only_o[3]), bits(got[3]))
    only_s = run_activations(P, seed, want="s")
    assert float(only_s[3].abs().max()) == 0.0 and float(only_s[2].abs().max()) > 0.0


def test_non_finite_rows_on_the_device():
    from gsr_scene import mip
    P = 1027
    rs, ro, f, gs, go = (t.to(DEV) for t in MR.activation_case(P, 77))
    want = run_activations(P, 77)
    rows = [0, 1, 2, 258, 1024, 1026]
    rs[0, 0], rs[1, 1], ro[2, 0], f[258, 0], rs[1024, 2], ro[1026, 0] = math.nan, math.inf, math.nan, math.nan, 200.0, math.nan
    a, b = rs.clone().requires_grad_(True), ro.clone().requires_grad_(True)
    s, o = mip.filtered_activations(a, b, f)
    ((s * gs).sum() + (o * go).sum()).backward()
    got = (s.detach().cpu(), o.detach().cpu(), a.grad.cpu(), b.grad.cpu())
    keep = torch.ones(P, dtype=torch.bool)
    keep[rows] = False
    for g, w in zip(got, want):
        assert torch.equal(bits(g[keep]), bits(w[keep])), "a clean row changed"
    assert float(got[2][rows].abs().max()) == 0.0 and float(got[3][rows].abs().max()) == 0.0
    assert not bool(torch.isfinite(torch.cat([got[0][rows], got[1][rows]], dim=1)).all(dim=1).any())
    means, cams = (t.clone() for t in MR.scene_reference(P, 65)[:2])      # and the sweep: a poisoned mean takes the fill value, nobody else moves
    clean, _ = run_sweep(P, 65)
    assert float(clean[rows].max()) < float(clean.max())
    means[rows, 0] = torch.tensor([math.nan, math.inf, -math.inf, math.nan, math.inf, math.nan])
    filt, seen = mip.compute_3d_filter(means.to(DEV), cams.to(DEV), return_seen=True)
    filt, seen = filt.reshape(-1).cpu(), seen.cpu()
    assert torch.equal(bits(filt[keep]), bits(clean[keep])) and not bool(seen[rows].any())
    assert filt[rows].tolist() == [float(clean[keep].max())] * len(rows)


def test_side_stream_and_bases_off_16_byte_alignment():
    from gsr_scene import mip
    P, C = 1027, 65
    want_f, want_seen = run_sweep(P, C)
    want = run_activations(P, 40 + P)
    means, cams = MR.scene_reference(P, C)[:2]
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        def shifted(t):      # a copy whose base sits 4 bytes past a 16-byte boundary
            buf = torch.empty(t.numel() + 4, device=DEV)
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t.to(DEV))
            assert v.data_ptr() % 16 == 4
            return v
        filt, seen = mip.compute_3d_filter(shifted(means), shifted(cams), return_seen=True)
        rs, ro, f, gs, go = (shifted(t) for t in MR.activation_case(P, 40 + P))
        a, b = rs.requires_grad_(True), ro.requires_grad_(True)
        s, o = mip.filtered_activations(a, b, f)
        ((s * gs).sum() + (o * go).sum()).backward()
    stream.synchronize()
    assert torch.equal(bits(filt.reshape(-1).cpu()), bits(want_f)) and torch.equal(seen.cpu(), want_seen)
    got = (s.detach().cpu(), o.detach().cpu(), a.grad.cpu(), b.grad.cpu())
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got, want))      # the scalar form and the 16-byte form: the same bits


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def e2e_scene(P=300, seed=13):
    """About 300 Gaussians around the plane z = 5 in front of helpers.make_camera(96, 80), one axis much thinner than the filter."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(P, generator=g) * 2 - 1) * 3.0
    y = (torch.rand(P, generator=g) * 2 - 1) * 2.3
    means = torch.stack([x, y, 5.0 + 0.3 * x + 0.05 * torch.randn(P, generator=g)], dim=1)
    raw_scales = torch.log(torch.stack([0.25 * torch.exp(0.2 * torch.randn(P, generator=g)), 0.1 * torch.exp(0.3 * torch.randn(P, generator=g)),
                                        0.004 * torch.exp(0.5 * torch.randn(P, generator=g))], dim=1))
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    raw_opacity = torch.randn(P, 1, generator=g) * 1.5 + 1.0
    colors = torch.rand(P, 3, generator=g)
    return means.contiguous(), raw_scales.contiguous(), q.contiguous(), raw_opacity.contiguous(), colors.contiguous()


def e2e_chain(kernels: bool):
    """compute_3d_filter -> filtered activations -> one antialiased rasterizer call -> a scalar; kernels = False: the activations are upstream's
    torch expressions in fp32 on the device, everything else is the same code.  -> loss, dL/draw_scales, dL/draw_opacity, the filter."""
    import diff_gaussian_rasterization as pkg
    import test_composite_cpu as T
    from gsr_scene import mip
    from helpers import make_camera
    cam = make_camera(96, 80)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device=DEV), True, DEV)
    assert S.antialiasing
    means, raw_scales, q, raw_opacity, colors = (t.to(DEV) for t in e2e_scene())
    vm = S.viewmatrix
    W, H = float(S.image_width), float(S.image_height)
    record = torch.cat([vm[:3, :3].reshape(-1), vm[3, :3], torch.tensor([W / (2 * S.tanfovx), H / (2 * S.tanfovy), W, H], device=DEV)])[None]
    filt = mip.compute_3d_filter(means, record)
    rs, ro = raw_scales.clone().requires_grad_(True), raw_opacity.clone().requires_grad_(True)
    scales, opacity = mip.filtered_activations(rs, ro, filt) if kernels else MR.filtered_activations_fp32(rs, ro, filt)
    color, radii, invdepth = pkg.GaussianRasterizer(S)(means3D=means, means2D=None, opacities=opacity, colors_precomp=colors, scales=scales,
                                                       rotations=q)
    g = torch.Generator().manual_seed(5)
    w = torch.rand(color.shape, generator=g).to(DEV)
    loss = (color * w).sum() + 0.3 * invdepth.sum()
    loss.backward()
    return float(loss.detach()), rs.grad.cpu(), ro.grad.cpu(), filt.cpu(), float((radii > 0).float().mean())


def test_antialiased_render_fed_by_the_filtered_activations():
    loss_k, ds_k, do_k, filt, visible = e2e_chain(True)
    loss_t, ds_t, do_t, _, _ = e2e_chain(False)
    thin = float((torch.exp(e2e_scene()[1][:, 2:3]) < filt).float().mean())
    print(f"[mip] gpu end to end: loss {loss_k:.6f} (torch chain {loss_t:.6f}), {visible * 100:.0f} % of the Gaussians on screen, {thin * 100:.0f} % with "
          f"their thin axis below the filter size (median {float(filt.median()):.4f})", flush=True)
    assert visible >= 0.5 and thin >= 0.5
    assert abs(loss_k - loss_t) <= 1e-5 * abs(loss_t)
    for name, a, b in (("raw_scales", ds_k, ds_t), ("raw_opacity", do_k, do_t)):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"[mip] gpu end to end: dL/d{name} differs by {err:.2e} of its maximum {float(b.abs().max()):.3e} (bar 1e-05)", flush=True)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0, name
        assert err <= 1e-5, (name, err)
