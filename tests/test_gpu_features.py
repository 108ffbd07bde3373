"""N-channel feature render on the MI355X (gsr_render_features / gsr_render_features_backward): the checks of tests/test_features_cpu.py on
tests/test_gpu_contrib.py's frame (20 K Gaussians, 256 x 256, the one shared oracle frame, lists over 128 entries, more than 1 % of the pixels
terminate) against the fp64 reference of tests/feature_reference.py with the same bars, the identities through the product itself, the bit contracts,
and the two hand-computable frames.  The bench-frame size is covered by tools/gpu_features_time.py."""
import functools

import pytest
import torch

import contrib_reference as CR
import feature_reference as R
import probe_reference as PR
import test_composite_cpu as T
import test_gpu_contrib as GC

pytestmark = pytest.mark.gpu

W = H = GC.W
P = 20_000
G = 16      # channels per forward walk (csrc/features.hip FEAT_G, pinned by tests/test_features_isa_cpu.py); the backward walks 4 at a time


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


@functools.lru_cache(maxsize=None)
def inputs(channels, seed=31):
    """(features [P,C] in [-1,1], upstream gradient [C,H,W] in [-0.5,0.5] with the fragile pixels zeroed), on the CPU: computed once, never modified."""
    aux, _ = GC.oracle_aux()
    g = torch.Generator().manual_seed(seed)
    f, up = torch.rand(P, channels, generator=g) * 2.0 - 1.0, torch.rand(channels, H, W, generator=g) - 0.5
    return f, torch.stack([CR.mask_fragile(up[c], aux) for c in range(channels)])


def feature_pass(pkg, rendered, f, grad_out):
    leaf = f.cuda().requires_grad_(True)
    out = pkg.render_features(rendered, leaf)
    out.backward(grad_out.cuda())
    return out.detach(), leaf.grad


@pytest.mark.parametrize("channels", [5, 2 * G + 3])
def test_gpu_features_match_the_reference_20k(channels):
    pkg = _pkg()
    aux, s0 = GC.oracle_aux()
    f, up = inputs(channels)
    stats = CR.reference(aux, s0)
    assert float(stats["terminated"].float().mean()) > 0.01 and stats["longest"] > 128
    out, lv, S = GC.render(pkg)
    got_F, got_g = feature_pass(pkg, out[0].clamp(0.0, 1.0), f, up)
    R.check_image(f"features_gpu_20k_c{channels}_image", got_F, R.forward(aux, s0, f), aux, float(f.abs().max()))
    R.check_gradient(f"features_gpu_20k_c{channels}_grad", got_g, R.gradient(aux, s0, up), aux)


def test_gpu_identities_against_the_product_itself():
    pkg = _pkg()
    cam, sc = GC.scene()
    lv = T.make_leaves(sc, "precomp", "cuda")
    out, S = T.render_pkg(pkg, cam, lv, "precomp", torch.zeros(3, device="cuda"), return_alpha=True, device="cuda")
    colors, means = lv["colors"].detach(), lv["means"].detach()
    vm = S.viewmatrix
    z = means[:, 0] * vm[0, 2] + means[:, 1] * vm[1, 2] + means[:, 2] * vm[2, 2] + vm[3, 2]
    f, up = inputs(3)
    as_colour = pkg.render_features(out[0], colors)
    as_alpha = pkg.render_features(out[0], torch.ones(P, 1, device="cuda"))
    as_depth = pkg.render_features(out[0], z[:, None].contiguous())
    probe = pkg.pixel_probe(out[0])
    got_F, got_g = feature_pass(pkg, out[0], f, up)
    sums = [pkg.contribution_stats(out[0], up[c].cuda()).weight_sum for c in range(3)]
    d_colour = float((as_colour - out[0].detach()).abs().max())
    d_alpha = float((as_alpha - out[3].detach()).abs().max())
    d_depth = float((as_depth[0] - probe.expected_depth).abs().max()) / float(z.abs().max())
    d_sum = max(float((got_g[:, c].double() - sums[c].double()).abs().max()) / float(sums[c].abs().max()) for c in range(3))
    lhs, rhs = float((up.cuda().double() * got_F.double()).sum()), float((got_g.double() * f.cuda().double()).sum())
    R.parity_report("features_gpu_identities", colour_abs_max=d_colour, alpha_abs_max=d_alpha, depth_rel_zmax=d_depth, grad_vs_weight_sum_rel_max=d_sum,
                    adjoint_rel=abs(lhs - rhs) / abs(lhs))
    assert d_colour <= 1e-5 * float(colors.abs().max()) and d_alpha <= 1e-5 and d_depth <= 1e-5 and d_sum < 1e-5
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 1e-5 * abs(lhs)


def test_gpu_channel_alone_bits_two_runs_and_nan_rows():
    pkg = _pkg()
    c_max = G + 1
    f, up = inputs(c_max)
    out, lv, S = GC.render(pkg)
    alone = [feature_pass(pkg, out[0], f[:, c:c + 1].contiguous(), up[c:c + 1]) for c in range(c_max)]
    for channels in (G - 1, G, G + 1):
        got_F, got_g = feature_pass(pkg, out[0], f[:, :channels].contiguous(), up[:channels])
        for c in range(channels):
            assert torch.equal(got_F[c], alone[c][0][0]) and torch.equal(got_g[:, c], alone[c][1][:, 0]), (channels, c)
    # two runs, and the standalone form on a frame of its own
    a = feature_pass(pkg, out[0], f, up)
    b = feature_pass(pkg, GC.render(pkg)[0][0], f, up)
    leaf = f.cuda().requires_grad_(True)
    F, radii = pkg.GaussianRasterizer(S).features(lv["means"], lv["opac"], leaf, scales=lv["scales"], rotations=lv["rot"])
    F.backward(up.cuda())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], F.detach()) and torch.equal(a[1], leaf.grad)
    assert torch.equal(radii, out[1])
    # rows of Gaussians that contribute nowhere never reach the image and get exact zero gradients
    nowhere = pkg.contribution_stats(out[0]).pixel_count == 0
    poisoned = f.clone()
    poisoned[nowhere.cpu()] = float("nan")
    c = feature_pass(pkg, out[0], poisoned, up)
    assert int(nowhere.sum()) > 1000 and int((nowhere & (out[1] > 0)).sum()) > 100
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1]) and float(a[1][nowhere].abs().max()) == 0.0 and float(a[1][~nowhere].abs().max()) > 0.0


def test_gpu_band():
    pkg = _pkg()
    band = (4, 11)
    f, up = inputs(5)
    cam, sc = GC.scene()
    lv = T.make_leaves(sc, "fused", "cuda")
    full = feature_pass(pkg, GC.render(pkg)[0][0], f, up)
    parts = []
    for b in ((0, 4), band, (11, 16)):
        out, S = T.render_pkg(pkg, cam, lv, "fused", torch.zeros(3, device="cuda"), return_alpha=False, tile_rows=b, device="cuda")
        parts.append(feature_pass(pkg, out[0], f, up))
    r0, r1 = band[0] * 16, band[1] * 16
    got_F = parts[1][0]
    assert torch.equal(got_F[:, r0:r1], full[0][:, r0:r1]) and float(got_F[:, :r0].abs().max()) == 0.0 and float(got_F[:, r1:].abs().max()) == 0.0
    assert float(full[0][:, :r0].abs().max()) > 0.0 and float(full[0][:, r1:].abs().max()) > 0.0
    d = float((sum(p[1].double() for p in parts) - full[1].double()).abs().max()) / float(full[1].abs().max())
    R.parity_report("features_gpu_band", bands_sum_vs_full_rel_max=d)
    assert d <= 1e-6


def test_gpu_hand_computable_frames():
    pkg = _pkg()
    ys, xs = torch.meshgrid(torch.arange(PR.HAND_H), torch.arange(PR.HAND_W), indexing="ij")
    far = (((xs - PR.HAND_PX) ** 2 + (ys - PR.HAND_PY) ** 2).double().sqrt() >= 12.0).cuda()
    for which, f, want, w in (("isolated", [[float("nan")] * 3, [2.0, -3.0, 0.5]], [0.95 * 2.0, 0.95 * -3.0, 0.95 * 0.5], (0.0, 0.95)),
                              ("layers", [[1.0, -2.0, 4.0], [3.0, 0.5, -1.0]], [0.3 * 3.0 + 0.63 * 1.0, 0.3 * 0.5 + 0.63 * -2.0, 0.3 * -1.0 + 0.63 * 4.0],
                               (0.63, 0.3))):
        cam, lv = PR.hand_frame(which)
        lv = {k: v.cuda() for k, v in lv.items()}
        rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device="cuda"), device="cuda"))
        leaf = torch.tensor(f, device="cuda").requires_grad_(True)
        F, radii = rast.features(lv["means"], lv["opac"], leaf, scales=lv["scales"], rotations=lv["rot"])
        at = F.detach()[:, PR.HAND_PY, PR.HAND_PX].cpu()
        assert float((at - torch.tensor(want)).abs().max()) <= 1e-5 * 4.0, (which, at)
        up = torch.zeros_like(F)
        up[:, PR.HAND_PY, PR.HAND_PX] = torch.tensor([1.0, 2.0, -1.0], device="cuda")
        F.backward(up)
        for i in range(2):
            assert float((leaf.grad[i].cpu() - w[i] * torch.tensor([1.0, 2.0, -1.0])).abs().max()) <= 2e-5, (which, i, leaf.grad)
        if which == "isolated":
            assert float(F.detach()[:, far].abs().max()) == 0.0 and radii.tolist()[0] == 0
