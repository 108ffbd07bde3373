"""Per-Gaussian blend-weight statistics on the MI355X (gsr_contribution_stats): the checks of tests/test_contrib_cpu.py at 20 K Gaussians / 256 x 256
against the fp64 reference of tests/contrib_reference.py with the same bars (one oracle frame, shared), the product identities and bit-reproducibility at
the bench frame (1 M Gaussians, 1920 x 1080), and the same identities on a frame with enough instances for the scratch offsets to pass 2^31 bytes."""
import functools

import pytest
import torch

from helpers import O, look_at_camera, make_camera, make_scene
import contrib_reference as R
import test_composite_cpu as T

pytestmark = pytest.mark.gpu

W = H = 256


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


@functools.lru_cache(maxsize=None)
def scene(which="first"):
    cam = make_camera(W, H) if which == "first" else look_at_camera(W, H, (0.4, -0.3, -1.0), (0.0, 0.1, 4.0))
    sc = make_scene(20_000, make_camera(W, H), seed=3, s_med=0.02)
    sc.opacities = R.raise_opacity(sc.opacities)
    return cam, sc


@functools.lru_cache(maxsize=None)
def oracle_aux():
    """The oracle's frame: computed once, shared by the tests, never modified."""
    cam, sc = scene()
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, False)
    with torch.no_grad():
        aux = O.rasterize(s=s0, want_fragile=True, return_aux=True, **T.call_kwargs(T.make_leaves(sc, "fused", grad=False), "fused", oracle=True))[3]
    return aux, s0


def render(pkg, which="first"):
    cam, sc = scene(which)
    lv = T.make_leaves(sc, "fused", "cuda")
    out, S = T.render_pkg(pkg, cam, lv, "fused", torch.zeros(3, device="cuda"), return_alpha=False, device="cuda")
    return out, lv, S


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("weights", ["masked", "signed"])
def test_gpu_statistics_match_the_reference_20k(weights):
    pkg = _pkg()
    aux, s0 = oracle_aux()
    g = torch.Generator().manual_seed(11)
    E = torch.rand(H, W, generator=g)
    if weights == "masked":       # fragile pixels and a further random 10 % excluded
        E = R.mask_fragile(E, aux)
        E[torch.rand(H, W, generator=g) < 0.1] = 0.0
    else:
        E = R.mask_fragile(E - 0.3, aux)
    ref = R.reference(aux, s0, E)
    out, lv, S = render(pkg)
    got = pkg.contribution_stats(out[0].clamp(0.0, 1.0), E.cuda())
    alone, radii = pkg.GaussianRasterizer(S).contributions(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], pixel_weight=E.cuda())
    nums = R.check(f"contrib_gpu_{weights}_20k", got, ref, aux, E_absmax=float(E.abs().max()))
    assert nums["terminated_share"] > 0.01
    assert equal(got, alone) and torch.equal(radii, out[1])
    if weights == "signed":
        assert float(got.weight_sum.min()) < 0.0 and float(got.weight_max.min()) == 0.0


def test_gpu_accumulate_and_two_runs_20k():
    pkg = _pkg()
    out_a, _, _ = render(pkg)
    out_b, _, _ = render(pkg, "second")
    a, b = pkg.contribution_stats(out_a[0]), pkg.contribution_stats(out_b[0])
    again = pkg.contribution_stats(render(pkg)[0][0])
    ones = pkg.contribution_stats(out_a[0], torch.ones(1, H, W, device="cuda"))
    assert equal(a, again) and equal(a, ones)
    acc = pkg.contribution_stats(out_a[0])
    assert pkg.contribution_stats(out_b[0], into=acc) is acc
    assert int(((a.pixel_count > 0) & (b.pixel_count > 0)).sum()) > 5000 and not torch.equal(a.pixel_count, b.pixel_count)
    assert torch.equal(acc.weight_sum, a.weight_sum + b.weight_sum)
    assert torch.equal(acc.weight_max, torch.maximum(a.weight_max, b.weight_max))
    assert torch.equal(acc.pixel_count, a.pixel_count + b.pixel_count)


def _identities(pkg, s_med, key):
    """On a 1920 x 1080 frame of 1 M Gaussians (bench.py's recipe with the given s_med): sum of weight_sum = sum of the alpha image (E = 1),
    weight_sum = the package's own dL/dcolors_precomp[:,0] of sum E C_0, pixel_count > 0 implies radii > 0, two runs give equal bits.  No oracle."""
    Wb, Hb, P = 1920, 1080, 1_000_000
    cam = make_camera(Wb, Hb)
    sc = make_scene(P, cam, seed=0, s_med=s_med).to("cuda")
    g = torch.Generator().manual_seed(5)
    E = torch.rand(Hb, Wb, generator=g).clamp_(min=1e-3).cuda()      # (strictly positive: see the check of the contributing set below)
    colors = torch.rand(P, 3, generator=g).cuda().requires_grad_(True)
    means = sc.means3D.clone().requires_grad_(True)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device="cuda"), device="cuda")
    rast = pkg.GaussianRasterizer(S, return_alpha=True)
    color, radii, invd, alpha = rast(means3D=means, means2D=None, opacities=sc.opacities, colors_precomp=colors, scales=sc.scales, rotations=sc.rotations)
    instances = pkg._last_R
    ones = pkg.contribution_stats(color)
    got = pkg.contribution_stats(color, E)
    again = pkg.contribution_stats(color, E)
    alone, radii2 = pkg.GaussianRasterizer(S).contributions(sc.means3D, sc.opacities, scales=sc.scales, rotations=sc.rotations, pixel_weight=E)
    (color[0] * E).sum().backward()
    assert equal(got, again) and equal(got, alone) and torch.equal(radii, radii2)
    alpha_total = float(alpha.detach().double().sum())
    d_alpha = abs(float(ones.weight_sum.double().sum()) - alpha_total) / alpha_total
    grad = colors.grad[:, 0].double()
    d_grad = float((got.weight_sum.double() - grad).abs().max()) / float(grad.abs().max())
    R.parity_report(key, instances=instances, contributing=int((ones.pixel_count > 0).sum()), sum_vs_alpha_rel=d_alpha, sum_vs_dcolor_rel_max=d_grad)
    # Who contributes, against an independent kernel: E > 0 and every blend weight is > 0, so a Gaussian's colour gradient from the blend backward is
    # non-zero exactly when it was blended into a pixel with E != 0.  (No lower bound on how many do: on the bench frame the lists are deep and the
    # pixels terminate early -- 64 902 of 876 281 visible Gaussians contribute, measured -- so most rows are the zero rows of hidden Gaussians.)
    assert int((radii > 0).sum()) > 500_000
    assert torch.equal(got.pixel_count > 0, colors.grad[:, 0] != 0) and int((got.pixel_count > 0).sum()) > 0
    assert bool((got.pixel_count <= ones.pixel_count).all()) and bool(((got.weight_max > 0) == (got.pixel_count > 0)).all())
    assert d_alpha <= 1e-5 and d_grad < 1e-5
    assert bool((radii[ones.pixel_count > 0] > 0).all())
    return instances


def test_gpu_identities_at_the_bench_frame():
    _identities(_pkg(), 0.012, "contrib_gpu_bench_frame")


def test_gpu_identities_with_scratch_offsets_past_2_31_bytes():
    """Four 16-byte slots per instance: the slot table passes 2^31 bytes from 33.6 M instances on, which the bench frame (7.9 M) does not reach.
    Larger splats on the same frame do."""
    instances = _identities(_pkg(), S_MED_LARGE, "contrib_gpu_large_frame")
    assert instances * 64 > 2 ** 31, instances


S_MED_LARGE = 0.035      # 42.0 M instances (the oracle's tile counts; 0.03 gives 32.4 M, short of the 33.6 M needed)
