"""Per-pixel probe on the MI355X (gsr_pixel_probe): the comparison of tests/test_probe_cpu.py on tests/test_gpu_contrib.py's frame (20 K Gaussians, 256 x 256,
the one shared oracle frame) against the fp64 reference of tests/probe_reference.py with the same bars; identities through the product itself and
bit-reproducibility at the bench frame (1 M Gaussians, 1920 x 1080); and the two hand-computable frames."""
import functools

import pytest
import torch

from helpers import make_camera, make_scene
import probe_reference as R
import test_composite_cpu as T
import test_gpu_contrib as GC

pytestmark = pytest.mark.gpu


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def reference(threshold):
    """Computed once per threshold on the shared oracle frame, never modified."""
    aux, s0 = GC.oracle_aux()
    return R.reference(aux, s0, threshold)


@pytest.mark.parametrize("threshold", [0.5, 0.9])
def test_gpu_probe_matches_the_reference_20k(threshold):
    pkg = _pkg()
    aux, s0 = GC.oracle_aux()
    out, lv, S = GC.render(pkg)
    got = pkg.pixel_probe(out[0].clamp(0.0, 1.0), threshold)
    alone, radii = pkg.GaussianRasterizer(S).probe(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], threshold=threshold)
    nums = R.check(f"probe_gpu_20k_t{threshold}", got, reference(threshold), aux)
    assert nums["terminated_share"] > 0.01 and nums["longest_list"] > 128
    assert equal(got, alone) and torch.equal(radii, out[1])
    stats = pkg.contribution_stats(out[0])
    assert int(got.count.sum()) == int(stats.pixel_count.sum())


def test_gpu_identities_at_the_bench_frame():
    """1920 x 1080, 1 M Gaussians (bench.py's recipe), no oracle: sum of count = sum of contribution_stats' pixel_count (exact), two calls give equal bits,
    ids in [-1, P), a median implies a contributor, and expected_depth against the product's own blend of a colour channel that carries z / z_max."""
    pkg = _pkg()
    Wb, Hb, P = 1920, 1080, 1_000_000
    cam = make_camera(Wb, Hb)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to("cuda")
    vm = cam.world_view_transform.cuda()
    m = sc.means3D
    z = m[:, 0] * vm[0, 2] + m[:, 1] * vm[1, 2] + m[:, 2] * vm[2, 2] + vm[3, 2]      # view-space depth, in torch
    z_max = float(z.max())
    colors = torch.zeros(P, 3, device="cuda")
    colors[:, 0] = (z / z_max).clamp(min=0.0)
    means = sc.means3D.clone().requires_grad_(True)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device="cuda"), device="cuda")
    color, radii, _ = pkg.GaussianRasterizer(S)(means3D=means, means2D=None, opacities=sc.opacities, colors_precomp=colors, scales=sc.scales,
                                                rotations=sc.rotations)
    got = pkg.pixel_probe(color)
    again = pkg.pixel_probe(color)
    stats = pkg.contribution_stats(color)
    alone, radii2 = pkg.GaussianRasterizer(S).probe(sc.means3D, sc.opacities, scales=sc.scales, rotations=sc.rotations)
    on = got.count > 0
    d_depth = float((got.expected_depth.double() - color[0].detach().double() * z_max)[on].abs().max()) / z_max
    total = int(got.count.sum())
    R.parity_report("probe_gpu_bench_frame", expected_depth_vs_colour_rel_zmax=d_depth, z_max=z_max, contributions=total,
                    pixels_with_contributor=int(on.sum()), pixels_with_median=int((got.median_id >= 0).sum()), count_max=int(got.count.max()))
    assert equal(got, again) and equal(got, alone) and torch.equal(radii, radii2)
    assert total == int(stats.pixel_count.sum()) > 0
    for ids in (got.median_id, got.top_id):
        assert int(ids.min()) >= -1 and int(ids.max()) < P
        assert bool((radii[ids[ids >= 0].long()] > 0).all())
    assert bool((got.count[got.median_id >= 0] >= 1).all()) and bool(((got.top_id >= 0) == on).all())
    assert int(on.sum()) > Wb * Hb // 2 and int((got.median_id >= 0).sum()) > Wb * Hb // 4
    assert d_depth < 1e-5
    # the median depth is the named Gaussian's depth: two fp32 evaluations of one four-term sum whose partial sums stay below 2 z_max, so they differ by
    # at most 4 roundings of 2 z_max 2^-24 = 5e-7 z_max
    med = got.median_id >= 0
    assert float((got.median_depth[med] - z[got.median_id[med].long()]).abs().max()) <= 1e-6 * z_max


def test_gpu_hand_computable_frames():
    pkg = _pkg()
    for which, check in (("isolated", R.check_isolated), ("layers", R.check_layers)):
        cam, lv = R.hand_frame(which)
        lv = {k: v.cuda() for k, v in lv.items()}
        rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device="cuda"), device="cuda"))
        check(lambda t: rast.probe(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], threshold=t))
