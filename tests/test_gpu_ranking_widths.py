"""The stable-ranking kernels of the binning chain on the GPU (csrc/tilesort.hip emit_scatter / bucket_scatter, csrc/depthsort.hip ds_scatter /
ds_segsort): the instantiations compiled for a digit width (match_digit<BITS>, 24-bit emission arithmetic, v_mbcnt ranks) against the
run-time-width kernels that `gsr_set_option("ranking_generic", 1)` forces.  Each frame is rendered both ways and every array
`debug.forward_with_views` exposes -- point_list, ranges, depth order, offsets, splat records, n_contrib, final_T -- and the image, the inverse
depth and the radii must be the same bytes.  The test hook `debug_last_ranking_widths` (hb << 4 | lb, 0 = generic) says which instantiations ran.

Frames: the smallest that select each pair of widths (tile id of n bits: low digit ceil(n / 2) bits, bucket digit the rest; 5..8 have an
instantiation, except a bucket digit of 8): 64x64 (2 / 2: generic either way), 640x360 (5 / 5), 1280x720 (6 / 6), 1920x1080 (6 / 7), 3840x2160
(7 / 8), 4096x2304 (8 / 8: emit_scatter generic, bucket_scatter<8>).
tests/test_simt_ranking_widths_cpu.py compares match_digit<BITS> with the loop form on the CPU."""
import copy

import pytest
import torch

from helpers import make_camera, make_scene, make_edge_scene, oracle_settings
from test_gpu_parity import gpu_settings

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("color", "invdepth", "radii", "splats", "tiles_touched", "depth_order", "offsets", "point_list", "ranges", "final_T", "n_contrib")


def forward(cam, sc):
    from diff_gaussian_rasterization.debug import forward_with_views
    rs = gpu_settings(oracle_settings(cam, bg=torch.tensor([0.2, 0.4, 0.6])), torch.device(DEV))
    out = forward_with_views(rs, sc.means3D, sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    res = {k: out[k].clone() for k in KEYS}
    res["R"] = torch.tensor([int(out["R"])])
    torch.cuda.synchronize()
    return res


def both_ways(cam, sc, hb, lb):
    """Renders with the width instantiations (checks that emit_scatter<hb> / bucket_scatter<lb> ran), then with the generic kernels; asserts that
    every array agrees byte for byte; returns the first result."""
    from diff_gaussian_rasterization import _lib
    sc = sc.to(DEV)
    _lib.set_option("ranking_generic", 0)
    auto = forward(cam, sc)
    if int(auto["R"]) > 0:
        _lib.set_option("debug_last_ranking_widths", hb << 4 | lb)      # (raises GsrError when other instantiations ran)
    _lib.set_option("ranking_generic", 1)
    try:
        forced = forward(cam, sc)
        if int(forced["R"]) > 0:
            _lib.set_option("debug_last_ranking_widths", 0)
    finally:
        _lib.set_option("ranking_generic", 0)
    for k in auto:
        a, b = auto[k].contiguous().view(torch.uint8), forced[k].contiguous().view(torch.uint8)
        assert torch.equal(a, b), f"{k}: the width instantiation and the generic kernel differ"
    return auto


def assert_is_a_binning(out, P):
    """The lists are sorted by depth inside every tile range and the ranges tile [0, R)."""
    R = int(out["R"])
    rg = out["ranges"].view(-1, 2).long().cpu()
    assert int((rg[:, 1] - rg[:, 0]).sum()) == R == out["point_list"].numel()
    assert int(out["point_list"].min()) >= 0 and int(out["point_list"].max()) < P


@pytest.mark.parametrize("W,H,hb,lb", [(64, 64, 0, 0), (640, 360, 5, 5), (1280, 720, 6, 6), (1920, 1080, 6, 7), (3840, 2160, 7, 8), (4096, 2304, 0, 8)])
def test_width_instantiations_and_generic_kernels_agree_byte_for_byte(W, H, hb, lb):
    P = 3000
    cam = make_camera(W, H)
    out = both_ways(cam, make_scene(P, cam, seed=3, s_med=0.03), hb, lb)
    R = int(out["R"])
    assert R > 4096, "more than one emission block"
    assert R % 4096 != 0, "the last block is partial (invalid lanes in the ranking loops)"
    assert_is_a_binning(out, P)


def test_a_block_with_more_than_1024_gaussians():
    """6 000 pin-point Gaussians, one tile each unless they straddle a tile edge (1.6 on average): a block of 4096 instances holds about 2 600
    Gaussians (the records beyond the 1024 staged in LDS are fetched from global memory: the second loop of generate_instances) and the depth
    sort's segments are full."""
    P = 6000
    cam = make_camera(640, 360)
    sc = make_scene(P, cam, seed=5, s_med=0.0004, overscan=0.9)
    out = both_ways(cam, sc, 5, 5)
    tt = out["tiles_touched"].long()
    assert int(tt.max()) <= 4 and int(tt.sum()) > 2 * 4096 and int(tt.sum()) < 2 * int((tt > 0).sum()), "under two tiles each, more than two blocks of them"
    assert_is_a_binning(out, P)


def test_empty_buckets():
    """Every Gaussian in the top-left corner of a 1920x1080 frame: most of the 64 buckets (and of their tiles) hold no instance at all."""
    P = 3000
    cam = make_camera(1920, 1080)
    sc = copy.copy(make_scene(P, cam, seed=7, s_med=0.03))
    sc.means3D = sc.means3D.clone()
    z = sc.means3D[:, 2]
    sc.means3D[:, 0] = -(0.55 + 0.4 * torch.rand(P, generator=torch.Generator().manual_seed(1))) * z * cam.tanfovx
    sc.means3D[:, 1] = -(0.55 + 0.4 * torch.rand(P, generator=torch.Generator().manual_seed(2))) * z * cam.tanfovy
    out = both_ways(cam, sc, 6, 7)
    rg = out["ranges"].view(-1, 2).long().cpu()
    per_bucket = (rg[:, 1] - rg[:, 0]).view(-1)
    nb = (per_bucket.numel() + 127) // 128
    filled = sum(int(per_bucket[b * 128:(b + 1) * 128].sum()) > 0 for b in range(nb))
    assert 0 < filled < nb // 2, "most buckets are empty"
    assert int(out["R"]) > 0
    assert_is_a_binning(out, P)


def test_depth_ties():
    """All Gaussians on eight depth planes: thousands of equal keys per value -- the order inside a tile is the index order of the stable sorts."""
    P = 3000
    cam = make_camera(640, 360)
    sc = copy.copy(make_edge_scene(P, cam, seed=9))
    sc.means3D = sc.means3D.clone()
    z_old = sc.means3D[:, 2].clone()
    z_new = 2.0 + (torch.arange(P) % 8).float()
    sc.means3D[:, 0] *= z_new / z_old.abs().clamp_min(0.2)
    sc.means3D[:, 1] *= z_new / z_old.abs().clamp_min(0.2)
    sc.means3D[:, 2] = z_new
    out = both_ways(cam, sc, 5, 5)
    assert_is_a_binning(out, P)
    # inside a tile, equal depths keep index order
    depth = sc.means3D[:, 2]
    rg = out["ranges"].view(-1, 2).long().cpu()
    pl = out["point_list"].long().cpu()
    busiest = int((rg[:, 1] - rg[:, 0]).argmax())
    ids = pl[rg[busiest, 0]:rg[busiest, 1]]
    assert ids.numel() > 16
    d = depth[ids]
    assert bool((d[1:] >= d[:-1]).all())
    same = d[1:] == d[:-1]
    assert bool(same.any()) and bool((ids[1:][same] > ids[:-1][same]).all())
