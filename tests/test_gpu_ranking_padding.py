"""Padding slots of the tile sort's ranking kernels on the GPU (csrc/tilesort.hip emit_scatter / bucket_scatter, option ranking_pad_last): the slots
that a partial block of 4096 does not have are ranked as ordinary items of the highest digit (1, the default) instead of carrying a validity predicate
per item (0).  Every frame is rendered four ways -- ranking_pad_last 1 / 0 with the digit-width instantiations and with the run-time-width kernels of
ranking_generic = 1; the hook debug_last_ranking_widths says which ran -- and the point list, the tile ranges, the instance count, the image, the inverse
depth and the radii must be the same bytes in all four; the bins are those of the CPU oracle (obtained as tests/test_gpu_bins_sweep.py does).

Frames (tests/ranking_padding_cases.py): 640x360 (tile-id halves of 5 / 5 bits) and 1920x1080 (6 / 7) with a few thousand Gaussians, plus one-tile
Gaussians behind them that steer
* level 1: the instance count R to 0, 1, 63, 64, 65, 4095 modulo 4096 and to R = 37 (fewer than a wave), once with the last emission block full of
  instances of the last tile row -- the highest bucket the frame has; at 1080p that row reaches into the top digit 63 itself, the padding's own digit --
  and once with the last block on the first tile row (bucket 0 only, the padding alone in the top digit);
* level 2: the number of words of one bucket to 4096 k and to 4096 k + 1, the bucket's last word on its last tile (the top low digit): at 4096 k + 1 the
  bucket's last workgroup ranks that one real item of the top low digit in front of 4095 padding items of the same digit.
The residues are conditions of the tests and are asserted on the rendered frame."""
import pytest
import torch

import ranking_padding_cases as K
from helpers import oracle_settings
from test_gpu_parity import gpu_settings

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("point_list", "ranges", "color", "invdepth", "radii")
FRAMES = [(640, 360, 3000, 5, 5), (1920, 1080, 2000, 6, 7)]


def forward(cam, sc):
    from diff_gaussian_rasterization.debug import forward_with_views
    rs = gpu_settings(oracle_settings(cam), torch.device(DEV))
    out = forward_with_views(rs, sc.means3D, sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    res = {k: out[k].clone() for k in KEYS}
    res["R"] = torch.tensor([int(out["R"])])
    torch.cuda.synchronize()
    return res


def four_ways(cam, sc, hb, lb):
    """pad_last 1 / 0 x width instantiations / generic kernels; asserts that all four agree byte for byte and with the oracle's bins; returns
    (the default form's result, the oracle's bins)."""
    from diff_gaussian_rasterization import _lib
    pre, bins = K.oracle_bins(cam, sc)
    d = sc.to(DEV)
    got = {}
    try:
        for generic in (0, 1):
            for pad in (1, 0):
                _lib.set_option("ranking_generic", generic)
                _lib.set_option("ranking_pad_last", pad)
                got[(generic, pad)] = forward(cam, d)
                if int(got[(generic, pad)]["R"]) > 0:
                    _lib.set_option("debug_last_ranking_widths", 0 if generic else hb << 4 | lb)      # (raises GsrError when other instantiations ran)
    finally:
        _lib.set_option("ranking_generic", 0)
        _lib.set_option("ranking_pad_last", 1)
    ref = got[(0, 1)]
    for way, res in got.items():
        for k in ref:
            assert torch.equal(ref[k].contiguous().view(torch.uint8), res[k].contiguous().view(torch.uint8)), \
                f"{k}: (ranking_generic, ranking_pad_last) = {way} differs from (0, 1)"
    assert int(ref["R"]) == int(bins["R"])
    assert torch.equal(ref["radii"].cpu(), pre["radii"].to(torch.int32)), "radii differ from the oracle's"
    assert torch.equal(ref["point_list"].cpu().to(torch.int64), bins["point_list"]), "point list differs from the oracle's"
    assert torch.equal(ref["ranges"].cpu().to(torch.int64), bins["ranges"]), "tile ranges differ from the oracle's"
    return ref, bins


def instance_tiles(bins):
    """tile id of every entry of the sorted point list"""
    rg = bins["ranges"].view(-1, 2)
    return torch.repeat_interleave(torch.arange(rg.shape[0]), rg[:, 1] - rg[:, 0])


@pytest.mark.parametrize("on_last_row", [True, False], ids=["last_row", "first_row"])
@pytest.mark.parametrize("residue", K.RESIDUES + (None,), ids=[f"R%4096={r}" for r in K.RESIDUES] + ["R<64"])
@pytest.mark.parametrize("W,H,P,hb,lb", FRAMES)
def test_level1_padding_at_every_residue_of_the_instance_count(W, H, P, hb, lb, residue, on_last_row):
    gx, gy, n_tiles, plb, phb = K.plan(W, H)
    assert (phb, plb) == (hb, lb)
    cam, sc = K.level1_frame(W, H, P, residue, on_last_row)
    out, bins = four_ways(cam, sc, hb, lb)
    R = int(out["R"])
    if residue is None:
        assert R == K.SMALL_R < 64
        n_last = R
    else:
        assert R % K.TS_ITEMS == residue and R > 2 * K.TS_ITEMS, R
        n_last = residue or K.TS_ITEMS
    # the last emission block holds the n_last deepest instances: all of them one-tile Gaussians (the highest ids) of the chosen row
    n_fill = sc.P - (0 if residue is None else P)
    assert n_fill >= n_last
    last_ids = torch.arange(sc.P - n_last, sc.P)
    buckets = instance_tiles(bins)[torch.isin(bins["point_list"], last_ids)] >> lb
    assert buckets.numel() == n_last
    top = (1 << hb) - 1
    if on_last_row:
        assert int(buckets.max()) == (n_tiles - 1) >> lb, "the last block holds instances of the highest bucket of the frame"
        if (n_tiles - 1) >> lb == top:      # (1080p; at 640x360 the tiles end in bucket 28 of 32)
            assert bool((buckets == top).any()), "real instances of the top digit beside the padding"
    else:
        assert int(buckets.max()) == 0 < top, "the padding is alone in the top digit"


@pytest.mark.parametrize("extra", [0, 1], ids=["4096k", "4096k+1"])
@pytest.mark.parametrize("W,H,P,hb,lb", FRAMES)
def test_level2_padding_in_a_bucket_of_4096k_and_4096k_plus_1_words(W, H, P, hb, lb, extra):
    cam, sc = K.level2_frame(W, H, P, extra)
    out, bins = four_ways(cam, sc, hb, lb)
    rg = out["ranges"].view(-1, 2).long().cpu()
    t0, nb2 = K.LEVEL2_BUCKET << lb, 1 << lb
    words = int((rg[t0:t0 + nb2, 1] - rg[t0:t0 + nb2, 0]).sum())
    assert words % K.TS_ITEMS == extra and words >= K.TS_ITEMS, words
    # the bucket's last word -- the deepest instance, the highest id of the frame -- lies on the bucket's last tile: the top low digit is present among the
    # real items of the bucket's last workgroup (at 4096 k + 1 it is that workgroup's only real item)
    pl = out["point_list"].long().cpu()
    assert int(pl[rg[t0 + nb2 - 1, 1] - 1]) == sc.P - 1
