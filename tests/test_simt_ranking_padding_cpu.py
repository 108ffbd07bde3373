"""Padding slots of the tile sort's ranking kernels (csrc/tilesort.hip, option ranking_pad_last) EXECUTED on the CPU, lane by lane, through the SIMT shim
of tests/simt/ and through the file's own launchers: the argument written at local_stable_sort -- slots that a partial block does not have, ranked as
ordinary items of the highest digit, end up behind every real item and are dropped at the final store -- checked without a GPU.

The cases of tests/test_gpu_ranking_padding.py at its smaller frame (640x360: 40 x 23 tiles, tile-id halves of 5 / 5 bits), built from rectangles in
depth order: a few hundred random ones, then at least 4096 one-tile rectangles that steer
* the instance count R to 0, 1, 63, 64, 65, 4095 modulo 4096 and to R = 37, with the last emission block on the last tile row (the highest bucket the
  frame has) and on the first (bucket 0: the padding alone in the top digit);
* the words of one bucket to 4096 k and 4096 k + 1, the bucket's last word on its last tile (the top low digit),
and, behind them, Gaussians without tiles as the depth sort leaves them (in a partial last block one of them owns the padding slots: a record of
width 0).  Each case runs ranking_pad_last 1 and 0 with the width instantiations and with the run-time-width kernels; the packed words of level 1, the
point list and the tile ranges must equal plain stable sorts every time."""
import ctypes as C
import shutil
import zlib

import numpy as np
import pytest

TS_ITEMS = 4096
GX, GY, LB, HB = 40, 23, 5, 5
RESIDUES = (0, 1, 63, 64, 65, 4095)
SMALL_R = 37
LEVEL2_BUCKET = 3

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def lib():
    from simt_build import build
    h = build("padding")
    h.simt_last_error.restype = C.c_char_p
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def base_rects(rng, P):
    out = []
    for _ in range(P):
        w, h = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        minx, miny = int(rng.integers(0, GX - w + 1)), int(rng.integers(0, GY - h + 1))
        out.append((minx, minx + w, miny, miny + h))
    return out


def one_tile(tiles):
    return [(int(t) % GX, int(t) % GX + 1, int(t) // GX, int(t) // GX + 1) for t in tiles]


DEAD = [(3, 3, 2, 2)] * 9      # zero tiles, behind everything


def count(rects):
    return sum((r[1] - r[0]) * (r[3] - r[2]) for r in rects)


def level1_case(residue, on_last_row):
    rng = np.random.default_rng(zlib.crc32(f"pad-l1-{residue}-{on_last_row}".encode()))
    row = GY - 1 if on_last_row else 0
    ncol = GX if on_last_row else min(GX, 1 << LB)
    tiles = lambda n: row * GX + (ncol - 1 - (n - 1 - np.arange(n)) % ncol)      # the last one on the row's last column
    if residue is None:
        return one_tile(tiles(SMALL_R)) + DEAD
    base = base_rects(rng, 500)
    n = (residue - count(base)) % TS_ITEMS + TS_ITEMS
    return base + one_tile(tiles(n)) + DEAD


def level2_case(extra):
    rng = np.random.default_rng(zlib.crc32(f"pad-l2-{extra}".encode()))
    base = base_rects(rng, 500)
    t0, nb2 = LEVEL2_BUCKET << LB, 1 << LB
    c0 = sum(1 for r in base for y in range(r[2], r[3]) for x in range(r[0], r[1]) if (y * GX + x) >> LB == LEVEL2_BUCKET)
    n = (extra - c0) % TS_ITEMS + TS_ITEMS
    return base + one_tile(t0 + (np.arange(n) - n) % nb2) + DEAD


def run_four_ways(lib, rects4):
    """Both levels through the launchers, ranking_pad_last 1 / 0 x widths / generic, against stable sorts.  Returns (R, tile of every instance in
    emission order)."""
    P, n_tiles, nb1 = len(rects4), GX * GY, 1 << HB
    rng = np.random.default_rng(5)
    tiles = np.array([(r[1] - r[0]) * (r[3] - r[2]) for r in rects4], dtype=np.int64)
    incl = np.cumsum(tiles)
    R = int(incl[-1])
    nblk = (R + TS_ITEMS - 1) // TS_ITEMS
    order = rng.permutation(P).astype(np.uint32)
    rect_sorted = np.array([[r[0] | (r[1] << 16), r[2] | (r[3] << 16)] for r in rects4], dtype=np.uint32)
    offsets = incl.astype(np.uint32)
    inst_tile, inst_id = [], []
    for j, (minx, maxx, miny, maxy) in enumerate(rects4):
        for y in range(miny, maxy):
            for x in range(minx, maxx):
                inst_tile.append(y * GX + x)
                inst_id.append(int(order[j]))
    inst_tile, inst_id = np.array(inst_tile, dtype=np.int64), np.array(inst_id, dtype=np.int64)
    ref_words = ((inst_id << LB) | (inst_tile & ((1 << LB) - 1)))[np.argsort(inst_tile >> LB, kind="stable")].astype(np.uint32)
    ref_list = inst_id[np.argsort(inst_tile, kind="stable")].astype(np.uint32)
    cnt = np.bincount(inst_tile, minlength=n_tiles)
    starts = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    ref_ranges = np.stack([np.where(cnt > 0, starts, 0), np.where(cnt > 0, starts + cnt, 0)], axis=1).astype(np.uint32)
    block_first = np.zeros((nblk + 2, 2), dtype=np.uint32)
    assert lib.simt_fill_block_first(P, ptr(offsets), ptr(block_first), nblk + 2) == 0, lib.simt_last_error()
    try:
        for generic in (0, 1):
            for pad in (1, 0):
                way = f"ranking_generic {generic}, ranking_pad_last {pad}"
                lib.simt_set_ranking(generic, pad)
                words = np.full(R, 0xFFFFFFFF, dtype=np.uint32)
                hist1 = np.zeros(nb1 * nblk, dtype=np.uint32)
                digit_total = np.zeros(nb1, dtype=np.uint32)
                bucket_base = np.zeros(nb1 + 1, dtype=np.uint32)
                blk2_start = np.zeros(nb1 + 1, dtype=np.uint32)
                splats = np.zeros((P, 16), dtype=np.float32)
                rc = lib.simt_level1(0, C.c_int64(R), GX, LB, HB, ptr(block_first), ptr(offsets), ptr(rect_sorted), ptr(order), ptr(words), ptr(hist1),
                                     ptr(digit_total), ptr(bucket_base), ptr(blk2_start), ptr(splats))
                assert rc == 0, lib.simt_last_error()
                assert np.array_equal(words, ref_words), f"{way}: packed words of level 1 differ"
                for scan_mode in (2, 1):
                    hist2 = np.zeros((nblk + 256 + nb1) * 256, dtype=np.uint32)
                    tile_base = np.zeros(65536, dtype=np.uint32)
                    point_list = np.full(R, 0xFFFFFFFF, dtype=np.uint32)
                    ranges = np.full((n_tiles, 2), 0xFFFFFFFF, dtype=np.uint32)
                    rc = lib.simt_level2(0, scan_mode, C.c_int64(R), n_tiles, LB, HB, ptr(words), ptr(bucket_base), ptr(blk2_start), ptr(hist2), ptr(tile_base),
                                         ptr(point_list), ptr(ranges))
                    assert rc == 0, lib.simt_last_error()
                    assert np.array_equal(point_list, ref_list), f"{way}, scan mode {scan_mode}: sorted point list differs"
                    assert np.array_equal(ranges, ref_ranges), f"{way}, scan mode {scan_mode}: tile ranges differ"
                assert lib.simt_last_ranking_widths() == (0 if generic else HB << 4 | LB), way
    finally:
        lib.simt_set_ranking(0, 1)
    return R, inst_tile


@pytest.mark.parametrize("on_last_row", [True, False], ids=["last_row", "first_row"])
@pytest.mark.parametrize("residue", RESIDUES + (None,), ids=[f"R%4096={r}" for r in RESIDUES] + ["R<64"])
def test_level1_padding_at_every_residue_of_the_instance_count(lib, residue, on_last_row):
    R, inst_tile = run_four_ways(lib, level1_case(residue, on_last_row))
    if residue is None:
        assert R == SMALL_R < 64
    else:
        assert R % TS_ITEMS == residue and R > TS_ITEMS
    last = inst_tile[(R - 1) // TS_ITEMS * TS_ITEMS:] >> LB      # buckets of the last emission block's real instances
    if on_last_row:
        assert int(last.max()) == (GX * GY - 1) >> LB and int(last[-1]) == (GX * GY - 1) >> LB
    else:
        assert int(last.max()) == 0


@pytest.mark.parametrize("extra", [0, 1], ids=["4096k", "4096k+1"])
def test_level2_padding_in_a_bucket_of_4096k_and_4096k_plus_1_words(lib, extra):
    R, inst_tile = run_four_ways(lib, level2_case(extra))
    in_bucket = inst_tile[inst_tile >> LB == LEVEL2_BUCKET]
    assert in_bucket.size % TS_ITEMS == extra and in_bucket.size >= TS_ITEMS
    assert int(in_bucket[-1]) & ((1 << LB) - 1) == (1 << LB) - 1, "the bucket's last word has the top low digit"
