"""Frames for the padding tests of the tile sort's ranking kernels (csrc/tilesort.hip, option ranking_pad_last): scenes whose instance count R, or
whose number of words in one level-1 bucket, is steered to a chosen residue modulo the 4096 slots of a workgroup.

The steering appends ONE-TILE Gaussians (a tiny isotropic splat centred in a tile: one instance each, whatever the rectangle rule) BEHIND every
Gaussian of the base scene, so they are the last instances of the emission order and of every bucket they fall into.  There are always at least 4096
of them, so the frame's last emission block (and the steered bucket's last level-2 block) holds nothing else.  Shared by
tests/test_gpu_ranking_padding.py; tests/test_simt_ranking_padding_cpu.py builds the same cases from rectangles (it drives the kernels directly)."""
import torch

from helpers import O, make_camera, make_scene, oracle_settings
from gsr_synth import Scene

TS_ITEMS = 4096
RESIDUES = (0, 1, 63, 64, 65, 4095)
SMALL_R = 37                      # the "R < 64" frame: a single wave's first item, partly filled
FILL_Z = 20.0                     # the base scenes end at z = 12


def plan(W, H):
    """(gx, gy, n_tiles, lb, hb) as gsr_tile_sort_plan splits the tile id."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nbits = 1
    while (1 << nbits) < gx * gy:
        nbits += 1
    lb = (nbits + 1) // 2
    return gx, gy, gx * gy, lb, nbits - lb


def one_tile_gaussians(cam, tiles):
    """One Gaussian per entry of `tiles` (tile ids, in this order = index order = depth-tie order), centred in its tile at depth FILL_Z."""
    W, H = cam.image_width, cam.image_height
    gx = (W + 15) // 16
    tiles = torch.as_tensor(tiles, dtype=torch.int64)
    tx, ty = tiles % gx, tiles // gx
    cx = (16 * tx + torch.clamp(16 * tx + 16, max=W) - 1).double() / 2      # centre of the tile's pixels
    cy = (16 * ty + torch.clamp(16 * ty + 16, max=H) - 1).double() / 2
    ndc_x, ndc_y = (2 * cx + 1) / W - 1, (2 * cy + 1) / H - 1               # pix = ((ndc + 1) * S - 1) / 2
    n = tiles.numel()
    means = torch.stack([ndc_x * FILL_Z * cam.tanfovx, ndc_y * FILL_Z * cam.tanfovy, torch.full((n,), FILL_Z, dtype=torch.float64)], dim=1).float()
    g = torch.Generator().manual_seed(1234)
    shs = torch.randn(n, 16, 3, generator=g) * 0.1
    rot = torch.zeros(n, 4)
    rot[:, 0] = 1.0
    return Scene(means.contiguous(), torch.full((n, 3), 1e-4), rot, torch.full((n, 1), 0.8), shs.contiguous(), 3, {})


def concat(a, b):
    return Scene(torch.cat([a.means3D, b.means3D]), torch.cat([a.scales, b.scales]), torch.cat([a.rotations, b.rotations]),
                 torch.cat([a.opacities, b.opacities]), torch.cat([a.shs, b.shs]), a.sh_degree, {})


def oracle_bins(cam, sc):
    s = oracle_settings(cam)
    with torch.no_grad():
        pre = O.preprocess(sc.means3D, sc.opacities, s, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
        bins = O.bin_and_sort(pre)
    return pre, bins


_base = {}


def base_frame(W, H, P):
    """(camera, base scene, its instance count, its instances per tile) -- computed once per frame size."""
    if (W, H) not in _base:
        cam = make_camera(W, H)
        sc = make_scene(P, cam, seed=3, s_med=0.03)
        _, bins = oracle_bins(cam, sc)
        rg = bins["ranges"].view(-1, 2)
        _base[(W, H)] = (cam, sc, int(bins["R"]), (rg[:, 1] - rg[:, 0]).clone())
    return _base[(W, H)]


def level1_frame(W, H, P, residue, on_last_row):
    """R == residue (mod 4096), or R == SMALL_R when residue is None.  on_last_row: the one-tile Gaussians sit on the frame's last tile row (the highest
    bucket that exists, the top digit itself where the frame has tiles of it), else on the first row (bucket 0)."""
    gx, gy, n_tiles, lb, hb = plan(W, H)
    row = gy - 1 if on_last_row else 0
    ncol = gx if on_last_row else min(gx, 1 << lb)      # (first row: the tiles of bucket 0 only)

    def tiles(n):      # cycling over the row's columns so that the LAST Gaussian -- the frame's last instance -- lies on the last of them
        return row * gx + (ncol - 1 - (n - 1 - torch.arange(n)) % ncol)

    if residue is None:
        cam = make_camera(W, H)
        return cam, one_tile_gaussians(cam, tiles(SMALL_R))
    cam, base, R0, _ = base_frame(W, H, P)
    n = (residue - R0) % TS_ITEMS + TS_ITEMS
    return cam, concat(base, one_tile_gaussians(cam, tiles(n)))


LEVEL2_BUCKET = 3


def level2_frame(W, H, P, extra):
    """Bucket LEVEL2_BUCKET holds 4096 k + extra words; its last word (the deepest instance) belongs to the bucket's last tile, the top low digit."""
    gx, gy, n_tiles, lb, hb = plan(W, H)
    cam, base, _, per_tile = base_frame(W, H, P)
    nb2 = 1 << lb
    t0 = LEVEL2_BUCKET << lb
    assert t0 + nb2 <= n_tiles
    c0 = int(per_tile[t0:t0 + nb2].sum())
    n = (extra - c0) % TS_ITEMS + TS_ITEMS
    return cam, concat(base, one_tile_gaussians(cam, t0 + (torch.arange(n) - n) % nb2))
