"""The one walk of a frame's tile lists that the references of its readers share (tests/contrib_reference.py, probe_reference.py, absgrad_reference.py,
feature_reference.py), built on the oracle without touching it: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band,
power / alpha / keep / Tincl / Texcl / dead exactly as oracle/torch_oracle.py:_blend_tile computes them, evaluated in `dtype` (the references: fp64).
tests/test_blend_reference_cpu.py holds the walk itself to a hand-computed frame.
Test infrastructure."""
from types import SimpleNamespace

import torch

from helpers import O

TILE = 16


def mask_fragile(w, aux):
    """A per-pixel weight [..., H, W] with the fragile pixels -- where a hard threshold sits inside rounding noise, the project's accepted notion -- zeroed."""
    w = w.clone()
    w[..., aux["fragile"]] = 0.0
    return w


def tiles(aux, s, dtype):
    """Per tile of the band with a non-empty range, one record: ids [N] (the tile's list, front to back: column j of every array below is list POSITION j,
    the Gaussian is ids[j]), window = (yy0, yy1, x0, x1) (its n pixels, row-major, are the rows), and in `dtype`, [n, N] unless noted:
    dx, dy (mean2D - pixel), A, B, Cc (the conic, [1, N]), power, a_raw (opacity * G, uncapped), alpha (capped at 0.99), keep, alpha_eff (alpha under keep,
    else 0), Tincl / Texcl (T after / before the entry), term (the entry that takes T below 1e-4), dead (term or behind it)."""
    W, H = int(s.image_width), int(s.image_height)
    gx, _ = aux["grid"]
    y0, y1 = aux["band"]
    xy_all, conic_all, op_all = (aux[k].detach().to(dtype) for k in ("means2D", "conic", "opacity"))
    op_all = op_all.reshape(-1)
    for t in range(y0 * gx, y1 * gx):
        tyi, txi = divmod(int(t), gx)
        x0, yy0 = txi * TILE, tyi * TILE
        x1, yy1 = min(x0 + TILE, W), min(yy0 + TILE, H)
        a, b = int(aux["ranges"][t, 0]), int(aux["ranges"][t, 1])
        if b <= a:
            continue
        ids = aux["point_list"][a:b].long()
        ys, xs = torch.meshgrid(torch.arange(yy0, yy1), torch.arange(x0, x1), indexing="ij")
        px, py = xs.reshape(-1).to(dtype), ys.reshape(-1).to(dtype)
        n = px.shape[0]
        xy, conic, opac = xy_all[ids], conic_all[ids], op_all[ids]
        dx = xy[None, :, 0] - px[:, None]
        dy = xy[None, :, 1] - py[:, None]
        A, B, Cc = conic[None, :, 0], conic[None, :, 1], conic[None, :, 2]
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        a_raw = opac[None, :] * torch.exp(power)
        alpha = torch.clamp(a_raw, max=O.ALPHA_MAX)
        keep = (power <= 0) & (alpha >= O.ALPHA_MIN)
        alpha_eff = torch.where(keep, alpha, torch.zeros_like(alpha))
        Tincl = torch.cumprod(1.0 - alpha_eff, dim=1)
        Texcl = torch.cat([torch.ones(n, 1, dtype=dtype), Tincl[:, :-1]], dim=1)
        term = keep & (Tincl < O.T_EPS)
        dead = torch.cumsum(term.to(torch.int32), dim=1) > 0
        yield SimpleNamespace(ids=ids, window=(yy0, yy1, x0, x1), n=n, dx=dx, dy=dy, A=A, B=B, Cc=Cc, power=power, a_raw=a_raw, alpha=alpha, keep=keep,
                              alpha_eff=alpha_eff, Tincl=Tincl, Texcl=Texcl, term=term, dead=dead)


def near_threshold(tile):
    """[n, N] bool: a pair the sequential loop evaluates (not behind the terminating entry) has alpha within 1e-4 relative of 1/255 or T (after it) within
    1e-4 relative of 1e-4 -- where a discrete output may legitimately differ between fp32 and fp64."""
    live = ~tile.dead | tile.term
    near_a = (tile.alpha - O.ALPHA_MIN).abs() < 1e-4 * O.ALPHA_MIN
    near_t = tile.keep & ((tile.Tincl - O.T_EPS).abs() < 1e-4 * O.T_EPS)
    return (near_a | near_t) & live
