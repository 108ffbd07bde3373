"""Reference for the N-channel feature render (include/gsr.h gsr_render_features / gsr_render_features_backward), built on the oracle without touching it,
and the bars both test files hold the product to (tests/test_features_cpu.py on the SIMT build, tests/test_gpu_features.py on the MI355X).

Forward: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, power / alpha / keep / Tincl / Texcl / dead exactly as
tests/contrib_reference.py (and oracle/torch_oracle.py:_blend_tile) compute them, evaluated in fp64; w = alpha_eff * Texcl under keep & ~dead, and
F[c] = sum w f[:,c].  Pixels outside the band are 0.
Gradient: dL/df[:,c] = contrib_reference.reference(aux, s, E=G_c)["weight_sum"], channel by channel: the same sum with the upstream gradient of the
channel as the pixel weight (gradient_per_channel); gradient() computes those sums for all channels from one evaluation of a tile's weights.

Pixels of aux["fragile"] -- where a hard threshold sits inside rounding noise, the project's accepted notion -- are excluded from image comparisons and get
a zero upstream gradient in gradient tests (contrib_reference.mask_fragile), for the product and the reference alike.

Bars, both the project's own (each measured distance is printed with helpers.parity_report under features_*):
  image      per channel within 1e-5 * max |f| absolute: a sum of blend weights (<= 1 in total) times values of at most max |f|, the image bar scaled;
  gradient   per channel within 1e-5 of max |reference| of that channel: the project's gradient bar;
  inputs     fragile pixels < 1 % of the frame (a condition on the scene, checked on the reference alone).
Test infrastructure."""
import torch

from helpers import O, parity_report
import contrib_reference as CR

TILE = 16
mask_fragile = CR.mask_fragile


def _tiles(aux, s, dtype):
    """Per tile of the band with a non-empty range: (ids, pixel window, w[pixels, entries]) with w = alpha_eff * Texcl under keep & ~dead."""
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
        alpha = torch.clamp(opac[None, :] * torch.exp(power), max=O.ALPHA_MAX)
        keep = (power <= 0) & (alpha >= O.ALPHA_MIN)
        alpha_eff = torch.where(keep, alpha, torch.zeros_like(alpha))
        Tincl = torch.cumprod(1.0 - alpha_eff, dim=1)
        Texcl = torch.cat([torch.ones(n, 1, dtype=dtype), Tincl[:, :-1]], dim=1)
        term = keep & (Tincl < O.T_EPS)
        dead = torch.cumsum(term.to(torch.int32), dim=1) > 0
        yield ids, (yy0, yy1, x0, x1), torch.where(keep & ~dead, alpha_eff * Texcl, torch.zeros_like(alpha))


def forward(aux, s, features, dtype=torch.float64):
    """-> F[C,H,W] in `dtype`."""
    f_all = features.detach().to(dtype)
    C = f_all.shape[1]
    F = torch.zeros(C, int(s.image_height), int(s.image_width), dtype=dtype)
    for ids, (yy0, yy1, x0, x1), w in _tiles(aux, s, dtype):
        F[:, yy0:yy1, x0:x1] = (w @ f_all[ids]).T.reshape(C, yy1 - yy0, x1 - x0)
    return F


def gradient_per_channel(aux, s, G, dtype=torch.float64):
    """The definition: dL/dfeatures[:,c] is contrib_reference's weight_sum with the channel's upstream gradient as the pixel weight."""
    return torch.stack([CR.reference(aux, s, E=G[c], dtype=dtype)["weight_sum"] for c in range(G.shape[0])], dim=1)


def gradient(aux, s, G, dtype=torch.float64):
    """-> dL/dfeatures [P,C] in `dtype` for the upstream gradient G[C,H,W] (mask its fragile pixels first): gradient_per_channel's sums with the weights
    of a tile evaluated once for all channels (tests/test_features_cpu.py holds the two to each other at fp64 rounding)."""
    G = G.detach().to(dtype)
    C = G.shape[0]
    out = torch.zeros(aux["means2D"].shape[0], C, dtype=dtype)
    for ids, (yy0, yy1, x0, x1), w in _tiles(aux, s, dtype):
        out.index_add_(0, ids, w.T @ G[:, yy0:yy1, x0:x1].reshape(C, -1).T)
    return out


def check_input(aux):
    frag = float(aux["fragile"].float().mean())
    assert frag < 0.01, frag
    return frag


def check_image(key, got, ref, aux, f_absmax):
    """The image bar on F `got` [C,H,W] against forward() output `ref`, outside aux["fragile"]; returns the measured numbers."""
    frag = check_input(aux)
    ok = ~aux["fragile"]
    g = got.detach().cpu().double()
    assert got.dtype == torch.float32 and g.shape == ref.shape
    err = (g - ref.double()).abs()[:, ok].amax(dim=1)
    nums = dict(image_abs_max=float(err.max()), image_abs_max_over_fmax=float(err.max()) / f_absmax, f_absmax=f_absmax, channels=int(g.shape[0]),
                fragile_share=frag)
    parity_report(key, **nums)
    assert float(ref.abs().max()) > 0.0
    assert bool((err <= 1e-5 * f_absmax).all()), nums
    return nums


def check_gradient(key, got, ref, aux):
    """The gradient bar on dL/dfeatures `got` [P,C] against gradient() output `ref`; returns the measured numbers."""
    frag = check_input(aux)
    g = got.detach().cpu().double()
    assert got.dtype == torch.float32 and g.shape == ref.shape
    scale = ref.double().abs().amax(dim=0)
    assert bool((scale > 0).all())
    rel = (g - ref.double()).abs().amax(dim=0) / scale
    nums = dict(grad_rel_max=float(rel.max()), channels=int(g.shape[1]), fragile_share=frag)
    parity_report(key, **nums)
    assert bool((rel < 1e-5).all()), nums
    return nums
