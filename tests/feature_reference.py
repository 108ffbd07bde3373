"""Reference for the N-channel feature render (include/gsr.h gsr_render_features / gsr_render_features_backward), built on the oracle without touching it,
and the bars both test files hold the product to (tests/test_features_cpu.py on the SIMT build, tests/test_gpu_features.py on the MI355X).

Forward: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, the record of the shared walk
(tests/blend_reference.py: power / alpha / keep / Tincl / Texcl / dead), evaluated in fp64; w = alpha_eff * Texcl under keep & ~dead, and
F[c] = sum w f[:,c].  Pixels outside the band are 0.
Gradient: dL/df[:,c] = contrib_reference.reference(aux, s, E=G_c)["weight_sum"], channel by channel: the same sum with the upstream gradient of the
channel as the pixel weight (gradient_per_channel); gradient() computes those sums for all channels from one evaluation of a tile's weights.

Pixels of aux["fragile"] -- where a hard threshold sits inside rounding noise, the project's accepted notion -- are excluded from image comparisons and get
a zero upstream gradient in gradient tests (blend_reference.mask_fragile), for the product and the reference alike.

Bars, both the project's own (each measured distance is printed with helpers.parity_report under features_*):
  image      per channel within 1e-5 * max |f| absolute: a sum of blend weights (<= 1 in total) times values of at most max |f|, the image bar scaled;
  gradient   per channel within 1e-5 of max |reference| of that channel: the project's gradient bar;
  inputs     fragile pixels < 1 % of the frame (a condition on the scene, checked on the reference alone).
Test infrastructure."""
import torch

from helpers import parity_report
from blend_reference import mask_fragile, tiles  # noqa: F401  (mask_fragile: the tests reach it through this module)
import contrib_reference as CR


def _weights(t):
    """w[pixels, entries] of a tile's record: alpha_eff * Texcl under keep & ~dead."""
    return torch.where(t.keep & ~t.dead, t.alpha_eff * t.Texcl, torch.zeros_like(t.alpha))


def forward(aux, s, features, dtype=torch.float64):
    """-> F[C,H,W] in `dtype`."""
    f_all = features.detach().to(dtype)
    C = f_all.shape[1]
    F = torch.zeros(C, int(s.image_height), int(s.image_width), dtype=dtype)
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        F[:, yy0:yy1, x0:x1] = (_weights(t) @ f_all[t.ids]).T.reshape(C, yy1 - yy0, x1 - x0)
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
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        out.index_add_(0, t.ids, _weights(t).T @ G[:, yy0:yy1, x0:x1].reshape(C, -1).T)
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
