"""Reference for the geometry / opacity gradients through the N-channel feature render (include/gsr.h gsr_render_features_backward_geometry), built on
the oracle without touching it, and the bars the test files hold the product to (tests/test_feature_geometry_cpu.py on the SIMT build,
tests/test_gpu_feature_geometry.py on the MI355X).

Reference: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, the record of the shared walk
(tests/blend_reference.py: power / alpha / keep / Tincl / Texcl / dead), evaluated in fp64 the way tests/absgrad_reference.py does.  For the contributors
i of a pixel (contrib = keep & ~dead), with G the upstream gradient dL/dF [C,H,W] and f the features [P,C]:
    s        = (f[ids] @ G_tile).T                       <feature row, dL/dF> per (pixel, entry)
    w        = alpha_eff * Texcl                         under contrib
    suffix   = reversed cumsum of s w, minus s w         sum_{j>i} s_j w_j
    dL/dalpha = Texcl s - suffix / (1 - alpha_eff)       (no background / T_final term: F has none)
    m        = a_raw dL/dalpha                           under contrib (the UNCAPPED opacity * G: the 0.99 cap is passed straight through)
and index_add_ onto the Gaussians of the six sums of the [P,12] records' words 0..5 (pixel units, (dx, dy) = mean2D - pixel, conic (A, B, C)):
    sum m (-A dx - B dy), sum m (-C dy - B dx), -1/2 sum m dx^2, -sum m dx dy, -1/2 sum m dy^2, sum G dL/dalpha  (G = a_raw / opacity).
Pixels of aux["fragile"] get dL = 0 in the tests' inputs (mask_fragile), for the product and the reference alike; the condition on the inputs is the
project's: fragile share < 1 %.

check_reference holds the reference itself to the oracle's autograd before it judges anything: the composed oracle renders the channels three at a time
through colors_precomp with bg = 0 (the last triple padded with zero columns), loss = sum <colour, G triple>, fp64 leaves; words 0, 1 scaled by
(0.5 W, 0.5 H) against its means2D.grad and word 5 against its opacity gradient, within REF_BAR = 2e-5 of max |grad|.  The distance is the fp32 rounding
of the frame's means2D / conic inside `aux` (measured 7.0e-6 / 1.2e-6 and 8.5e-6 / 3.5e-6 on the two prototype frames, C = 5), hence the factor 2.

Bars on the product (each measured distance is printed with helpers.parity_report under feature_geometry_*):
  records    words 0..5 within BAR = 1e-5 of the reference's max per word: the project's gradient bar; words 6..11 exact zeros.
Test infrastructure."""
import torch

from helpers import O, parity_report
from blend_reference import mask_fragile, tiles  # noqa: F401  (mask_fragile: the tests reach it through this module)

BAR = 1e-5
REF_BAR = 2e-5


def reference(aux, s, features, G, dtype=torch.float64):
    """features [P,C], G = dL/dF [C,H,W] (mask its fragile pixels first) -> dict(records [P,6] in `dtype`, pairs = contributing (pixel, Gaussian) pairs)."""
    W, H = int(s.image_width), int(s.image_height)
    P = aux["means2D"].shape[0]
    f_all = features.detach().to(dtype)
    C = f_all.shape[1]
    G = G.detach().reshape(C, H, W).to(dtype)
    op_all = aux["opacity"].detach().to(dtype).reshape(-1)
    rec = torch.zeros(P, 6, dtype=dtype)
    pairs = 0
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        ids, dx, dy, A, B, Cc, Texcl = t.ids, t.dx, t.dy, t.A, t.B, t.Cc, t.Texcl
        contrib = t.keep & ~t.dead
        zero = torch.zeros_like(t.alpha)
        s_i = (f_all[ids] @ G[:, yy0:yy1, x0:x1].reshape(C, -1)).T                                          # [n, N]
        w = torch.where(contrib, t.alpha_eff * Texcl, zero)
        sw = torch.where(contrib, s_i, zero) * w
        suffix = torch.flip(torch.cumsum(torch.flip(sw, dims=[1]), dim=1), dims=[1]) - sw                  # sum_{j>i} s_j w_j
        dL_dalpha = torch.where(contrib, Texcl * s_i - suffix / (1.0 - t.alpha_eff), zero)
        m = torch.where(contrib, t.a_raw * dL_dalpha, zero)
        Gs = torch.where(contrib, t.a_raw / op_all[ids][None, :] * dL_dalpha, zero)
        rec.index_add_(0, ids, torch.stack([(m * (-A * dx - B * dy)).sum(0), (m * (-Cc * dy - B * dx)).sum(0), -0.5 * (m * dx * dx).sum(0),
                                            -(m * dx * dy).sum(0), -0.5 * (m * dy * dy).sum(0), Gs.sum(0)], dim=1))
        pairs += int(contrib.sum())
    return dict(records=rec, pairs=pairs)


def composed_oracle(cam, lv, form, features, G, aa=False):
    """The composed oracle: the channels three at a time through colors_precomp with bg = 0, loss = sum <colour, G triple>, on fp64 copies of the leaves
    `lv` (tests/test_composite_cpu.make_leaves) and of `features` -> dict of gradients (means2D in the units of means2D.grad; features [P,C])."""
    import test_composite_cpu as T
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, aa)
    keys = ("means", "opac", "cov") if form == "precomp" else ("means", "opac", "scales", "rot")
    leaves = {k: lv[k].detach().double().requires_grad_(True) for k in keys}
    f = features.detach().double().requires_grad_(True)
    P, C = f.shape
    m2 = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    kw = {k: v for k, v in T.call_kwargs({**leaves, "colors": None, "shs": None}, form, oracle=True).items() if k not in ("shs", "colors_precomp", "means2D")}
    G = G.detach().double()
    loss = 0.0
    for c0 in range(0, C, 3):
        n = min(3, C - c0)
        cols = torch.cat([f[:, c0:c0 + n], torch.zeros(P, 3 - n, dtype=torch.float64)], dim=1)
        colour = O.rasterize(s=s0, means2D=m2, colors_precomp=cols, **kw)[0]
        loss = loss + (colour[:n] * G[c0:c0 + n]).sum()
    loss.backward()
    out = {k: v.grad for k, v in leaves.items()}
    out.update(means2D=m2.grad, features=f.grad)
    return out


def check_reference(key, ref, oracle, aux, s):
    """The reference's words 0, 1 (scaled to the units of means2D.grad) and 5 against the composed oracle's autograd: REF_BAR of max |grad|."""
    W, H = int(s.image_width), int(s.image_height)
    rec = ref["records"]
    want2, wanto = oracle["means2D"].double(), oracle["opac"].double().reshape(-1)
    got2 = rec[:, :2] * torch.tensor([0.5 * W, 0.5 * H], dtype=rec.dtype)
    got_o = rec[:, 5]      # (frames without antialiasing: word 5 is dL/d(opacity * aa factor))
    d2 = float((got2 - want2[:, :2]).abs().max()) / float(want2[:, :2].abs().max())
    do = float((got_o - wanto).abs().max()) / float(wanto.abs().max())
    frag = float(aux["fragile"].float().mean())
    parity_report(key, means2D_vs_autograd=d2, opacity_vs_autograd=do, fragile_share=frag, pairs=ref["pairs"])
    assert frag < 0.01, frag
    assert d2 < REF_BAR and do < REF_BAR, (d2, do)
    return d2, do


def check_records(key, got, ref, aux):
    """The bars of the module docstring on the [P,12] records `got` against reference() output `ref`; returns the measured numbers."""
    frag = float(aux["fragile"].float().mean())
    g = got.detach().cpu().double()
    want = ref["records"]
    assert got.dtype == torch.float32 and tuple(g.shape) == (want.shape[0], 12)
    scale = want.abs().amax(dim=0)
    assert bool((scale > 0).all()) and ref["pairs"] > 0
    rel = (g[:, :6] - want).abs().amax(dim=0) / scale
    names = ("px", "py", "A", "B", "C", "opacity")
    nums = {f"{n}_rel_max": float(rel[k]) for k, n in enumerate(names)}
    nums.update(fragile_share=frag, pairs=ref["pairs"])
    parity_report(key, **nums)
    assert frag < 0.01, frag
    assert float(g[:, 6:].abs().max()) == 0.0
    assert float(g[want.abs().amax(dim=1) == 0].abs().sum()) == 0.0      # rows without a contributing pixel
    assert bool((rel < BAR).all()), nums
    return nums
