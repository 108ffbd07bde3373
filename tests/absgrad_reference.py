"""Reference for the absolute screen-space gradients (include/gsr.h gsr_backward_blend_abs), built on the oracle without touching it, and the bars both
test files hold the product to (tests/test_absgrad_cpu.py on the SIMT build, tests/test_gpu_absgrad.py on the MI355X).

Reference: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, the record of the shared walk
(tests/blend_reference.py: power / alpha / keep / Tincl / Texcl / dead), evaluated in fp64.  For the contributors i of a pixel (keep & ~dead), with
s_i = <c_i, dL/dC> + dL/dD / depth_i, w_i = alpha_i T_i, T_final the product of (1 - alpha) over the contributors, B the background and dL/dA the gradient of
the alpha image 1 - T_final, the closed form of the blend's derivative with suffix sums:
    dL/dalpha_i = T_i s_i - (sum_{j>i} s_j w_j + T_final (<B, dL/dC> - dL/dA)) / (1 - alpha_i)
then m_i = opacity G_i dL/dalpha_i (the UNCAPPED opacity * G: the 0.99 cap is passed straight through), the per-pixel components
    ex = m (A dx + B dy),   ey = m (C dy + B dx)            (dx, dy) = mean2D - pixel
and index_add_ onto the Gaussians of |ex|, |ey| (the absolute gradient) and of -ex, -ey (the signed one), scaled by (0.5 W, 0.5 H): the units of means2D.grad.
The SIGNED sums are what the oracle's own autograd returns for means2D: check_signed holds them to it at the project's gradient bar before the reference
judges anything.  Pixels of aux["fragile"] get dL = 0 in the tests' inputs (mask_fragile), for the product and the reference alike.

Bars (each measured distance is printed with helpers.parity_report under absgrad_*):
  abs_x, abs_y   per Gaussian within 1e-5 of max |reference| per component: the project's gradient bar; the quantity has no cancellation;
  signed         reference vs the oracle's autograd: within 1e-5 of max |grad| per component;
  inputs         fragile pixels < 1 % of the frame.
Test infrastructure."""
import torch

from helpers import parity_report
from blend_reference import mask_fragile, tiles  # noqa: F401  (mask_fragile: the tests reach it through this module)

BAR = 1e-5


def reference(aux, s, dL_dC, dL_dD=None, dL_dA=None, bg=None, dtype=torch.float64):
    """dL_dC [3,H,W], dL_dD [H,W] / [1,H,W] or None, dL_dA (gradient of the alpha image) likewise, bg [3] or [3,H,W] (None: zeros)
    -> dict(abs [P,2], signed [P,2] in `dtype`, units of means2D.grad; pairs = number of contributing (pixel, Gaussian) pairs)."""
    W, H = int(s.image_width), int(s.image_height)
    P = aux["means2D"].shape[0]
    gC = dL_dC.detach().reshape(3, H, W).to(dtype)
    gD = torch.zeros(H, W, dtype=dtype) if dL_dD is None else dL_dD.detach().reshape(H, W).to(dtype)
    gA = torch.zeros(H, W, dtype=dtype) if dL_dA is None else dL_dA.detach().reshape(H, W).to(dtype)
    bg = torch.zeros(3) if bg is None else bg.detach()
    Bimg = (bg.reshape(3, 1, 1).expand(3, H, W) if bg.dim() == 1 else bg).to(dtype)
    bgdot = (Bimg * gC).sum(0) - gA                                  # <B, dL/dC> - dL/dA
    rgb_all = aux["rgb"].detach().to(dtype)
    invd_all = 1.0 / aux["depths"].detach().to(dtype)
    ab, sg = torch.zeros(P, 2, dtype=dtype), torch.zeros(P, 2, dtype=dtype)
    pairs = 0
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        ids, dx, dy, A, B, Cc, Texcl, dead = t.ids, t.dx, t.dy, t.A, t.B, t.Cc, t.Texcl, t.dead
        contrib = t.keep & ~dead
        first_dead = torch.argmax(dead.to(torch.int8), dim=1)
        T_final = torch.where(dead[:, -1], torch.gather(Texcl, 1, first_dead[:, None])[:, 0], t.Tincl[:, -1])
        gc = gC[:, yy0:yy1, x0:x1].reshape(3, -1)                       # [3, n]
        s_i = (rgb_all[ids] @ gc).T + invd_all[ids][None, :] * gD[yy0:yy1, x0:x1].reshape(-1)[:, None]      # [n, N]
        w = torch.where(contrib, t.alpha_eff * Texcl, torch.zeros_like(t.alpha))
        sw = s_i * w
        suffix = torch.flip(torch.cumsum(torch.flip(sw, dims=[1]), dim=1), dims=[1]) - sw                  # sum_{j>i} s_j w_j
        tail = (T_final * bgdot[yy0:yy1, x0:x1].reshape(-1))[:, None]
        dL_dalpha = Texcl * s_i - (suffix + tail) / (1.0 - t.alpha_eff)
        m = torch.where(contrib, t.a_raw * dL_dalpha, torch.zeros_like(t.alpha))
        ex = m * (A * dx + B * dy)
        ey = m * (Cc * dy + B * dx)
        ab.index_add_(0, ids, torch.stack([ex.abs().sum(0), ey.abs().sum(0)], dim=1))
        sg.index_add_(0, ids, -torch.stack([ex.sum(0), ey.sum(0)], dim=1))
        pairs += int(contrib.sum())
    scale = torch.tensor([0.5 * W, 0.5 * H], dtype=dtype)
    return dict(abs=ab * scale, signed=sg * scale, pairs=pairs)


def check_signed(key, ref, oracle_means2D_grad):
    """The reference's signed sums against the oracle's own autograd gradient of means2D: 1e-5 of max |grad| per component."""
    want = oracle_means2D_grad.detach().double()[:, :2]
    d = [float((ref["signed"][:, k] - want[:, k]).abs().max()) / float(want[:, k].abs().max()) for k in (0, 1)]
    parity_report(key, signed_vs_autograd_x=d[0], signed_vs_autograd_y=d[1])
    assert max(d) < BAR, d
    return d


def check(key, got_abs, got_grad, ref, aux):
    """The bars of the module docstring on means2D.absgrad `got_abs` [P,3] (and the package's own means2D.grad `got_grad`, reported against the
    reference's signed sums) against reference() output `ref`; returns the measured numbers."""
    frag = float(aux["fragile"].float().mean())
    ga = got_abs.detach().cpu().double()
    assert got_abs.dtype == torch.float32 and tuple(got_abs.shape) == (ref["abs"].shape[0], 3)
    scale = [float(ref["abs"][:, k].max()) for k in (0, 1)]
    assert min(scale) > 0.0 and ref["pairs"] > 0
    d_abs = [float((ga[:, k] - ref["abs"][:, k]).abs().max()) / scale[k] for k in (0, 1)]
    nums = dict(abs_x_rel_max=d_abs[0], abs_y_rel_max=d_abs[1], fragile_share=frag, pairs=ref["pairs"],
                cancellation=float(ref["signed"].abs().sum()) / float(ref["abs"].sum()))
    if got_grad is not None:
        gg = got_grad.detach().cpu().double()
        nums.update(signed_x_rel_max=float((gg[:, 0] - ref["signed"][:, 0]).abs().max()) / float(ref["signed"][:, 0].abs().max()),
                    signed_y_rel_max=float((gg[:, 1] - ref["signed"][:, 1]).abs().max()) / float(ref["signed"][:, 1].abs().max()))
    parity_report(key, **nums)
    assert frag < 0.01, frag
    assert float(ga[:, 2].abs().max()) == 0.0 and float(ga.min()) >= 0.0
    assert max(d_abs) < BAR, nums
    return nums
