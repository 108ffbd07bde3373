"""Reference for the per-Gaussian blend-weight statistics (include/gsr.h gsr_contribution_stats), built on the oracle without touching it, and
the bars both test files hold the product to (tests/test_contrib_cpu.py on the SIMT build, tests/test_gpu_contrib.py on the MI355X).

Reference: from `aux` of O.rasterize(..., want_fragile=True, return_aux=True), per tile of the band, the record of the shared walk
(tests/blend_reference.py: power / alpha / keep / Tincl / Texcl / dead), evaluated in fp64; contrib = keep & ~dead & (E != 0), w = alpha * Texcl * E, scattered onto the
Gaussians (index_add_ of the sums and counts, amax onto a zero vector).  Pixels of aux["fragile"] -- where a hard threshold sits inside rounding
noise, the project's accepted notion -- get E = 0 in the tests' inputs (mask_fragile), for the product and the reference alike.

Bars (each measured distance is printed with helpers.parity_report under contrib_*):
  weight_sum   per Gaussian within 1e-5 of max |reference|: the quantity is the colour gradient dL/dcolors_precomp[:,0] of sum E C_0, and this is
               the project's gradient bar;
  weight_max   within 1e-5 absolute for max |E| <= 1: one blend weight times E, the image bar;
  pixel_count  equal.  A mismatching Gaussian is a finding and is reported; it is acceptable only if, in fp64, one of its evaluated pairs has alpha or T
               within 1e-4 relative of its threshold (1/255, 1e-4), and more than 1 mismatching Gaussian per 1000 contributing ones fails;
  inputs       fragile pixels < 1 % of the frame.
Test infrastructure."""
import torch

from helpers import parity_report
from blend_reference import mask_fragile, near_threshold, tiles  # noqa: F401  (mask_fragile: the tests reach it through this module)


def raise_opacity(opacities, logits=3.0):
    """Post-sigmoid opacities with their logits raised: dense frames whose pixels terminate."""
    return torch.sigmoid(torch.logit(opacities.double()) + logits).float()


def reference(aux, s, E=None, dtype=torch.float64):
    """-> dict(weight_sum[P], weight_max[P] in `dtype`, pixel_count[P] int64, near[P] bool: a pair of the Gaussian that the sequential loop evaluates at a
    pixel with E != 0 has alpha within 1e-4 relative of 1/255 or T (after it) within 1e-4 relative of 1e-4, terminated [H,W] bool, longest list)."""
    W, H = int(s.image_width), int(s.image_height)
    P = aux["means2D"].shape[0]
    E = torch.ones(H, W, dtype=dtype) if E is None else E.detach().reshape(H, W).to(dtype)
    wsum, wmax = torch.zeros(P, dtype=dtype), torch.zeros(P, dtype=dtype)
    count, near = torch.zeros(P, dtype=torch.int64), torch.zeros(P, dtype=torch.int64)
    terminated = torch.zeros(H, W, dtype=torch.bool)
    longest = 0
    for t in tiles(aux, s, dtype):
        yy0, yy1, x0, x1 = t.window
        longest = max(longest, t.ids.shape[0])
        e = E[yy0:yy1, x0:x1].reshape(-1)
        on = (e != 0)[:, None]
        contrib = t.keep & ~t.dead & on
        w = torch.where(contrib, t.alpha_eff * t.Texcl * e[:, None], torch.zeros_like(t.alpha))
        wsum.index_add_(0, t.ids, w.sum(0))
        count.index_add_(0, t.ids, contrib.sum(0))
        wmax.scatter_reduce_(0, t.ids, w.max(0).values, reduce="amax", include_self=True)
        near.index_add_(0, t.ids, (near_threshold(t) & on).sum(0))
        terminated[yy0:yy1, x0:x1] = t.dead[:, -1].reshape(yy1 - yy0, x1 - x0)
    return dict(weight_sum=wsum, weight_max=wmax, pixel_count=count, near=near > 0, terminated=terminated, longest=longest)


def check(key, got, ref, aux, E_absmax=1.0):
    """The bars of the module docstring on a ContributionStats `got` against reference() output `ref`; returns the measured numbers."""
    frag = float(aux["fragile"].float().mean())
    gs, gm, gc = got.weight_sum.detach().cpu().double(), got.weight_max.detach().cpu().double(), got.pixel_count.detach().cpu().long()
    scale = float(ref["weight_sum"].abs().max())
    d_sum = float((gs - ref["weight_sum"]).abs().max()) / scale
    d_max = float((gm - ref["weight_max"]).abs().max())
    bad = gc != ref["pixel_count"]
    n_bad, n_contrib = int(bad.sum()), int((ref["pixel_count"] > 0).sum())
    unexplained = int((bad & ~ref["near"]).sum())
    nums = dict(sum_rel_max=d_sum, max_abs=d_max, count_mismatch=n_bad, count_mismatch_unexplained=unexplained, contributing=n_contrib,
                fragile_share=frag, terminated_share=float(ref["terminated"].float().mean()), longest_list=ref["longest"])
    parity_report(key, **nums)
    assert frag < 0.01, frag
    assert E_absmax <= 1.0
    assert got.weight_sum.dtype == torch.float32 and got.weight_max.dtype == torch.float32 and got.pixel_count.dtype == torch.int32
    assert n_contrib > 0 and scale > 0.0
    assert d_sum < 1e-5, nums
    assert d_max < 1e-5, nums
    assert float(gm.min()) >= 0.0
    assert unexplained == 0 and n_bad * 1000 <= n_contrib, nums
    return nums
