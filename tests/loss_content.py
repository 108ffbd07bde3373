"""Image content for the loss-kernel tests (csrc/ssim.hip), shared by the CPU-shim and the GPU tests, and the bars both hold the kernels to.

Uniform noise against noisy noise has large local variances, so sigma^2 = E[x^2] - mu^2 loses nothing in fp32.  Rendered images and photographs
are smooth (sigma^2 << mu^2: the subtraction cancels) and the rendered image is not clamped to [0, 1].  `pair(name, shape)` returns the named
(prediction, target) pair as fp32 CPU tensors, deterministic in (name, shape).

Bars.  E = max over EVERY pixel of |kernel - fp64 oracle|:
    gradient: E <= max(2e-5 max|grad|, 1.5 x the distance of the oracle evaluated in fp32 from the oracle evaluated in fp64)
    value   : |v - v64| <= max(2e-6, 1.5 x |v32 - v64|)
The fp32 term comes from the reference alone (oracle.losses on the same inputs), never from the kernel; 1.5 is the factor the needle scenes
use.  `identical` has a true gradient of zero: |grad| <= 2e-5 g_ref with g_ref the oracle's max|grad| for `smooth_plus_noise` at the same
shape, and the value within 2e-6 of the oracle's (0 for the loss, 1 for SSIM).  Test infrastructure."""
import math

import torch

NAMES = ("noise", "smooth_plus_noise", "smooth_target_noisy_prediction", "constants", "identical", "unclamped_prediction",
         "black_prediction", "saturated", "edges")


def smooth(shape):
    """A smooth analytic image in [0.15, 0.85]: a few periods across the frame, another phase in every plane."""
    H, W = shape[-2], shape[-1]
    planes = 1
    for s in shape[:-2]:
        planes *= s
    y = torch.linspace(0.0, 1.0, H, dtype=torch.float64)[:, None] if H > 1 else torch.zeros(1, 1, dtype=torch.float64)
    x = torch.linspace(0.0, 1.0, W, dtype=torch.float64)[None, :] if W > 1 else torch.zeros(1, 1, dtype=torch.float64)
    out = torch.empty((planes, H, W), dtype=torch.float64)
    for p in range(planes):
        out[p] = 0.5 + 0.22 * torch.sin(2 * math.pi * (1.5 * x + 0.13 * p)) * torch.cos(2 * math.pi * 1.1 * y + 0.4 * p) \
            + 0.18 * (x - 0.5) * (y + 0.3)
    return out.reshape(shape).float()


def _gen(name, shape):
    return torch.Generator().manual_seed(1000 * NAMES.index(name) + shape[-1] + 7 * shape[-2])


def pair(name, shape):
    """(prediction, target), fp32 on the CPU.  Gradients are taken with respect to the prediction."""
    shape = tuple(shape)
    g = _gen(name, shape)
    H, W = shape[-2], shape[-1]
    if name == "noise":                                   # what the suite had: large variances everywhere
        a = torch.rand(shape, generator=g)
        b = (a + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
        if H > 3 or W > 5:                                # (not the whole image: that is the `identical` class)
            b[..., :3, :5] = a[..., :3, :5]               # exact ties: zero L1 gradient there
        return a, b
    if name == "smooth_plus_noise":
        a = smooth(shape)
        return a, a + 0.01 * torch.randn(shape, generator=g)
    if name == "smooth_target_noisy_prediction":
        b = smooth(shape)
        return b + 0.003 * torch.randn(shape, generator=g), b
    if name == "constants":
        return torch.full(shape, 0.7), torch.full(shape, 0.4)
    if name == "identical":
        a = smooth(shape) + 0.01 * torch.randn(shape, generator=g)
        return a, a.clone()
    if name == "unclamped_prediction":                    # the rendered image is not clamped: about [-0.3, 1.3]
        b = torch.rand(shape, generator=g)
        a = 0.5 + 1.6 * (b - 0.5) + 0.02 * torch.randn(shape, generator=g)
        return a, b
    if name == "black_prediction":
        return torch.zeros(shape), (smooth(shape) + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    if name == "saturated":                               # large regions at exactly 0 and exactly 1 in BOTH images
        s = 0.5 + 3.0 * (smooth(shape) - 0.5)
        return (s + 0.02 * torch.randn(shape, generator=g)).clamp(0, 1), s.clamp(0, 1)
    if name == "edges":                                   # a step edge and a one-pixel line on a flat field; the prediction has both one pixel off
        def field(dx, dy):
            t = torch.full(shape, 0.2)
            t[..., :, min(W - 1, W // 2 + dx):] = 0.8
            t[..., min(H - 1, H // 3 + dy), :] = 1.0
            return t
        return field(1, 1), field(0, 0)
    raise KeyError(name)


def oracle_eval(kind, lam, pred, target, upstream, dtype, device="cpu"):
    """oracle.losses in `dtype`: kind "train" -> train_loss(pred, target, lam), "ssim" -> ssim(pred, target).  Returns (value, d(upstream * value)/dpred)
    as a Python float and an fp64 tensor on `device`."""
    from oracle.losses import train_loss, ssim
    a = pred.detach().to(device=device, dtype=dtype).requires_grad_(True)
    b = target.detach().to(device=device, dtype=dtype)
    v = train_loss(a, b, lam) if kind == "train" else ssim(a, b)
    (v * upstream).backward()
    return float(v.detach().double().item()), a.grad.detach().double()


def references(kind, lam, pred, target, upstream, device="cpu"):
    """((v64, g64), (v32, g32)): the oracle in fp64 and the SAME oracle in fp32 on the same (fp32-representable) inputs."""
    return (oracle_eval(kind, lam, pred, target, upstream, torch.float64, device), oracle_eval(kind, lam, pred, target, upstream, torch.float32, device))


def check(key, value, grad, refs, report, tight=False, identical_g_ref=None):
    """Reports the measured ratios, then asserts the bars of the module docstring.  tight: the noise bars alone (2e-6, 2e-5 max|grad|).
    identical_g_ref: the scale for the `identical` class.  grad: a tensor (any device, any float dtype) or None for a value-only check."""
    (v64, g64), (v32, g32) = refs
    ev, ev32 = abs(float(value) - v64), abs(v32 - v64)
    assert math.isfinite(float(value)) and math.isfinite(v32)
    if grad is None:
        report(key, value_err=ev, fp32_ref_value_err=ev32)
        assert ev <= (2e-6 if tight else max(2e-6, 1.5 * ev32)), (key, ev, ev32)
        return
    gd = grad.detach().to(g64.device).double()
    assert gd.shape == g64.shape and bool(torch.isfinite(gd).all()) and bool(torch.isfinite(g32).all())
    gmax = g64.abs().max().item()
    e, e32 = (gd - g64).abs().max().item(), (g32 - g64).abs().max().item()      # every pixel, no mask
    scale = identical_g_ref if identical_g_ref is not None else gmax
    report(key, kernel_over_fp64=e / scale, fp32_ref_over_fp64=e32 / scale, max_abs_grad=gmax, value_err=ev, fp32_ref_value_err=ev32)
    if identical_g_ref is not None:
        assert gmax <= 1e-12 * identical_g_ref, gmax       # the class is what it says
        assert e <= 2e-5 * identical_g_ref, (key, e, identical_g_ref)
        assert ev <= 2e-6, (key, ev)
        return
    assert gmax > 0 and e32 > 0, (key, gmax, e32)          # the fp32 reference is finite and non-zero: the bar below is what it reads
    assert ev <= (2e-6 if tight else max(2e-6, 1.5 * ev32)), (key, ev, ev32)
    assert e <= (2e-5 * gmax if tight else max(2e-5 * gmax, 1.5 * e32)), (key, e / gmax, e32 / gmax)
