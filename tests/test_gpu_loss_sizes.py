"""The loss kernels of csrc/ssim.hip -- fused training loss and mean SSIM, forward and backward -- at the sizes and launch shapes training runs
(3 x 1080 x 1920: forward segments of 30 rows, backward of 60; 3 x 2160 x 3840: 120 and the 128 clamp with a 112-row tail; an odd size), on
the image content of tests/loss_content.py, against the fp64 formula of oracle/losses.py.  The older parity tests
(tests/test_gpu_parity.py::test_fused_*_matches_reference_formula) stop at 150 rows of noise: one launch plan, no cancellation.

The reference is plain torch ON THE DEVICE (grouped conv2d through torch's own depthwise kernels, MIOpen off, so that the fp32 evaluation is
the formula in fp32 and not a Winograd or FFT algorithm); a test pins it to the CPU evaluation.  Bars: tests/loss_content.py."""
import pytest
import torch

from helpers import parity_report
import loss_content as LC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = {"67x93": (3, 67, 93), "1080p": (3, 1080, 1920), "4k": (3, 2160, 3840), "odd": (3, 1087, 1931), "batch4": (4, 3, 540, 960)}
KINDS = [("train", 0.2), ("train", 1.0), ("ssim", None)]
KIND_IDS = ["train_0.2", "train_1.0", "mean_ssim"]
UP = 3.0

_pairs, _refs = {}, {}


def images(content, size):
    """(prediction, target) on the device, once per (content, size)."""
    k = (content, size)
    if k not in _pairs:
        a, b = LC.pair(content, SIZES[size])
        _pairs[k] = (a.to(DEV), b.to(DEV))
    return _pairs[k]


def refs(content, size, kind, lam):
    """fp64 and fp32 evaluation of oracle.losses on the device, once per (content, size, kind, lambda) for every parametrization that shares it."""
    k = (content, size, kind, lam)
    if k not in _refs:
        a, b = images(content, size)
        with torch.backends.cudnn.flags(enabled=False):
            _refs[k] = LC.references(kind, lam, a, b, UP, device=DEV)
        torch.cuda.synchronize()
    return _refs[k]


def identical_scale(content, size, kind, lam):
    return refs("smooth_plus_noise", size, kind, lam)[0][1].abs().max().item() if content == "identical" else None


def run_kernel(kind, lam, a, b, upstream=UP):
    """(value as a 0-dim device tensor, d(upstream * value)/da) through the shipped wrappers."""
    from fused_ssim import fused_ssim, fused_train_loss
    a1 = a.detach().clone().requires_grad_(True)
    v = fused_train_loss(a1, b, lam) if kind == "train" else fused_ssim(a1, b)
    (v * upstream).backward()
    torch.cuda.synchronize()
    return v.detach(), a1.grad


@pytest.fixture
def ssim_option():
    """set(name, value) for the two SSIM options; the product defaults are back when the test ends (ssim_target_waves: value 0)."""
    from diff_gaussian_rasterization import _lib
    yield _lib.set_option
    _lib.set_option("ssim_variant", 0)
    _lib.set_option("ssim_target_waves", 0)


def test_device_reference_is_the_cpu_reference():
    """The fp64 reference computed on the device IS oracle.losses on the CPU (to fp64 rounding), and the fp32 one sits at the CPU fp32 evaluation's
    distance from it (same formula, another summation order)."""
    a, b = LC.pair("smooth_plus_noise", SIZES["67x93"])
    for (kind, lam) in KINDS:
        (v64, g64), (v32, g32) = refs("smooth_plus_noise", "67x93", kind, lam)
        (c64, h64), (c32, h32) = LC.references(kind, lam, a, b, UP)
        gmax = h64.abs().max().item()
        assert abs(v64 - c64) < 1e-13 and (g64.cpu() - h64).abs().max().item() < 1e-12 * gmax
        e_dev, e_cpu = (g32.cpu() - h64).abs().max().item(), (h32 - h64).abs().max().item()
        parity_report(f"gpu_loss/reference/{kind if lam is None else f'train_{lam}'}", fp32_device_over_fp64=e_dev / gmax, fp32_cpu_over_fp64=e_cpu / gmax)
        assert 0.25 * e_cpu <= e_dev <= 4.0 * e_cpu, (e_dev, e_cpu)


CASES = [("67x93", v, c) for v in (0, 1) for c in LC.NAMES] + [("1080p", 0, c) for c in LC.NAMES] \
    + [(s, v, c) for (s, v) in (("1080p", 1), ("4k", 0), ("odd", 0), ("batch4", 0)) for c in ("noise", "smooth_plus_noise")]


@pytest.mark.parametrize("kind,lam", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("size,variant,content", CASES, ids=[f"{s}-{'tiled' if v else 'marching'}-{c}" for s, v, c in CASES])
def test_loss_against_fp64_oracle(ssim_option, size, variant, content, kind, lam):
    """Value and gradient, every pixel: `noise` at the tight bars (2e-6, 2e-5 max|grad|), every other class at the content bars."""
    ssim_option("ssim_variant", variant)
    a, b = images(content, size)
    v, g = run_kernel(kind, lam, a, b)
    assert g.dtype == torch.float32 and g.shape == a.shape
    LC.check(f"gpu_loss/{size}/{'tiled' if variant else 'marching'}/{content}/{kind if lam is None else f'train_{lam}'}", v.item(), g,
             refs(content, size, kind, lam), parity_report, tight=(content == "noise"), identical_g_ref=identical_scale(content, size, kind, lam))


@pytest.mark.parametrize("kind,lam", [("train", 0.2), ("ssim", None)], ids=["train_0.2", "mean_ssim"])
@pytest.mark.parametrize("content", ["noise", "smooth_plus_noise"])
@pytest.mark.parametrize("waves", [256, 16384])
def test_target_waves_sweep_at_1080p(ssim_option, waves, content, kind, lam):
    """ssim_target_waves 256: segments of 128 rows in both directions; 16384: 16 rows, 7 344 waves -- the launch without the LDS cap.  Same bars;
    and the settings agree with the default plan to 1e-6 / 2e-6 max|grad|: only the order in which the waves' partial sums are added differs."""
    a, b = images(content, "1080p")
    v0, g0 = run_kernel(kind, lam, a, b)
    ssim_option("ssim_target_waves", waves)
    v, g = run_kernel(kind, lam, a, b)
    r = refs(content, "1080p", kind, lam)
    LC.check(f"gpu_loss/1080p/waves_{waves}/{content}/{kind if lam is None else f'train_{lam}'}", v.item(), g, r, parity_report, tight=(content == "noise"))
    gmax = r[0][1].abs().max().item()
    dv, dg = abs(v.item() - v0.item()), (g.double() - g0.double()).abs().max().item()
    parity_report(f"gpu_loss/1080p/waves_{waves}_vs_default/{content}/{kind if lam is None else f'train_{lam}'}", value_diff=dv, grad_diff_over_max=dg / gmax)
    assert dv <= 1e-6 and dg <= 2e-6 * gmax, (dv, dg / gmax)


def test_target_waves_zero_restores_the_default_plan():
    """gsr_set_option("ssim_target_waves", 0): forward 4096 / backward 2048 again -- the same bits as a run before the option was touched."""
    from diff_gaussian_rasterization import _lib
    a, b = images("noise", "1080p")
    _lib.set_option("ssim_target_waves", 0)          # (whatever an earlier test of this process left)
    v0, g0 = run_kernel("train", 0.2, a, b)
    try:
        _lib.set_option("ssim_target_waves", 256)
        v1, g1 = run_kernel("train", 0.2, a, b)
    finally:
        _lib.set_option("ssim_target_waves", 0)
    v2, g2 = run_kernel("train", 0.2, a, b)
    parity_report("gpu_loss/1080p/waves_reset", value_bits_differ_at_256=int(not torch.equal(v0, v1)), grad_bits_differ_at_256=int(not torch.equal(g0, g1)))
    assert torch.equal(v0, v2) and torch.equal(g0, g2)


@pytest.mark.parametrize("kind,lam", [("train", 0.2), ("ssim", None)], ids=["train_0.2", "mean_ssim"])
def test_bit_reproducible_at_1080p(kind, lam):
    a, b = images("smooth_plus_noise", "1080p")
    v0, g0 = run_kernel(kind, lam, a, b)
    v1, g1 = run_kernel(kind, lam, a, b)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)


# ---- wrapper inputs: each equals the contiguous fp32 call bit for bit where the kernel sees the same floats ----
WRAP = (3, 270, 481)


@pytest.mark.parametrize("kind,lam", [("train", 0.2), ("ssim", None)], ids=["train_0.2", "mean_ssim"])
def test_non_contiguous_prediction(kind, lam):
    """A permuted view of an HWC tensor: same bits as its contiguous copy, gradient in the leaf's own HWC shape."""
    from fused_ssim import fused_ssim, fused_train_loss
    a, b = (t.to(DEV) for t in LC.pair("noise", WRAP))
    v0, g0 = run_kernel(kind, lam, a, b)
    hwc = a.permute(1, 2, 0).contiguous().requires_grad_(True)
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous()
    v = fused_train_loss(view, b, lam) if kind == "train" else fused_ssim(view, b)
    (v * UP).backward()
    assert hwc.grad.dtype == hwc.dtype and hwc.grad.shape == hwc.shape
    assert torch.equal(v.detach(), v0) and torch.equal(hwc.grad.permute(2, 0, 1), g0)


@pytest.mark.parametrize("kind,lam", [("train", 0.2), ("ssim", None)], ids=["train_0.2", "mean_ssim"])
def test_fp64_prediction(kind, lam):
    """An fp64 prediction holding fp32-representable values: the kernel sees the same floats; the gradient comes back as fp64."""
    from fused_ssim import fused_ssim, fused_train_loss
    a, b = (t.to(DEV) for t in LC.pair("noise", WRAP))
    v0, g0 = run_kernel(kind, lam, a, b)
    a64 = a.double().requires_grad_(True)
    v = fused_train_loss(a64, b, lam) if kind == "train" else fused_ssim(a64, b)
    (v * UP).backward()
    assert a64.grad.dtype == torch.float64 and a64.grad.shape == a64.shape
    assert torch.equal(v.detach().float(), v0) and torch.equal(a64.grad, g0.double())


@pytest.mark.parametrize("kind,lam", [("train", 0.2), ("ssim", None)], ids=["train_0.2", "mean_ssim"])
def test_fp16_target(kind, lam):
    """An fp16 target is the fp32 call on the target's fp16 values."""
    a, b = (t.to(DEV) for t in LC.pair("noise", WRAP))
    b16 = b.half()
    v0, g0 = run_kernel(kind, lam, a, b16.float())
    v, g = run_kernel(kind, lam, a, b16)
    assert g.dtype == torch.float32 and g.shape == a.shape
    assert torch.equal(v, v0) and torch.equal(g, g0)


def test_shape_mismatch_is_refused():
    """A smaller target would be read out of bounds: refused in Python, nothing is launched."""
    from fused_ssim import fused_ssim, fused_train_loss, FusedSSIMMap
    from diff_gaussian_rasterization._lib import GsrError
    a = torch.rand(3, 40, 50, device=DEV, requires_grad=True)
    for bad in (torch.rand(3, 39, 50, device=DEV), torch.rand(3, 40, 49, device=DEV), torch.rand(1, 40, 50, device=DEV)):
        with pytest.raises(GsrError, match="differ in shape"):
            fused_ssim(a, bad)
        with pytest.raises(GsrError, match="differ in shape"):
            fused_train_loss(a, bad)
        with pytest.raises(GsrError, match="differ in shape"):
            FusedSSIMMap.apply(a[None], bad[None])
    with torch.no_grad(), pytest.raises(GsrError, match="differ in shape"):
        fused_ssim(a, torch.rand(3, 40, 49, device=DEV), train=False)
