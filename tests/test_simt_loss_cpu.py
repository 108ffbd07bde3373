"""The fused training loss of csrc/ssim.hip -- (1 - lambda) L1 + lambda (1 - SSIM) computed inside the marching-wave SSIM kernels, forward and
backward -- and the mean-SSIM form, executed on the CPU from the source through the SIMT shim (DPP wave shifts, raw buffer loads / stores with
the hardware's out-of-range behaviour) against the fp64 formula of the reference's utils/loss_utils.py:40-87 / train.py:119-126 (restated in
oracle/losses.py, pinned to the reference by a golden vector): the shapes, mixes and bars of the GPU tests
(tests/test_gpu_parity.py::test_fused_train_loss_matches_reference_formula, ::test_fused_ssim_matches_reference_formula).
Test infrastructure: tests/_build/libsimt_loss.so is never part of the product."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_build", "libsimt_loss.so")
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def lib():
    from simt_build import build
    h = build("loss", fp_contract_off=True)
    h.simt_loss_last_error.restype = C.c_char_p
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _images(shape):
    g = torch.Generator().manual_seed(shape[-1])
    a = torch.rand(shape, generator=g)
    b = (a + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    b[..., :3, :5] = a[..., :3, :5]                    # exact ties: zero L1 gradient there
    return a, b


@pytest.mark.parametrize("shape,lam", [((3, 67, 93), 0.2), ((3, 128, 160), 0.2), ((3, 16, 16), 0.5), ((3, 11, 300), 0.0), ((3, 40, 40), 1.0), ((2, 150, 55), 0.2)])
def test_fused_train_loss_source_on_the_cpu(lib, shape, lam):
    from oracle.losses import train_loss
    a, b = _images(shape)
    a2 = a.clone().double().requires_grad_(True)
    v2 = train_loss(a2, b.double(), lam)
    (v2 * 3.0).backward()
    a_np, b_np = np.ascontiguousarray(a.numpy()), np.ascontiguousarray(b.numpy())
    loss = np.zeros(4, dtype=np.float32)
    grad = np.zeros(shape, dtype=np.float32)
    assert lib.simt_train_loss(shape[0], shape[1], shape[2], ptr(a_np), ptr(b_np), C.c_float(lam), C.c_float(3.0), ptr(loss), ptr(grad)) == 0, lib.simt_loss_last_error()
    assert abs(float(loss[0]) - v2.item()) < 2e-6
    d = np.abs(grad.astype(np.float64) - a2.grad.numpy()).max()
    assert d <= 2e-5 * a2.grad.abs().max().item(), d


@pytest.mark.parametrize("shape", [(3, 67, 93), (1, 16, 16), (3, 5, 7), (3, 11, 300)])
def test_fused_mean_ssim_source_on_the_cpu(lib, shape):
    from oracle.losses import ssim as torch_ssim
    a, b = _images(shape)
    a2 = a.clone().double().requires_grad_(True)
    v2 = torch_ssim(a2, b.double())
    (v2 * 3.0).backward()
    a_np, b_np = np.ascontiguousarray(a.numpy()), np.ascontiguousarray(b.numpy())
    mean = np.zeros(4, dtype=np.float32)
    grad = np.zeros(shape, dtype=np.float32)
    assert lib.simt_ssim_mean(shape[0], shape[1], shape[2], ptr(a_np), ptr(b_np), C.c_float(3.0), ptr(mean), ptr(grad)) == 0, lib.simt_loss_last_error()
    assert abs(float(mean[0]) - v2.item()) < 2e-6
    d = np.abs(grad.astype(np.float64) - a2.grad.numpy()).max()
    assert d <= 2e-5 * a2.grad.abs().max().item(), d


# ================================================================================================
# Launch plans and image content.  The cases above all clamp to seg = 16 with one plan for both directions; training runs 30 <= seg <= 128 with
# a backward that walks other segments than the forward that wrote the derivative maps (march_plan in csrc/ssim.hip).  Lowered wave targets reach
# those plans at a few hundred rows; every case first asserts, from the plan read out of the library, that it IS in the regime it names.
# ================================================================================================
from helpers import parity_report  # noqa: E402
import loss_content as LC  # noqa: E402

MPF, HALO, MW = 5, 5, 54          # csrc/ssim.hip: rows in flight, window half width, output columns per wave


@pytest.fixture(autouse=True)
def _defaults_restored(lib):
    """Every test ends with the product defaults: 4096 / 2048 waves (through the product's own reset, value 0), variant 0."""
    yield
    lib.simt_loss_restore_defaults()
    tw = (C.c_int * 2)()
    lib.simt_loss_get_target_waves(tw)
    assert tuple(tw) == (4096, 2048)


def _plan(lib, shape, bwd):
    out = (C.c_int * 4)()
    lib.simt_loss_march_plan(shape[0], shape[1], shape[2], int(bwd), out)
    return dict(nsx=out[0], nsy=out[1], seg=out[2], lds=out[3], tail=shape[1] - (out[1] - 1) * out[2])


def _run_train(lib, a, b, lam, upstream=3.0):
    shape = tuple(a.shape)
    a_np, b_np = np.ascontiguousarray(a.numpy()), np.ascontiguousarray(b.numpy())
    loss = np.zeros(4, dtype=np.float32)
    grad = np.full(shape, np.nan, dtype=np.float32)
    assert lib.simt_train_loss(shape[0], shape[1], shape[2], ptr(a_np), ptr(b_np), C.c_float(lam), C.c_float(upstream), ptr(loss), ptr(grad)) == 0, lib.simt_loss_last_error()
    return float(loss[0]), torch.from_numpy(grad)


def _run_mean(lib, a, b, upstream=3.0):
    shape = tuple(a.shape)
    a_np, b_np = np.ascontiguousarray(a.numpy()), np.ascontiguousarray(b.numpy())
    mean = np.zeros(4, dtype=np.float32)
    grad = np.full(shape, np.nan, dtype=np.float32)
    assert lib.simt_ssim_mean(shape[0], shape[1], shape[2], ptr(a_np), ptr(b_np), C.c_float(upstream), ptr(mean), ptr(grad)) == 0, lib.simt_loss_last_error()
    return float(mean[0]), torch.from_numpy(grad)


def _run(lib, kind, a, b, lam):
    return _run_train(lib, a, b, lam) if kind == "train" else _run_mean(lib, a, b)


# (name, wave targets forward / backward or None for the defaults, shape, regime)
def _mid(f, b, s):          # 16 < seg < 128, seg not a multiple of MPF, H not a multiple of seg -- in both directions
    return all(16 < p["seg"] < 128 and p["seg"] % MPF and s[1] % p["seg"] for p in (f, b))


PLANS = [
    ("mid_seg_34_23", (12, 18), (3, 67, 93), lambda f, b, s: _mid(f, b, s) and f["seg"] != b["seg"] and f["nsy"] != b["nsy"]),
    # (backward: one segment per strip wanted, 257 rows -> clamped to 128)
    ("fwd_65_bwd_clamped_128_one_row_tail", (40, 10), (1, 257, 540),
     lambda f, b, s: f["seg"] == 65 and f["nsy"] == 4 and b["seg"] == 128 and s[1] > 128 and b["nsy"] == 3 and b["tail"] == 1),
    ("seg_17_one_row_tail", (20, 20), (1, 324, 54), lambda f, b, s: _mid(f, b, s) and f["seg"] == 17 and f["tail"] == 1 and b["tail"] == 1),
    ("seg_17_tail_below_halo", (20, 20), (1, 326, 54), lambda f, b, s: _mid(f, b, s) and 1 < f["tail"] < HALO and 1 < b["tail"] < HALO),
    ("fwd_clamped_128_one_row_tail", (1, 1), (1, 129, 60), lambda f, b, s: f["seg"] == 128 and f["nsy"] == 2 and f["tail"] == 1 and b == f),
    ("seg_16_one_row_tail", None, (1, 97, 54), lambda f, b, s: f["seg"] == 16 and f["tail"] == 1 and b["tail"] == 1),
    ("one_segment_longer_than_image", None, (2, 9, 113), lambda f, b, s: f["nsy"] == 1 and f["seg"] > s[1] and b["nsy"] == 1 and b["seg"] > s[1]),
    ("one_segment_seg_40", (3, 3), (1, 40, 113), lambda f, b, s: f["nsy"] == 1 and f["seg"] == 40 and b == f),
] + [
    # the last strip holds `last` output columns: 54 / 108 a full one, 55 a single column, 59 / 113 five columns whose right neighbours are
    # all outside the image, 60 six
    (f"width_{w}", (2 * n, 3 * n), (1, 37, w), (lambda n, last: lambda f, b, s: f["nsx"] == n and s[2] - (n - 1) * MW == last and f["seg"] == 19 and b["seg"] == 16)(n, last))
    for w, n, last in ((54, 1, 54), (55, 2, 1), (59, 2, 5), (60, 2, 6), (108, 2, 54), (113, 3, 5))
] + [
    ("one_column", None, (3, 50, 1), lambda f, b, s: f["nsx"] == 1 and f["nsy"] == 4),
    ("one_row", None, (3, 1, 70), lambda f, b, s: f["nsx"] == 2 and f["nsy"] == 1 and f["seg"] > s[1]),
    ("one_pixel", None, (1, 1, 1), lambda f, b, s: f["nsx"] == 1 and f["nsy"] == 1),
    ("planes_24", (96, 48), (24, 40, 60), lambda f, b, s: s[0] == 24 and f["seg"] == 20 and b["seg"] == 40),
]


@pytest.mark.parametrize("name,targets,shape,regime", PLANS, ids=[p[0] for p in PLANS])
def test_train_loss_launch_plans_on_the_cpu(lib, name, targets, shape, regime):
    """Fused loss (lambda 0.2), value and gradient on noise at the tight bars -- 2e-6, 2e-5 max|grad|, every pixel -- under launch plans the
    older cases never reach (see PLANS)."""
    if targets is not None:
        lib.simt_loss_set_target_waves(*targets)
    f, b = _plan(lib, shape, 0), _plan(lib, shape, 1)
    print(f"[plan] {name}: shape {shape} targets {targets} forward {f} backward {b}", flush=True)
    assert regime(f, b, shape), (name, f, b)
    pred, target = LC.pair("noise", shape)
    refs = LC.references("train", 0.2, pred, target, 3.0)
    v, g = _run_train(lib, pred, target, 0.2)
    LC.check(f"simt_loss_plan/{name}/train", v, g, refs, parity_report, tight=True)


MEAN_PLANS = [p for p in PLANS if p[0] in ("mid_seg_34_23", "fwd_65_bwd_clamped_128_one_row_tail", "seg_17_one_row_tail", "width_55", "one_pixel")]


@pytest.mark.parametrize("name,targets,shape,regime", MEAN_PLANS, ids=[p[0] for p in MEAN_PLANS])
def test_mean_ssim_launch_plans_on_the_cpu(lib, name, targets, shape, regime):
    """Mean SSIM (ssim_mean_kernel over the waves' partial sums, MODE 1 backward) under the same plans."""
    if targets is not None:
        lib.simt_loss_set_target_waves(*targets)
    f, b = _plan(lib, shape, 0), _plan(lib, shape, 1)
    print(f"[plan] {name}: shape {shape} targets {targets} forward {f} backward {b}", flush=True)
    assert regime(f, b, shape), (name, f, b)
    pred, target = LC.pair("noise", shape)
    refs = LC.references("ssim", None, pred, target, 3.0)
    v, g = _run_mean(lib, pred, target)
    LC.check(f"simt_loss_plan/{name}/ssim", v, g, refs, parity_report, tight=True)


def test_training_sizes_take_the_plans_the_cases_above_stand_for(lib):
    """The default plans at the training sizes, read out, not executed: 1080p forward seg 30 / backward 60, 4K forward 120 / backward at the
    128 clamp with a 112-row tail; the option sweep of the GPU tests: 256 waves -> seg 128 both ways, 16384 -> seg 16 without the LDS cap."""
    assert _plan(lib, (3, 1080, 1920), 0) | {"lds": 0} == dict(nsx=36, nsy=36, seg=30, lds=0, tail=30)
    assert _plan(lib, (3, 1080, 1920), 1)["seg"] == 60
    assert _plan(lib, (3, 2160, 3840), 0)["seg"] == 120
    b = _plan(lib, (3, 2160, 3840), 1)
    assert (b["seg"], b["nsy"], b["tail"]) == (128, 17, 112)
    lib.simt_loss_set_target_waves(256, 256)
    assert _plan(lib, (3, 1080, 1920), 0)["seg"] == 128 and _plan(lib, (3, 1080, 1920), 1)["seg"] == 128
    lib.simt_loss_set_target_waves(16384, 16384)
    p = _plan(lib, (3, 1080, 1920), 0)
    assert p["seg"] == 16 and 3 * p["nsx"] * p["nsy"] > 4864 and p["lds"] == 0


# ---- the LDS-tiled kernels: variant 1, every no-grad mean, every plane of 2 GB or more ----
@pytest.mark.parametrize("shape,lam", [((3, 67, 93), 0.2), ((2, 33, 130), 1.0)])
def test_tiled_train_loss_on_the_cpu(lib, shape, lam):
    lib.simt_loss_set_variant(1)
    pred, target = LC.pair("noise", shape)
    refs = LC.references("train", lam, pred, target, 3.0)
    v, g = _run_train(lib, pred, target, lam)
    LC.check(f"simt_loss_tiled/train/{shape[1]}x{shape[2]}", v, g, refs, parity_report, tight=True)


@pytest.mark.parametrize("shape", [(3, 67, 93), (1, 16, 64), (2, 17, 65)])
def test_mean_ssim_without_maps_on_the_cpu(lib, shape):
    """torch.no_grad() evaluation: no derivative maps, so the tiled forward whatever the variant; tile-exact and tile-plus-one shapes."""
    pred, target = LC.pair("noise", shape)
    refs = LC.references("ssim", None, pred, target, 1.0)
    mean = np.zeros(4, dtype=np.float32)
    a_np, b_np = np.ascontiguousarray(pred.numpy()), np.ascontiguousarray(target.numpy())
    assert lib.simt_ssim_mean_no_maps(shape[0], shape[1], shape[2], ptr(a_np), ptr(b_np), ptr(mean)) == 0, lib.simt_loss_last_error()
    LC.check(f"simt_loss_tiled/mean_no_maps/{shape[1]}x{shape[2]}", float(mean[0]), None, refs, parity_report, tight=True)


@pytest.mark.parametrize("variant,targets", [(0, (12, 18)), (1, None)], ids=["marching", "tiled"])
def test_ssim_map_pair_on_the_cpu(lib, variant, targets):
    """gsr_launch_ssim_forward / _backward: the SSIM MAP against oracle.losses with the map kept, and dL/dimg1 for a random dL/dmap."""
    import torch.nn.functional as F
    from oracle.losses import _window
    shape = (3, 67, 93)
    lib.simt_loss_set_variant(variant)
    if targets is not None:
        lib.simt_loss_set_target_waves(*targets)
        assert _plan(lib, shape, 0)["seg"] == 34 and _plan(lib, shape, 1)["seg"] == 23
    pred, target = LC.pair("noise", shape)
    gmap = torch.randn(shape, generator=torch.Generator().manual_seed(5))

    def oracle_map(a, b):          # oracle.losses.ssim without its final mean
        a, b = a[None], b[None]
        c = a.shape[1]
        w = _window(c, a.device, a.dtype)
        mu1, mu2 = F.conv2d(a, w, padding=5, groups=c), F.conv2d(b, w, padding=5, groups=c)
        s1 = F.conv2d(a * a, w, padding=5, groups=c) - mu1 * mu1
        s2 = F.conv2d(b * b, w, padding=5, groups=c) - mu2 * mu2
        s12 = F.conv2d(a * b, w, padding=5, groups=c) - mu1 * mu2
        return (((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2)))[0]

    a2 = pred.double().requires_grad_(True)
    m2 = oracle_map(a2, target.double())
    assert abs(m2.mean().item() - LC.oracle_eval("ssim", None, pred, target, 1.0, torch.float64)[0]) < 1e-14      # the restatement IS the oracle's map
    (m2 * gmap.double()).sum().backward()
    a_np, b_np, g_np = (np.ascontiguousarray(t.numpy()) for t in (pred, target, gmap))
    m = np.full(shape, np.nan, dtype=np.float32)
    grad = np.full(shape, np.nan, dtype=np.float32)
    assert lib.simt_ssim_map(shape[0], shape[1], shape[2], ptr(a_np), ptr(b_np), ptr(g_np), ptr(m), ptr(grad)) == 0, lib.simt_loss_last_error()
    em = np.abs(m.astype(np.float64) - m2.detach().numpy()).max()
    eg = np.abs(grad.astype(np.float64) - a2.grad.numpy()).max()
    gmax = a2.grad.abs().max().item()
    parity_report(f"simt_loss_map_pair/{'tiled' if variant else 'marching'}", map_err=em, grad_over_fp64=eg / gmax)
    assert em <= 2e-6, em              # SSIM values are O(1): the value bar, per pixel
    assert eg <= 2e-5 * gmax, eg / gmax


# ---- image content ----
CONTENT_SHAPE = (3, 67, 93)


@pytest.mark.parametrize("kind,lam", [("train", 0.2), ("train", 1.0), ("ssim", None)], ids=["train_0.2", "train_1.0", "mean_ssim"])
@pytest.mark.parametrize("content", LC.NAMES)
def test_loss_content_on_the_cpu(lib, content, kind, lam):
    """Every content class of tests/loss_content.py at the bars stated there, under a training-like plan (forward seg 34, backward 23).

    `edges` is the class that shows what sigma^2 = E[x^2] - mu^2 costs when it is not ONE fused operation: the image is translation-invariant along
    the edge and the line, so the cancellation error on the fringe of either feature (4-5 pixels away, sigma^2 ~ C2) is the same number in every pixel
    of a fringe row / column and does not average out of the mean.  With the product and the difference rounded separately (what this host build,
    without FMA contraction, made of `ex2 - mu1 * mu1`) |SSIM - fp64| was 2.71e-6 against a bar of 2.64e-6; with the fmaf the source now spells out
    -- the instruction the gfx950 build always had -- 1.70e-6."""
    lib.simt_loss_set_target_waves(12, 18)
    assert _plan(lib, CONTENT_SHAPE, 0)["seg"] == 34 and _plan(lib, CONTENT_SHAPE, 1)["seg"] == 23
    pred, target = LC.pair(content, CONTENT_SHAPE)
    refs = LC.references(kind, lam, pred, target, 3.0)
    g_ref = None
    if content == "identical":
        sp, st = LC.pair("smooth_plus_noise", CONTENT_SHAPE)
        g_ref = LC.oracle_eval(kind, lam, sp, st, 3.0, torch.float64)[1].abs().max().item()
    v, g = _run(lib, kind, pred, target, lam)
    LC.check(f"simt_loss_content/{content}/{kind if lam is None else f'train_{lam}'}", v, g, refs, parity_report, tight=(content == "noise"), identical_g_ref=g_ref)
