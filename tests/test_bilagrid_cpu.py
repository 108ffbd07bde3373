"""The bilateral-grid appearance model without a GPU: tests/bilagrid_reference.py against torch's grid_sample and against gradients worked out
by hand, then the kernels of csrc/bilagrid.hip -- compiled for the host with the whole library (tests/simt) and called through the C ABI on
guarded numpy buffers, and through the fused_bilagrid package on the CPU -- against that reference.  Bars: tests/bilagrid_reference.py."""
import ctypes as C
import math
import shutil

import numpy as np
import pytest
import torch

import bilagrid_reference as BR
from test_mcmc_cpu import Guarded
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# (H, W, L, Gh, Gw): cells without pixels; a few pixels per cell; one cell, two tiles; unequal sizes on every axis; one pixel;
# one cell of 3 x 3 tiles with a ragged last column and row
SHAPES = [(5, 7, 8, 16, 16), (37, 53, 8, 16, 16), (64, 64, 2, 2, 2), (33, 130, 3, 5, 4), (1, 1, 2, 2, 2), (70, 150, 2, 2, 2)]
GRID_SAMPLE_SHAPES = [(37, 53, 8, 16, 16), (5, 7, 8, 16, 16), (64, 64, 2, 2, 2), (33, 130, 3, 5, 4)]


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GRID_SAMPLE_SHAPES)
def test_reference_is_grid_sample(shape):
    H, W, L, Gh, Gw = shape
    grid, image, dL = (t.double() for t in BR.make_case(H, W, L, Gh, Gw, seed=H + W))
    assert not bool((BR.guidance(image) * (L - 1) == L - 1).any())      # (the one point where torch's gradient is one-sided)
    a = BR.slice_with_grads(grid, image, dL, BR.slice_image)
    b = BR.slice_with_grads(grid, image, dL, BR.slice_grid_sample)
    for name, x, y in zip(("out", "dgrid", "dimage"), a, b):
        err = float((x - y).abs().max() / y.abs().max())
        print(f"[bilagrid] reference against grid_sample {shape} {name}: {err:.2e}", flush=True)
        assert err <= 1e-12, (name, err)
    if H * W >= 1000:
        g = BR.guidance(image)
        assert bool((g < 0).any()) and bool((g > 1).any())      # the guidance clamps on both sides


def test_reference_convention_at_the_upper_bound_and_beyond():
    """A grid whose only non-zero channel is the offset of the red output, 2 z: out_r = 2 fz, so d out_r / d rgb = 2 (L - 1) (0.299, 0.587,
    0.114) wherever the unclamped fz lies in [0, L - 1] -- at fz == L - 1 exactly (a white pixel) too -- and 0 beyond."""
    L = 4
    grid = torch.zeros(12, L, 3, 3, dtype=torch.float64)
    grid[3] = 2.0 * torch.arange(L, dtype=torch.float64)[:, None, None]
    image = torch.tensor([[1.0, 1.2, 0.5, -0.1, 0.0]], dtype=torch.float64).expand(3, 5).reshape(3, 1, 5).contiguous()
    image[:, 0, 0] = torch.tensor([1.0 / BR.LUMA[0], 0.0, 0.0], dtype=torch.float64)      # (grey 1.0 has guidance 1 - 1e-16 in fp64: this one is exact)
    assert float(BR.guidance(image)[0, 0]) * (L - 1) == L - 1
    dL = torch.zeros(3, 1, 5, dtype=torch.float64)
    dL[0] = 1.0
    out, dgrid, dimage = BR.slice_with_grads(grid, image, dL)
    assert torch.allclose(out[0, 0], torch.tensor([6.0, 6.0, 3.0, 0.0, 0.0], dtype=torch.float64), atol=1e-12) and float(out[1:].abs().max()) == 0.0
    slope = 2.0 * (L - 1) * torch.tensor(BR.LUMA, dtype=torch.float64)
    want = torch.stack([slope, torch.zeros(3, dtype=torch.float64), slope, torch.zeros(3, dtype=torch.float64), slope], dim=1)      # [3, 5]
    assert torch.allclose(dimage[:, 0], want, atol=1e-12), dimage[:, 0]
    # the grid gradient of the offset channel: every pixel's weight, 1 in all, lands on the levels it lies between
    assert float(dgrid[3].sum()) == pytest.approx(5.0, abs=1e-12) and float(dgrid[3, L - 1].sum()) == pytest.approx(2.0, abs=1e-12)


def test_reference_total_variation_is_the_mean_squared_difference():
    X = torch.randn(3, 12, 4, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = sum(torch.diff(X, dim=d).pow(2).mean() for d in (2, 3, 4))
    assert float(BR.total_variation(X)) == pytest.approx(float(want), rel=1e-14)
    assert float(BR.total_variation(BR.identity_grids(2, 4, 5, 6, torch.float64))) == 0.0


# ---- the kernels through the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    h = C.CDLL(simt_lib)
    h.gsr_last_error.restype = C.c_char_p
    vp, i = C.c_void_p, C.c_int
    h.gsr_bilagrid_scratch_bytes.restype, h.gsr_bilagrid_scratch_bytes.argtypes = C.c_size_t, [i] * 5
    h.gsr_bilagrid_slice.argtypes = [i] * 5 + [vp] * 4
    h.gsr_bilagrid_slice_backward.argtypes = [i] * 5 + [vp] * 6 + [C.c_size_t, vp]
    h.gsr_bilagrid_tv_partial_count.restype, h.gsr_bilagrid_tv_partial_count.argtypes = C.c_int64, [i] * 4
    h.gsr_bilagrid_tv.argtypes = [i] * 4 + [vp] * 4
    h.gsr_bilagrid_tv_backward.argtypes = [i] * 4 + [vp] * 4
    return h


def run_slice(lib, grid, image, dL=None, offset=0, with_image_grad=True):
    """-> out, dL/dgrid, dL/dimage (torch; the last two None without dL, the last None without with_image_grad).  Every buffer is guarded;
    offset 4: the base pointers sit 4 bytes off a 64-byte boundary."""
    _, L, Gh, Gw = grid.shape
    _, H, W = image.shape
    bg, bi = Guarded(grid.numpy(), offset), Guarded(image.numpy(), offset)
    bo = Guarded(np.full((3, H, W), 7.0, np.float32), offset)
    assert lib.gsr_bilagrid_slice(H, W, L, Gh, Gw, bg.ptr, bi.ptr, bo.ptr, None) == 0, lib.gsr_last_error()
    bufs = [bg, bi, bo]
    dgrid = dimage = None
    if dL is not None:
        nbytes = lib.gsr_bilagrid_scratch_bytes(H, W, L, Gh, Gw)
        assert nbytes > 0 and nbytes % 4 == 0
        bd, bs = Guarded(dL.numpy(), offset), Guarded(np.full(nbytes // 4, np.nan, np.float32), offset)
        bdg = Guarded(np.full((12, L, Gh, Gw), 7.0, np.float32), offset)
        bdi = Guarded(np.full((3, H, W), 7.0, np.float32), offset) if with_image_grad else None
        assert lib.gsr_bilagrid_slice_backward(H, W, L, Gh, Gw, bg.ptr, bi.ptr, bd.ptr, bdg.ptr, bdi.ptr if bdi else None, bs.ptr, nbytes,
                                               None) == 0, lib.gsr_last_error()
        bufs += [bd, bs, bdg] + ([bdi] if bdi else [])
        assert np.array_equal(bd.a.view(np.int32), dL.numpy().view(np.int32)), "an input was written"
        dgrid = torch.from_numpy(bdg.a.copy())
        dimage = torch.from_numpy(bdi.a.copy()) if bdi else None
    assert all(b.intact() for b in bufs), "the bytes around a buffer were overwritten"
    assert np.array_equal(bg.a.view(np.int32), grid.numpy().view(np.int32)) and np.array_equal(bi.a.view(np.int32), image.numpy().view(np.int32))
    return torch.from_numpy(bo.a.copy()), dgrid, dimage


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("kind", ["uniform", "white", "black"])
@pytest.mark.parametrize("shape", SHAPES)
def test_slice_kernels_are_the_reference(lib, shape, kind):
    H, W, L, Gh, Gw = shape
    grid, image, dL = BR.make_case(H, W, L, Gh, Gw, seed=7 * H + W, kind=kind)
    out, dgrid, dimage = run_slice(lib, grid, image, dL)
    BR.check_against_reference(out, dgrid, dimage, grid, image, dL, f"{shape} {kind}", allow_excuses=kind == "uniform")
    # without the image gradient: the same bits of the grid gradient; and a second run: the same bits of everything
    out2, dgrid2, none = run_slice(lib, grid, image, dL, with_image_grad=False)
    assert none is None and torch.equal(bits(dgrid2), bits(dgrid)) and torch.equal(bits(out2), bits(out))
    if kind == "uniform" and shape != (37, 53, 8, 16, 16):      # (that shape is the slow one on the host: its second run is the one above)
        out3, dgrid3, dimage3 = run_slice(lib, grid, image, dL)
        assert torch.equal(bits(dgrid3), bits(dgrid)) and torch.equal(bits(dimage3), bits(dimage)) and torch.equal(bits(out3), bits(out))


def test_slice_kernels_with_base_pointers_off_16_byte_alignment(lib):
    H, W, L, Gh, Gw = 33, 130, 3, 5, 4
    grid, image, dL = BR.make_case(H, W, L, Gh, Gw, seed=99)
    out, dgrid, dimage = run_slice(lib, grid, image, dL, offset=4)
    BR.check_against_reference(out, dgrid, dimage, grid, image, dL, "offset 4")
    out0, dgrid0, dimage0 = run_slice(lib, grid, image, dL, offset=0)
    assert torch.equal(bits(out), bits(out0)) and torch.equal(bits(dgrid), bits(dgrid0)) and torch.equal(bits(dimage), bits(dimage0))


def test_slice_kernels_with_a_large_guidance_axis(lib):
    """L above 16 takes the backward's second instantiation (LDS sized for 64 levels)."""
    H, W, L, Gh, Gw = 9, 21, 33, 3, 4
    grid, image, dL = BR.make_case(H, W, L, Gh, Gw, seed=5)
    out, dgrid, dimage = run_slice(lib, grid, image, dL)
    BR.check_against_reference(out, dgrid, dimage, grid, image, dL, "L 33")
    _, dgrid2, _ = run_slice(lib, grid, image, dL, with_image_grad=False)
    assert torch.equal(bits(dgrid2), bits(dgrid))


@pytest.mark.parametrize("poison", [math.nan, math.inf, -math.inf])
def test_non_finite_pixels_stay_in_bounds_and_to_themselves(lib, poison):
    H, W, L, Gh, Gw = 33, 130, 3, 5, 4
    grid, image, dL = BR.make_case(H, W, L, Gh, Gw, seed=3)
    out, dgrid, dimage = run_slice(lib, grid, image, dL)
    bad = image.clone()
    spots = [(0, 0, 0), (1, 17, 29), (2, H - 1, 30), (0, 20, 5)]      # (all in the first cell column: x < 43)
    for c, y, x in spots:
        bad[c, y, x] = poison
    bad[:, 9, 9] = poison      # all three channels: inf - inf has no place either
    out_b, dgrid_b, dimage_b = run_slice(lib, grid, bad, dL)      # (the guards are checked inside)
    keep = torch.ones(H, W, dtype=torch.bool)
    for _, y, x in spots + [(0, 9, 9)]:
        keep[y, x] = False
    assert torch.equal(bits(out_b)[:, keep], bits(out)[:, keep]), "a finite pixel's output changed"
    assert torch.equal(bits(dimage_b)[:, keep], bits(dimage)[:, keep]), "a finite pixel's image gradient changed"
    assert not bool(torch.isfinite(out_b[:, ~keep]).all())
    # the grid gradient keeps its bits away from the vertices the poisoned pixels touch: here, the vertex columns right of the first cell column
    assert bool(torch.isfinite(dgrid_b[:, :, :, 2:]).all()) and torch.equal(bits(dgrid_b[:, :, :, 2:]), bits(dgrid[:, :, :, 2:]))
    assert not bool(torch.isfinite(dgrid_b[:, :, :, :2]).all())


def test_invalid_arguments_are_refused_before_any_launch(lib):
    H, W, L, Gh, Gw = 5, 7, 2, 2, 2
    grid, image, dL = BR.make_case(H, W, L, Gh, Gw, seed=1)
    bg, bi, bd = Guarded(grid.numpy()), Guarded(image.numpy()), Guarded(dL.numpy())
    nbytes = lib.gsr_bilagrid_scratch_bytes(H, W, L, Gh, Gw)
    out, dg, di = Guarded(np.full((3, H, W), 7.0, np.float32)), Guarded(np.full((12, L, Gh, Gw), 7.0, np.float32)), Guarded(np.full((3, H, W), 7.0, np.float32))
    sc = Guarded(np.full(nbytes // 4, 7.0, np.float32))
    untouched = lambda: all(bool((b.a == 7.0).all()) and b.intact() for b in (out, dg, di, sc))      # noqa: E731
    fwd = lambda h, w, l, gh, gw, g=bg.ptr, i=bi.ptr, o=out.ptr: lib.gsr_bilagrid_slice(h, w, l, gh, gw, g, i, o, None)      # noqa: E731
    bwd = lambda h, w, l, gh, gw, g=bg.ptr, i=bi.ptr, d=bd.ptr, o=dg.ptr, s=sc.ptr, n=nbytes: lib.gsr_bilagrid_slice_backward(      # noqa: E731
        h, w, l, gh, gw, g, i, d, o, di.ptr, s, n, None)
    for sizes, status in (((0, W, L, Gh, Gw), -1), ((H, 0, L, Gh, Gw), -1), ((H, -3, L, Gh, Gw), -1), ((H, W, 1, Gh, Gw), -4), ((H, W, L, 1, Gw), -4),
                          ((H, W, L, Gh, 65), -4), ((H, W, 65, Gh, Gw), -4), ((H, W, L, 0, Gw), -4), ((1 << 24, W, L, Gh, Gw), -4)):
        assert fwd(*sizes) == status and lib.gsr_last_error(), sizes
        assert bwd(*sizes) == status, sizes
        assert lib.gsr_bilagrid_scratch_bytes(*sizes) == 0, sizes
    assert b"2..64" in (fwd(H, W, L, Gh, 65), lib.gsr_last_error())[1]
    for kw in (dict(g=None), dict(i=None), dict(o=None)):
        assert fwd(H, W, L, Gh, Gw, **kw) == -1 and b"NULL" in lib.gsr_last_error(), kw
    for kw in (dict(g=None), dict(i=None), dict(d=None), dict(o=None), dict(s=None)):
        assert bwd(H, W, L, Gh, Gw, **kw) == -1 and b"NULL" in lib.gsr_last_error(), kw
    assert bwd(H, W, L, Gh, Gw, n=nbytes - 4) == -1 and b"scratch" in lib.gsr_last_error()
    assert bwd(H, W, L, Gh, Gw, n=0) == -1
    assert untouched()
    X = Guarded(BR.identity_grids(1, L, Gh, Gw).numpy())
    tv, part, dX, one = Guarded(np.full(1, 7.0, np.float32)), Guarded(np.full(4, 7.0, np.float64)), Guarded(np.full((1, 12, L, Gh, Gw), 7.0, np.float32)), Guarded(np.ones(1, np.float32))
    for sizes, status in (((0, L, Gh, Gw), -1), ((-1, L, Gh, Gw), -1), ((1, 1, Gh, Gw), -4), ((1, L, Gh, 65), -4)):
        assert lib.gsr_bilagrid_tv(*sizes, X.ptr, part.ptr, tv.ptr, None) == status and lib.gsr_last_error(), sizes
        assert lib.gsr_bilagrid_tv_backward(*sizes, X.ptr, one.ptr, dX.ptr, None) == status, sizes
        assert lib.gsr_bilagrid_tv_partial_count(*sizes) == 0, sizes
    assert lib.gsr_bilagrid_tv(1, L, Gh, Gw, None, part.ptr, tv.ptr, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_bilagrid_tv(1, L, Gh, Gw, X.ptr, None, tv.ptr, None) == -1
    assert lib.gsr_bilagrid_tv(1, L, Gh, Gw, X.ptr, part.ptr, None, None) == -1
    assert lib.gsr_bilagrid_tv_backward(1, L, Gh, Gw, X.ptr, None, dX.ptr, None) == -1
    assert lib.gsr_bilagrid_tv_backward(1, L, Gh, Gw, X.ptr, one.ptr, None, None) == -1
    assert all(bool((b.a == 7.0).all()) and b.intact() for b in (tv, part, dX))


def run_tv(lib, X, dL_dtv=1.0):
    N, _, L, Gh, Gw = X.shape
    n = lib.gsr_bilagrid_tv_partial_count(N, L, Gh, Gw)
    assert n >= 1
    bx, bp, bt = Guarded(X.numpy()), Guarded(np.full(n, np.nan, np.float64)), Guarded(np.full(1, 7.0, np.float32))
    bg, bd = Guarded(np.full(X.shape, 7.0, np.float32)), Guarded(np.full(1, dL_dtv, np.float32))
    assert lib.gsr_bilagrid_tv(N, L, Gh, Gw, bx.ptr, bp.ptr, bt.ptr, None) == 0, lib.gsr_last_error()
    assert lib.gsr_bilagrid_tv_backward(N, L, Gh, Gw, bx.ptr, bd.ptr, bg.ptr, None) == 0, lib.gsr_last_error()
    assert all(b.intact() for b in (bx, bp, bt, bg, bd)) and np.array_equal(bx.a.view(np.int32), X.numpy().view(np.int32))
    return float(bt.a[0]), torch.from_numpy(bg.a.copy())


@pytest.mark.parametrize("N", [1, 3])
def test_total_variation_kernels_are_the_reference(lib, N):
    X = (BR.identity_grids(N, 8, 16, 16) + 0.3 * torch.randn(N, 12, 8, 16, 16, generator=torch.Generator().manual_seed(N))).contiguous()
    x64 = X.double().requires_grad_(True)
    want = BR.total_variation(x64)
    (1.7 * want).backward()
    tv, grad = run_tv(lib, X, dL_dtv=1.7)
    want = want.detach()
    e_tv, e_grad = abs(tv - float(want)) / float(want), float((grad.double() - x64.grad).abs().max() / x64.grad.abs().max())
    print(f"[bilagrid] total variation N {N}: loss {e_tv:.2e}, gradient {e_grad:.2e} (bar 1e-6)", flush=True)
    assert e_tv <= 1e-6 and e_grad <= 1e-6
    tv2, grad2 = run_tv(lib, X, dL_dtv=1.7)
    assert tv2 == tv and torch.equal(bits(grad2), bits(grad))
    small = torch.randn(N, 12, 2, 3, 5, generator=torch.Generator().manual_seed(8))      # unequal sizes, the smallest guidance axis
    s64 = small.double().requires_grad_(True)
    w = BR.total_variation(s64)
    w.backward()
    w = w.detach()
    tv, grad = run_tv(lib, small)
    assert abs(tv - float(w)) <= 1e-6 * float(w) and float((grad.double() - s64.grad).abs().max()) <= 1e-6 * float(s64.grad.abs().max())


def test_total_variation_of_identity_grids_is_exactly_zero(lib):
    tv, grad = run_tv(lib, BR.identity_grids(3, 8, 16, 16))
    assert tv == 0.0 and float(grad.abs().max()) == 0.0


# ---- through the package on the CPU -----------------------------------------------------------------------------------------------------------
def test_package_on_the_host_build(simt_lib):  # noqa: F811
    import fused_bilagrid as FB
    from diff_gaussian_rasterization import GsrError
    H, W, L, Gh, Gw = 33, 130, 3, 5, 4
    grid, image, dL = BR.make_case(H, W, L, Gh, Gw, seed=21)
    with package_on_the_cpu(simt_lib):
        model = FB.BilateralGrid(3, grid_X=Gw, grid_Y=Gh, grid_W=L)
        assert model.grids.shape == (3, 12, L, Gh, Gw) and torch.equal(model.grids.detach(), BR.identity_grids(3, L, Gh, Gw))
        assert torch.allclose(model(image, 1), image, atol=1e-6)      # the identity map
        assert float(model.tv_loss()) == 0.0
        with torch.no_grad():
            model.grids[2] = grid
        im = image.clone().requires_grad_(True)
        out = model(im, 2)
        tv = model.tv_loss()
        ((out * dL).sum() + 10.0 * tv).backward()
        x64 = model.grids.detach().double().requires_grad_(True)
        want_tv = BR.total_variation(x64)
        (10.0 * want_tv).backward()
        assert float(tv) == pytest.approx(float(want_tv), rel=1e-6)
        d_tv = x64.grad
        d_slice = model.grids.grad.double() - d_tv
        assert float(d_slice[:2].abs().max()) <= 1e-6 * float(d_tv.abs().max())      # only slice 2 receives the image's gradient
        BR.check_against_reference(out.detach(), d_slice[2].float(), im.grad, grid, image, dL, "package")
        # no image gradient unless it is asked for
        model.grids.grad = None
        model(image, 2).backward(dL)
        assert float((model.grids.grad[2].double() - d_slice[2]).abs().max()) <= 1e-5 * float(d_slice[2].abs().max())
        frozen = FB.slice_image(model.grids.detach(), im, 2)
        assert frozen.requires_grad
        for bad_grids, bad_image, idx, msg in ((model.grids[:, :11], image, 0, r"\(3, 11, 3, 5, 4\)"), (model.grids, image[:2], 0, r"\(2, 33, 130\)"),
                                               (model.grids, image.double(), 0, "float64"), (model.grids, image, 3, "idx 3"),
                                               (model.grids.detach()[:, :, :1], image, 0, r"2\.\.64")):
            with pytest.raises(GsrError, match=msg):
                FB.slice_image(bad_grids, bad_image, idx)
        with pytest.raises(GsrError, match=r"\(12, 3, 5, 4\)"):
            FB.total_variation_loss(model.grids[0])
    with pytest.raises(GsrError, match="must live on a HIP device"):      # the product has no CPU path
        FB.slice_image(model.grids, image, 0)


def test_recorded_fp32_distance_of_the_training_loop():
    """E2E_FP32_MEASURED of tests/bilagrid_reference.py is a measurement: the loop in fp32 torch must show at least half of what is recorded, so
    that the bar of tests/test_gpu_bilagrid.py (ten times the recorded figure) is not wider than stated, and the loss must fall."""
    first64, last64 = BR.e2e_reference(torch.float64)
    first32, last32 = BR.e2e_reference(torch.float32)
    rel = abs(last32 - last64) / last64
    print(f"[bilagrid] 50 Adam steps on the CPU: fp64 {first64:.6e} -> {last64:.6e}, fp32 {first32:.6e} -> {last32:.6e}, relative difference "
          f"{rel:.2e}; recorded {BR.E2E_FP32_MEASURED:g}", flush=True)
    assert last64 < 0.5 * first64
    assert 0.5 * BR.E2E_FP32_MEASURED <= rel <= 1.5 * BR.E2E_FP32_MEASURED
