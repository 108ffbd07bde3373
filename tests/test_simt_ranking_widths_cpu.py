"""The compile-time-width forms of the ranking primitives (csrc/gsr_wave.h) on the CPU, through the SIMT shim of tests/simt/:

* match_digit<BITS> against the run-time-width loop form, BITS = 1 .. 11, random digits and random valid masks (all valid, none, one lane, a
  prefix of the lanes -- the shape the kernels produce -- and arbitrary ones); lanes_below against popcount(mask & lt_mask) on the same masks;
* the 24-bit emission arithmetic (mul_u24, div_small24) against the full-width forms and the integer division, over the operand range of the
  fused tile sort (instance index in a rectangle and rectangle width up to 65536 tiles) including its corners;
* the whole library (tests/_build/libgsr_simt.so): a 640 x 360 frame -- the smallest whose tile-id halves (5 / 5 bits) have instantiations -- and
  a 64 x 64 one (generic either way) with `ranking_generic` 0 and 1: the same bins, the same image, and the hook `debug_last_ranking_widths`
  names the instantiations that ran.
tests/test_gpu_ranking_widths.py is the comparison of the compiled kernels on the GPU."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

from helpers import make_camera, make_scene, oracle_settings

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

MAX_BITS = 11


@pytest.fixture(scope="module")
def harness():
    from simt_build import build
    return build("ranking")


def valid_masks(rng):
    """[n][256] flags: per wave all / none / one lane / a prefix / arbitrary."""
    out = []
    for kind in ("all", "none", "one", "prefix", "prefix", "random", "random", "sparse"):
        v = np.zeros((4, 64), np.uint8)
        for w in range(4):
            if kind == "all":
                v[w] = 1
            elif kind == "one":
                v[w, rng.integers(64)] = 1
            elif kind == "prefix":
                v[w, :rng.integers(1, 64)] = 1
            elif kind == "random":
                v[w] = rng.integers(0, 2, 64)
            elif kind == "sparse":
                v[w] = rng.random(64) < 0.1
        out.append(v.reshape(256))
    return out


def test_match_digit_template_equals_the_loop_form(harness):
    rng = np.random.default_rng(7)
    loop = np.zeros((MAX_BITS, 256), np.uint64)
    tmpl = np.zeros((MAX_BITS, 256), np.uint64)
    below = np.zeros((MAX_BITS, 256, 2), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cases = 0
    for valid in valid_masks(rng):
        for span in (1 << MAX_BITS, 8, 2, 1):      # all digits different ... all equal
            digit = rng.integers(0, span, 256).astype(np.uint32) | (rng.integers(0, 2, 256).astype(np.uint32) << 20)      # (a bit above the width is ignored)
            assert harness.simt_ranking_match(p(digit), p(valid), p(loop), p(tmpl), p(below)) == 0
            assert np.array_equal(loop, tmpl), "match_digit<BITS> and match_digit(bits) differ"
            assert np.array_equal(below[..., 0], below[..., 1]), "lanes_below is not popcount(mask & lt_mask)"
            # ... and both are the definition
            for bits in (1, 6, 7, 9, MAX_BITS):
                d = digit & ((1 << bits) - 1)
                for w in range(4):
                    dw, vw = d[w * 64:(w + 1) * 64], valid[w * 64:(w + 1) * 64]
                    for lane in (0, 17, 63):
                        want = sum(1 << l for l in range(64) if vw[l] and dw[l] == dw[lane])
                        assert int(loop[bits - 1, w * 64 + lane]) == want
            cases += 1
    assert cases == 32


def test_24_bit_emission_arithmetic(harness):
    rng = np.random.default_rng(11)
    n = 200_000
    b = rng.integers(1, 1 << 16, n).astype(np.uint32)
    q = rng.integers(0, 1 << 16, n).astype(np.uint64)
    a = np.minimum(q * b + rng.integers(0, 1 << 16, n).astype(np.uint64) % b, (1 << 24) - 1).astype(np.uint32)
    a = np.where(a // b < (1 << 16), a, b - 1).astype(np.uint32)
    x = rng.integers(0, 1 << 16, n).astype(np.uint32)
    y = rng.integers(0, (1 << 16) + 1, n).astype(np.uint32)
    # corners: exact multiples and their neighbours (where the reciprocal estimate is off by one), the largest operands
    k = 4096
    b[:k] = rng.integers(1, 1 << 8, k)
    a[:k] = (rng.integers(1, 1 << 16, k) * b[:k].astype(np.uint64)).clip(0, (1 << 24) - 1) + rng.integers(-1, 2, k)
    a[k], b[k], x[k], y[k] = 65535, 1, 65535, 65536
    a[k + 1], b[k + 1], x[k + 1], y[k + 1] = (1 << 24) - 1, 65535, 65536, 65536
    a[k + 2], b[k + 2] = 0, 65535
    assert int((a // b).max()) < (1 << 16) + 1
    p = lambda t: np.ascontiguousarray(t).ctypes.data_as(C.c_void_p)
    assert harness.simt_ranking_arith(n, p(a), p(b), p(x), p(y)) == 0


@pytest.mark.parametrize("W,H,P,hb,lb", [(640, 360, 700, 5, 5), (64, 64, 3000, 0, 0)])
def test_whole_library_same_bins_with_and_without_the_width_instantiations(W, H, P, hb, lb):
    from simt_build import build_library
    import test_simt_abi_cpu as A
    lib = C.CDLL(build_library())
    lib.gsr_last_error.restype = C.c_char_p
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=3, s_med=0.03)
    s = oracle_settings(cam)
    assert lib.gsr_set_option(b"ranking_generic", 2) != 0
    assert lib.gsr_set_option(b"ranking_generic", 0) == 0
    a = A.forward(lib, s, sc, no_backward=True)
    assert a["R"] > 4096 and a["R"] % 4096 != 0
    assert lib.gsr_set_option(b"debug_last_ranking_widths", hb << 4 | lb) == 0, lib.gsr_last_error()
    with A.option(lib, b"ranking_generic", 1, 0):
        b = A.forward(lib, s, sc, no_backward=True)
        assert lib.gsr_set_option(b"debug_last_ranking_widths", 0) == 0, lib.gsr_last_error()
        if hb:
            assert lib.gsr_set_option(b"debug_last_ranking_widths", hb << 4 | lb) != 0
    assert a["R"] == b["R"]
    for k in ("point_list", "ranges", "tiles_touched", "depth_order", "color", "radii"):
        if k in a:
            assert torch.equal(a[k], b[k]), k
