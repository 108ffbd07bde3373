"""The 3D smoothing filter of Mip-Splatting without a GPU: tests/mip_reference.py pinned to hand cases, the kernels of csrc/mip.hip -- compiled for
the host with the whole library (tests/simt) and called through the C ABI on guarded numpy buffers -- against it, and gsr_scene.mip with the
package on the CPU.  Bars and the fragile set: tests/mip_reference.py."""
import ctypes as C
import math
import shutil
import types

import numpy as np
import pytest
import torch

import mip_reference as MR
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

GUARD, GUARD_BYTE = 64, 0xA5
SWEEP_P = (1, 63, 64, 65, 257, 1027)
SWEEP_C = (1, 2, 17, 65)          # (the kernel stages cameras in no chunk: every record is a scalar load of its own)
ACT_P = (1, 3, 64, 65, 1027)


# ---- the reference, by hand ---------------------------------------------------------------------------------------------------------------
def axis_camera(focal_x=500.0, width=640.0, height=480.0, shift=(0.0, 0.0, 0.0)):
    """A camera at `shift` looking down +z, no rotation: cam = xyz - shift."""
    return torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, -shift[0], -shift[1], -shift[2], focal_x, 1.01 * focal_x, width, height], dtype=torch.float64)


def test_reference_on_the_optical_axis():
    f, seen = MR.compute_3d_filter(torch.tensor([[0.0, 0.0, 2.0]]), axis_camera()[None])
    assert float(f[0]) == pytest.approx(2.0 / 500.0 * math.sqrt(0.2), rel=1e-15) and bool(seen[0])


def test_reference_unseen_takes_the_largest_seen_distance():
    means = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, -1.0], [0.1, 0.0, 3.0], [100.0, 0.0, 1.0]])      # seen, behind, seen, off screen
    f, seen = MR.compute_3d_filter(means, axis_camera()[None])
    assert seen.tolist() == [True, False, True, False]
    assert f.tolist() == pytest.approx([2.0 / 500 * math.sqrt(0.2), 3.0 / 500 * math.sqrt(0.2), 3.0 / 500 * math.sqrt(0.2), 3.0 / 500 * math.sqrt(0.2)])


def test_reference_minimum_over_cameras_and_focal_of_a_blind_camera():
    cams = torch.stack([axis_camera(500.0), axis_camera(400.0, shift=(0.0, 0.0, 1.5)),        # sees the point at z = 0.5
                        axis_camera(800.0, shift=(0.0, 0.0, 50.0))])                            # sees nothing: the point is behind it
    f, seen = MR.compute_3d_filter(torch.tensor([[0.0, 0.0, 2.0]]), cams)
    assert float(f[0]) == pytest.approx(0.5 / 800.0 * math.sqrt(0.2), rel=1e-15) and bool(seen[0])


def test_reference_screen_margin_and_departures():
    cam = axis_camera(500.0, 640.0, 480.0)
    # x / z fx + W / 2 = 1.15 W  <=>  x / z = 0.65 W / fx = 0.832: inside just below, outside just above; the same in y with 0.65 H / fy
    means = torch.tensor([[0.83, 0.0, 1.0], [0.84, 0.0, 1.0], [-0.83, 0.0, 1.0], [-0.84, 0.0, 1.0], [0.0, 0.61, 1.0], [0.0, 0.62, 1.0],
                          [0.0, 0.0, 0.21], [0.0, 0.0, 0.19]])
    _, seen = MR.compute_3d_filter(means, cam[None])
    assert seen.tolist() == [True, False, True, False, True, False, True, False]
    f, seen = MR.compute_3d_filter(torch.tensor([[0.0, 0.0, -1.0], [5.0, 0.0, 1.0]]), cam[None])      # nothing seen: 100000 stays
    assert not bool(seen.any()) and f.tolist() == pytest.approx([100000.0 / 500 * math.sqrt(0.2)] * 2)
    f, seen = MR.compute_3d_filter(torch.tensor([[0.0, 0.0, 2.0], [math.nan, 0.0, 2.0], [0.0, 0.0, math.inf]]), cam[None])
    assert seen.tolist() == [True, False, False] and f.tolist() == pytest.approx([2.0 / 500 * math.sqrt(0.2)] * 3)


def test_reference_activations_limits():
    rs, ro = torch.tensor([[-1.0, 0.5, -3.0]]), torch.tensor([[0.7]])
    s, o = MR.filtered_activations(rs, ro, torch.zeros(1, 1))
    assert torch.allclose(s, torch.exp(rs.double()), rtol=1e-15) and torch.allclose(o, torch.sigmoid(ro.double()), rtol=1e-15)
    f = 1e6
    s, o = MR.filtered_activations(rs, ro, torch.full((1, 1), f))
    want = torch.sigmoid(ro.double()) * torch.exp(rs.double()).prod() / f ** 3      # f >> s: opacity' -> sigma prod s_i / f
    assert float(o) == pytest.approx(float(want), rel=1e-10) and torch.allclose(s, torch.full((1, 3), f, dtype=torch.float64), rtol=1e-10)


# ---- the kernels through the C ABI ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    h = C.CDLL(simt_lib)
    h.gsr_last_error.restype = C.c_char_p
    vp = C.c_void_p
    h.gsr_mip_filter_scratch_bytes.restype = C.c_size_t
    h.gsr_mip_filter_scratch_bytes.argtypes = [C.c_int]
    h.gsr_mip_filter_3d.argtypes = [C.c_int, vp, C.c_int] + [vp] * 5
    h.gsr_mip_activations.argtypes = [C.c_int] + [vp] * 6
    h.gsr_mip_activations_backward.argtypes = [C.c_int] + [vp] * 8
    return h


class Guarded:
    """A copy of `a` with GUARD bytes of GUARD_BYTE before and behind it, its first element 64-byte aligned plus `offset` bytes."""
    def __init__(self, a, offset=0):
        a = np.ascontiguousarray(a)
        self.raw = np.full(a.nbytes + 2 * GUARD + 128, GUARD_BYTE, dtype=np.uint8)
        self.start = (-(self.raw.ctypes.data + GUARD) % 64) + GUARD + offset
        self.a = self.raw[self.start:self.start + a.nbytes].view(a.dtype).reshape(a.shape)
        self.a[...] = a

    @property
    def ptr(self):
        return C.c_void_p(self.a.ctypes.data)

    def intact(self):
        return bool((self.raw[:self.start] == GUARD_BYTE).all()) and bool((self.raw[self.start + self.a.nbytes:] == GUARD_BYTE).all())


def run_sweep(lib, means, cams, want_seen=True):
    """-> filter_3D [P] fp32, seen [P] uint8 or None (torch).  The scratch starts as garbage: the call clears what it needs."""
    P, Cn = int(means.shape[0]), int(cams.shape[0])
    m, c = Guarded(means.numpy()), Guarded(cams.numpy())
    out = Guarded(np.full(P, 7.0, dtype=np.float32))
    seen = Guarded(np.full(P, 9, dtype=np.uint8)) if want_seen else None
    nbytes = int(lib.gsr_mip_filter_scratch_bytes(P))
    assert nbytes >= 8
    scratch = Guarded(np.full(nbytes, 0x5A, dtype=np.uint8))
    rc = lib.gsr_mip_filter_3d(P, m.ptr, Cn, c.ptr, out.ptr, seen.ptr if seen else None, scratch.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    assert all(b.intact() for b in (m, c, out, scratch) + ((seen,) if seen else ())), "the bytes around a buffer were overwritten"
    assert np.array_equal(m.a.view(np.int32), means.numpy().view(np.int32)) and np.array_equal(c.a.view(np.int32), cams.numpy().view(np.int32))
    return torch.from_numpy(out.a.copy()), (torch.from_numpy(seen.a.copy()) if seen else None)


@pytest.mark.parametrize("Cn", SWEEP_C)
@pytest.mark.parametrize("P", SWEEP_P)
def test_sweep_is_upstreams_loop(lib, P, Cn):
    means, cams = MR.scene_reference(P, Cn)[:2]
    got, seen = run_sweep(lib, means, cams)
    assert set(seen.tolist()) <= {0, 1}
    MR.check_sweep("host", got, seen, P, Cn)
    got2, none = run_sweep(lib, means, cams, want_seen=False)      # seen = NULL: the same bits
    assert none is None and torch.equal(got2.view(torch.int32), got.view(torch.int32))


def test_sweep_scenes_exercise_the_unseen_fill():
    for Cn, lo, hi in ((1, 0.2, 0.7), (2, 0.4, 0.9), (65, 0.999, 1.0)):
        share = float(MR.scene_reference(1027, Cn)[3].double().mean())
        assert lo <= share <= hi, (Cn, share)


def test_recorded_sweep_error_is_what_the_host_build_shows(lib):
    """MEASURED['sweep_units'] of tests/mip_reference.py is a measurement: the host build must show at least half of it, so that the bar is not
    wider than 4 x what is seen."""
    worst = 0.0
    for P in SWEEP_P:
        for Cn in SWEEP_C:
            means, cams, want, _, compared, units = MR.scene_reference(P, Cn)
            got, _ = run_sweep(lib, means, cams)
            worst = max(worst, float(((got.double() - want).abs() / units)[compared].max()))
    print(f"[mip] sweep: largest host-build error {worst:.3f} units; recorded {MR.MEASURED['sweep_units']:g}", flush=True)
    assert 0.5 * MR.MEASURED["sweep_units"] <= worst <= MR.MEASURED["sweep_units"] * 1.0001
    assert MR.BARS["sweep_units"] <= MR.SWEEP_CAP_UNITS


def test_sweep_all_unseen_and_exactly_one_seen(lib):
    cam = axis_camera(500.0).float()[None]
    means = torch.tensor([[0.0, 0.0, -1.0], [50.0, 0.0, 1.0], [0.0, 0.0, 0.1]])
    got, seen = run_sweep(lib, means, cam)
    want = np.float32(np.float32(100000.0) / np.float32(500.0)) * np.float32(0.2 ** 0.5)
    assert seen.tolist() == [0, 0, 0] and got.tolist() == [float(want)] * 3
    means = torch.cat([means, torch.tensor([[0.0, 0.0, 2.5]])])[[0, 3, 1, 2]]      # exactly one seen: everybody takes its distance
    got, seen = run_sweep(lib, means, cam)
    want = np.float32(np.float32(2.5) / np.float32(500.0)) * np.float32(0.2 ** 0.5)
    assert seen.tolist() == [0, 1, 0, 0] and got.tolist() == [float(want)] * 4


def test_sweep_focal_maximum_comes_from_a_blind_camera(lib):
    cams = torch.stack([axis_camera(500.0), axis_camera(800.0, shift=(0.0, 0.0, 50.0))]).float()
    got, seen = run_sweep(lib, torch.tensor([[0.0, 0.0, 2.0]]), cams)
    assert seen.tolist() == [1] and float(got[0]) == float(np.float32(np.float32(2.0) / np.float32(800.0)) * np.float32(0.2 ** 0.5))


def test_sweep_contains_non_finite_means(lib):
    P, Cn = 1027, 17
    means, cams = (t.clone() for t in MR.scene_reference(P, Cn)[:2])
    want, want_seen = run_sweep(lib, means, cams)
    bad = means.clone()
    rows = [0, 63, 64, 255, 256, 700, 1023, 1024, 1026]
    assert float(want[rows].max()) < float(want.max())      # (none of them holds the largest distance: the fill value stays what it was)
    for k, row in enumerate(rows):
        bad[row, k % 3] = (math.nan, math.inf, -math.inf)[k % 3]
    got, seen = run_sweep(lib, bad, cams)
    keep = torch.ones(P, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32)), "a clean row changed"
    assert torch.equal(seen[keep], want_seen[keep]) and seen[rows].tolist() == [0] * len(rows)
    clean_top = float(want[keep].max())
    assert got[rows].tolist() == [clean_top] * len(rows)      # the poisoned rows carry the fill value: the largest distance of a seen one


def test_sweep_refusals(lib):
    one = Guarded(np.zeros(16, dtype=np.float32))
    assert lib.gsr_mip_filter_scratch_bytes(-1) == 0 and lib.gsr_mip_filter_scratch_bytes(0) > 0
    assert lib.gsr_mip_filter_3d(0, None, 1, None, None, None, None, None) == 0                     # P == 0: nothing to do
    assert lib.gsr_mip_filter_3d(-1, one.ptr, 1, one.ptr, one.ptr, None, one.ptr, None) == -1 and b"P < 0" in lib.gsr_last_error()
    assert lib.gsr_mip_filter_3d(1, one.ptr, 0, one.ptr, one.ptr, None, one.ptr, None) == -1 and b"camera" in lib.gsr_last_error()
    assert lib.gsr_mip_filter_3d(0, None, 0, None, None, None, None, None) == -1
    for k in range(4):
        args = [one.ptr, one.ptr, one.ptr, one.ptr]
        args[k] = None
        assert lib.gsr_mip_filter_3d(1, args[0], 1, args[1], args[2], None, args[3], None) == -1 and b"NULL" in lib.gsr_last_error()
    off = C.c_void_p(one.a.ctypes.data + 2)
    assert lib.gsr_mip_filter_3d(1, one.ptr, 1, one.ptr, one.ptr, None, off, None) == -1 and b"aligned" in lib.gsr_last_error()
    assert lib.gsr_mip_activations(0, None, None, None, None, None, None) == 0
    assert lib.gsr_mip_activations(-1, None, None, None, None, None, None) == -1
    assert lib.gsr_mip_activations(3, None, None, None, None, None, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mip_activations_backward(0, None, None, None, None, None, None, None, None) == 0
    assert lib.gsr_mip_activations_backward(-1, None, None, None, None, None, None, None, None) == -1
    assert lib.gsr_mip_activations_backward(3, None, None, None, None, None, None, None, None) == -1 and b"NULL" in lib.gsr_last_error()


# ---- activations ----------------------------------------------------------------------------------------------------------------------------
def run_activations(lib, rs, ro, f, gs, go, offset=0):
    """-> scales' [P,3], opacity' [P], dL/draw_scales [P,3], dL/draw_opacity [P] (torch); gs / go may be None."""
    P = int(rs.shape[0])
    ins = [Guarded(t.numpy(), offset) for t in (rs, ro.reshape(-1), f.reshape(-1))]
    grads = [None if t is None else Guarded(t.reshape(s).numpy(), offset) for t, s in ((gs, (P, 3)), (go, (P,)))]
    outs = [Guarded(np.full(s, 7.0, dtype=np.float32), offset) for s in ((P, 3), (P,), (P, 3), (P,))]
    before = [b.a.copy() for b in ins]
    assert lib.gsr_mip_activations(P, *[b.ptr for b in ins], outs[0].ptr, outs[1].ptr, None) == 0, lib.gsr_last_error()
    assert lib.gsr_mip_activations_backward(P, *[b.ptr for b in ins], *[g.ptr if g else None for g in grads], outs[2].ptr, outs[3].ptr,
                                            None) == 0, lib.gsr_last_error()
    assert all(b.intact() for b in ins + outs + [g for g in grads if g]), "the bytes around a buffer were overwritten"
    for b, a in zip(ins, before):
        assert np.array_equal(b.a.view(np.int32), a.view(np.int32)), "an input was written"
    return tuple(torch.from_numpy(o.a.copy()) for o in outs)


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("P", ACT_P)
def test_activations_are_upstreams_expression(lib, P):
    seed = 40 + P
    rs, ro, f, gs, go = MR.activation_case(P, seed)
    got = run_activations(lib, rs, ro, f, gs, go)
    MR.check_activations("host", got, P, seed)
    other = run_activations(lib, rs, ro, f, gs, go, offset=4)      # the 16-byte form and the scalar form are the same arithmetic
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, other))
    # an absent incoming gradient is a zero, through the same arithmetic; and what depends on one gradient only has the bits of the pair
    only_s = run_activations(lib, rs, ro, f, gs, None)
    zero_o = run_activations(lib, rs, ro, f, gs, torch.zeros_like(go))
    assert torch.equal(bits(only_s[2]), bits(zero_o[2])) and torch.equal(bits(only_s[3]), bits(zero_o[3]))
    only_o = run_activations(lib, rs, ro, f, None, go)
    zero_s = run_activations(lib, rs, ro, f, torch.zeros_like(gs), go)
    assert torch.equal(bits(only_o[2]), bits(zero_s[2])) and torch.equal(bits(only_o[3]), bits(zero_s[3]))
    assert torch.equal(bits(only_o[3]), bits(got[3])), "dL/draw_opacity depends on dL/dopacity alone"
    if P >= 3:
        det1 = torch.square(torch.exp(rs)).prod(dim=1)      # upstream's fp32 det1 leaves the normal range on some rows; the kernel does not care
        assert bool((det1 < 1.1754944e-38).any()) and bool(torch.isfinite(got[1]).all()) and bool((got[1] > 0).all())
        assert bool((f == 0).any()) and bool((f > 0).any())


def test_recorded_activation_errors_are_what_the_host_build_shows(lib):
    worst = {}
    for P in ACT_P:
        rs, ro, f, gs, go = MR.activation_case(P, 40 + P)
        fig = MR.check_activations("host (recorded)", run_activations(lib, rs, ro, f, gs, go), P, 40 + P)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in fig.items()}
    print("[mip] activations: largest host-build errors " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()), flush=True)
    for k, v in worst.items():
        assert 0.5 * MR.MEASURED[k] <= v <= MR.MEASURED[k] * 1.0001, (k, v, MR.MEASURED[k])
    assert MR.BARS["draw_scales"] <= MR.GRAD_CAP and MR.BARS["draw_opacity"] <= MR.GRAD_CAP


@pytest.mark.parametrize("offset", [0, 4])
def test_activations_contain_non_finite_rows(lib, offset):
    P = 1027
    rs, ro, f, gs, go = MR.activation_case(P, 77)
    want = run_activations(lib, rs, ro, f, gs, go, offset)
    brs, bro, bf = rs.clone(), ro.clone(), f.clone()
    poison = {0: ("s", math.nan), 1: ("s", math.inf), 2: ("o", math.nan), 3: ("f", math.nan), 6: ("s", -math.inf), 258: ("o", math.inf),
              513: ("o", -math.inf), 1020: ("s", 200.0), 1024: ("s", math.nan), 1025: ("f", math.inf), 1026: ("o", math.nan)}
    for row, (what, value) in poison.items():
        if what == "s":
            brs[row, row % 3] = value
        elif what == "o":
            bro[row, 0] = value
        else:
            bf[row, 0] = value
    got = run_activations(lib, brs, bro, bf, gs, go, offset)
    rows = torch.tensor(sorted(poison))
    keep = torch.ones(P, dtype=torch.bool)
    keep[rows] = False
    for g, w in zip(got, want):
        assert torch.equal(bits(g[keep]), bits(w[keep])), "a clean row changed"
    assert float(got[2][rows].abs().max()) == 0.0 and float(got[3][rows].abs().max()) == 0.0, "a poisoned row has a gradient"
    assert float(want[2][rows].abs().max()) > 0.0 and float(want[3][rows].abs().max()) > 0.0      # (they do have gradients without the poison)
    for row, (what, value) in poison.items():
        row_out = torch.cat([got[0][row], got[1][row:row + 1]])
        if math.isnan(value) or (what, value) in (("s", math.inf), ("s", 200.0), ("f", math.inf)):
            assert not bool(torch.isfinite(row_out).all()), (row, what, value)      # NaN, and what overflows: non-finite outputs, in this row only
        else:
            assert bool(torch.isfinite(row_out).all()), (row, what, value)          # the saturating infinities give their limits
    assert float(got[1][6]) == 0.0 and float(got[1][513]) == 0.0                    # exp(-inf) = 0 and sigmoid(-inf) = 0: opacity 0


# ---- through gsr_scene.mip with the package on the CPU --------------------------------------------------------------------------------------
def camera_objects(cams, flavour):
    """The packed records as camera objects of Mip-Splatting (`focal`) or of the reference (`fov`)."""
    out = []
    for c in cams.double():
        R, T, (fx, fy, w, h) = c[:9].reshape(3, 3).numpy(), c[9:12].numpy(), (float(v) for v in c[12:16])
        cam = types.SimpleNamespace(R=R, T=T, image_width=int(w), image_height=int(h))
        if flavour == "focal":
            cam.focal_x, cam.focal_y = fx, fy
        else:
            cam.FoVx, cam.FoVy = 2.0 * math.atan(w / (2.0 * fx)), 2.0 * math.atan(h / (2.0 * fy))
        out.append(cam)
    return out


def test_pack_cameras_from_both_flavours():
    from gsr_scene import mip
    cams = MR.scene_reference(1027, 17)[1]
    a = mip.pack_cameras(camera_objects(cams, "focal"), "cpu")
    b = mip.pack_cameras(camera_objects(cams, "fov"), "cpu")
    assert a.shape == (17, 16) and a.dtype == torch.float32 and torch.equal(a, cams)
    assert torch.allclose(b, cams, rtol=1e-6, atol=0) and mip.pack_cameras(cams, "cpu") is not None and torch.equal(mip.pack_cameras(cams, "cpu"), cams)
    with pytest.raises(Exception, match="at least one camera"):
        mip.pack_cameras([], "cpu")
    with pytest.raises(Exception, match=r"packed cameras must be \[C,16\]"):
        mip.pack_cameras(torch.zeros(3, 15), "cpu")
    with pytest.raises(Exception, match="camera 0 needs R, T"):
        mip.pack_cameras([types.SimpleNamespace(R=np.eye(3), T=np.zeros(3))], "cpu")


def test_package_on_the_cpu(simt_lib):  # noqa: F811
    from gsr_scene import mip
    P, Cn = 1027, 2
    means, cams = MR.scene_reference(P, Cn)[:2]
    rs, ro, f, gs, go = MR.activation_case(P, 40 + P)
    with package_on_the_cpu(simt_lib) as pkg:
        filt, seen = mip.compute_3d_filter(means, camera_objects(cams, "focal"), return_seen=True)
        assert filt.shape == (P, 1) and filt.dtype == torch.float32 and seen.shape == (P,) and seen.dtype == torch.bool
        MR.check_sweep("package", filt.reshape(-1), seen, P, Cn)
        assert torch.equal(mip.compute_3d_filter(means, cams), filt) and not filt.requires_grad
        assert mip.compute_3d_filter(means[:0], cams).shape == (0, 1)
        a, b = rs.clone().requires_grad_(True), ro.clone().requires_grad_(True)
        s, o = mip.filtered_activations(a, b, f)
        assert s.shape == (P, 3) and o.shape == (P, 1)
        ((s * gs).sum() + (o * go).sum()).backward()
        MR.check_activations("package", (s.detach(), o.detach(), a.grad, b.grad), P, 40 + P)
        a2, b2 = rs.clone().requires_grad_(True), ro.clone().requires_grad_(True)      # one output unused: its gradient goes in as NULL
        s2, _ = mip.filtered_activations(a2, b2, f)
        (s2 * gs).sum().backward()
        assert float(b2.grad.abs().max()) == 0.0 and float(a2.grad.abs().max()) > 0.0
        # fuse: plain activations of the fused raw parameters are the filtered values
        fs, fo = mip.fuse(rs, ro, f)
        assert fs.shape == (P, 3) and fo.shape == (P, 1) and not fs.requires_grad
        assert torch.allclose(torch.exp(fs), s.detach(), rtol=1e-5, atol=0)
        assert torch.allclose(torch.sigmoid(fo), o.detach(), rtol=2e-5, atol=1e-30)
        big = mip.fuse(torch.zeros(1, 3), torch.full((1, 1), 40.0), torch.zeros(1, 1))[1]      # sigmoid = 1: clamped, the logit stays finite
        assert bool(torch.isfinite(big).all())
        with pytest.raises(pkg.GsrError, match=r"raw_opacity must be a float32 tensor of shape \(1027, 1\)"):
            mip.filtered_activations(rs, ro.reshape(-1), f)
        with pytest.raises(pkg.GsrError, match="filter_3D must be a float32 tensor"):
            mip.filtered_activations(rs, ro, f.double())
        with pytest.raises(pkg.GsrError, match=r"means3D must be a float32 tensor of shape \[P,3\]"):
            mip.compute_3d_filter(means.reshape(-1), cams)
    with pytest.raises(Exception, match="must live on a HIP device"):      # no CPU path in the product
        mip.compute_3d_filter(means, cams)
    with pytest.raises(Exception, match="must live on a HIP device"):
        mip.filtered_activations(rs, ro, f)
