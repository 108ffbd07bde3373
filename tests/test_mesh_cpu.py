"""TSDF fusion and marching tetrahedra without a GPU: tests/mesh_reference.py pinned to hand cases, the kernels of csrc/tsdf.hip -- compiled for the
host with the whole library (tests/simt) and called through the C ABI on guarded numpy buffers -- against it, the invariants of the extracted
meshes, and gsr_scene.mesh with the package on the CPU.  Bars and the fragile set: tests/mesh_reference.py."""
import ctypes as C
import math
import shutil

import numpy as np
import pytest
import torch

import mesh_reference as MR
from test_mip_cpu import GUARD_BYTE, Guarded, camera_objects
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

SWEEP_DIMS = ((2, 2, 2), (1, 5, 5), (9, 8, 7), (33, 21, 18), (70, 5, 3))      # the last: two bricks along x, the second one partial
SWEEP_V = (1, 2, 17)
SWEEP_IMAGES = ((1, 1), (30, 40))      # (H, W)


@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    h = C.CDLL(simt_lib)
    h.gsr_last_error.restype = C.c_char_p
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    h.gsr_tsdf_integrate.argtypes = [i] * 3 + [f] * 6 + [i, vp, i, i] + [vp] * 6
    h.gsr_mesh_scratch_bytes.restype = C.c_size_t
    h.gsr_mesh_scratch_bytes.argtypes = [i] * 3
    h.gsr_mesh_count.argtypes = [i] * 3 + [vp, vp, f, vp, vp, vp]
    h.gsr_mesh_emit.argtypes = [i] * 3 + [f] * 4 + [vp] * 3 + [i] * 2 + [vp] * 4
    return h


class Scratch128(Guarded):
    """`n` bytes of `fill` between guards, 128-byte aligned (Guarded aligns to 64: the aligned half of 64 bytes more, the rest is guard)."""
    def __init__(self, n, fill):
        super().__init__(np.full(n + 64, GUARD_BYTE, dtype=np.uint8))
        self.start += self.a.ctypes.data % 128
        self.a = self.raw[self.start:self.start + n]
        self.a[...] = fill
        assert self.a.ctypes.data % 128 == 0


def run_integrate(lib, dims, origin, voxel, trunc, near, cams, depth, color=None, state=None):
    """-> (tsdf, weight, rgb or None) fp32 [nz,ny,nx] after one call on a fresh volume (or on `state`); guards checked, inputs unchanged."""
    nx, ny, nz = dims
    V, H, W = depth.shape
    fresh = (np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((3, nz, ny, nx), np.float32))
    t, w, c = (Guarded(np.asarray(a, dtype=np.float32)) for a in (state or fresh))
    ins = [Guarded(np.asarray(a, dtype=np.float32)) for a in (cams, depth)] + ([Guarded(color)] if color is not None else [])
    before = [b.a.copy() for b in ins]
    rc = lib.gsr_tsdf_integrate(nx, ny, nz, *(float(v) for v in origin), float(voxel), float(trunc), float(near), V, ins[0].ptr, H, W, ins[1].ptr,
                                ins[2].ptr if color is not None else None, t.ptr, w.ptr, c.ptr if color is not None else None, None)
    assert rc == 0, lib.gsr_last_error()
    assert all(b.intact() for b in ins + [t, w, c]), "the bytes around a buffer were overwritten"
    for b, a in zip(ins, before):
        assert np.array_equal(b.a.view(np.int32), a.view(np.int32)), "an input was written"
    return t.a.copy(), w.a.copy(), (c.a.copy() if color is not None else None)


def run_extract(lib, dims, origin, voxel, tsdf, weight, rgb=None, min_weight=1.0, fill=0x5A):
    """-> (vertices [Nv,3] fp32, faces [Nf,3] int32, colors or None).  The scratch starts as garbage: the calls write what they read."""
    nx, ny, nz = dims
    t, w = Guarded(np.asarray(tsdf, np.float32)), Guarded(np.asarray(weight, np.float32))
    c = Guarded(np.asarray(rgb, np.float32)) if rgb is not None else None
    nbytes = int(lib.gsr_mesh_scratch_bytes(nx, ny, nz))
    assert nbytes > 0 or nx * ny * nz == 0
    scratch = Scratch128(max(nbytes, 128), fill)
    counts = Guarded(np.full(2, -7, dtype=np.int32))
    rc = lib.gsr_mesh_count(nx, ny, nz, t.ptr, w.ptr, float(min_weight), scratch.ptr, counts.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    nv, nf = (int(v) for v in counts.a)
    assert nv >= 0 and nf >= 0
    vertices, faces = Guarded(np.full((nv, 3), 7.0, np.float32)), Guarded(np.full((nf, 3), -9, np.int32))
    colors = Guarded(np.full((nv, 3), 7.0, np.float32)) if rgb is not None else None
    rc = lib.gsr_mesh_emit(nx, ny, nz, *(float(v) for v in origin), float(voxel), t.ptr, c.ptr if c else None, scratch.ptr, nv, nf, vertices.ptr,
                           colors.ptr if colors else None, faces.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    assert all(b.intact() for b in (t, w, scratch, counts, vertices, faces) + ((c, colors) if c else ())), "the bytes around a buffer were overwritten"
    assert np.array_equal(t.a.view(np.int32), np.asarray(tsdf, np.float32).view(np.int32)), "the volume was written"
    return vertices.a.copy(), faces.a.copy(), (colors.a.copy() if colors else None)


# ---- the rule, by hand: the reference and the kernel ------------------------------------------------------------------------------------------
def axis_camera(focal=4.0, width=4.0, height=4.0):
    """A camera at the origin looking down +z, no rotation."""
    return np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, focal, focal, width, height]], dtype=np.float32)


def one_voxel(lib, z, depth_value, trunc=0.25, near=0.05):
    """One voxel at (0, 0, z) under a constant 4 x 4 depth map -> ((tsdf, weight) of the reference, (tsdf, weight) of the kernel)."""
    depth = np.full((1, 4, 4), depth_value, dtype=np.float32)
    ref = MR.integrate((1, 1, 1), (0.0, 0.0, z), 0.1, trunc, near, axis_camera(), depth)
    t, w, _ = run_integrate(lib, (1, 1, 1), (0.0, 0.0, z), 0.1, trunc, near, axis_camera(), depth)
    return (float(ref["tsdf"][0]), float(ref["weight"][0])), (float(t.reshape(-1)[0]), float(w.reshape(-1)[0]))


def test_one_voxel_on_the_optical_axis(lib):
    ref, got = one_voxel(lib, 2.0, 2.125)      # sdf = 0.125 = trunc / 2, every number exact in fp32
    assert ref == (0.5, 1.0) and got == (0.5, 1.0)
    ref, got = one_voxel(lib, 2.0, 9.0)        # far in front of the surface: clamped to 1
    assert ref == (1.0, 1.0) and got == (1.0, 1.0)


def test_sdf_of_exactly_minus_trunc_counts(lib):
    ref, got = one_voxel(lib, 2.0, 1.75)
    assert ref == (-1.0, 1.0) and got == (-1.0, 1.0)
    ref, got = one_voxel(lib, 2.0, 1.5)        # behind the band: not an observation, the fresh voxel stays
    assert ref == (1.0, 0.0) and got == (1.0, 0.0)


def test_a_voxel_behind_the_camera_or_the_near_plane(lib):
    for z in (-2.0, 0.03):
        ref, got = one_voxel(lib, z, 2.0)
        assert ref == (1.0, 0.0) and got == (1.0, 0.0), z


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_an_invalid_depth_pixel(lib, bad):
    ref, got = one_voxel(lib, 2.0, bad)
    assert ref == (1.0, 0.0) and got == (1.0, 0.0)


def test_off_the_image_and_the_pixel_convention(lib):
    """x / z fx + W / 2 with W = 4, fx = 4, z = 2: x = 0.999 -> pixel 3 (inside), x = 1.001 -> 4 (outside), x = -1.001 -> -1 (outside); the depth
    map tells the columns apart."""
    depth = np.zeros((1, 4, 4), dtype=np.float32)
    depth[0, :, 3], depth[0, :, 0], depth[0, :, 2] = 2.125, 1.875, 9.0
    for x, want in ((0.999, (0.5, 1.0)), (1.001, (1.0, 0.0)), (-1.001, (1.0, 0.0)), (-0.999, (-0.5, 1.0)), (0.001, (1.0, 1.0))):
        ref = MR.integrate((1, 1, 1), (x, 0.0, 2.0), 0.1, 0.25, 0.05, axis_camera(), depth)
        t, w, _ = run_integrate(lib, (1, 1, 1), (x, 0.0, 2.0), 0.1, 0.25, 0.05, axis_camera(), depth)
        assert (float(ref["tsdf"][0]), float(ref["weight"][0])) == want, x
        assert (float(t.reshape(-1)[0]), float(w.reshape(-1)[0])) == want, x


def test_two_sequential_calls(lib):
    dims, V, (H, W) = (9, 8, 7), 17, (30, 40)
    origin, cams, depth, color, _ = MR.integrate_case(dims, V, H, W, True)
    args = (dims, origin, np.float32(MR.VOXEL), np.float32(MR.TRUNC), np.float32(MR.NEAR))
    first = MR.integrate(*args, cams[:5], depth[:5], color[:5])
    ref = MR.integrate(*args, cams[5:], depth[5:], color[5:], state=(first["tsdf"], first["weight"], first["rgb"]))
    ref["fragile"] = ref["fragile"] | first["fragile"]
    ref["unit"] = np.maximum(ref["unit"], first["unit"])
    a = run_integrate(lib, *args, cams[:5], depth[:5], color[:5])
    b = run_integrate(lib, *args, cams[5:], depth[5:], color[5:], state=a)
    MR.check_integrate("host, two calls", b[0], b[1], b[2], ref, 12, calls=2)
    # ... and a weight is the count of observations over both calls
    assert float(b[1].max()) > float(a[1].max()) and float(b[1].max()) <= 17


# ---- the kernels over the sweep -------------------------------------------------------------------------------------------------------------
def sweep_case(lib, dims, V, H, W, color):
    origin, cams, depth, col, ref = MR.integrate_case(dims, V, H, W, color)
    got = run_integrate(lib, dims, origin, np.float32(MR.VOXEL), np.float32(MR.TRUNC), np.float32(MR.NEAR), cams, depth, col)
    return origin, got, ref


@pytest.mark.parametrize("V", SWEEP_V)
@pytest.mark.parametrize("dims", SWEEP_DIMS)
def test_integrate_is_the_rule(lib, dims, V):
    for H, W in SWEEP_IMAGES:
        for color in (False, True):
            origin, got, ref = sweep_case(lib, dims, V, H, W, color)
            MR.check_integrate(f"host {dims} V {V} {W}x{H} colour {color}", got[0], got[1], got[2], ref, V)
            again = sweep_case(lib, dims, V, H, W, color)[1]
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got[:2], again[:2]))
            if color:      # colour changes no bit of tsdf and weight
                plain = sweep_case(lib, dims, V, H, W, False)[1]
                assert np.array_equal(plain[0].view(np.int32), got[0].view(np.int32)) and np.array_equal(plain[1], got[1])
            # the extraction of what was fused (dims without a cell: an empty mesh)
            v, f, c = run_extract(lib, dims, origin, np.float32(MR.VOXEL), got[0], got[1], got[2])
            MR.check_mesh(f"host {dims} V {V}", v, f, c, got[0], got[1], got[2], dims, origin, np.float32(MR.VOXEL))
            if min(dims) < 2:
                assert len(v) == 0 and len(f) == 0


def test_sweep_scenes_observe_something():
    """The cases are not vacuous: at the largest size most voxels are observed, some are not, some are clamped and some are inside the band."""
    ref = MR.integrate_case((33, 21, 18), 17, 30, 40, False)[4]
    seen = ref["weight"] > 0
    assert 0.3 < seen.mean() < 1.0 and (ref["tsdf"][seen] < 0).any() and (np.abs(ref["tsdf"][seen]) < 1).mean() > 0.05
    assert ref["weight"].max() >= 5
    one = MR.integrate_case((9, 8, 7), 2, 1, 1, False)[4]
    assert (one["weight"] > 0).any()


def test_recorded_errors_are_what_the_host_build_shows(lib):
    """MEASURED of tests/mesh_reference.py is a measurement: the host build must show at least half of it, so that the device's bar is not wider than
    4 x what is seen; and it stays below the derived bar."""
    worst = {"tsdf_units": 0.0, "rgb_units": 0.0}
    for dims in SWEEP_DIMS:
        for V in SWEEP_V:
            for H, W in SWEEP_IMAGES:
                _, got, ref = sweep_case(lib, dims, V, H, W, True)
                fig = MR.check_integrate("host (recorded)", got[0], got[1], got[2], ref, V)
                worst = {k: max(v, fig[k]) for k, v in worst.items()}
    print("[mesh] largest host-build errors " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()), flush=True)
    for k, v in worst.items():
        assert 0.5 * MR.MEASURED[k] <= v <= MR.MEASURED[k] * 1.0001, (k, v, MR.MEASURED[k])
    assert MR.MEASURED["tsdf_units"] <= MR.derived_units(1) and MR.MEASURED["rgb_units"] <= MR.rgb_derived_units(17)


def test_non_finite_input_is_contained(lib):
    dims, V, (H, W) = (33, 21, 18), 17, (30, 40)
    origin, cams, depth, _, _ = MR.integrate_case(dims, V, H, W, False)
    args = (dims, origin, np.float32(MR.VOXEL), np.float32(MR.TRUNC), np.float32(MR.NEAR))
    bad = cams.copy()
    bad[3, 4], bad[9, 13], bad[16, 10] = np.nan, np.inf, -np.inf
    keep = np.ones(V, dtype=bool)
    keep[[3, 9, 16]] = False
    want = run_integrate(lib, *args, cams[keep], depth[keep])      # a record with a non-finite entry contributes to no voxel: the call without it
    got = run_integrate(lib, *args, bad, depth)
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1], want[1])
    holes = depth.copy()
    holes[:, ::3, ::2] = np.nan
    zeros = depth.copy()
    zeros[:, ::3, ::2] = 0.0
    a, b = run_integrate(lib, *args, cams, holes), run_integrate(lib, *args, cams, zeros)      # a NaN pixel is an invalid pixel, nothing more
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and np.isfinite(a[0]).all()


def test_refusals(lib):
    one = Guarded(np.zeros(64, dtype=np.float32))
    p = one.ptr

    def integrate(nx=1, ny=1, nz=1, voxel=0.1, trunc=0.2, near=0.05, V=1, H=1, W=1, cams=p, depth=p, color=None, tsdf=p, weight=p, rgb=None):
        return lib.gsr_tsdf_integrate(nx, ny, nz, 0.0, 0.0, 0.0, voxel, trunc, near, V, cams, H, W, depth, color, tsdf, weight, rgb, None)

    assert integrate(V=0, cams=None, depth=None, tsdf=None, weight=None) == 0           # no view: nothing to do
    assert integrate(nx=0, cams=None, depth=None, tsdf=None, weight=None) == 0          # an empty volume
    assert integrate(nx=-1) == -1 and b"dimensions" in lib.gsr_last_error()
    assert integrate(nx=2048, ny=2048, nz=512) == -1 and b"2^31" in lib.gsr_last_error()
    assert integrate(V=-1) == -1 and b"V < 0" in lib.gsr_last_error()
    assert integrate(H=0) == -1 and b"1 x 1" in lib.gsr_last_error()
    assert integrate(W=0) == -1 and b"1 x 1" in lib.gsr_last_error()
    for kw in ({"voxel": 0.0}, {"trunc": -1.0}, {"near": -0.1}, {"voxel": math.nan}, {"trunc": math.inf}):
        assert integrate(**kw) == -1 and b"voxel_size > 0" in lib.gsr_last_error(), kw
    for kw in ({"cams": None}, {"depth": None}, {"tsdf": None}, {"weight": None}):
        assert integrate(**kw) == -1 and b"NULL" in lib.gsr_last_error(), kw
    assert integrate(color=p) == -1 and b"together" in lib.gsr_last_error()
    assert integrate(rgb=p) == -1 and b"together" in lib.gsr_last_error()
    # the extraction
    assert lib.gsr_mesh_scratch_bytes(-1, 2, 2) == 0 and lib.gsr_mesh_scratch_bytes(1024, 1024, 1024) == 0 and lib.gsr_mesh_scratch_bytes(512, 512, 512) > 0
    counts = Guarded(np.full(2, -7, dtype=np.int32))
    assert lib.gsr_mesh_count(1, 5, 5, None, None, 1.0, None, counts.ptr, None) == 0 and counts.a.tolist() == [0, 0]      # no cell: no launch
    assert lib.gsr_mesh_count(1024, 1024, 1024, p, p, 1.0, p, counts.ptr, None) == -1 and b"178956970" in lib.gsr_last_error()
    assert lib.gsr_mesh_count(2, 2, 2, p, p, math.nan, p, counts.ptr, None) == -1 and b"NaN" in lib.gsr_last_error()
    assert lib.gsr_mesh_count(2, 2, 2, p, p, 1.0, p, None, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mesh_count(2, 2, 2, None, p, 1.0, p, counts.ptr, None) == -1 and b"NULL" in lib.gsr_last_error()
    off = C.c_void_p(one.a.ctypes.data + 4)
    assert lib.gsr_mesh_count(2, 2, 2, p, p, 1.0, off, counts.ptr, None) == -1 and b"aligned" in lib.gsr_last_error()
    assert lib.gsr_mesh_emit(2, 2, 2, 0.0, 0.0, 0.0, 1.0, None, None, None, 0, 0, None, None, None, None) == 0          # nv == 0: no launch
    assert lib.gsr_mesh_emit(2, 2, 2, 0.0, 0.0, 0.0, 1.0, p, None, p, -1, 0, p, None, p, None) == -1 and b"nv < 0" in lib.gsr_last_error()
    assert lib.gsr_mesh_emit(2, 2, 2, 0.0, 0.0, 0.0, 1.0, p, None, p, 1, 1, None, None, p, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mesh_emit(2, 2, 2, 0.0, 0.0, 0.0, 1.0, p, p, p, 1, 1, p, None, p, None) == -1 and b"together" in lib.gsr_last_error()
    assert one.intact() and counts.intact()


# ---- the extraction on given volumes ----------------------------------------------------------------------------------------------------------
def extraction_volumes():
    sphere, sphere_volume = MR.analytic_volume("sphere")
    torus, torus_volume = MR.analytic_volume("torus")
    noise, ones = MR.noise_volume()
    holes, weight = MR.noise_volume(unobserved=0.15)
    full = np.ones_like(sphere)
    return {"sphere": (sphere, full, sphere_volume, 2), "torus": (torus, full, torus_volume, 0), "noise": (noise, ones, None, None),
            "noise with holes": (holes, weight, None, None)}


@pytest.mark.parametrize("name", ["sphere", "torus", "noise", "noise with holes"])
def test_extraction_equals_the_reference_and_is_a_manifold(lib, name):
    tsdf, weight, analytic, euler = extraction_volumes()[name]
    n = tsdf.shape[0]
    dims, origin, voxel = (n, n, n), (0.0, 0.0, 0.0), 1.0
    rgb = np.random.default_rng(3).random((3, n, n, n), dtype=np.float32)
    v, f, c = run_extract(lib, dims, origin, voxel, tsdf, weight, rgb)
    MR.check_mesh(f"host {name}", v, f, c, tsdf, weight, rgb, dims, origin, voxel)
    assert len(f) > 0
    inv = MR.mesh_invariants(v, f)
    print(f"[mesh] {name}: {inv}", flush=True)
    assert inv["unused"] == 0, "a vertex no face uses"
    assert inv["directed_max"] == 1, "a directed edge occurs twice: two faces disagree about their winding"
    if name != "noise with holes":
        assert inv["per_edge"] == [2], "an open or non-manifold edge on a fully observed volume"
        assert inv["volume"] > 0, "the faces look inward"
    else:
        assert set(inv["per_edge"]) <= {1, 2} and 1 in inv["per_edge"], "holes cut the surface open, nothing else"
        assert (weight == 0).mean() > 0.1
    if analytic is not None:
        assert inv["euler"] == euler
        assert abs(inv["volume"] - analytic) <= 0.05 * analytic, (inv["volume"], analytic)
    if name == "noise":
        assert (tsdf == 0).mean() > 0.05 and np.isfinite(v).all()
        zero_area = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1) == 0
        assert zero_area.any(), "exact zeros collapse faces: they are kept (and wound by the case, not by their geometry)"
    # without colours the same mesh; another garbage in the scratch changes nothing
    v2, f2, none = run_extract(lib, dims, origin, voxel, tsdf, weight, None, fill=0xC3)
    assert none is None and np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f)


def test_min_weight_and_non_finite_voxels_decide_what_is_observed(lib):
    tsdf, _, _, _ = extraction_volumes()["sphere"]
    n = tsdf.shape[0]
    weight = np.full_like(tsdf, 2.0)
    weight[:, :, : n // 2] = 1.0
    args = ((n, n, n), (0.5, -1.0, 2.0), 0.25)
    for mw, whole in ((1.0, True), (2.0, False), (2.5, None)):
        v, f, _ = run_extract(lib, *args, tsdf, weight, None, min_weight=mw)
        MR.check_mesh(f"host min_weight {mw}", v, f, None, tsdf, weight, None, *args, min_weight=mw)
        assert (len(f) == 0) if whole is None else (MR.mesh_invariants(v, f)["per_edge"] == ([2] if whole else [1, 2]))
    poisoned = tsdf.copy()
    poisoned[10, 10, 3], poisoned[4, 9, 9], poisoned[15, 8, 12] = np.nan, np.inf, -np.inf
    v, f, _ = run_extract(lib, *args, poisoned, weight, None)
    MR.check_mesh("host non-finite voxels", v, f, None, poisoned, weight, None, *args)
    assert np.isfinite(v).all() and len(f) > 0


# ---- through gsr_scene.mesh with the package on the CPU ---------------------------------------------------------------------------------------
def test_package_on_the_cpu(simt_lib, tmp_path):  # noqa: F811
    from gsr_scene import mesh
    dims, V, (H, W) = (33, 21, 18), 17, (30, 40)
    origin, cams, depth, color, ref = MR.integrate_case(dims, V, H, W, True)
    t = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    with package_on_the_cpu(simt_lib) as pkg:
        vol = mesh.TSDFVolume(origin.tolist(), float(np.float32(MR.VOXEL)), dims, float(np.float32(MR.TRUNC)), "cpu", color=True, near=float(np.float32(MR.NEAR)))
        assert vol.tsdf.shape == (18, 21, 33) and float(vol.tsdf.min()) == 1.0 and float(vol.weight.max()) == 0.0 and vol.rgb.shape == (3, 18, 21, 33)
        assert vol.integrate(t(depth), camera_objects(t(cams), "focal"), t(color)) is vol
        MR.check_integrate("package", vol.tsdf.numpy(), vol.weight.numpy(), vol.rgb.numpy(), ref, V)
        m = vol.extract()
        assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.colors.shape == m.vertices.shape and len(m.faces) > 0
        MR.check_mesh("package", m.vertices.numpy(), m.faces.numpy(), m.colors.numpy(), vol.tsdf.numpy(), vol.weight.numpy(), vol.rgb.numpy(), dims,
                      origin, np.float32(MR.VOXEL))
        # the sphere comes back: a depth map is sampled at the nearest pixel centre, whose footprint at distance 2 is 2 / 44 = 0.045, and the zero
        # crossing is interpolated over one voxel (0.05): every vertex within the sum of the two of radius 0.37
        radius = m.vertices.double().norm(dim=1)
        assert float((radius - MR.SPHERE_RADIUS).abs().max()) < MR.VOXEL + 2.0 / 44.0
        # [H,W] with one camera is [1,H,W]; packed records pass as they are
        plain = mesh.TSDFVolume(origin.tolist(), float(np.float32(MR.VOXEL)), dims, float(np.float32(MR.TRUNC)), "cpu")
        plain.integrate(t(depth[0]), t(cams[:1]))
        single = MR.integrate(dims, origin, np.float32(MR.VOXEL), np.float32(MR.TRUNC), np.float32(0.05), cams[:1], depth[:1])
        MR.check_integrate("package, one view", plain.tsdf.numpy(), plain.weight.numpy(), None, single, 1)
        assert plain.extract().colors is None
        empty = mesh.TSDFVolume((0, 0, 0), 0.1, (1, 5, 5), 0.4, "cpu").extract()
        assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
        # the PLY round trip
        path = str(tmp_path / "mesh.ply")
        mesh.save_mesh_ply(path, m)
        back = mesh.load_mesh_ply(path)
        assert torch.equal(back.vertices.view(torch.int32), m.vertices.view(torch.int32)) and torch.equal(back.faces, m.faces)
        assert float((back.colors - m.colors).abs().max()) <= 0.5 / 255 + 1e-6
        mesh.save_mesh_ply(path, back)
        again = mesh.load_mesh_ply(path)
        assert torch.equal(again.colors, back.colors) and torch.equal(again.vertices.view(torch.int32), back.vertices.view(torch.int32))
        head = open(path, "rb").read(400)
        assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices\n" in head
        mesh.save_mesh_ply(path, mesh.Mesh(m.vertices, m.faces, None))
        assert mesh.load_mesh_ply(path).colors is None
        mesh.save_mesh_ply(path, empty)
        assert mesh.load_mesh_ply(path).faces.shape == (0, 3)
        open(path, "wb").write(b"ply\nformat ascii 1.0\nend_header\n")
        with pytest.raises(pkg.GsrError, match="not binary little-endian"):
            mesh.load_mesh_ply(path)
        # probe depth
        probe = pkg.PixelProbe(*([torch.full((2, 2), 3.0)] * 2 + [torch.zeros(2, 2, dtype=torch.int32)] * 2 + [torch.zeros(2, 2)] + [torch.zeros(2, 2, dtype=torch.int32)]))
        assert mesh.depth_from_probe(probe) is probe.median_depth
        alpha = torch.tensor([[[0.5, 1.0], [0.0, 0.25]]])
        assert mesh.depth_from_probe(probe, alpha, "expected").tolist() == [[6.0, 3.0], [0.0, 12.0]]
        with pytest.raises(pkg.GsrError, match="needs the rendered alpha"):
            mesh.depth_from_probe(probe, kind="expected")
        with pytest.raises(pkg.GsrError, match="kind must be"):
            mesh.depth_from_probe(probe, kind="mean")
        # the error messages
        with pytest.raises(pkg.GsrError, match=r"depth must be a float32 tensor of shape \[V,H,W\] or \[H,W\]"):
            vol.integrate(t(depth).double(), t(cams), t(color))
        with pytest.raises(pkg.GsrError, match="3 cameras for 17 depth maps"):
            vol.integrate(t(depth), t(cams[:3]), t(color))
        wrong = cams.copy()
        wrong[4, 14] = 41.0
        with pytest.raises(pkg.GsrError, match=r"camera 4 is 41 x 30 \(W x H\), the depth maps are 40 x 30"):
            vol.integrate(t(depth), t(wrong), t(color))
        with pytest.raises(pkg.GsrError, match="color goes with a volume made with color=True"):
            vol.integrate(t(depth), t(cams))
        with pytest.raises(pkg.GsrError, match="color goes with a volume made with color=True"):
            plain.integrate(t(depth), t(cams), t(color))
        with pytest.raises(pkg.GsrError, match="color must be a float32 tensor of shape"):
            vol.integrate(t(depth), t(cams), t(color)[:, :2])
        with pytest.raises(pkg.GsrError, match="2\\^31 or more"):
            mesh.TSDFVolume((0, 0, 0), 0.1, (2048, 2048, 512), 0.4, "cpu")
        with pytest.raises(pkg.GsrError, match="voxel_size > 0"):
            mesh.TSDFVolume((0, 0, 0), 0.0, (4, 4, 4), 0.4, "cpu")
        with pytest.raises(pkg.GsrError, match="three numbers"):
            mesh.TSDFVolume((0, 0), 0.1, (4, 4, 4), 0.4, "cpu")
    with pytest.raises(Exception, match="must live on a HIP device"):      # no CPU path in the product
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4, "cpu")
