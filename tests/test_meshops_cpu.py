"""Mesh clean-up without a GPU: tests/meshops_reference.py pinned to hand cases, and the kernels of csrc/meshops.hip -- compiled for the host with the
whole library (tests/simt) and called through the C ABI on guarded numpy buffers whose scratch starts as garbage -- against it: labels, face counts
and the compaction EQUAL, normals and smoothed positions within MO.HOST_MAX_ULP fp32 ulps at every vertex (no fragile set); then gsr_scene.mesh's
filter_components with the package on the CPU.  One sub-run repeats the composed case under SIMT_SCHEDULE=<seed> (waves and workgroups shuffled)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshops_reference as MO
import test_mesh_cpu as TM
from test_mesh_cpu import Scratch128
from test_mip_cpu import Guarded
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def open_lib(path):
    h = C.CDLL(path)
    h.gsr_last_error.restype = C.c_char_p
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    h.gsr_tsdf_integrate.argtypes = [i] * 3 + [f] * 6 + [i, vp, i, i] + [vp] * 6
    h.gsr_mesh_scratch_bytes.restype = C.c_size_t
    h.gsr_mesh_scratch_bytes.argtypes = [i] * 3
    h.gsr_mesh_count.argtypes = [i] * 3 + [vp, vp, f, vp, vp, vp]
    h.gsr_mesh_emit.argtypes = [i] * 3 + [f] * 4 + [vp] * 3 + [i] * 2 + [vp] * 4
    h.gsr_meshops_scratch_bytes.restype = C.c_size_t
    h.gsr_meshops_scratch_bytes.argtypes = [i] * 2
    h.gsr_mesh_components.argtypes = [i] * 2 + [vp] * 5
    h.gsr_mesh_components_rounds.argtypes = []
    h.gsr_mesh_compact_count.argtypes = [i] * 2 + [vp] * 5
    h.gsr_mesh_compact_emit.argtypes = [i] * 2 + [vp] * 5 + [i] * 2 + [vp] * 4
    h.gsr_mesh_vertex_normals.argtypes = [i] * 2 + [vp] * 5
    h.gsr_mesh_smooth.argtypes = [i] * 2 + [vp, vp, i, f, f, vp, vp, vp]
    return h


@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    return open_lib(simt_lib)


# ---- the calls on guarded buffers ---------------------------------------------------------------------------------------------------------------
def scratch_for(lib, nv, nf, fill):
    nbytes = int(lib.gsr_meshops_scratch_bytes(nv, nf))
    assert nbytes >= 128
    return Scratch128(nbytes, fill)


def checked(bufs, inputs):
    assert all(b.intact() for b in bufs), "the bytes around a buffer were overwritten"
    for b, before in inputs:
        assert MO.same_bits(b.a, before), "an input was written"


def round_cap(nv):
    return 2 * int(np.ceil(np.log2(nv + 1))) + 8


def run_components(lib, nv, faces, fill=0x5A):
    f = Guarded(np.asarray(faces, np.int32).reshape(-1, 3))
    nf = len(f.a)
    label, count, scratch = Guarded(np.full(nv, -7, np.int32)), Guarded(np.full(nv, -9, np.int32)), scratch_for(lib, nv, nf, fill)
    rc = lib.gsr_mesh_components(nv, nf, f.ptr, label.ptr, count.ptr, scratch.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    assert 0 <= lib.gsr_mesh_components_rounds() <= round_cap(nv)
    checked((f, label, count, scratch), [(f, np.asarray(faces, np.int32).reshape(-1, 3))])
    return label.a.copy(), count.a.copy()


def run_compact(lib, vertices, colors, faces, keep, fill=0x5A):
    v, f = Guarded(np.asarray(vertices, np.float32).reshape(-1, 3)), Guarded(np.asarray(faces, np.int32).reshape(-1, 3))
    c = Guarded(np.asarray(colors, np.float32).reshape(-1, 3)) if colors is not None else None
    k = Guarded(np.asarray(keep).astype(np.uint8)) if keep is not None else None
    nv, nf = len(v.a), len(f.a)
    ins = [(b, b.a.copy()) for b in (v, f, c, k) if b is not None]
    scratch, counts = scratch_for(lib, nv, nf, fill), Guarded(np.full(2, -7, np.int32))
    rc = lib.gsr_mesh_compact_count(nv, nf, f.ptr, k.ptr if k else None, scratch.ptr, counts.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    nv2, nf2 = (int(x) for x in counts.a)
    assert 0 <= nv2 <= nv and 0 <= nf2 <= nf
    vo, fo = Guarded(np.full((nv2, 3), 7.0, np.float32)), Guarded(np.full((nf2, 3), -9, np.int32))
    co = Guarded(np.full((nv2, 3), 7.0, np.float32)) if c else None
    rc = lib.gsr_mesh_compact_emit(nv, nf, v.ptr, c.ptr if c else None, f.ptr, k.ptr if k else None, scratch.ptr, nv2, nf2, vo.ptr,
                                   co.ptr if co else None, fo.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    checked([b for b in (v, f, c, k, scratch, counts, vo, fo, co) if b is not None], ins)
    return vo.a.copy(), (co.a.copy() if co else None), fo.a.copy()


def run_normals(lib, vertices, faces, fill=0x5A):
    v, f = Guarded(np.asarray(vertices, np.float32).reshape(-1, 3)), Guarded(np.asarray(faces, np.int32).reshape(-1, 3))
    nv, nf = len(v.a), len(f.a)
    ins = [(b, b.a.copy()) for b in (v, f)]
    out, scratch = Guarded(np.full((nv, 3), 7.0, np.float32)), scratch_for(lib, nv, nf, fill)
    rc = lib.gsr_mesh_vertex_normals(nv, nf, v.ptr, f.ptr, out.ptr, scratch.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    checked((v, f, out, scratch), ins)
    return out.a.copy()


def run_smooth(lib, vertices, faces, iterations, lam, mu, fill=0x5A):
    v, f = Guarded(np.asarray(vertices, np.float32).reshape(-1, 3)), Guarded(np.asarray(faces, np.int32).reshape(-1, 3))
    nv, nf = len(v.a), len(f.a)
    ins = [(b, b.a.copy()) for b in (v, f)]
    out, scratch = Guarded(np.full((nv, 3), 7.0, np.float32)), scratch_for(lib, nv, nf, fill)
    rc = lib.gsr_mesh_smooth(nv, nf, v.ptr, f.ptr, iterations, lam, mu, out.ptr, scratch.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    checked((v, f, out, scratch), ins)
    return out.a.copy()


SMOOTH_CASES = ((1, 0.5, -0.53), (5, 0.5, -0.53), (2, 0.5, 0.0))      # (iterations, lambda, mu)


def keep_masks(nv, faces):
    nf = len(faces)
    rng = np.random.default_rng(nf + 1)
    return [None, rng.random(nf) < 0.6, np.zeros(nf, bool), MO.filter_keep(nv, faces, keep_largest=1), (rng.random(nf) < 0.5).astype(np.uint8) * 200]


def all_outputs(lib, vertices, colors, faces, fill=0x5A):
    """Every operation once -> a list of arrays (the bits two runs must share)."""
    nv = len(vertices)
    out = list(run_components(lib, nv, faces, fill))
    for keep in keep_masks(nv, faces):
        out += [a for a in run_compact(lib, vertices, colors, faces, keep, fill) if a is not None]
    out.append(run_normals(lib, vertices, faces, fill))
    out += [run_smooth(lib, vertices, faces, *s, fill=fill) for s in SMOOTH_CASES]
    return out


def check_case(lib, name, vertices, colors, faces):
    """Every operation against the reference; -> the largest ulp distance of normals and smoothed positions."""
    vertices, faces = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(vertices)
    label, count = run_components(lib, nv, faces)
    want_label, want_count = MO.components(nv, faces)
    assert np.array_equal(label, want_label), f"{name}: labels"
    assert np.array_equal(count, want_count), f"{name}: face counts"
    assert int(count.sum()) == int(MO.is_face(nv, faces).sum())
    for keep in keep_masks(nv, faces):
        for col in (colors, None):
            got, want = run_compact(lib, vertices, col, faces, keep), MO.compact(vertices, col, faces, keep)
            assert MO.same_bits(got[0], want[0]) and MO.same_bits(got[2], want[2]), f"{name}: compaction"
            assert (col is None and got[1] is None) or MO.same_bits(got[1], want[1]), f"{name}: compacted colours"
    worst = 0
    if nv:
        worst = int(MO.ulp_distance(run_normals(lib, vertices, faces), MO.vertex_normals(vertices, faces)).max())
        for it, lam, mu in SMOOTH_CASES:
            worst = max(worst, int(MO.ulp_distance(run_smooth(lib, vertices, faces, it, lam, mu), MO.smooth(vertices, faces, it, lam, mu)).max()))
        assert MO.same_bits(run_smooth(lib, vertices, faces, 3, 0.0, 0.0), vertices), f"{name}: lambda = mu = 0 must return the input"
        assert MO.same_bits(run_smooth(lib, vertices, faces, 0, 0.5, -0.53), vertices), f"{name}: no iteration must return the input"
    print(f"[meshops] {name}: {nv} vertices, {len(faces)} rows, {lib.gsr_mesh_components_rounds()} rounds at the last labelling, "
          f"largest distance {worst} ulp", flush=True)
    assert worst <= MO.HOST_MAX_ULP, f"{name}: {worst} ulp, MO.HOST_MAX_ULP records {MO.HOST_MAX_ULP}"
    return worst


# ---- the reference, by hand ---------------------------------------------------------------------------------------------------------------------
def test_reference_tetrahedron(lib):
    v, f = MO.tetrahedron()
    label, count = MO.components(4, f)
    assert label.tolist() == [0, 0, 0, 0] and count.tolist() == [4, 0, 0, 0]
    n = MO.vertex_normals(v, f)
    third = np.float32(1.0 / np.sqrt(3.0))
    assert MO.ulp_distance(np.abs(n), np.full((4, 3), third)).max() <= 1 and np.array_equal(np.sign(n), np.sign(v))      # +-(1,1,1) / sqrt 3, outward
    # one smoothing step with weight 1 moves a vertex to the mean of the other three: the opposite face's centre, -v / 3
    assert np.allclose(MO.smooth_step(v, f.astype(np.int64), 1.0), -v / 3, atol=1e-6)
    check_case(lib, "tetrahedron", v, None, f)


def test_reference_two_tetrahedra_sharing_one_vertex(lib):
    """Connectivity is by vertex: one component (Open3D's edge-adjacent triangle clusters would be two)."""
    v, f = MO.two_tetrahedra_sharing_a_vertex()
    assert len(v) == 7 and len(f) == 8
    edges = lambda g: {tuple(sorted(e)) for t in g.tolist() for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}  # noqa: E731
    assert not edges(f[:4]) & edges(f[4:]), "the two share a vertex, no edge"
    label, count = MO.components(7, f)
    assert label.tolist() == [0] * 7 and count.tolist() == [8] + [0] * 6
    inv = TM.MR.mesh_invariants(v, f)
    assert inv["directed_max"] == 1 and inv["per_edge"] == [2] and inv["volume"] > 0
    check_case(lib, "two tetrahedra", v, None, f)


def test_reference_rows_that_are_no_faces(lib):
    v, f = MO.tetrahedron()
    v = np.concatenate([v, [[5, 5, 5], [6, 6, 6]]]).astype(np.float32)      # vertices 4, 5: no face uses them
    rows = np.concatenate([[[-1, 0, 1]], f[:2], [[0, 1, 6]], f[2:], [[2, 2, 3]], [[4, 5, 5]]]).astype(np.int32)
    assert MO.is_face(6, rows).tolist() == [False, True, True, False, True, True, False, False]
    label, count = MO.components(6, rows)
    assert label.tolist() == [0, 0, 0, 0, 4, 5] and count.tolist() == [4, 0, 0, 0, 0, 0]
    cv, _, cf = MO.compact(v, None, rows, None)
    assert MO.same_bits(cv, v[:4]) and np.array_equal(cf, f)
    assert MO.same_bits(MO.vertex_normals(v, rows), MO.vertex_normals(v, f)) and not MO.vertex_normals(v, rows)[4:].any()
    assert MO.same_bits(MO.smooth(v, rows, 2, 0.5, -0.53)[4:], v[4:])
    check_case(lib, "rows that are no faces", v, None, rows)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------
def test_empty_and_tiny_inputs(lib):
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    check_case(lib, "nothing", none_v, None, none_f)
    five = np.random.default_rng(1).random((5, 3)).astype(np.float32)
    check_case(lib, "five vertices, no face", five, five, none_f)
    label, count = run_components(lib, 5, none_f)
    assert label.tolist() == [0, 1, 2, 3, 4] and not count.any() and lib.gsr_mesh_components_rounds() == 0
    check_case(lib, "one face", five, five, np.array([[3, 1, 4]], np.int32))
    check_case(lib, "faces, no vertex", none_v, None, np.array([[0, 1, 2]], np.int32))


@pytest.mark.parametrize("order", ["random", "reverse"])
def test_triangle_strip(lib, order):
    """700 faces: many hook rounds, long parent chains in the compress, three workgroups, three sort blocks."""
    v, f = MO.strip(700, order)
    check_case(lib, f"strip, {order} ids", v, None, f)
    label, _ = run_components(lib, len(v), f)
    assert not label.any() and 1 <= lib.gsr_mesh_components_rounds() <= round_cap(len(v))


_extracted = {}


def extracted(lib, name):
    if name not in _extracted:
        if name == "fused":
            origin, got, _ = TM.sweep_case(lib, (33, 21, 18), 17, 30, 40, True)
            _extracted[name] = TM.run_extract(lib, (33, 21, 18), origin, np.float32(TM.MR.VOXEL), got[0], got[1], got[2])
        else:
            tsdf, weight, _, _ = TM.extraction_volumes()[name]
            n = tsdf.shape[0]
            rgb = np.random.default_rng(3).random((3, n, n, n), dtype=np.float32)
            _extracted[name] = TM.run_extract(lib, (n, n, n), (0.0, 0.0, 0.0), 1.0, tsdf, weight, rgb)
    return _extracted[name]


@pytest.mark.parametrize("name", ["sphere", "torus", "noise", "noise with holes", "fused"])
def test_extracted_meshes(lib, name):
    v, f, c = extracted(lib, name)
    assert len(f) > 100
    check_case(lib, name, v, c, f)
    if name == "sphere":      # one closed surface: one component, and the normals look away from the centre
        label, count = run_components(lib, len(v), f)
        assert not label.any() and int(count[0]) == len(f)
        centre = (20 - 1) / 2.0 + np.array([0.13, -0.21, 0.07])
        n = run_normals(lib, v, f)
        assert (np.einsum("ij,ij->i", n.astype(np.float64), v - centre) > 0).all() and np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1, atol=1e-6)
        # Taubin smoothing keeps the size (plain Laplacian smoothing shrinks): the mean radius moves by less than 1 %, without mu by more
        r0 = np.linalg.norm(v - centre, axis=1)
        r1 = np.linalg.norm(run_smooth(lib, v, f, 5, 0.5, -0.53) - centre, axis=1)
        r2 = np.linalg.norm(run_smooth(lib, v, f, 5, 0.5, 0.0) - centre, axis=1)
        assert abs(r1.mean() - r0.mean()) < 0.01 * r0.mean() and r1.std() < 0.1 and r0.mean() - r2.mean() > 2 * abs(r1.mean() - r0.mean())
    if name == "noise":
        assert len(np.unique(MO.components(len(v), f)[0])) >= 3, "several components"


def test_composed_mesh(lib):
    v, c, f = MO.composed()
    nv = len(v)
    assert (~MO.is_face(nv, f)).sum() == 15
    label, count = MO.components(nv, f)
    assert sorted(count[count > 0].tolist()) == [4, 20, 60, 512] and len(np.unique(label)) == 4 + 7
    check_case(lib, "composed", v, c, f)


def composed_bits(lib, out=None, fill=0x5A):
    sv, sf = MO.strip(700, "random")
    res = all_outputs(lib, *MO.composed(), fill=fill) + all_outputs(lib, sv, None, sf, fill=fill)[:2]
    if out:
        np.savez(out, *res)
    return res


def test_two_runs_and_a_shuffled_schedule_give_the_same_bits(lib, simt_lib, tmp_path):  # noqa: F811
    """Other garbage in the scratch changes nothing, and neither does the order of waves and workgroups: integer atomics whose result does not
    depend on their order, no floating-point atomics, every sum in a fixed order."""
    first, second = composed_bits(lib), composed_bits(lib, fill=0xC3)
    assert len(first) == len(second) and all(MO.same_bits(a, b) for a, b in zip(first, second))
    script = tmp_path / "run.py"
    script.write_text(
        "import sys\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {os.path.join(ROOT, 'gaussian-splatting_amd')!r}]\n"
        "import test_meshops_cpu as T\n"
        "T.composed_bits(T.open_lib(sys.argv[1]), sys.argv[2])\n")
    out = tmp_path / "shuffled.npz"
    subprocess.run([sys.executable, str(script), simt_lib, str(out)], check=True, env=dict(os.environ, SIMT_SCHEDULE="7"), cwd=ROOT, timeout=900)
    with np.load(out) as z:
        shuffled = [z[k] for k in z.files]
    assert len(first) == len(shuffled) and all(MO.same_bits(a, b) for a, b in zip(first, shuffled))


def test_non_finite_positions_stay_local(lib):
    v, c, f = MO.composed()
    nv = len(v)
    big = MO.components(nv, f)[0]
    on_sphere = np.flatnonzero(big == np.bincount(big).argmax())
    bad = v.copy()
    sources = [int(on_sphere[10]), int(on_sphere[200])]
    bad[sources[0], 1], bad[sources[1], 2] = np.nan, np.inf
    # labels, counts and compaction do not read positions
    assert all(MO.same_bits(a, b) for a, b in zip(run_components(lib, nv, f), MO.components(nv, f)))
    got, want = run_compact(lib, bad, c, f, None), MO.compact(bad, c, f, None)
    assert MO.same_bits(got[0], want[0]) and MO.same_bits(got[2], want[2])
    far = MO.edge_distance(nv, f, sources, 1) > 1
    clean, poisoned = run_normals(lib, v, f), run_normals(lib, bad, f)
    assert far.sum() > 50 and MO.same_bits(poisoned[far], clean[far]) and not np.isfinite(poisoned[~far]).all()
    assert MO.ulp_distance(poisoned, MO.vertex_normals(bad, f)).max() <= MO.HOST_MAX_ULP
    for it in (1, 2):
        far = MO.edge_distance(nv, f, sources, 2 * it) > 2 * it
        clean, poisoned = run_smooth(lib, v, f, it, 0.5, -0.53), run_smooth(lib, bad, f, it, 0.5, -0.53)
        assert far.sum() > 50 and MO.same_bits(poisoned[far], clean[far]) and not np.isfinite(poisoned[~far]).all()
        assert MO.ulp_distance(poisoned, MO.smooth(bad, f, it, 0.5, -0.53)).max() <= MO.HOST_MAX_ULP


def test_refusals(lib):
    one = Scratch128(4096, 0)
    p = one.ptr
    assert lib.gsr_meshops_scratch_bytes(-1, 0) == 0 and lib.gsr_meshops_scratch_bytes(0, -1) == 0 and lib.gsr_meshops_scratch_bytes(5, 715827883) == 0
    assert lib.gsr_meshops_scratch_bytes(0, 0) >= 128 and lib.gsr_meshops_scratch_bytes(1300000, 2700000) > 0
    assert lib.gsr_mesh_components(-1, 0, p, p, p, p, None) == -1 and b"0 <= nv" in lib.gsr_last_error()
    assert lib.gsr_mesh_components(3, 715827883, p, p, p, p, None) == -1 and b"2^31" in lib.gsr_last_error()
    assert lib.gsr_mesh_components(0, 0, None, None, None, None, None) == 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.gsr_mesh_components(3, 1, *args, None) == -1 and b"NULL" in lib.gsr_last_error()
    off = C.c_void_p(one.a.ctypes.data + 4)
    assert lib.gsr_mesh_components(3, 1, p, p, p, off, None) == -1 and b"aligned" in lib.gsr_last_error()
    counts = Guarded(np.full(2, -7, np.int32))
    assert lib.gsr_mesh_compact_count(0, 3, None, None, None, counts.ptr, None) == 0 and counts.a.tolist() == [0, 0]
    assert lib.gsr_mesh_compact_count(3, 1, p, None, p, None, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mesh_compact_count(3, 1, None, None, p, counts.ptr, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mesh_compact_count(3, 1, p, None, off, counts.ptr, None) == -1 and b"aligned" in lib.gsr_last_error()
    assert lib.gsr_mesh_compact_emit(3, 1, None, None, None, None, None, 0, 0, None, None, None, None) == 0      # nv_out == 0: no launch
    assert lib.gsr_mesh_compact_emit(3, 1, p, None, p, None, p, -1, 0, p, None, p, None) == -1 and b"nv_out < 0" in lib.gsr_last_error()
    assert lib.gsr_mesh_compact_emit(3, 1, p, None, p, None, p, 3, 1, None, None, p, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mesh_compact_emit(3, 1, p, p, p, None, p, 3, 1, p, None, p, None) == -1 and b"together" in lib.gsr_last_error()
    assert lib.gsr_mesh_vertex_normals(3, 1, None, p, p, p, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_mesh_vertex_normals(3, -1, p, p, p, p, None) == -1 and b"0 <= nv" in lib.gsr_last_error()
    assert lib.gsr_mesh_smooth(3, 1, p, p, -1, 0.5, -0.53, p, p, None) == -1 and b"iterations" in lib.gsr_last_error()
    assert lib.gsr_mesh_smooth(3, 1, p, p, 1, float("nan"), -0.53, p, p, None) == -1 and b"NaN" in lib.gsr_last_error()
    assert lib.gsr_mesh_smooth(3, 1, p, p, 1, 0.5, -0.53, p, p, None) == -1 and b"must not be the input" in lib.gsr_last_error()
    assert lib.gsr_mesh_smooth(3, 1, p, p, 1, 0.5, -0.53, None, p, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert one.intact() and counts.intact() and not one.a.any()


# ---- through gsr_scene.mesh with the package on the CPU ---------------------------------------------------------------------------------------
FILTERS = [dict(keep_largest=1), dict(keep_largest=2), dict(min_faces=50), dict(min_faces=50, keep_largest=3), dict(min_faces=5, keep_largest=1),
           dict(min_faces=10000), dict(), dict(keep_largest=99)]


def test_filter_components_and_the_package_on_the_cpu(simt_lib):  # noqa: F811
    from gsr_scene import mesh
    v, c, f = MO.composed(second_60=True)      # two blobs of 60 faces: keep_largest=2 meets a tie at its threshold
    nv = len(v)
    sizes = sorted(MO.components(nv, f)[1][MO.components(nv, f)[1] > 0].tolist())
    assert sizes == [4, 20, 60, 60, 512]
    t = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    with package_on_the_cpu(simt_lib) as pkg:
        m = mesh.Mesh(t(v), t(f), t(c))
        comp = mesh.components(m)
        want = MO.components(nv, f)
        assert comp.vertex_label.dtype == torch.int32 and np.array_equal(comp.vertex_label.numpy(), want[0]) and np.array_equal(comp.face_count.numpy(), want[1])
        kept_faces = {}
        for kw in FILTERS:
            got = mesh.filter_components(m, **kw)
            keep = MO.filter_keep(nv, f, **kw)
            wv, wc, wf = MO.compact(v, c, f, keep)
            assert MO.same_bits(got.vertices.numpy(), wv) and MO.same_bits(got.colors.numpy(), wc) and MO.same_bits(got.faces.numpy(), wf), kw
            kept_faces[tuple(sorted(kw.items()))] = len(wf)
        assert list(kept_faces.values()) == [512, 632, 632, 632, 512, 0, 656, 656]      # keep_largest=2: the two blobs of 60 tie and both stay
        empty = mesh.filter_components(m, min_faces=10000)
        assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.colors.shape == (0, 3)
        assert mesh.filter_components(empty, keep_largest=1).faces.shape == (0, 3) and mesh.components(empty).vertex_label.shape == (0,)
        # compact with bool and uint8 masks; without colours
        mask = np.random.default_rng(8).random(len(f)) < 0.5
        for k in (t(mask), t(mask.astype(np.uint8) * 3)):
            got = mesh.compact(mesh.Mesh(t(v), t(f), None), k)
            wv, _, wf = MO.compact(v, None, f, mask)
            assert got.colors is None and MO.same_bits(got.vertices.numpy(), wv) and MO.same_bits(got.faces.numpy(), wf)
        # normals and smoothing through the package
        assert MO.ulp_distance(mesh.vertex_normals(m).numpy(), MO.vertex_normals(v, f)).max() <= MO.HOST_MAX_ULP
        s = mesh.smooth(m, iterations=2)
        assert s.faces is not None and torch.equal(s.faces, m.faces) and torch.equal(s.colors, m.colors)
        assert MO.ulp_distance(s.vertices.numpy(), MO.smooth(v, f, 2, 0.5, -0.53)).max() <= MO.HOST_MAX_ULP
        assert MO.same_bits(m.vertices.numpy(), v)
        # the error messages
        with pytest.raises(pkg.GsrError, match=r"faces must be an int32 tensor of shape \[Nf,3\], got \(\d+, 3\) torch.int64"):
            mesh.components(mesh.Mesh(t(v), t(f).long(), None))
        with pytest.raises(pkg.GsrError, match=r"faces must be an int32 tensor of shape \[Nf,3\], got \(\d+,\) torch.int32"):
            mesh.vertex_normals(mesh.Mesh(t(v), t(f).reshape(-1), None))
        with pytest.raises(pkg.GsrError, match=r"vertices must be a float32 tensor of shape \[Nv,3\], got \(\d+, 3\) torch.float64"):
            mesh.smooth(mesh.Mesh(t(v).double(), t(f), None))
        with pytest.raises(pkg.GsrError, match="colors must be None or a float32 tensor of shape"):
            mesh.compact(mesh.Mesh(t(v), t(f), t(c)[:5]), None)
        with pytest.raises(pkg.GsrError, match="keep_face must be a bool or uint8 tensor of shape"):
            mesh.compact(m, t(mask[:7]))
        with pytest.raises(pkg.GsrError, match="keep_face must be a bool or uint8 tensor of shape"):
            mesh.compact(m, t(mask.astype(np.int32)))
        with pytest.raises(pkg.GsrError, match="keep_largest must be None or >= 1"):
            mesh.filter_components(m, keep_largest=0)
        with pytest.raises(pkg.GsrError, match="iterations must be >= 0"):
            mesh.smooth(m, iterations=-1)
        with pytest.raises(pkg.GsrError, match="expected a Mesh"):
            mesh.components((t(v), t(f)))
    with pytest.raises(Exception, match="must live on a HIP device"):      # no CPU path in the product
        mesh.components(mesh.Mesh(t(v), t(f), None))
