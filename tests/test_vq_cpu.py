"""Vector quantisation without a GPU: tests/vq_reference.py pinned to hand cases, the kernels of csrc/vq.hip -- compiled for the host with the whole
library (tests/simt; the matrix instruction through the __shfl form of csrc/gsr_mfma.h, the same fmaf chain) and called through the C ABI on
guarded numpy buffers -- against it, and gsr_scene.compress with the package on the CPU.  Bars: tests/vq_reference.py."""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import vq_reference as VR
from test_mip_cpu import Guarded
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (P, K, D): every P of {1, 31, 32, 33, 129, 1027}, K of {1, 2, 31, 33, 129, 4097} and D of {1, 2, 3, 7, 45, 48, 64} at least once; a workgroup owns 256
# rows (two tiles of 32 per wave), a stage 64 centroids (two tiles), the dimension is padded to 8, 16, 32, 48 or 64.  P K D <= 8 M, and the large K with
# the small D: a matrix instruction is 34 fiber round trips per wave in the host build.
SHAPES = [(1, 1, 1), (31, 2, 2), (32, 31, 3), (33, 33, 7), (129, 129, 45), (1027, 31, 48), (1027, 129, 3), (1, 4097, 2), (31, 4097, 7), (33, 129, 64),
          (129, 33, 64), (1027, 2, 45)]


# ---- the reference, by hand ---------------------------------------------------------------------------------------------------------------
def test_reference_two_clusters_in_one_dimension():
    rows = np.array([[0.0], [0.2], [0.1], [5.0], [5.2]])
    idx, d2 = VR.assign64(rows, np.array([[1.0], [4.0]]))
    assert idx.tolist() == [0, 0, 0, 1, 1] and d2.tolist() == pytest.approx([1.0, 0.64, 0.81, 1.0, 1.44])
    c, m = VR.update64(rows, None, idx, np.array([[1.0], [4.0]]))
    assert c[:, 0].tolist() == pytest.approx([0.1, 5.1]) and m.tolist() == [3.0, 2.0]


def test_reference_tie_goes_to_the_lower_index():
    idx, d2 = VR.assign64(np.array([[0.0, 0.0]]), np.array([[3.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]]))
    assert idx.tolist() == [1] and d2.tolist() == [1.0]


def test_reference_empty_cluster_keeps_its_centroid():
    c, m = VR.update64(np.array([[1.0], [3.0]]), None, np.array([0, 0]), np.array([[0.0], [77.0]]))
    assert c[:, 0].tolist() == [2.0, 77.0] and m.tolist() == [2.0, 0.0]


def test_reference_weighted_mean_and_bad_weights():
    rows = np.array([[1.0], [2.0], [4.0], [100.0], [200.0]])
    c, m = VR.update64(rows, np.array([1.0, 3.0, 0.5, -2.0, math.nan]), np.array([0, 0, 0, 0, 0]), np.array([[9.0]]))
    assert float(c[0, 0]) == pytest.approx((1.0 + 6.0 + 2.0) / 4.5) and m.tolist() == [4.5]


def test_reference_leaves_out_unassigned_rows():
    rows = np.array([[1.0], [math.nan], [3.0]])
    idx, d2 = VR.assign64(rows, np.array([[0.0], [math.inf]]))
    assert idx.tolist() == [0, -1, 0] and d2.tolist() == [1.0, 0.0, 9.0]
    c, m = VR.update64(rows, None, idx, np.array([[0.0], [5.0]]))
    assert c[:, 0].tolist() == [2.0, 5.0] and m.tolist() == [2.0, 0.0]
    assert VR.assign64(rows, np.array([[math.nan], [math.inf]]))[0].tolist() == [-1, -1, -1]


# ---- the kernels through the C ABI ----------------------------------------------------------------------------------------------------------
def open_lib(path):
    h = C.CDLL(path)
    h.gsr_last_error.restype = C.c_char_p
    vp = C.c_void_p
    h.gsr_vq_scratch_bytes.restype = C.c_size_t
    h.gsr_vq_scratch_bytes.argtypes = [C.c_int] * 3
    h.gsr_vq_assign.argtypes = [C.c_int] * 3 + [vp] * 6
    h.gsr_vq_update.argtypes = [C.c_int] * 3 + [vp] * 7
    return h


@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    return open_lib(simt_lib)


def scratch_for(lib, P, D, K):
    nbytes = int(lib.gsr_vq_scratch_bytes(P, D, K))
    assert nbytes > 0
    return Guarded(np.full(nbytes, 0x5A, dtype=np.uint8))      # garbage: the calls clear what they need


def run_assign(lib, rows, codebook):
    """-> idx [P] int32, dist2 [P] fp32 (numpy)."""
    (P, D), K = rows.shape, int(codebook.shape[0])
    r, c = Guarded(rows.numpy()), Guarded(codebook.numpy())
    idx, d2 = Guarded(np.full(P, 77, dtype=np.int32)), Guarded(np.full(P, 7.0, dtype=np.float32))
    scratch = scratch_for(lib, P, D, K)
    rc = lib.gsr_vq_assign(P, D, K, r.ptr, c.ptr, idx.ptr, d2.ptr, scratch.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    assert all(b.intact() for b in (r, c, idx, d2, scratch)), "the bytes around a buffer were overwritten"
    assert np.array_equal(r.a.view(np.int32), rows.numpy().view(np.int32)) and np.array_equal(c.a.view(np.int32), codebook.numpy().view(np.int32))
    return idx.a.copy(), d2.a.copy()


def run_update(lib, rows, weights, idx, codebook):
    """-> codebook' [K,D] fp32 (torch), mass [K] fp32 (numpy)."""
    (P, D), K = rows.shape, int(codebook.shape[0])
    r, c, i = Guarded(rows.numpy()), Guarded(codebook.numpy()), Guarded(np.asarray(idx, dtype=np.int32))
    w = Guarded(weights.numpy()) if weights is not None else None
    mass = Guarded(np.full(K, 7.0, dtype=np.float32))
    scratch = scratch_for(lib, P, D, K)
    rc = lib.gsr_vq_update(P, D, K, r.ptr, w.ptr if w else None, i.ptr, c.ptr, mass.ptr, scratch.ptr, None)
    assert rc == 0, lib.gsr_last_error()
    assert all(b.intact() for b in (r, c, i, mass, scratch) + ((w,) if w else ())), "the bytes around a buffer were overwritten"
    return torch.from_numpy(c.a.copy()), mass.a.copy()


@pytest.mark.parametrize("kind", list(VR.KINDS))
@pytest.mark.parametrize("P,K,D", SHAPES)
def test_assignment_is_the_fp64_argmin_within_the_fp32_bound(lib, P, K, D, kind):
    rows, cb = VR.case(P, K, D, kind)
    idx, d2 = run_assign(lib, rows, cb)
    want = VR.check_assign(f"host {P}x{K}x{D} {kind}", rows, cb, idx, d2)
    if kind == "centred" and D >= 3:
        assert np.array_equal(idx, want)      # (without an offset the fp32 scores never reorder these draws)


def test_shapes_cover_every_size_of_the_issue():
    assert {s[0] for s in SHAPES} == {1, 31, 32, 33, 129, 1027} and {s[1] for s in SHAPES} == {1, 2, 31, 33, 129, 4097}
    assert {s[2] for s in SHAPES} == {1, 2, 3, 7, 45, 48, 64} and all(p * k * d <= 8 << 20 for p, k, d in SHAPES)


def test_exact_tie_goes_to_the_lowest_index(lib):
    """Duplicated centroids give bit-equal scores: across lanes, across the two tiles of a stage, and across stages."""
    rows, cb = VR.case(129, 200, 7, "centred", seed=3)
    for k in (5, 33, 70, 150):      # row 10's own position four times: another tile of the stage, the next stage, a later one
        cb[k] = rows[10]
    for k in (40, 41, 199):         # row 20's: the neighbouring lane, the last stage
        cb[k] = rows[20]
    idx, d2 = run_assign(lib, rows, cb)
    VR.check_assign("host ties", rows, cb, idx, d2)
    assert idx[10] == 5 and idx[20] == 40 and d2[10] == 0 and d2[20] == 0 and not np.isin(idx, [33, 70, 150, 41, 199]).any()


@pytest.mark.parametrize("P,K,D", [(1027, 33, 2), (129, 129, 45), (300, 7, 64)])
def test_planted_clusters_are_recovered(lib, P, K, D):
    rows, label, init = VR.planted(P, K, D)
    idx, d2 = run_assign(lib, rows, init)
    assert np.array_equal(idx, label.numpy())
    cb, mass = run_update(lib, rows, None, idx, init)
    VR.check_update("host planted", rows, None, idx, init, cb, mass)
    idx2, _ = run_assign(lib, rows, cb)
    assert np.array_equal(idx2, label.numpy()) and np.array_equal(mass, np.bincount(label.numpy(), minlength=K).astype(np.float32))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("P,K,D", [(1, 1, 1), (33, 2, 3), (129, 33, 64), (1027, 40, 45), (1027, 3, 7), (70, 4097, 2)])
def test_update_is_the_fp64_weighted_mean(lib, P, K, D, weighted):
    """(1027, 3, 7): segments longer than a chunk of 256 rows; (70, 4097, 2): most clusters empty, 13 key bits."""
    rows, cb = VR.case(P, K, D, "offset10", seed=1)
    idx, _ = run_assign(lib, rows, cb)
    weights = None
    if weighted:
        weights = torch.rand(P, generator=torch.Generator().manual_seed(P + K)) + 0.01
        weights[::7] = 0.0
    got, mass = run_update(lib, rows, weights, idx, cb)
    VR.check_update(f"host {P}x{K}x{D} w={weighted}", rows, weights, idx, cb, got, mass)
    if K > P:
        assert int((mass == 0).sum()) >= K - P


def test_unassigned_rows_and_bad_weights_are_left_out(lib):
    P, K, D = 300, 9, 5
    rows, cb = VR.case(P, K, D, "centred", seed=2)
    idx, _ = run_assign(lib, rows, cb)
    idx[[0, 17, 299]] = -1
    idx[idx == 4] = 3                                   # cluster 4 ends empty
    weights = torch.ones(P)
    weights[5], weights[6], weights[7], weights[8] = -1.0, math.nan, math.inf, 0.0
    bad_rows = rows.clone()
    bad_rows[0], bad_rows[17, 2], bad_rows[8, 1] = math.nan, math.inf, math.nan      # rows nobody owns, and one of weight 0: whatever they hold
    got, mass = run_update(lib, bad_rows, weights, idx, cb)
    VR.check_update("host left out", rows, weights, idx, cb, got, mass)
    assert mass[4] == 0 and bool(torch.isfinite(got).all())


POISON = [math.nan, math.inf, -math.inf]


@pytest.mark.parametrize("value", POISON)
def test_a_poisoned_row_stays_to_itself(lib, value):
    rows, cb = VR.case(129, 70, 7, "centred", seed=4)
    want_i, want_d = run_assign(lib, rows, cb)
    bad = rows.clone()
    for row, col in ((0, 0), (31, 6), (32, 3), (100, 1), (128, 5)):
        bad[row, col] = value
    idx, d2 = run_assign(lib, bad, cb)
    keep = np.ones(129, dtype=bool)
    keep[[0, 31, 32, 100, 128]] = False
    assert (idx[~keep] == -1).all() and (d2[~keep] == 0).all()
    assert np.array_equal(idx[keep], want_i[keep]) and np.array_equal(d2[keep].view(np.int32), want_d[keep].view(np.int32))


@pytest.mark.parametrize("value", POISON)
def test_a_poisoned_centroid_never_wins(lib, value):
    rows, cb = VR.case(129, 70, 7, "centred", seed=5)
    clean_i, _ = run_assign(lib, rows, cb)
    bad = cb.clone()
    losers = [int(np.bincount(clean_i).argmax()), 0, 69]
    for k in losers:
        bad[k, k % 7] = value
    idx, d2 = run_assign(lib, rows, bad)
    assert not np.isin(idx, losers).any() and idx.min() >= 0
    want, _ = VR.assign64(rows.numpy(), bad.numpy())
    assert np.array_equal(idx, want)
    bad[:, 2] = value                                   # no centroid is finite
    idx, d2 = run_assign(lib, rows, bad)
    assert (idx == -1).all() and (d2 == 0).all()


def test_limits_are_refused(lib):
    buf = Guarded(np.zeros(4096, dtype=np.float32))
    for P, D, K in ((-1, 3, 4), (5, 0, 4), (5, 65, 4), (5, 3, 0), (5, 3, 65537)):
        assert lib.gsr_vq_scratch_bytes(P, D, K) == 0
        assert lib.gsr_vq_assign(P, D, K, buf.ptr, buf.ptr, buf.ptr, buf.ptr, buf.ptr, None) != 0 and b"vq:" in lib.gsr_last_error()
        assert lib.gsr_vq_update(P, D, K, buf.ptr, None, buf.ptr, buf.ptr, buf.ptr, buf.ptr, None) != 0
    assert lib.gsr_vq_scratch_bytes(5, 64, 65536) > 0 and lib.gsr_vq_assign(0, 3, 4, None, None, None, None, None, None) == 0
    mass = Guarded(np.full(4, 7.0, dtype=np.float32))
    assert lib.gsr_vq_update(0, 3, 4, None, None, None, buf.ptr, mass.ptr, None, None) == 0 and (mass.a == 0).all() and mass.intact()


def lloyd_step_bits(lib, out=None):
    rows, cb = VR.case(300, 129, 45, "offset10", seed=6)
    weights = torch.rand(300, generator=torch.Generator().manual_seed(9)) + 0.01
    idx, d2 = run_assign(lib, rows, cb)
    got, mass = run_update(lib, rows, weights, idx, cb)
    res = [torch.from_numpy(idx), torch.from_numpy(d2).view(torch.int32), got.view(torch.int32), torch.from_numpy(mass).view(torch.int32)]
    if out:
        torch.save(res, out)
    return res


def test_two_runs_and_a_shuffled_schedule_give_the_same_bits(lib, simt_lib, tmp_path):  # noqa: F811
    """No floating-point atomics and a fixed order of every sum: a second run, and runs with the waves and workgroups shuffled, are bit-equal."""
    first, second = lloyd_step_bits(lib), lloyd_step_bits(lib)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, ctypes as C\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {os.path.join(ROOT, 'gaussian-splatting_amd')!r}]\n"
        "import test_vq_cpu as T\n"
        "T.lloyd_step_bits(T.open_lib(sys.argv[1]), sys.argv[2])\n")
    for sched in ("5", "11"):
        env = dict(os.environ, SIMT_SCHEDULE=sched)
        out = tmp_path / f"s{sched}.pt"
        subprocess.run([sys.executable, str(script), simt_lib, str(out)], check=True, env=env, cwd=ROOT, timeout=900)
        assert all(torch.equal(a, b) for a, b in zip(first, torch.load(out)))


# ---- gsr_scene.compress with the package on the CPU -----------------------------------------------------------------------------------------
def lloyd_by_hand(GC, rows, init, weights, iters):
    """kmeans' own loop over GC._Lloyd on the centred rows, keeping every iteration's codebook: -> [(codebook, idx, inertia)] (no re-seeding)."""
    P, D = rows.shape
    w64 = torch.from_numpy(VR.clean_weights(None if weights is None else weights.numpy(), P))
    mean = (rows.double() * w64[:, None]).sum(dim=0) / w64.sum()
    x, cb = (rows.double() - mean).float().contiguous(), (init.double() - mean).float().contiguous()
    L = GC._Lloyd(P, D, int(init.shape[0]), rows.device)
    out = []
    for _ in range(iters):
        idx, dist2 = L.assign(x, cb)
        out.append((cb.clone(), idx, float((w64 * dist2.double()).sum())))
        L.update(x, weights, idx, cb)
    return x, out


def test_kmeans_on_the_cpu_package(simt_lib):  # noqa: F811
    from gsr_scene import compress as GC
    P, K, D = 600, 12, 6
    rows = VR.case(P, 1, D, "offset10", seed=9)[0]      # ONE blob: nothing to separate, the inertia falls by a few per cent per step
    weights = torch.rand(P, generator=torch.Generator().manual_seed(3)) + 0.1
    with package_on_the_cpu(simt_lib) as pkg:
        for w in (None, weights):
            cb, idx, inertia = GC.kmeans(rows, K, weights=w, iters=6, init=rows[:K].clone())
            assert cb.shape == (K, D) and cb.dtype == torch.float32 and idx.shape == (P,) and idx.dtype == torch.int32
            assert inertia.shape == (6,) and inertia.dtype == torch.float64 and int(idx.min()) >= 0 and int(idx.max()) < K
            x, steps = lloyd_by_hand(GC, rows, rows[:K], w, 6)
            assert [s[2] for s in steps] == inertia.tolist() and torch.equal(steps[-1][1], idx)
            for (_, _, before), (c_now, i_now, after) in zip(steps[:-1], steps[1:]):
                tol = VR.lloyd_step_tolerance(x.numpy(), None if w is None else w.numpy(), c_now.numpy(), i_now.numpy(), before, after)
                print(f"[kmeans] inertia {before:.9g} -> {after:.9g}, may rise by {tol:.3g}")
                assert after <= before + tol and tol < 1e-3 * before      # Lloyd: no step raises the inertia beyond what the fp32 arithmetic may lose
            assert float(inertia[-1]) < 0.99 * float(inertia[0])
            # the codebook is the fp64 weighted mean of the last assignment, taken over the rows as given
            want, mass = VR.update64(rows.numpy(), None if w is None else w.numpy(), idx.numpy(), cb.double().numpy())
            assert (mass > 0).all() and (np.abs(cb.double().numpy() - want) <= VR.ulp32(want)).all()
            again = GC.kmeans(rows, K, weights=w, iters=6, init=rows[:K].clone())
            assert all(torch.equal(a, b) for a, b in zip((cb, idx, inertia), again))
        cb, idx, inertia = GC.kmeans(rows, K, iters=3, generator=torch.Generator().manual_seed(11))      # K distinct rows drawn with the generator
        pick = torch.randperm(P, generator=torch.Generator().manual_seed(11))[:K]
        assert all(torch.equal(a, b) for a, b in zip((cb, idx, inertia), GC.kmeans(rows, K, iters=3, init=rows[pick].clone())))
        # K = P from the rows themselves: every row is its own centroid, bit for bit, whatever the mean
        small = VR.case(97, 1, 6, "offset10", seed=8)[0]
        cb, idx, inertia = GC.kmeans(small, 97, iters=2, init=small.clone())
        assert torch.equal(cb.view(torch.int32), small.view(torch.int32)) and torch.equal(idx, torch.arange(97, dtype=torch.int32))
        assert inertia.tolist() == [0.0, 0.0]
        # empty clusters are re-seeded: three far-away initial centroids end up used
        init = rows[:K].clone()
        init[:3] += 1e4
        cb, idx, inertia = GC.kmeans(rows, K, iters=4, init=init)
        assert len(set(idx.tolist())) == K
        # more empty clusters than rows off their centroid, one of the rows not finite: nothing to seed with, every centroid stays finite
        few = torch.cat([small[:1].expand(4, -1), torch.full((1, 6), math.nan)]).contiguous()
        init = torch.cat([small[:1], small[:1] + 1e4, small[:1] + 2e4]).contiguous()
        cb, idx, inertia = GC.kmeans(few, 3, iters=3, init=init)
        assert idx.tolist() == [0, 0, 0, 0, -1] and bool(torch.isfinite(cb).all()) and torch.equal(cb[0], small[0]) and inertia.tolist() == [0.0] * 3
        with pytest.raises(ValueError, match="K = 98 centroids for P = 97 rows"):
            GC.kmeans(small, 98)
        with pytest.raises(ValueError, match="1 <= D <= 64"):
            GC.kmeans(torch.zeros(70, 65), 2)
        with pytest.raises(pkg.GsrError, match="rows must be a float32 tensor"):
            GC.kmeans(rows.double(), 2)
    with pytest.raises(Exception, match="must live on a HIP device"):      # no CPU path in the product
        GC.kmeans(rows, K)


def toy_model(P, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"xyz": r(P, 3), "features_dc": r(P, 1, 3), "features_rest": 0.1 * r(P, 15, 3), "opacity": r(P, 1), "scaling": r(P, 3) - 4.0,
            "rotation": r(P, 4)}


def test_compress_save_load_decompress_on_the_cpu_package(simt_lib, tmp_path):  # noqa: F811
    from gsr_scene import compress as GC
    P = 200
    model = toy_model(P)
    with package_on_the_cpu(simt_lib):
        c = GC.compress(model, {"features_rest": 16, "scaling": 8, "rotation": 8}, iters=3, generator=torch.Generator().manual_seed(1))
        with pytest.raises(ValueError, match="'opacity' holds non-finite values"):
            bad = dict(model, opacity=model["opacity"].clone())
            bad["opacity"][3] = math.nan
            GC.compress(bad, {"scaling": 8})
        with pytest.raises(KeyError):
            GC.compress(model, {"colour": 8})
        with pytest.raises(TypeError, match="'scaling' must be a float32 tensor"):
            GC.compress(dict(model, scaling=model["scaling"].double()), {"scaling": 8})
    assert set(c) == set(model)
    for key in ("xyz", "features_dc", "opacity"):
        assert c[key] is model[key]
    for key, K in (("features_rest", 16), ("scaling", 8), ("rotation", 8)):
        e = c[key]
        assert e["codebook"].shape == (K, model[key][0].numel()) and e["idx"].dtype == torch.uint16 and e["idx"].shape == (P,)
        assert e["shape"] == tuple(model[key].shape)
    path = str(tmp_path / "scene.npz")
    GC.save_compressed(path, c)
    assert os.path.getsize(path) < 0.6 * sum(t.numel() * 4 for t in model.values())
    back = GC.load_compressed(path)
    assert set(back) == set(c)
    out = GC.decompress(back)
    for key, t in model.items():
        if isinstance(c[key], dict):
            e = c[key]
            assert torch.equal(back[key]["codebook"].view(torch.int32), e["codebook"].view(torch.int32)) and back[key]["shape"] == e["shape"]
            index = torch.from_numpy(e["idx"].numpy().astype(np.int64))
            assert torch.equal(out[key].view(torch.int32), e["codebook"][index].reshape(t.shape).view(torch.int32)), key
        else:
            assert torch.equal(out[key].view(torch.int32), t.view(torch.int32)), key
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(GC.decompress(c).values(), (out[k] for k in c)))
    # rotations are clustered as unit quaternions with w >= 0
    q = out["rotation"]
    assert bool((q[:, 0] >= 0).all()) and float(q.norm(dim=1).max()) <= 1.0 + 1e-6
