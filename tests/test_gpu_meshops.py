"""Mesh clean-up on the MI355X: gsr_scene.mesh's components / compact / filter_components / vertex_normals / smooth on the device against
tests/meshops_reference.py (numpy, fp64) over the cases of tests/test_meshops_cpu.py, which runs the same kernel source on the host, plus one 64^3
sphere-and-blobs volume through TSDFVolume.extract.  Integer outputs and the compaction EQUAL; normals and smoothed positions within
MO.DEVICE_MAX_ULP (the host build's figure + 1 fp32 ulp for the device's fp64 divide and square root: derived in the reference's docstring) at every
vertex; run-to-run bits; a side stream; the error messages; and the recipe of INTEGRATION.md 3o end to end on Gaussians on a sphere."""
import numpy as np
import pytest
import torch

import meshops_reference as MO
import mesh_reference as MR
from test_meshops_cpu import FILTERS, SMOOTH_CASES, keep_masks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def device_mesh(v, c, f):
    from gsr_scene import mesh
    return mesh.Mesh(dev(np.asarray(v, np.float32).reshape(-1, 3)), dev(np.asarray(f, np.int32).reshape(-1, 3)), dev(c))


def all_outputs(m, masks):
    """Every operation once -> a list of numpy arrays."""
    from gsr_scene import mesh
    comp = mesh.components(m)
    out = [host(comp.vertex_label), host(comp.face_count)]
    for keep in masks:
        got = mesh.compact(m, dev(keep))
        out += [host(got.vertices), host(got.faces)] + ([host(got.colors)] if got.colors is not None else [])
    out.append(host(mesh.vertex_normals(m)))
    out += [host(mesh.smooth(m, it, lam, mu).vertices) for it, lam, mu in SMOOTH_CASES]
    return out


def check_case(name, v, c, f):
    from gsr_scene import mesh
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
    nv, m, masks = len(v), device_mesh(v, c, f), keep_masks(len(v), f)
    first = all_outputs(m, masks)
    want_label, want_count = MO.components(nv, f)
    assert np.array_equal(first[0], want_label), f"{name}: labels"
    assert np.array_equal(first[1], want_count), f"{name}: face counts"
    at = 2
    for keep in masks:
        wv, wc, wf = MO.compact(v, c, f, keep)
        assert MO.same_bits(first[at], wv) and MO.same_bits(first[at + 1], wf), f"{name}: compaction"
        at += 2
        if c is not None:
            assert MO.same_bits(first[at], wc), f"{name}: compacted colours"
            at += 1
    worst = 0
    if nv:
        worst = int(MO.ulp_distance(first[at], MO.vertex_normals(v, f)).max())
        for k, (it, lam, mu) in enumerate(SMOOTH_CASES):
            worst = max(worst, int(MO.ulp_distance(first[at + 1 + k], MO.smooth(v, f, it, lam, mu)).max()))
        assert MO.same_bits(host(mesh.smooth(m, 3, 0.0, 0.0).vertices), v) and MO.same_bits(host(mesh.smooth(m, 0).vertices), v)
        assert MO.same_bits(host(m.vertices), v), "the input was written"
    print(f"[meshops] gpu {name}: {nv} vertices, {len(f)} rows, largest distance {worst} ulp", flush=True)
    assert worst <= MO.DEVICE_MAX_ULP, f"{name}: {worst} ulp"
    second = all_outputs(m, masks)
    assert len(first) == len(second) and all(MO.same_bits(a, b) for a, b in zip(first, second)), f"{name}: two runs differ"
    return m, first, masks


def test_hand_cases_and_empty_inputs():
    v, f = MO.tetrahedron()
    check_case("tetrahedron", v, None, f)
    v7, f8 = MO.two_tetrahedra_sharing_a_vertex()
    check_case("two tetrahedra", v7, None, f8)
    v6 = np.concatenate([v, [[5, 5, 5], [6, 6, 6]]]).astype(np.float32)
    rows = np.concatenate([[[-1, 0, 1]], f[:2], [[0, 1, 6]], f[2:], [[2, 2, 3]], [[4, 5, 5]]]).astype(np.int32)
    check_case("rows that are no faces", v6, v6, rows)
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    check_case("nothing", none_v, None, none_f)
    check_case("five vertices, no face", v6[:5], v6[:5], none_f)
    check_case("one face", v6[:5], v6[:5], np.array([[3, 1, 4]], np.int32))
    check_case("faces, no vertex", none_v, None, np.array([[0, 1, 2]], np.int32))


@pytest.mark.parametrize("order", ["random", "reverse"])
def test_triangle_strip(order):
    v, f = MO.strip(700, order)
    check_case(f"strip, {order} ids", v, None, f)


def test_composed_mesh_a_side_stream_and_non_finite_positions():
    from gsr_scene import mesh
    v, c, f = MO.composed()
    nv = len(v)
    m, first, masks = check_case("composed", v, c, f)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        side = all_outputs(m, masks)
    stream.synchronize()
    assert all(MO.same_bits(a, b) for a, b in zip(first, side)), "a side stream gives other bits"
    # a NaN and an inf stay within 1 edge (normals) and 2 * iterations edges (smoothing); labels, counts and compaction do not read positions
    label = MO.components(nv, f)[0]
    on_sphere = np.flatnonzero(label == np.bincount(label).argmax())
    sources = [int(on_sphere[10]), int(on_sphere[200])]
    bad = v.copy()
    bad[sources[0], 1], bad[sources[1], 2] = np.nan, np.inf
    b = device_mesh(bad, c, f)
    comp = mesh.components(b)
    assert np.array_equal(host(comp.vertex_label), first[0]) and np.array_equal(host(comp.face_count), first[1])
    assert MO.same_bits(host(mesh.compact(b, None).faces), MO.compact(bad, c, f, None)[2])
    far = MO.edge_distance(nv, f, sources, 1) > 1
    clean, poisoned = host(mesh.vertex_normals(m)), host(mesh.vertex_normals(b))
    assert far.sum() > 50 and MO.same_bits(poisoned[far], clean[far]) and not np.isfinite(poisoned[~far]).all()
    for it in (1, 2):
        far = MO.edge_distance(nv, f, sources, 2 * it) > 2 * it
        clean, poisoned = host(mesh.smooth(m, it).vertices), host(mesh.smooth(b, it).vertices)
        assert far.sum() > 50 and MO.same_bits(poisoned[far], clean[far]) and not np.isfinite(poisoned[~far]).all()


def test_filter_components_on_the_device():
    from gsr_scene import mesh
    v, c, f = MO.composed(second_60=True)
    m = device_mesh(v, c, f)
    for kw in FILTERS:
        got = mesh.filter_components(m, **kw)
        wv, wc, wf = MO.compact(v, c, f, MO.filter_keep(len(v), f, **kw))
        assert MO.same_bits(host(got.vertices), wv) and MO.same_bits(host(got.colors), wc) and MO.same_bits(host(got.faces), wf), kw
    one = mesh.filter_components(m, keep_largest=1)
    assert len(one.faces) == 512 and not host(mesh.components(one).vertex_label).any()


def volume_mesh(tsdf, weight=None, voxel=1.0):
    from gsr_scene import mesh
    n = tsdf.shape[0]
    vol = mesh.TSDFVolume((0.0, 0.0, 0.0), voxel, (n, n, n), 3.0 * voxel, DEV, color=True)
    vol.tsdf.copy_(dev(tsdf))
    vol.weight.copy_(dev(np.ones_like(tsdf) if weight is None else weight))
    vol.rgb.copy_(dev(np.random.default_rng(3).random((3, n, n, n), dtype=np.float32)))
    return vol.extract()


@pytest.mark.parametrize("name", ["sphere", "torus", "noise", "noise with holes"])
def test_extracted_meshes(name):
    from test_mesh_cpu import extraction_volumes
    tsdf, weight, _, _ = extraction_volumes()[name]
    m = volume_mesh(tsdf, weight)
    assert len(m.faces) > 100
    check_case(name, host(m.vertices), host(m.colors), host(m.faces))


def test_a_sphere_and_blobs_volume_of_64_cubed():
    from gsr_scene import mesh
    n = 64
    m = volume_mesh(MO.blob_field(n), voxel=1.0 / n)
    v, c, f = host(m.vertices), host(m.colors), host(m.faces)
    assert 15000 < len(f) < 40000, len(f)
    check_case("64^3 sphere and blobs", v, c, f)
    count = host(mesh.components(m).face_count)
    # (24 blobs of 1.2 .. 2.2 voxels in radius, some of which may merge, beside a sphere of 12.8: by area the sphere holds about 70 % of the faces)
    assert (count > 0).sum() >= 20 and count.max() > 0.5 * len(f)
    kept = mesh.filter_components(m, keep_largest=1)
    assert len(kept.faces) == count.max() and not host(mesh.components(kept).vertex_label).any()
    inv = MR.mesh_invariants(host(kept.vertices), host(kept.faces))
    assert inv["unused"] == 0 and inv["directed_max"] == 1 and inv["per_edge"] == [2] and inv["euler"] == 2
    n_out = host(mesh.vertex_normals(kept)).astype(np.float64)
    assert (np.einsum("ij,ij->i", n_out, host(kept.vertices) - 0.5) > 0).all(), "normals point to positive tsdf"


def test_error_messages():
    import diff_gaussian_rasterization as pkg
    from gsr_scene import mesh
    v, f = MO.tetrahedron()
    m = device_mesh(v, None, f)
    with pytest.raises(pkg.GsrError, match=r"faces must be an int32 tensor of shape \[Nf,3\], got \(4, 3\) torch.int64"):
        mesh.components(mesh.Mesh(m.vertices, m.faces.long(), None))
    with pytest.raises(pkg.GsrError, match=r"faces must be an int32 tensor of shape \[Nf,3\], got \(12,\) torch.int32"):
        mesh.vertex_normals(mesh.Mesh(m.vertices, m.faces.reshape(-1), None))
    with pytest.raises(pkg.GsrError, match=r"vertices must be a float32 tensor of shape \[Nv,3\], got \(4, 3\) torch.float16"):
        mesh.smooth(mesh.Mesh(m.vertices.half(), m.faces, None))
    with pytest.raises(pkg.GsrError, match=r"faces on cpu, vertices on cuda:0"):
        mesh.filter_components(mesh.Mesh(m.vertices, m.faces.cpu(), None), keep_largest=1)
    with pytest.raises(pkg.GsrError, match=r"keep_face on cpu, vertices on cuda:0"):
        mesh.compact(m, torch.ones(4, dtype=torch.bool))
    with pytest.raises(pkg.GsrError, match=r"keep_face must be a bool or uint8 tensor of shape \(4,\), got \(3,\) torch.bool"):
        mesh.compact(m, torch.ones(3, dtype=torch.bool, device=DEV))
    with pytest.raises(pkg.GsrError, match="must live on a HIP device"):
        mesh.components(mesh.Mesh(m.vertices.cpu(), m.faces.cpu(), None))


def test_the_recipe_on_gaussians_on_a_sphere(tmp_path):
    """extract -> filter_components -> smooth -> vertex_normals -> save."""
    import diff_gaussian_rasterization as pkg
    from gsr_scene import mesh
    from test_gpu_mesh import settings_of
    P, V, H, W = 4000, 6, 48, 64
    g = torch.Generator().manual_seed(11)
    n = torch.randn(P, 3, generator=g)
    means = (MR.SPHERE_RADIUS * n / n.norm(dim=1, keepdim=True)).to(DEV)
    scales = torch.full((P, 3), 0.012, device=DEV)
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV).repeat(P, 1)
    opac = torch.full((P, 1), 0.99, device=DEV)
    cams = torch.from_numpy(MR.look_at_cameras(V, H, W))
    depth = torch.stack([mesh.depth_from_probe(pkg.GaussianRasterizer(settings_of(pkg, cams[v], H, W)).probe(means, opac, scales=scales, rotations=rot)[0])
                         for v in range(V)])
    dims, voxel = (24, 23, 22), np.float32(0.04)
    origin = (np.array([0.011, -0.006, 0.017]) - 0.5 * voxel * (np.array(dims) - 1)).astype(np.float32)
    vol = mesh.TSDFVolume(origin.tolist(), float(voxel), dims, float(4 * voxel), DEV, near=0.05).integrate(depth, cams.to(DEV))
    raw = vol.extract()
    kept = mesh.filter_components(raw, keep_largest=1)
    assert 0 < len(kept.faces) <= len(raw.faces)
    comp = mesh.components(kept)
    assert not host(comp.vertex_label).any() and int(comp.face_count[0]) == len(kept.faces), "one component"
    smoothed = mesh.smooth(kept, iterations=5)
    normals = mesh.vertex_normals(smoothed)
    v, f = host(smoothed.vertices), host(smoothed.faces)
    inv = MR.mesh_invariants(v, f)
    assert inv["unused"] == 0 and inv["directed_max"] == 1, "every directed edge is used at most once"
    assert MO.same_bits(f, host(kept.faces)) and np.isfinite(v).all()
    assert MO.ulp_distance(v, MO.smooth(host(kept.vertices), f, 5, 0.5, -0.53)).max() <= MO.DEVICE_MAX_ULP
    assert MO.ulp_distance(host(normals), MO.vertex_normals(v, f)).max() <= MO.DEVICE_MAX_ULP
    path = str(tmp_path / "clean.ply")
    mesh.save_mesh_ply(path, smoothed)
    back = mesh.load_mesh_ply(path)
    assert MO.same_bits(back.vertices.numpy(), v) and MO.same_bits(back.faces.numpy(), f)
    print(f"[meshops] gpu recipe: {len(raw.faces)} -> {len(kept.faces)} faces, {inv}", flush=True)
