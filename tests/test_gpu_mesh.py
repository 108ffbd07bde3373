"""TSDF fusion and marching tetrahedra on the MI355X: gsr_scene.mesh on the device against tests/mesh_reference.py (fp64 on the CPU) over the sweeps
and volumes of tests/test_mesh_cpu.py, which runs the same kernel source on the host -- weights EQUAL off the fragile set, tsdf / rgb within 4 x
the host build's largest error, meshes EQUAL to the reference extraction; run-to-run bits; a scratch full of garbage; and one end-to-end case:
Gaussians on a sphere -> probe median depth of six cameras -> integrate -> extract."""
import math

import numpy as np
import pytest
import torch

import mesh_reference as MR
from test_mesh_cpu import SWEEP_DIMS, SWEEP_IMAGES, SWEEP_V, extraction_volumes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def fused(dims, V, H, W, color):
    """The case of tests/mesh_reference.py through gsr_scene.mesh -> (origin, volume, reference)."""
    from gsr_scene import mesh
    origin, cams, depth, col, ref = MR.integrate_case(dims, V, H, W, color)
    vol = mesh.TSDFVolume(origin.tolist(), float(np.float32(MR.VOXEL)), dims, float(np.float32(MR.TRUNC)), DEV, color=color, near=float(np.float32(MR.NEAR)))
    vol.integrate(dev(depth), dev(cams), dev(col))
    return origin, vol, ref


def host(vol):
    return vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), (None if vol.rgb is None else vol.rgb.cpu().numpy())


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("V", SWEEP_V)
@pytest.mark.parametrize("dims", SWEEP_DIMS)
def test_integrate_on_the_device_is_the_rule(dims, V):
    for H, W in SWEEP_IMAGES:
        for color in (False, True):
            origin, vol, ref = fused(dims, V, H, W, color)
            got = host(vol)
            MR.check_integrate(f"gpu {dims} V {V} {W}x{H} colour {color}", *got, ref, V, bar=MR.bars(V))
            assert same_bits(got, host(fused(dims, V, H, W, color)[1])), "two runs differ"
            m = vol.extract()
            MR.check_mesh(f"gpu {dims} V {V}", m.vertices.cpu().numpy(), m.faces.cpu().numpy(), None if m.colors is None else m.colors.cpu().numpy(),
                          *got, dims, origin, np.float32(MR.VOXEL))


def test_two_calls_and_a_side_stream():
    from gsr_scene import mesh
    dims, V, (H, W) = (70, 5, 3), 17, (30, 40)
    origin, cams, depth, color, _ = MR.integrate_case(dims, V, H, W, True)
    args = (dims, origin, np.float32(MR.VOXEL), np.float32(MR.TRUNC), np.float32(MR.NEAR))
    first = MR.integrate(*args, cams[:5], depth[:5], color[:5])
    ref = MR.integrate(*args, cams[5:], depth[5:], color[5:], state=(first["tsdf"], first["weight"], first["rgb"]))
    ref["fragile"], ref["unit"] = ref["fragile"] | first["fragile"], np.maximum(ref["unit"], first["unit"])

    def run():
        vol = mesh.TSDFVolume(origin.tolist(), float(args[2]), dims, float(args[3]), DEV, color=True, near=float(args[4]))
        vol.integrate(dev(depth[:5]), dev(cams[:5]), dev(color[:5])).integrate(dev(depth[5:]), dev(cams[5:]), dev(color[5:]))
        return vol, vol.extract()

    vol, m = run()
    MR.check_integrate("gpu, two calls", *host(vol), ref, 12, calls=2, bar=MR.bars(12))
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        vol2, m2 = run()
    stream.synchronize()
    assert same_bits(host(vol), host(vol2)) and torch.equal(m.faces, m2.faces) and torch.equal(m.vertices.view(torch.int32), m2.vertices.view(torch.int32))


def test_the_recipe_with_device_cuda_and_camera_objects():
    """The documented call form: device="cuda" (no index) while every tensor says cuda:0; camera objects in batches, packed records the second time."""
    import types
    from gsr_scene import mesh
    dims, V, (H, W) = (9, 8, 7), 17, (30, 40)
    origin, cams, depth, _, ref = MR.integrate_case(dims, V, H, W, False)
    want = host(fused(dims, V, H, W, False)[1])
    objs = [types.SimpleNamespace(R=c[:9].reshape(3, 3), T=c[9:12], focal_x=float(c[12]), focal_y=float(c[13]), image_width=W, image_height=H) for c in cams.copy()]
    vol = mesh.TSDFVolume(origin.tolist(), float(np.float32(MR.VOXEL)), dims, float(np.float32(MR.TRUNC)), "cuda", near=float(np.float32(MR.NEAR)))
    assert vol.device == torch.device("cuda:0") == vol.tsdf.device
    vol.integrate(torch.from_numpy(depth.copy()).to("cuda"), objs)
    assert same_bits(host(vol), want)
    packed = torch.from_numpy(cams.copy()).to("cuda")
    again = mesh.TSDFVolume(origin.tolist(), float(np.float32(MR.VOXEL)), dims, float(np.float32(MR.TRUNC)), "cuda", near=float(np.float32(MR.NEAR)))
    for lo in (0, 5):      # two batches; the second call of a batch finds its records checked already
        hi = 5 if lo == 0 else V
        again.integrate(torch.from_numpy(depth[lo:hi].copy()).to("cuda"), packed[lo:hi])
    assert len(again._sizes_checked) == 2
    again.integrate(torch.zeros((5, H, W), device="cuda"), packed[0:5])      # (all pixels invalid: nothing changes)
    assert len(again._sizes_checked) == 2 and torch.equal(again.weight, vol.weight)      # (a weight is a count: two calls fold to the same)
    wrong = packed.clone()
    wrong[4, 14] = 41.0
    import diff_gaussian_rasterization as pkg
    with pytest.raises(pkg.GsrError, match=r"camera 4 is 41 x 30 \(W x H\), the depth maps are 40 x 30"):
        again.integrate(torch.from_numpy(depth.copy()).to("cuda"), wrong)


def test_non_finite_input_on_the_device():
    from gsr_scene import mesh
    dims, V, (H, W) = (33, 21, 18), 17, (30, 40)
    origin, cams, depth, _, _ = MR.integrate_case(dims, V, H, W, False)

    def run(c, d):
        vol = mesh.TSDFVolume(origin.tolist(), float(np.float32(MR.VOXEL)), dims, float(np.float32(MR.TRUNC)), DEV, near=float(np.float32(MR.NEAR)))
        return host(vol.integrate(dev(d), dev(c)))

    bad = cams.copy()
    bad[3, 4], bad[9, 13], bad[16, 10] = np.nan, np.inf, -np.inf
    keep = np.ones(V, dtype=bool)
    keep[[3, 9, 16]] = False
    assert same_bits(run(bad, depth), run(cams[keep], depth[keep])), "a record with a non-finite entry is a view that is not there"
    holes, zeros = depth.copy(), depth.copy()
    holes[:, ::3, ::2], zeros[:, ::3, ::2] = np.nan, 0.0
    a = run(cams, holes)
    assert same_bits(a, run(cams, zeros)) and np.isfinite(a[0]).all()


def extract_through_the_library(tsdf, weight, rgb, dims, origin, voxel, fill):
    """gsr_mesh_count / gsr_mesh_emit on device tensors with a scratch that starts as `fill`."""
    import diff_gaussian_rasterization as pkg
    lib = pkg._lib.load()
    nx, ny, nz = dims
    t, w, c = dev(tsdf), dev(weight), dev(rgb)
    scratch = torch.full((int(lib.gsr_mesh_scratch_bytes(nx, ny, nz)) + 128,), fill, dtype=torch.uint8, device=DEV)
    scratch = scratch[(-scratch.data_ptr()) % 128:]
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        stream = pkg._stream_ptr(torch.device(DEV))
        pkg._lib.check(lib.gsr_mesh_count(nx, ny, nz, pkg._ptr(t), pkg._ptr(w), 1.0, pkg._ptr(scratch), pkg._ptr(counts), stream), "gsr_mesh_count")
        nv, nf = counts.tolist()
        v = torch.full((nv, 3), 7.0, device=DEV)
        f = torch.full((nf, 3), -9, dtype=torch.int32, device=DEV)
        col = torch.full((nv, 3), 7.0, device=DEV) if rgb is not None else None
        pkg._lib.check(lib.gsr_mesh_emit(nx, ny, nz, *(float(o) for o in origin), float(voxel), pkg._ptr(t), pkg._ptr(c), pkg._ptr(scratch), nv, nf,
                                         pkg._ptr(v), pkg._ptr(col), pkg._ptr(f), stream), "gsr_mesh_emit")
    return v.cpu().numpy(), f.cpu().numpy(), (None if col is None else col.cpu().numpy())


@pytest.mark.parametrize("name", ["sphere", "torus", "noise", "noise with holes"])
def test_extraction_on_the_device(name):
    tsdf, weight, analytic, euler = extraction_volumes()[name]
    n = tsdf.shape[0]
    dims, origin, voxel = (n, n, n), (0.0, 0.0, 0.0), 1.0
    rgb = np.random.default_rng(3).random((3, n, n, n), dtype=np.float32)
    v, f, c = extract_through_the_library(tsdf, weight, rgb, dims, origin, voxel, 0x5A)
    MR.check_mesh(f"gpu {name}", v, f, c, tsdf, weight, rgb, dims, origin, voxel)
    inv = MR.mesh_invariants(v, f)
    assert inv["unused"] == 0 and inv["directed_max"] == 1
    if name != "noise with holes":
        assert inv["per_edge"] == [2] and inv["volume"] > 0
    if analytic is not None:
        assert inv["euler"] == euler and abs(inv["volume"] - analytic) <= 0.05 * analytic
    v2, f2, c2 = extract_through_the_library(tsdf, weight, rgb, dims, origin, voxel, 0xC3)      # other garbage in the scratch, a second run
    assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f) and np.array_equal(c2.view(np.int32), c.view(np.int32))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def settings_of(pkg, record, H, W):
    """GaussianRasterizationSettings of one camera record (cam = xyz R + T, principal point in the centre)."""
    import gsr_synth
    R, T, fx, fy = record[:9].reshape(3, 3).double(), record[9:12].double(), float(record[12]), float(record[13])
    wvt = torch.eye(4, dtype=torch.float64)
    wvt[:3, :3], wvt[3, :3] = R, T
    tanx, tany = W / (2.0 * fx), H / (2.0 * fy)
    proj = gsr_synth.projection_matrix(0.01, 100.0, 2.0 * math.atan(tanx), 2.0 * math.atan(tany)).double().transpose(0, 1)
    f32 = lambda t: t.float().contiguous().to(DEV)  # noqa: E731
    return pkg.GaussianRasterizationSettings(H, W, tanx, tany, torch.zeros(3, device=DEV), 1.0, f32(wvt), f32(wvt @ proj), 0, f32(wvt.inverse()[3, :3]),
                                             False, False, False)


def test_gaussians_on_a_sphere_to_a_mesh():
    import diff_gaussian_rasterization as pkg
    from gsr_scene import mesh
    P, V, H, W = 4000, 6, 48, 64
    g = torch.Generator().manual_seed(11)
    n = torch.randn(P, 3, generator=g)
    means = (MR.SPHERE_RADIUS * n / n.norm(dim=1, keepdim=True)).to(DEV)
    scales = torch.full((P, 3), 0.012, device=DEV)      # spacing ~ sqrt(4 pi r^2 / P) = 0.021: the shell is closed
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV).repeat(P, 1)
    opac = torch.full((P, 1), 0.99, device=DEV)
    cams = torch.from_numpy(MR.look_at_cameras(V, H, W))
    depth = torch.stack([mesh.depth_from_probe(pkg.GaussianRasterizer(settings_of(pkg, cams[v], H, W)).probe(means, opac, scales=scales, rotations=rot)[0])
                         for v in range(V)])
    assert depth.shape == (V, H, W) and float((depth > 0).float().mean()) > 0.05
    dims, voxel = (24, 23, 22), np.float32(0.04)
    origin = (np.array([0.011, -0.006, 0.017]) - 0.5 * voxel * (np.array(dims) - 1)).astype(np.float32)
    trunc, near = np.float32(4 * voxel), np.float32(0.05)
    vol = mesh.TSDFVolume(origin.tolist(), float(voxel), dims, float(trunc), DEV, near=float(near)).integrate(depth, cams.to(DEV))
    got = host(vol)
    ref = MR.integrate(dims, origin, voxel, trunc, near, cams.numpy(), depth.cpu().numpy())
    MR.check_integrate("gpu end to end", *got, ref, V, bar=MR.bars(V))
    m = vol.extract()
    v, f = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    MR.check_mesh("gpu end to end", v, f, None, got[0], got[1], None, dims, origin, voxel)      # the reference extraction of the KERNEL's volume
    assert len(f) >= 1
    inv = MR.mesh_invariants(v, f)
    radius = np.linalg.norm(v, axis=1)
    print(f"[mesh] gpu end to end: {len(v)} vertices, {len(f)} faces, radius {radius.min():.3f} .. {radius.max():.3f} (Gaussians at {MR.SPHERE_RADIUS}), "
          f"{inv}", flush=True)
    assert inv["unused"] == 0 and inv["directed_max"] == 1
