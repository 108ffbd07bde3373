"""A triangle mesh out of a trained scene: render a depth map per camera with the per-pixel probe, fuse them into a TSDF volume, extract the
surface by marching tetrahedra and write mesh.ply (gsr_scene.mesh).

    python tools/extract_mesh.py [--ply point_cloud.ply] [--cameras cameras.npy] [--views 48] [--image 540x960] [--resolution 256]
                                 [--trunc-voxels 4] [--depth median|expected] [--min-weight 2] [--save-cameras used.npy] [--out mesh.ply]
                                 [--keep-largest N] [--min-faces N] [--smooth K]

Without --ply the scene is synthetic: Gaussians on a sphere.  Cameras: --cameras takes the training views as packed records, a [V,16] float
array in a .npy file or a tensor in a .pt file -- what gsr_scene.mip.pack_cameras(scene.getTrainCameras(), "cpu") returns: R[9] row-major and
T[3] with cam = xyz R + T, focal_x, focal_y, width, height; all of one size, the principal point in the centre.  Without it the views are a
synthetic orbit (gsr_synth.look_at_camera) around the centre of the point cloud at --orbit times its extent, of --views views of --image.
--save-cameras writes the records that were used.  The volume is the cloud's central bounding box (the 1 % .. 99 % quantiles, enlarged by 10 %),
--resolution voxels along its longest side.
Clean-up (all off by default, the mesh is then the raw extraction): --keep-largest N and --min-faces N keep the faces of the
components with at least max(min-faces, the N-th largest component's face count) faces (2DGS's post_process_mesh; floaters go), --smooth K applies K
Taubin iterations (the voxel staircase goes).  With any of them the vertices and faces before and after are printed."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402
import gsr_scene  # noqa: E402
import gsr_synth  # noqa: E402
from gsr_scene import mesh  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ply", default=None, help="a trained point_cloud.ply; default: a synthetic sphere of Gaussians")
ap.add_argument("--cameras", default=None, help="packed [V,16] camera records (.npy or .pt); default: a synthetic orbit")
ap.add_argument("--save-cameras", default=None, help="write the records that were used to this .npy file")
ap.add_argument("--sh-degree", type=int, default=3)
ap.add_argument("--views", type=int, default=48)
ap.add_argument("--image", default="540x960", help="H x W of the rendered depth maps")
ap.add_argument("--orbit", type=float, default=2.5, help="radius of the camera orbit in units of the cloud's extent")
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--trunc-voxels", type=float, default=4.0)
ap.add_argument("--depth", default="median", choices=["median", "expected"])
ap.add_argument("--min-weight", type=float, default=2.0)
ap.add_argument("--batch", type=int, default=16, help="views per integrate call")
ap.add_argument("--out", default="mesh.ply")
ap.add_argument("--keep-largest", type=int, default=None, help="keep the N largest connected components (ties at the threshold stay)")
ap.add_argument("--min-faces", type=int, default=0, help="drop connected components with fewer faces")
ap.add_argument("--smooth", type=int, default=0, help="Taubin smoothing iterations (lambda 0.5, mu -0.53)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("extract_mesh.py: no HIP device")
dev = torch.device("cuda:0")
H, W = (int(v) for v in args.image.split("x"))

if args.ply:
    g = gsr_scene.load_gaussians_ply(args.ply, args.sh_degree, dev)
    means, scales, opacity = g["xyz"].contiguous(), torch.exp(g["scaling"]).contiguous(), torch.sigmoid(g["opacity"]).contiguous()
    rotations = torch.nn.functional.normalize(g["rotation"]).contiguous()
else:
    P = 200_000
    n = torch.randn(P, 3, generator=torch.Generator().manual_seed(0))
    means = (n / n.norm(dim=1, keepdim=True)).to(dev)
    scales = torch.full((P, 3), 1.5 * math.sqrt(4 * math.pi / P), device=dev)
    rotations = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(P, 1)
    opacity = torch.full((P, 1), 0.95, device=dev)
print(f"{means.shape[0]} Gaussians", flush=True)

lo, hi = torch.quantile(means[:: max(1, means.shape[0] // 1_000_000)], torch.tensor([0.01, 0.99], device=dev), dim=0)
centre, half = 0.5 * (lo + hi), 0.55 * (hi - lo)
extent = float(half.max())
voxel = 2.0 * extent / (args.resolution - 1)
dims = tuple(int(math.ceil(2.0 * float(h) / voxel)) + 1 for h in half)
origin = tuple(float(c - h) for c, h in zip(centre, half))
volume = mesh.TSDFVolume(origin, voxel, dims, args.trunc_voxels * voxel, dev, near=0.05 * extent)
print(f"volume {dims[0]} x {dims[1]} x {dims[2]} voxels of {voxel:.5g}, truncation {args.trunc_voxels * voxel:.5g}", flush=True)


def orbit_records():
    """[V,16] fp32: a spiral of look-at cameras around the cloud, every side of the scene seen; the records of gsr_scene.mip.pack_cameras
    (cam = xyz R + T is the upper part of a gsr_synth camera's world_view_transform)."""
    rows = []
    for v in range(args.views):
        phi, ct = 2.399963 * v, 0.7 - 1.4 * (v + 0.5) / args.views
        st = math.sqrt(1.0 - ct * ct)
        eye = [float(centre[0]) + args.orbit * extent * st * math.cos(phi), float(centre[1]) + args.orbit * extent * ct,
               float(centre[2]) + args.orbit * extent * st * math.sin(phi)]
        up = (0.0, -1.0, 0.0) if abs(ct) < 0.95 else (1.0, 0.0, 0.0)
        cam = gsr_synth.look_at_camera(W, H, eye, [float(c) for c in centre], up=up)
        wvt = cam.world_view_transform
        rows.append(torch.cat([wvt[:3, :3].reshape(-1), wvt[3, :3], torch.tensor([W / (2 * cam.tanfovx), H / (2 * cam.tanfovy), float(W), float(H)])]))
    return torch.stack(rows).float()


def settings_of(rec):
    """The rasterizer's settings of one record: viewmatrix = [[R, 0], [T, 1]], the reference's projection for the record's field of view."""
    R, T, fx, fy = rec[:9].reshape(3, 3).double(), rec[9:12].double(), float(rec[12]), float(rec[13])
    wvt = torch.eye(4, dtype=torch.float64)
    wvt[:3, :3], wvt[3, :3] = R, T
    tanx, tany = W / (2.0 * fx), H / (2.0 * fy)
    proj = gsr_synth.projection_matrix(0.01, 100.0, 2.0 * math.atan(tanx), 2.0 * math.atan(tany)).double().transpose(0, 1)
    f32 = lambda t: t.float().contiguous().to(dev)  # noqa: E731
    return pkg.GaussianRasterizationSettings(H, W, tanx, tany, bg, 1.0, f32(wvt), f32(wvt @ proj), 0, f32(wvt.inverse()[3, :3]), False, False, False)


if args.cameras:
    loaded = torch.load(args.cameras, map_location="cpu") if args.cameras.endswith(".pt") else torch.from_numpy(np.load(args.cameras))
    records = gsr_scene.mip.pack_cameras(loaded, "cpu")
    W, H = int(records[0, 14]), int(records[0, 15])
    if not bool(((records[:, 14] == W) & (records[:, 15] == H)).all()):
        sys.exit(f"extract_mesh.py: {args.cameras} holds cameras of more than one size; fuse them size by size")
    print(f"{records.shape[0]} cameras of {W} x {H} from {args.cameras}", flush=True)
else:
    records = orbit_records()
if args.save_cameras:
    np.save(args.save_cameras, records.numpy())
bg = torch.zeros(3, device=dev)
depths = []
for v in range(records.shape[0]):
    rast = pkg.GaussianRasterizer(settings_of(records[v]))
    probe, _ = rast.probe(means, opacity, scales=scales, rotations=rotations)
    alpha = None
    if args.depth == "expected":      # the alpha image: one more render, of constant colour one
        alpha = rast(means3D=means, means2D=None, opacities=opacity, colors_precomp=torch.ones_like(means), scales=scales, rotations=rotations)[0][0].detach()
    depths.append(mesh.depth_from_probe(probe, alpha, args.depth))
    if len(depths) == args.batch or v == records.shape[0] - 1:
        volume.integrate(torch.stack(depths), records[v + 1 - len(depths):v + 1])
        depths = []
observed = float((volume.weight >= args.min_weight).float().mean())
m = volume.extract(args.min_weight)
if args.keep_largest is not None or args.min_faces > 0 or args.smooth > 0:
    before = (m.vertices.shape[0], m.faces.shape[0])
    if args.keep_largest is not None or args.min_faces > 0:
        m = mesh.filter_components(m, min_faces=args.min_faces, keep_largest=args.keep_largest)
    if args.smooth > 0:
        m = mesh.smooth(m, iterations=args.smooth)
    parts = int((mesh.components(m).face_count > 0).sum())
    print(f"clean-up: {before[0]} vertices, {before[1]} faces -> {m.vertices.shape[0]} vertices, {m.faces.shape[0]} faces in {parts} component(s)", flush=True)
mesh.save_mesh_ply(args.out, m)
print(f"{observed * 100:.1f} % of the voxels observed by >= {args.min_weight:g} views; wrote {args.out}: {m.vertices.shape[0]} vertices, {m.faces.shape[0]} faces",
      flush=True)
