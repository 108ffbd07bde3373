"""What do TSDF fusion and mesh extraction (gsr_tsdf_integrate, gsr_mesh_count + gsr_mesh_emit, csrc/tsdf.hip) cost beside the same update written
as per-view torch operations on the same device, in the same process?

    python tools/gpu_mesh_time.py [--dims 256,512] [--views 64,256] [--reps 3] [--rounds 3] [--torch-views 8] [--out profiles/mesh_time.json]

Scene: a sphere of radius 0.6 in the volume [-1,1]^3, seen by V cameras on an orbit of radius 2.5 through 1920 x 1080 analytic depth maps (the
background is invalid).  Integrate: the kernel through the C ABI on a fresh volume (no allocation in the timed call) and the package call, beside
the per-view torch formulation -- a dozen passes over the whole volume per camera -- timed on the first --torch-views views and reported per view
(a full 256-view torch call at 512^3 would take most of a minute).  Reported: time, (voxel, view) pairs per second, the share of the fp32 vector
peak (157.3 TFLOP/s) the pairs stand for at PAIR_OPS operations each, counted from the source -- nine fused multiply-adds (18), two products,
three divisions, three sums, a minimum, eight comparisons -- and the bytes the call must move (16 per voxel: tsdf and weight read and written once,
plus every depth map once) over the time, against the measured HBM peak (6.29 TB/s).  Extraction: count + the host read of the two counts + emit
on the fused volume; bytes: 8 per voxel read by the classification plus the mesh written.  Device-event time of `reps` calls (the extraction: as many calls as fill 50 ms), the variants
alternating round by round; the median round is reported with its spread.  Before timing, kernel and torch are compared at the timed size."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402
import mesh_reference as MR  # noqa: E402
from gsr_scene import mesh  # noqa: E402

HBM_PEAK = 6.29e12
FP32_VECTOR_PEAK = 157.3e12
PAIR_OPS = 35
MIN_WINDOW = 0.05      # seconds of work per timed window, at least

ap = argparse.ArgumentParser()
ap.add_argument("--dims", default="256,512")
ap.add_argument("--views", default="64,256")
ap.add_argument("--image", default="1080x1920", help="H x W of the depth maps")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--torch-views", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_mesh_time.py: no HIP device")
dev = torch.device("cuda:0")
lib = pkg._lib.load()
stream = pkg._stream_ptr(dev)
Pt = pkg._ptr
H, W = (int(v) for v in args.image.split("x"))
RADIUS, ORBIT, NEAR = 0.6, 2.5, 0.05


def ok(rc, what):
    pkg._lib.check(rc, what)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def measure(variants):
    """variants: [(name, fn, reps)] -> {name: [seconds per call, one per round]}; warm-up, then the variants alternating round by round."""
    for _, fn, _ in variants:
        fn()
    torch.cuda.synchronize()
    # reps None: as many calls as fill MIN_WINDOW seconds (a window of three sub-millisecond calls would time the clock and the scheduler)
    variants = [(name, fn, reps if reps is not None else max(args.reps, min(5000, int(math.ceil(MIN_WINDOW / max(timed(fn, 3), 1e-7))))))
                for name, fn, reps in variants]
    times = {v[0]: [] for v in variants}
    for _ in range(args.rounds):
        for name, fn, reps in variants:
            times[name].append(timed(fn, reps))
    return times


def row(name, ts, extra):
    t = statistics.median(ts)
    out = {"ms": t * 1e3, "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3}
    out.update({k: f(t) for k, f in extra.items()})
    print(f"  {name:58s} {t * 1e3:10.3f} ms ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})   " + "   ".join(f"{k} {v:.4g}" for k, v in out.items() if not k.startswith("ms")),
          flush=True)
    return out


def orbit(V):
    rows = []
    for v in range(V):
        phi, ct = 2.399963 * v + 0.3, 0.8 - 1.6 * (v + 0.5) / V
        st = math.sqrt(1.0 - ct * ct)
        rows.append(MR.camera_record((ORBIT * st * math.cos(phi), ORBIT * st * math.sin(phi), ORBIT * ct), 0.1 * v, 1.2 * W, float(W), float(H)))
    return torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev)


def sphere_depth(cams):
    """[V,H,W] view-space z of the sphere through the pixel centres, 0 on the background; on the device, view by view."""
    ys, xs = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5, indexing="ij")
    out = torch.empty((cams.shape[0], H, W), device=dev)
    for v, rec in enumerate(cams):
        R, T, fx, fy = rec[:9].reshape(3, 3), rec[9:12], rec[12], rec[13]
        dirs = torch.stack([(xs - W / 2.0) / fx, (ys - H / 2.0) / fy, torch.ones_like(xs)], dim=-1) @ R.T
        o = -T @ R.T
        a, b, c = (dirs * dirs).sum(-1), 2.0 * (dirs @ o), (o @ o) - RADIUS * RADIUS
        disc = b * b - 4 * a * c
        t = (-b - torch.sqrt(disc.clamp_min(0.0))) / (2 * a)
        out[v] = torch.where((disc > 0) & (t > 0), t, torch.zeros_like(t))
    return out


def torch_integrate(points, tsdf, weight, cams, depth, trunc):
    """The update of include/gsr.h as per-view torch operations; points [N,3], tsdf / weight [N] (updated in place)."""
    s, n = torch.zeros_like(tsdf), torch.zeros_like(tsdf)
    for v in range(cams.shape[0]):
        rec = cams[v]
        cam = points @ rec[:9].reshape(3, 3) + rec[9:12][None, :]
        z = cam[:, 2]
        u, w = torch.floor(rec[12] * cam[:, 0] / z + W / 2.0), torch.floor(rec[13] * cam[:, 1] / z + H / 2.0)
        on = (z > NEAR) & (u >= 0) & (u < W) & (w >= 0) & (w < H)
        at = torch.where(on, w * W + u, torch.zeros_like(u)).long()
        d = depth[v].reshape(-1)[at]
        sdf = d - z
        take = on & torch.isfinite(d) & (d > 0) & (sdf >= -trunc)
        s += torch.where(take, (sdf / trunc).clamp(max=1.0), torch.zeros_like(sdf))
        n += take
    hit = n > 0
    tsdf.copy_(torch.where(hit, (tsdf * weight + s) / (weight + n).clamp_min(1.0), tsdf))
    weight += n


result = {"reps": args.reps, "extract_window_s_at_least": MIN_WINDOW, "rounds": args.rounds, "image": [H, W], "pair_ops": PAIR_OPS, "fp32_vector_peak_tflops": FP32_VECTOR_PEAK / 1e12,
          "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "torch_views": args.torch_views, "integrate": {}, "extract": {}}
for n in (int(v) for v in args.dims.split(",")):
    voxel = 2.0 / (n - 1)
    trunc = 4 * voxel
    origin = (-1.0, -1.0, -1.0)
    N = n ** 3
    grid = torch.arange(n, device=dev, dtype=torch.float32) * voxel - 1.0
    points = torch.stack(torch.meshgrid(grid, grid, grid, indexing="ij"), dim=-1).flip(-1).reshape(N, 3).contiguous()      # [nz,ny,nx] order, (x, y, z) columns
    tsdf, weight = torch.empty(N, device=dev), torch.empty(N, device=dev)
    for V in (int(v) for v in args.views.split(",")):
        cams = orbit(V)
        depth = sphere_depth(cams)

        def fresh():
            tsdf.fill_(1.0)
            weight.zero_()

        def k_integrate():
            ok(lib.gsr_tsdf_integrate(n, n, n, *origin, voxel, trunc, NEAR, V, Pt(cams), H, W, Pt(depth), None, Pt(tsdf), Pt(weight), None, stream),
               "gsr_tsdf_integrate")
        vol = mesh.TSDFVolume(origin, voxel, (n, n, n), trunc, dev, near=NEAR)
        Vt = min(V, args.torch_views)
        # kernel and torch on the first Vt views of a fresh volume
        fresh()
        ok(lib.gsr_tsdf_integrate(n, n, n, *origin, voxel, trunc, NEAR, Vt, Pt(cams), H, W, Pt(depth), None, Pt(tsdf), Pt(weight), None, stream), "integrate")
        kt, kw = tsdf.clone(), weight.clone()
        fresh()
        torch_integrate(points, tsdf, weight, cams[:Vt], depth[:Vt], trunc)
        differ = int((kw != weight).sum())
        gap = (kt - tsdf)[kw == weight].abs()
        worst, moved = float(gap.max()), int((gap > 1e-4).sum())
        del kt, kw, gap
        # (a floor that falls the other way reads the neighbouring depth pixel: across a silhouette that is another surface, and on a voxel that one
        # view observed the whole difference lands in tsdf while the count stays what it was)
        print(f"integrate, {n}^3 voxels, V {V}, {W} x {H}: {args.rounds} rounds, median round (min .. max); over the first {Vt} views {differ} of {N} weights "
              f"differ from the torch formulation (decisions within rounding of a threshold); where the weights agree tsdf differs by more than 1e-4 on "
              f"{moved} voxels (another pixel read), by {worst:.2e} at most", flush=True)
        fresh()
        pairs = N * V
        nbytes = 16 * N + 4 * V * H * W
        times = measure([("kernel: gsr_tsdf_integrate", k_integrate, args.reps),
                         ("package: TSDFVolume.integrate", lambda: vol.integrate(depth, cams), args.reps),
                         (f"torch: per-view update, {Vt} views", lambda: torch_integrate(points, tsdf, weight, cams[:Vt], depth[:Vt], trunc), 1)])
        entry = {"weights_that_differ": differ, "tsdf_differs_by_more_than_1e-4": moved, "tsdf_difference_max": worst}
        for name, ts in times.items():
            if name.startswith("torch"):
                entry[name] = row(name, ts, {"ms_per_view": lambda t: t * 1e3 / Vt, "pairs_per_s": lambda t: N * Vt / t,
                                             "ms_scaled_to_all_views": lambda t: t * 1e3 * V / Vt})
            else:
                entry[name] = row(name, ts, {"ms_per_view": lambda t: t * 1e3 / V, "pairs_per_s": lambda t: pairs / t,
                                             "fraction_of_fp32_vector_peak": lambda t: pairs * PAIR_OPS / t / FP32_VECTOR_PEAK, "bytes": lambda t: nbytes,
                                             "tb_per_s": lambda t: nbytes / t / 1e12, "fraction_of_hbm_peak": lambda t: nbytes / t / HBM_PEAK})
        result["integrate"][f"{n}^3 x {V}"] = entry
        if V == max(int(v) for v in args.views.split(",")):      # the extraction, on the volume fused from all views
            fresh()
            k_integrate()
            scratch = torch.empty(int(lib.gsr_mesh_scratch_bytes(n, n, n)) + 128, dtype=torch.uint8, device=dev)
            scratch = scratch[(-scratch.data_ptr()) % 128:]
            counts = torch.empty(2, dtype=torch.int32, device=dev)

            def k_count():
                ok(lib.gsr_mesh_count(n, n, n, Pt(tsdf), Pt(weight), 1.0, Pt(scratch), Pt(counts), stream), "gsr_mesh_count")
            k_count()
            nv, nf = counts.tolist()
            vertices, faces = torch.empty((nv, 3), device=dev), torch.empty((nf, 3), dtype=torch.int32, device=dev)

            def k_emit():
                ok(lib.gsr_mesh_emit(n, n, n, *origin, voxel, Pt(tsdf), None, Pt(scratch), nv, nf, Pt(vertices), None, Pt(faces), stream), "gsr_mesh_emit")

            def k_both():
                k_count()
                counts.tolist()
                k_emit()
            vol.tsdf.copy_(tsdf.reshape(n, n, n))
            vol.weight.copy_(weight.reshape(n, n, n))
            print(f"extract, {n}^3 voxels: {nv} vertices, {nf} faces", flush=True)
            mbytes = 8 * N + 12 * nv + 12 * nf
            extra = {"bytes": lambda t: mbytes, "tb_per_s": lambda t: mbytes / t / 1e12, "fraction_of_hbm_peak": lambda t: mbytes / t / HBM_PEAK,
                     "voxels_per_s": lambda t: N / t}
            times = measure([("kernel: gsr_mesh_count", k_count, None), ("kernel: gsr_mesh_emit", k_emit, None),
                             ("kernels: count + host read + emit", k_both, None), ("package: TSDFVolume.extract", lambda: vol.extract(), None)])
            result["extract"][f"{n}^3"] = {"vertices": nv, "faces": nf, **{name: row(name, ts, extra) for name, ts in times.items()}}
            del scratch, vertices, faces
        del cams, depth, vol
        torch.cuda.empty_cache()
    del points, tsdf, weight
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out, flush=True)
