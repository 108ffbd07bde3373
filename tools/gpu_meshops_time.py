"""What does the mesh clean-up (csrc/meshops.hip: gsr_mesh_components, gsr_mesh_compact_count + _emit, gsr_mesh_vertex_normals, gsr_mesh_smooth) cost on
the meshes the extraction yields, beside the same operations written in plain torch on the same device, in the same process?

    python tools/gpu_meshops_time.py [--dims 256,512] [--samples 20] [--torch-samples 5] [--out profiles/meshops_time.json]

Scene: the sphere of radius 0.6 in the volume [-1,1]^3 of tools/gpu_mesh_time.py as an analytic signed distance, plus a 16^3 lattice of small blobs
(2 .. 3.2 voxels in radius) outside a shell around it -- some thousand floaters -- extracted with TSDFVolume.extract.  Timed, each as the median
of --samples windows after a warm-up, a window being as many calls as fill 50 ms, by device events (the calls that read a word back end in a
synchronise of their own):
  components         gsr_mesh_components: labels and face counts, every round's host read included; the number of rounds is recorded
  compact            count + the host read of the two counts + emit, with the mask of filter_components(keep_largest=1)
  filter_components  the package call: components + threshold and mask in torch + compaction
  vertex_normals     corner sort + bounds + the per-vertex sum
  smooth             corner sort + bounds + 2 x 10 steps; and the marginal cost of one more iteration
Beside each time stand the bytes the operation must move at least -- every array it reads or writes counted once per pass at its own size, every
gather at the size of what it fetches; the formulas are in `bytes_of` -- and their rate against the measured HBM peak (6.29 TB/s): every kernel
here is a streaming or gather pass, none is bound by arithmetic.  Context, --torch-samples windows of one call: label propagation with
scatter_reduce(amin) and pointer jumping until nothing changes, fp64 normals with index_add_, boolean mask + cumsum compaction.  Before timing,
the labels, the counts and the compaction are compared with the torch formulation at the timed size."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
import torch  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402
from gsr_scene import mesh  # noqa: E402

HBM_PEAK = 6.29e12
MIN_WINDOW = 0.05      # seconds of work per timed window, at least
SMOOTH_ITERATIONS = 10

ap = argparse.ArgumentParser()
ap.add_argument("--dims", default="256,512")
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--torch-samples", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshops_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_meshops_time.py: no HIP device")
dev = torch.device("cuda:0")
lib = pkg._lib.load()
stream = pkg._stream_ptr(dev)
Pt = pkg._ptr


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


def measure(fn, samples, window=True):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps = max(1, min(2000, int(math.ceil(MIN_WINDOW / max(timed(fn, 2), 1e-7))))) if window else 1
    return [timed(fn, reps) for _ in range(samples)], reps


def row(name, ts, reps, nbytes=None):
    t = statistics.median(ts)
    out = {"ms": t * 1e3, "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3, "samples": len(ts), "calls_per_sample": reps}
    if nbytes is not None:
        out.update({"bytes": nbytes, "tb_per_s": nbytes / t / 1e12, "fraction_of_hbm_peak": nbytes / t / HBM_PEAK})
    print(f"  {name:46s} {t * 1e3:9.3f} ms ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})" +
          (f"   {nbytes / 1e6:9.1f} MB  {nbytes / t / 1e12:6.3f} TB/s  {100 * nbytes / t / HBM_PEAK:5.1f} % of HBM peak" if nbytes is not None else ""), flush=True)
    return out


def field(n):
    """tsdf [n,n,n] of the sphere and the blob lattice, in units of a truncation of 4 voxels, clamped to [-1, 1]."""
    voxel = 2.0 / (n - 1)
    g = torch.arange(n, device=dev, dtype=torch.float32) * voxel - 1.0
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    d = r - 0.6
    period = n // 16
    idx = torch.arange(n, device=dev)
    cell, local = idx // period, (idx % period).float() - 0.5 * (period - 1)
    cz, cy, cx = torch.meshgrid(cell, cell, cell, indexing="ij")
    lz, ly, lx = torch.meshgrid(local, local, local, indexing="ij")
    radius = 2.0 + 0.3 * ((cx * 7 + cy * 13 + cz * 29) % 5).float()      # voxels
    blob = (torch.sqrt(lx * lx + ly * ly + lz * lz) - radius) * voxel
    centre_r = torch.sqrt(sum(((c.float() + 0.5) * period * voxel - 1.0) ** 2 for c in (cx, cy, cz)))
    d = torch.where((centre_r - 0.6).abs() > 0.15, torch.minimum(d, blob), d)
    return (d / (4 * voxel)).clamp(-1.0, 1.0)


def scratch_of(nv, nf):
    s = torch.empty(int(lib.gsr_meshops_scratch_bytes(nv, nf)) + 128, dtype=torch.uint8, device=dev)
    return s[(-s.data_ptr()) % 128:]


# ---- the same operations in plain torch ----------------------------------------------------------------------------------------------------------
def torch_components(nv, f):
    """Label propagation: every edge pulls both ends to the smaller label (scatter_reduce amin), then one pointer jump; until nothing changes."""
    u = torch.cat([f[:, 0], f[:, 1], f[:, 2]]).long()
    w = torch.cat([f[:, 1], f[:, 2], f[:, 0]]).long()
    label = torch.arange(nv, device=dev)
    rounds = 0
    while True:
        rounds += 1
        low = torch.minimum(label[u], label[w])
        new = label.scatter_reduce(0, u, low, "amin").scatter_reduce(0, w, low, "amin")
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    count = torch.bincount(label[f[:, 0].long()], minlength=nv)
    return label, count, rounds


def torch_normals(v, f):
    p = v.double()
    a, b, c = p[f[:, 0].long()], p[f[:, 1].long()], p[f[:, 2].long()]
    cross = torch.cross(b - a, c - a, dim=1)
    n = torch.zeros_like(p)
    for k in range(3):
        n.index_add_(0, f[:, k].long(), cross)
    return (n / n.norm(dim=1, keepdim=True).clamp_min(1e-300)).float()


def torch_compact(v, f, keep):
    kf = f[keep].long()
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=dev)
    used[kf.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    return v[used], new[kf].int()


def bytes_of(nv, nf, nv2, nf2, rounds, sort_passes):
    """The least each operation moves.  n3 = 3 nf corners.  A face row is 12 bytes, a position 12, a label 4, a keep flag 1."""
    n3 = 3 * nf
    sort = 8 * n3 + sort_passes * (4 * n3 + 16 * n3) + 4 * nv + 4 * nv      # keys and values written; per pass: keys read, pairs read and written; bounds
    return {
        # init (labels, counts written) + per round: hook (faces read, three labels gathered) and compress (label read and written) + the count (faces, a label, an add)
        "components": 8 * nv + rounds * (12 * nf + 12 * nf + 8 * nv) + 12 * nf + 4 * nf + 4 * nf,
        # marks cleared; mark: faces, flags read, three marks written; count: marks, faces, flags; emit: marks, remap written, kept positions copied; faces, flags, three remaps, rows written
        "compact": 4 * nv + (13 * nf + 12 * nf2) + (4 * nv + 13 * nf) + (4 * nv + 4 * nv2 + 24 * nv2) + (13 * nf + 12 * nf2 + 12 * nf2),
        # sort + per corner: its index, its face row, three positions; per vertex: two bounds, a normal written
        "vertex_normals": sort + n3 * (4 + 12 + 36) + 8 * nv + 12 * nv,
        # per step and corner: its index, its face row, two positions; per vertex: two bounds, its position read and written
        "smooth_step": n3 * (4 + 12 + 24) + 8 * nv + 24 * nv,
        "sort": sort,
    }


result = {"samples": args.samples, "torch_samples": args.torch_samples, "window_s_at_least": MIN_WINDOW, "hbm_peak_tb_per_s": HBM_PEAK / 1e12,
          "smooth_iterations": SMOOTH_ITERATIONS, "sizes": {}}
for n in (int(v) for v in args.dims.split(",")):
    voxel = 2.0 / (n - 1)
    vol = mesh.TSDFVolume((-1.0, -1.0, -1.0), voxel, (n, n, n), 4 * voxel, dev)
    vol.tsdf.copy_(field(n))
    vol.weight.fill_(1.0)
    m = vol.extract()
    del vol
    torch.cuda.empty_cache()
    v, f = m.vertices, m.faces
    nv, nf = int(v.shape[0]), int(f.shape[0])
    scratch = scratch_of(nv, nf)
    label, count = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nv, dtype=torch.int32, device=dev)

    def k_components():
        ok(lib.gsr_mesh_components(nv, nf, Pt(f), Pt(label), Pt(count), Pt(scratch), stream), "gsr_mesh_components")
    k_components()
    rounds = int(lib.gsr_mesh_components_rounds())
    parts = int((count > 0).sum())
    largest = int(count.max())
    t_label, t_count, t_rounds = torch_components(nv, f)
    assert torch.equal(t_label.int(), label) and torch.equal(t_count.int(), count), "the kernel's labels differ from the torch formulation"
    keep = (count[label[f[:, 0].long()].long()] >= largest).view(torch.uint8)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ok(lib.gsr_mesh_compact_count(nv, nf, Pt(f), Pt(keep), Pt(scratch), Pt(counts), stream), "gsr_mesh_compact_count")
    nv2, nf2 = counts.tolist()
    v2, f2 = torch.empty((nv2, 3), device=dev), torch.empty((nf2, 3), dtype=torch.int32, device=dev)

    def k_compact():
        ok(lib.gsr_mesh_compact_count(nv, nf, Pt(f), Pt(keep), Pt(scratch), Pt(counts), stream), "gsr_mesh_compact_count")
        counts.tolist()
        ok(lib.gsr_mesh_compact_emit(nv, nf, Pt(v), None, Pt(f), Pt(keep), Pt(scratch), nv2, nf2, Pt(v2), None, Pt(f2), stream), "gsr_mesh_compact_emit")
    k_compact()
    tv, tf = torch_compact(v, f, keep.bool())
    assert torch.equal(tv, v2) and torch.equal(tf, f2), "the kernel's compaction differs from the torch formulation"
    normals, smoothed = torch.empty((nv, 3), device=dev), torch.empty((nv, 3), device=dev)

    def k_normals():
        ok(lib.gsr_mesh_vertex_normals(nv, nf, Pt(v), Pt(f), Pt(normals), Pt(scratch), stream), "gsr_mesh_vertex_normals")

    def k_smooth(iterations):
        ok(lib.gsr_mesh_smooth(nv, nf, Pt(v), Pt(f), iterations, 0.5, -0.53, Pt(smoothed), Pt(scratch), stream), "gsr_mesh_smooth")
    k_normals()
    gap = float((normals - torch_normals(v, f)).abs().max())
    nbits = max(1, nv.bit_length())
    b = bytes_of(nv, nf, nv2, nf2, rounds, (nbits + 7) // 8)
    print(f"{n}^3 voxels: {nv} vertices, {nf} faces in {parts} components (the largest {largest} faces); components settle in {rounds} rounds "
          f"(torch label propagation: {t_rounds}); keep_largest=1 leaves {nv2} vertices, {nf2} faces; normals differ from torch's index_add_ by {gap:.1e} at most",
          flush=True)
    entry = {"vertices": nv, "faces": nf, "components": parts, "largest_component_faces": largest, "component_rounds": rounds,
             "torch_label_propagation_rounds": t_rounds, "kept_vertices": nv2, "kept_faces": nf2, "normals_max_difference_from_torch": gap}
    S = args.samples
    entry["kernel: gsr_mesh_components"] = row("kernel: gsr_mesh_components", *measure(k_components, S), b["components"])
    entry["kernels: compact count + host read + emit"] = row("kernels: compact count + host read + emit", *measure(k_compact, S), b["compact"])
    entry["package: filter_components(keep_largest=1)"] = row("package: filter_components(keep_largest=1)",
                                                              *measure(lambda: mesh.filter_components(m, keep_largest=1), S))
    entry["kernel: gsr_mesh_vertex_normals"] = row("kernel: gsr_mesh_vertex_normals", *measure(k_normals, S), b["vertex_normals"])
    ts10, reps10 = measure(lambda: k_smooth(SMOOTH_ITERATIONS), S)
    ts11, reps11 = measure(lambda: k_smooth(SMOOTH_ITERATIONS + 1), S)
    entry["kernel: gsr_mesh_smooth, 10 iterations"] = row("kernel: gsr_mesh_smooth, 10 iterations", ts10, reps10, b["sort"] + 2 * SMOOTH_ITERATIONS * b["smooth_step"])
    per_iteration = statistics.median(ts11) - statistics.median(ts10)
    entry["smooth_ms_per_further_iteration"] = per_iteration * 1e3
    entry["smooth_step_tb_per_s"] = 2 * b["smooth_step"] / max(per_iteration, 1e-9) / 1e12
    print(f"  one more smoothing iteration (two steps)       {per_iteration * 1e3:9.3f} ms   {2 * b['smooth_step'] / 1e6:9.1f} MB  {entry['smooth_step_tb_per_s']:6.3f} TB/s",
          flush=True)
    T = args.torch_samples
    entry["torch: scatter_reduce(amin) label propagation"] = row("torch: scatter_reduce(amin) label propagation", *measure(lambda: torch_components(nv, f), T, False))
    entry["torch: mask + cumsum compaction"] = row("torch: mask + cumsum compaction", *measure(lambda: torch_compact(v, f, keep.bool()), T, False))
    entry["torch: index_add_ normals (fp64)"] = row("torch: index_add_ normals (fp64)", *measure(lambda: torch_normals(v, f), T, False))
    result["sizes"][f"{n}^3"] = entry
    del m, v, f, scratch, label, count, keep, v2, f2, normals, smoothed, tv, tf, t_label, t_count
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out, flush=True)
