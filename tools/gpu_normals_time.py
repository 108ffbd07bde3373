"""What do the normal-consistency kernels (gsr_gaussian_normals, gsr_depth_normals, gsr_normal_loss and their backwards, csrc/normals.hip) cost
beside the same computation written in fp32 torch (the expressions of tests/normals_reference.py, run on the device) in the same process?

    python tools/gpu_normals_time.py [--sizes 1080x1920,2160x3840] [--points 1000000] [--reps 20] [--rounds 5] [--out profiles/normals_time.json]

The three forward / backward pairs: per-Gaussian normals at `points` rows; depth -> normals and the fused loss per image size (the kernels
through the C ABI: no allocation in the timed call; torch: the forward under no_grad, the backward as autograd.grad on a retained graph).
Device-event time of `reps` calls, the variants alternating round by round; the median round is reported with the ALGORITHMIC bytes over that
time and the fraction of the measured HBM peak (6.29 TB/s): per-Gaussian forward 28 B per row (scales and quaternion; the kernel also reads the
mean for the sign and writes the normal, 52 B in all, printed as `moved`), its backward 56 (68 moved); depth -> normals 16 B per pixel forward
and 20 backward; the loss 20 B per pixel forward (depth, three normal planes, weight) and 36 backward with both gradients.  The images are
smaller than the 256 MiB Infinity Cache: the fractions are of the HBM figure all the same, as an upper bound of what memory could cost."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402
import normals_reference as NR  # noqa: E402

HBM_PEAK = 6.29e12

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1080x1920,2160x3840")
ap.add_argument("--points", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_normals_time.py: no HIP device")
dev = torch.device("cuda:0")
lib = pkg._lib.load()
stream = pkg._stream_ptr(dev)
P = pkg._ptr
TX, TY = NR.TANFOV


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def measure(variants):
    """variants: [(name, fn, algorithmic bytes, bytes moved)] -> {name: {...}}; warm-up, then `rounds` rounds with the variants alternating."""
    for _, fn, _, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {v[0]: [] for v in variants}
    for _ in range(args.rounds):
        for name, fn, _, _ in variants:
            times[name].append(timed(fn, args.reps))
    out = {}
    for name, _, nbytes, moved in variants:
        t = statistics.median(times[name])
        out[name] = {"us": t * 1e6, "us_min": min(times[name]) * 1e6, "us_max": max(times[name]) * 1e6, "bytes": nbytes, "bytes_moved": moved,
                     "tb_per_s": nbytes / t / 1e12, "tb_per_s_moved": moved / t / 1e12, "fraction_of_hbm_peak": nbytes / t / HBM_PEAK}
        print(f"  {name:44s} {t * 1e6:9.1f} us ({min(times[name]) * 1e6:.1f} .. {max(times[name]) * 1e6:.1f})   {nbytes / 1e6:8.1f} MB   "
              f"{nbytes / t / 1e12:6.2f} TB/s ({moved / t / 1e12:.2f} moved)   {100 * nbytes / t / HBM_PEAK:5.1f} % of HBM peak", flush=True)
    return out


def ok(rc, what):
    pkg._lib.check(rc, what)


result = {"reps": args.reps, "rounds": args.rounds, "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "gaussians": {}, "images": {}}
gen = torch.Generator(device=dev).manual_seed(0)

# ---- per-Gaussian normals -----------------------------------------------------------------------------------------------------------------------
n = args.points
q = torch.randn(n, 4, device=dev, generator=gen)
q = (q / q.norm(dim=1, keepdim=True)).contiguous()
s = torch.exp(torch.randn(n, 3, device=dev, generator=gen) * 0.6 - 3.0)
m = torch.randn(n, 3, device=dev, generator=gen) + torch.tensor([0.0, 0.0, 5.0], device=dev)
vm = NR.view_matrix().to(dev)
dn = torch.randn(n, 3, device=dev, generator=gen)
out_n, out_q = torch.empty(n, 3, device=dev), torch.empty(n, 4, device=dev)
tq = q.clone().requires_grad_(True)
t_n = NR.gaussian_normals(s, tq, m, vm)
ok(lib.gsr_gaussian_normals(n, P(s), P(q), P(m), P(vm), P(out_n), stream), "gsr_gaussian_normals")
print(f"per-Gaussian normals, {n} rows: {args.rounds} rounds of {args.reps} calls, median round (min .. max)", flush=True)
print(f"  (largest difference of the two forwards: {float((out_n - t_n.detach()).abs().max()):.2e})", flush=True)
variants = [("kernel: gaussian normals forward", lambda: ok(lib.gsr_gaussian_normals(n, P(s), P(q), P(m), P(vm), P(out_n), stream), "fwd"), 28 * n, 52 * n),
            ("torch: gaussian normals forward", lambda: NR.gaussian_normals(s, q, m, vm), 28 * n, 52 * n),
            ("kernel: gaussian normals backward", lambda: ok(lib.gsr_gaussian_normals_backward(n, P(s), P(q), P(m), P(vm), P(dn), P(out_q), stream), "bwd"),
             56 * n, 68 * n),
            ("torch: gaussian normals backward", lambda: torch.autograd.grad(t_n, [tq], dn, retain_graph=True), 56 * n, 68 * n)]
with torch.no_grad():
    fwd = measure(variants[:2])
result["gaussians"][str(n)] = {**fwd, **measure(variants[2:])}
del t_n, tq
torch.cuda.empty_cache()

# ---- depth -> normals and the fused loss --------------------------------------------------------------------------------------------------------
for size in args.sizes.split(","):
    H, W = (int(v) for v in size.split("x"))
    npix = H * W
    u = ((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W * 2 - 1)[None, :]
    v = ((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H * 2 - 1)[:, None]
    depth = (4.0 + 0.2 * u - 0.1 * v + 0.15 * torch.sin(2.2 * u + 1.0) * torch.cos(1.7 * v)).contiguous()
    normals = torch.randn(3, H, W, device=dev, generator=gen)
    normals = (normals / normals.norm(dim=0, keepdim=True)).contiguous()
    weight = torch.rand(H, W, device=dev, generator=gen)
    dL = torch.randn(3, H, W, device=dev, generator=gen)
    nd, gz, gn = torch.empty(3, H, W, device=dev), torch.empty(H, W, device=dev), torch.empty(3, H, W, device=dev)
    count = int(lib.gsr_normal_loss_partial_count(H, W))
    partials, loss, one = torch.empty(count, dtype=torch.float64, device=dev), torch.empty((), device=dev), torch.ones(1, device=dev)

    def k_map():
        ok(lib.gsr_depth_normals(H, W, TX, TY, P(depth), P(nd), stream), "gsr_depth_normals")

    def k_map_bwd():
        ok(lib.gsr_depth_normals_backward(H, W, TX, TY, P(depth), P(dL), P(gz), stream), "gsr_depth_normals_backward")

    def k_loss():
        ok(lib.gsr_normal_loss(H, W, TX, TY, P(depth), P(normals), P(weight), P(partials), P(loss), stream), "gsr_normal_loss")

    def k_loss_bwd(both=True):
        ok(lib.gsr_normal_loss_backward(H, W, TX, TY, P(depth), P(normals), P(weight), P(one), P(gn) if both else None, P(gz), stream),
           "gsr_normal_loss_backward")
    tz, tn = depth.clone().requires_grad_(True), normals.clone().requires_grad_(True)
    t_nd = NR.depth_to_normal(tz, TX, TY)
    t_loss = NR.normal_consistency_loss(tz, tn, TX, TY, weight)
    k_map()
    k_loss()
    print(f"{H} x {W}: {args.rounds} rounds of {args.reps} calls, median round (min .. max)", flush=True)
    print(f"  (largest difference of the two normal maps: {float((nd - t_nd.detach()).abs().max()):.2e}; losses {float(loss):.7f} / "
          f"{float(t_loss.detach()):.7f})", flush=True)
    variants = [("kernel: depth -> normals forward", k_map, 16 * npix, 16 * npix),
                ("torch: depth -> normals forward", lambda: NR.depth_to_normal(depth, TX, TY), 16 * npix, 16 * npix),
                ("kernel: loss forward", k_loss, 20 * npix, 20 * npix),
                ("torch: loss forward", lambda: NR.normal_consistency_loss(depth, normals, TX, TY, weight), 20 * npix, 20 * npix),
                ("kernel: depth -> normals backward", k_map_bwd, 20 * npix, 20 * npix),
                ("torch: depth -> normals backward", lambda: torch.autograd.grad(t_nd, [tz], dL, retain_graph=True), 20 * npix, 20 * npix),
                ("kernel: loss backward, depth + normals", k_loss_bwd, 36 * npix, 36 * npix),
                ("torch: loss backward, depth + normals", lambda: torch.autograd.grad(t_loss, [tz, tn], retain_graph=True), 36 * npix, 36 * npix),
                ("kernel: loss backward, depth only", lambda: k_loss_bwd(False), 24 * npix, 24 * npix)]
    with torch.no_grad():
        fwd = measure(variants[:4])
    result["images"][size] = {**fwd, **measure(variants[4:]), "loss_partials": count}
    del t_nd, t_loss, tz, tn
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", args.out, flush=True)
