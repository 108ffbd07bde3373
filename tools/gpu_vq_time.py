"""What do the two steps of a Lloyd iteration (gsr_vq_assign, gsr_vq_update, csrc/vq.hip) cost beside the only way torch offers on this stack --
torch.cdist in row chunks (which materialises P x K distance blocks) + argmin for the assignment, index_add_ (floating-point atomics) for the
update -- in the same process?

    python tools/gpu_vq_time.py [--P 1000000] [--D 45] [--K 4096,65536] [--reps 5] [--rounds 5] [--out profiles/vq_time.json]

Sweep: every K, weighted and unweighted update; the kernels through the C ABI (no allocation in the timed call).  The assignment is reported as
time of the call (the vq_norms launch included), as TFLOP/s of the 2 P K D operations the algorithm needs and their fraction of the 157.3 TFLOP/s
fp32 matrix peak, beside the 122 TFLOP/s of an untuned LDS-tiled GEMM on the same instruction; the 2 P K DP operations the matrix pipe executes
(DP: D padded to the kernel's pair count) are listed beside them.
The update is reported as time and as TB/s of the rows it reads.  Device-event time of `reps` calls, the variants alternating round by round;
the median round is reported with its spread.  Before timing, the two assignments are compared at the timed size."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
import torch  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
UNTUNED_GEMM = 122e12

ap = argparse.ArgumentParser()
ap.add_argument("--P", type=int, default=1000000)
ap.add_argument("--D", type=int, default=45)
ap.add_argument("--K", default="4096,65536")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cdist-rows", type=int, default=16384, help="rows per torch.cdist chunk (a chunk is rows x K floats)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_vq_time.py: no HIP device")
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


def measure(variants):
    """variants: [(name, fn, reps)] -> {name: [seconds per call, one per round]}; warm-up, then the variants alternating round by round."""
    for _, fn, _ in variants:
        fn()
    torch.cuda.synchronize()
    times = {v[0]: [] for v in variants}
    for _ in range(args.rounds):
        for name, fn, reps in variants:
            times[name].append(timed(fn, reps))
    return times


def row(name, ts, extra):
    t = statistics.median(ts)
    out = {"us": t * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6}
    out.update({k: f(t) for k, f in extra.items()})
    print(f"  {name:52s} {t * 1e6:11.1f} us ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})   " + "   ".join(f"{k} {v:.4g}" for k, v in out.items() if not k.startswith("us")),
          flush=True)
    return out


def torch_assign(x, cb, chunk):
    idx = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        idx[i:i + chunk] = torch.cdist(x[i:i + chunk], cb).argmin(dim=1)
    return idx


def torch_update(x, w, idx, K):
    sums = torch.zeros(K, x.shape[1], device=x.device).index_add_(0, idx, x if w is None else x * w[:, None])
    mass = torch.zeros(K, device=x.device).index_add_(0, idx, torch.ones_like(x[:, 0]) if w is None else w)
    return sums / mass.clamp_min(1e-30)[:, None], mass


P, D = args.P, args.D
DP = 2 * (4 if D <= 8 else 8 if D <= 16 else 16 if D <= 32 else 24 if D <= 48 else 32)      # vq_pairs of csrc/vq.hip
g = torch.Generator().manual_seed(1)
rows = torch.randn(P, D, generator=g).to(dev)
weights = (torch.rand(P, generator=g) + 0.01).to(dev)
result = {"P": P, "D": D, "DP": DP, "reps": args.reps, "rounds": args.rounds, "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK / 1e12,
          "untuned_gemm_tflops": UNTUNED_GEMM / 1e12, "K": {}}
for K in (int(v) for v in args.K.split(",")):
    cb = rows[torch.randperm(P, generator=g)[:K].to(dev)].clone()
    idx, dist2, mass = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, device=dev), torch.empty(K, device=dev)
    scratch = torch.empty(int(lib.gsr_vq_scratch_bytes(P, D, K)), dtype=torch.uint8, device=dev)
    new = cb.clone()

    def k_assign():
        ok(lib.gsr_vq_assign(P, D, K, Pt(rows), Pt(cb), Pt(idx), Pt(dist2), Pt(scratch), stream), "gsr_vq_assign")

    def k_update(w):
        ok(lib.gsr_vq_update(P, D, K, Pt(rows), Pt(w), Pt(idx), Pt(new), Pt(mass), Pt(scratch), stream), "gsr_vq_update")
    k_assign()
    want = torch_assign(rows, cb, args.cdist_rows)
    differ = int((idx.long() != want).sum())
    print(f"P {P} D {D} K {K}: {args.rounds} rounds of {args.reps} calls, median round (min .. max); {differ} of {P} rows are assigned differently from "
          f"torch.cdist + argmin (fp32 near-ties)", flush=True)
    idx64 = idx.long()
    flops, useful = 2.0 * P * K * DP, 2.0 * P * K * D
    times = measure([("kernel: gsr_vq_assign", k_assign, args.reps),
                     ("torch: chunked cdist + argmin", lambda: torch_assign(rows, cb, args.cdist_rows), max(1, args.reps // 5))])
    # the shares are of the operations the algorithm NEEDS (2 P K D); the call includes the vq_norms launch
    extra = {"tflops_useful": lambda t: useful / t / 1e12, "fraction_of_fp32_matrix_peak": lambda t: useful / t / FP32_MATRIX_PEAK,
             "of_the_untuned_gemm": lambda t: useful / t / UNTUNED_GEMM, "tflops_executed": lambda t: flops / t / 1e12}
    entry = {"differ": differ, **{name: row(name, ts, extra) for name, ts in times.items()}}
    times = measure([("kernel: gsr_vq_update", lambda: k_update(None), args.reps), ("kernel: gsr_vq_update, weighted", lambda: k_update(weights), args.reps),
                     ("torch: index_add_", lambda: torch_update(rows, None, idx64, K), args.reps),
                     ("torch: index_add_, weighted", lambda: torch_update(rows, weights, idx64, K), args.reps)])
    entry.update({name: row(name, ts, {"tb_per_s_of_the_rows": lambda t: 4.0 * P * D / t / 1e12}) for name, ts in times.items()})
    result["K"][str(K)] = entry
    del want, idx64, scratch
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out, flush=True)
