"""What do the kernels of the 3D smoothing filter (gsr_mip_filter_3d, gsr_mip_activations and its backward, csrc/mip.hip) cost beside upstream's
torch expressions -- the camera loop of compute_3D_filter and the activation chain, fp32 on the device -- in the same process?

    python tools/gpu_mip_time.py [--P 1000000,6000000] [--C 64,256] [--reps 20] [--rounds 5] [--out profiles/mip_time.json]

Sweep: every (P, C); the kernel through the C ABI (no allocation in the timed call) and the package call (pack once, allocate, launch), beside
upstream's loop with the camera matrices on the device already (its `torch.tensor(camera.R, device=...)` uploads left out, in its favour).
Reported: time, (Gaussian, camera) pairs per second, and the fraction of the fp32 vector peak (157.3 TFLOP/s) the pairs stand for at
PAIR_FLOPS operations each, counted from the source: nine fused multiply-adds (18), four products, four comparisons, a minimum and a select.
Activations: forward (20 B in, 16 B out per Gaussian) and backward (36 B in with both gradients, 16 B out) beside upstream's chain (forward
under no_grad, backward as autograd.grad on a retained graph), and beside the two streaming kernels of the library at the same P: the MCMC noise
pass (68 B per Gaussian) and the fused Adam step on 3 P elements (28 B per element), as TB/s of the bytes the algorithm moves and the fraction
of the measured HBM peak (6.29 TB/s).  Device-event time of `reps` calls, the variants alternating round by round; the median round is
reported with its spread.  Before timing, the two sweeps and the two activation chains are compared at the timed size."""
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
import mip_reference as MR  # noqa: E402
from gsr_scene import mip  # noqa: E402

HBM_PEAK = 6.29e12
FP32_VECTOR_PEAK = 157.3e12
PAIR_FLOPS = 28

ap = argparse.ArgumentParser()
ap.add_argument("--P", default="1000000,6000000")
ap.add_argument("--C", default="64,256")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--torch-sweep-reps", type=int, default=1, help="calls of upstream's camera loop per round (one call is C x ~25 launches)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mip_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_mip_time.py: no HIP device")
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
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {v[0]: [] for v in variants}
    for _ in range(args.rounds):
        for name, fn, reps in variants:
            times[name].append(timed(fn, reps))
    return times


def upstream_sweep(xyz, cams):
    """compute_3D_filter of the Mip-Splatting code base on device tensors; cams: [(R [3,3], T [3], focal_x, focal_y, W, H)]."""
    distance = torch.ones((xyz.shape[0]), device=xyz.device) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    focal_length = 0.0
    for R, T, focal_x, focal_y, width, height in cams:
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * focal_x + width / 2.0
        y = y / z * focal_y + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15), torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], xyz_cam[:, 2][valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < focal_x:
            focal_length = focal_x
    distance[~valid_points] = distance[valid_points].max()
    return (distance / focal_length * (0.2 ** 0.5))[..., None]


def row(name, ts, extra):
    t = statistics.median(ts)
    out = {"us": t * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6}
    out.update({k: f(t) for k, f in extra.items()})
    print(f"  {name:52s} {t * 1e6:11.1f} us ({min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})   " + "   ".join(f"{k} {v:.4g}" for k, v in out.items() if not k.startswith("us")),
          flush=True)
    return out


result = {"reps": args.reps, "rounds": args.rounds, "pair_flops": PAIR_FLOPS, "fp32_vector_peak_tflops": FP32_VECTOR_PEAK / 1e12,
          "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "sweep": {}, "activations": {}}
sizes = [int(v) for v in args.P.split(",")]
ncams = [int(v) for v in args.C.split(",")]

for n in sizes:
    for C in ncams:
        means, cams = MR.make_scene(n, C, seed=7)
        means, cams = means.to(dev), cams.to(dev)
        objs = [(c[:9].reshape(3, 3).contiguous(), c[9:12].contiguous(), float(c[12]), float(c[13]), float(c[14]), float(c[15])) for c in cams]
        out = torch.empty(n, device=dev)
        scratch = torch.empty(int(lib.gsr_mip_filter_scratch_bytes(n)), dtype=torch.uint8, device=dev)

        def k_sweep():
            ok(lib.gsr_mip_filter_3d(n, Pt(means), C, Pt(cams), Pt(out), None, Pt(scratch), stream), "gsr_mip_filter_3d")
        k_sweep()
        want = upstream_sweep(means, objs).reshape(-1)
        differ = int((((out - want).abs() > 1e-5 * want.abs())).sum())
        print(f"sweep, P {n} C {C}: {args.rounds} rounds, median round (min .. max); {differ} of {n} values differ from upstream's fp32 loop by more "
              f"than 1e-5 (decisions within rounding of a threshold)", flush=True)
        pairs = n * C
        times = measure([("kernel: gsr_mip_filter_3d", k_sweep, args.reps),
                         ("package: compute_3d_filter (packed cameras)", lambda: mip.compute_3d_filter(means, cams), args.reps),
                         ("torch: upstream's camera loop", lambda: upstream_sweep(means, objs), args.torch_sweep_reps)])
        extra = {"pairs_per_s": lambda t: pairs / t, "fraction_of_fp32_vector_peak": lambda t: pairs * PAIR_FLOPS / t / FP32_VECTOR_PEAK}
        result["sweep"][f"{n}x{C}"] = {"differ": differ, **{name: row(name, ts, extra) for name, ts in times.items()}}
        del want, objs
        torch.cuda.empty_cache()

for n in sizes:
    rs, ro, f, gs, go = (t.to(dev) for t in MR.activation_case(n, 1))
    so, oo, ds, do_ = torch.empty(n, 3, device=dev), torch.empty(n, 1, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 1, device=dev)

    def k_fwd():
        ok(lib.gsr_mip_activations(n, Pt(rs), Pt(ro), Pt(f), Pt(so), Pt(oo), stream), "gsr_mip_activations")

    def k_bwd():
        ok(lib.gsr_mip_activations_backward(n, Pt(rs), Pt(ro), Pt(f), Pt(gs), Pt(go), Pt(ds), Pt(do_), stream), "gsr_mip_activations_backward")
    trs, tro = rs.clone().requires_grad_(True), ro.clone().requires_grad_(True)
    ts_, to_ = MR.filtered_activations_fp32(trs, tro, f)
    k_fwd()
    k_bwd()
    finite = torch.isfinite(to_.detach()).reshape(-1)
    print(f"activations, P {n}: {args.rounds} rounds of {args.reps} calls, median round (min .. max); upstream's fp32 opacity is finite on "
          f"{int(finite.sum())} of {n} rows, largest relative difference of the scales {float(((so - ts_.detach()).abs() / ts_.detach()).max()):.2e}", flush=True)
    # the two streaming kernels of the library the figures stand beside
    xyz, rot, noise = torch.randn(n, 3, device=dev), torch.randn(n, 4, device=dev), torch.randn(n, 3, device=dev)
    ap_, ag, am, av = (torch.randn(3 * n, device=dev) for _ in range(4))
    av.abs_()

    def k_noise():
        ok(lib.gsr_mcmc_inject_noise(n, Pt(xyz), Pt(rs), Pt(rot), Pt(ro), Pt(noise), 0, 1e-6, 100.0, 0.995, stream), "gsr_mcmc_inject_noise")

    def k_adam():
        ok(lib.gsr_adam_step(Pt(ap_), Pt(ag), Pt(am), Pt(av), 3 * n, 1e-3, 0.9, 0.999, 1e-15, 10, stream), "gsr_adam_step")
    fwd_variants = [("kernel: activations forward", k_fwd, args.reps), ("torch: activations forward", lambda: MR.filtered_activations_fp32(rs, ro, f), args.reps)]
    bwd_variants = [("kernel: activations backward", k_bwd, args.reps),
                    ("torch: activations backward", lambda: torch.autograd.grad([ts_, to_], [trs, tro], [gs, go], retain_graph=True), args.reps),
                    ("kernel: gsr_mcmc_inject_noise", k_noise, args.reps), ("kernel: gsr_adam_step, 3 P elements", k_adam, args.reps)]
    with torch.no_grad():
        times = measure(fwd_variants)
    times.update(measure(bwd_variants))
    nbytes = {"kernel: activations forward": 36 * n, "torch: activations forward": 36 * n, "kernel: activations backward": 52 * n,
              "torch: activations backward": 52 * n, "kernel: gsr_mcmc_inject_noise": 68 * n, "kernel: gsr_adam_step, 3 P elements": 28 * 3 * n}
    result["activations"][str(n)] = {
        name: row(name, ts, {"bytes": (lambda t, b=nbytes[name]: b), "tb_per_s": (lambda t, b=nbytes[name]: b / t / 1e12),
                             "fraction_of_hbm_peak": (lambda t, b=nbytes[name]: b / t / HBM_PEAK)}) for name, ts in times.items()}
    del ts_, to_, trs, tro
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out, flush=True)
