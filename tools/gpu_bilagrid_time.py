"""What do the bilateral-grid kernels (gsr_bilagrid_*, csrc/bilagrid.hip) cost beside the same computation written with torch's grid_sample /
tensor ops on the same GPU, in the same process?

    python tools/gpu_bilagrid_time.py [--sizes 1080x1920,2160x3840] [--grid 16x16x8] [--reps 20] [--rounds 5] [--out profiles/bilagrid_time.json]

Per image size: slice forward, slice backward with and without the image gradient (the kernels through the C ABI: no allocation in the timed
call; torch: autograd.grad through the 5-D grid_sample on a retained graph, its atomics included); total variation forward and backward at N = 1
and N = 200.  Device-event time of `reps` calls, the variants alternating round by round; the median round is reported with the bytes the
computation has to move (forward 24 B per pixel, backward 36 or 48 B per pixel plus the partial blocks, written once and read once; TV 4 B per
element forward, 8 B backward) over that time and the fraction of the measured HBM peak (6.29 TB/s).  The images are smaller than the 256 MiB
Infinity Cache: the fractions are of the HBM figure all the same, as an upper bound of what memory could cost."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402

HBM_PEAK = 6.29e12

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1080x1920,2160x3840")
ap.add_argument("--grid", default="16x16x8", help="Gw x Gh x L")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilagrid_time.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_bilagrid_time.py: no HIP device")
dev = torch.device("cuda:0")
lib = pkg._lib.load()
Gw, Gh, L = (int(v) for v in args.grid.split("x"))
stream = pkg._stream_ptr(dev)
P = pkg._ptr


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def measure(variants):
    """variants: [(name, fn, bytes)] -> {name: {...}}; warm-up, then `rounds` rounds with the variants alternating."""
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, fn, _ in variants:
            times[name].append(timed(fn, args.reps))
    out = {}
    for name, _, nbytes in variants:
        t = statistics.median(times[name])
        out[name] = {"us": t * 1e6, "us_min": min(times[name]) * 1e6, "us_max": max(times[name]) * 1e6, "bytes": nbytes,
                     "tb_per_s": nbytes / t / 1e12, "fraction_of_hbm_peak": nbytes / t / HBM_PEAK}
        print(f"  {name:44s} {t * 1e6:9.1f} us ({min(times[name]) * 1e6:.1f} .. {max(times[name]) * 1e6:.1f})   {nbytes / 1e6:8.1f} MB   "
              f"{nbytes / t / 1e12:6.2f} TB/s   {100 * nbytes / t / HBM_PEAK:5.1f} % of HBM peak", flush=True)
    return out


def torch_slice(grid, image):
    """The slice through torch's 5-D grid_sample (what lib_bilagrid does), planar image in and out."""
    _, H, W = image.shape
    u = ((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W)[None, :].expand(H, W)
    v = ((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H)[:, None].expand(H, W)
    g = 0.299 * image[0] + 0.587 * image[1] + 0.114 * image[2]
    coords = torch.stack([u * 2 - 1, v * 2 - 1, g * 2 - 1], dim=-1)[None, None]
    A = F.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].view(3, 4, H, W)
    return (A[:, :3] * image[None]).sum(1) + A[:, 3]


def torch_tv(X):
    return sum(torch.diff(X, dim=d).pow(2).mean() for d in (2, 3, 4))


result = {"grid": {"Gw": Gw, "Gh": Gh, "L": L}, "reps": args.reps, "rounds": args.rounds, "hbm_peak_tb_per_s": HBM_PEAK / 1e12, "slice": {}, "tv": {}}
gen = torch.Generator(device=dev).manual_seed(0)
for size in args.sizes.split(","):
    H, W = (int(v) for v in size.split("x"))
    grid = torch.randn(12, L, Gh, Gw, device=dev, generator=gen) * 0.3
    image = torch.rand(3, H, W, device=dev, generator=gen)
    dL = torch.randn(3, H, W, device=dev, generator=gen)
    out, dgrid, dimage = torch.empty_like(image), torch.empty_like(grid), torch.empty_like(image)
    nbytes = int(lib.gsr_bilagrid_scratch_bytes(H, W, L, Gh, Gw))
    scratch = torch.empty(nbytes // 4, device=dev)
    npix = H * W

    def k_fwd():
        pkg._lib.check(lib.gsr_bilagrid_slice(H, W, L, Gh, Gw, P(grid), P(image), P(out), stream), "gsr_bilagrid_slice")

    def k_bwd(with_image):
        pkg._lib.check(lib.gsr_bilagrid_slice_backward(H, W, L, Gh, Gw, P(grid), P(image), P(dL), P(dgrid), P(dimage) if with_image else None,
                                                       P(scratch), nbytes, stream), "gsr_bilagrid_slice_backward")
    tg, ti = grid.clone().requires_grad_(True), image.clone().requires_grad_(True)
    t_out = torch_slice(tg, ti)
    print(f"{H} x {W}, grid {Gw} x {Gh} x {L}: {args.rounds} rounds of {args.reps} calls, median round (min .. max)", flush=True)
    with torch.no_grad():
        diff = float((torch_slice(grid, image) - (k_fwd(), out)[1]).abs().max())
    print(f"  (largest difference of the two forwards: {diff:.2e})", flush=True)
    variants = [("kernel: slice forward", k_fwd, 24 * npix),
                ("torch: slice forward", lambda: torch_slice(grid, image), 24 * npix),
                ("kernel: backward, grid + image gradient", lambda: k_bwd(True), 48 * npix + 2 * nbytes),
                ("torch: backward, grid + image gradient", lambda: torch.autograd.grad(t_out, [tg, ti], dL, retain_graph=True), 48 * npix),
                ("kernel: backward, grid gradient only", lambda: k_bwd(False), 36 * npix + 2 * nbytes),
                ("torch: backward, grid gradient only", lambda: torch.autograd.grad(t_out, [tg], dL, retain_graph=True), 36 * npix)]
    with torch.no_grad():
        fwd = measure(variants[:2])
    result["slice"][size] = {**fwd, **measure(variants[2:]), "scratch_bytes": nbytes, "forward_max_difference": diff}
    del t_out, tg, ti, scratch
    torch.cuda.empty_cache()

for N in (1, 200):
    X = torch.randn(N, 12, L, Gh, Gw, device=dev, generator=gen)
    n = X.numel()
    count = int(lib.gsr_bilagrid_tv_partial_count(N, L, Gh, Gw))
    partials, tv, dX = torch.empty(count, dtype=torch.float64, device=dev), torch.empty((), device=dev), torch.empty_like(X)
    one = torch.ones(1, device=dev)
    tx = X.clone().requires_grad_(True)
    t_tv = torch_tv(tx)
    print(f"total variation, N = {N} ({n} elements)", flush=True)
    variants = [("kernel: tv forward", lambda: pkg._lib.check(lib.gsr_bilagrid_tv(N, L, Gh, Gw, P(X), P(partials), P(tv), stream), "gsr_bilagrid_tv"), 4 * n),
                ("torch: tv forward", lambda: torch_tv(X), 4 * n),
                ("kernel: tv backward", lambda: pkg._lib.check(lib.gsr_bilagrid_tv_backward(N, L, Gh, Gw, P(X), P(one), P(dX), stream), "gsr_bilagrid_tv_backward"), 8 * n),
                ("torch: tv backward", lambda: torch.autograd.grad(t_tv, [tx], retain_graph=True), 8 * n)]
    with torch.no_grad():
        fwd = measure(variants[:2])
    result["tv"][str(N)] = {**fwd, **measure(variants[2:])}

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", args.out, flush=True)
