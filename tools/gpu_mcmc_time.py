"""What does the MCMC noise pass (gsr_mcmc_inject_noise, csrc/mcmc.hip) cost, beside upstream's torch expression and beside the fused Adam step
(gsr_adam_step_multi) on the same box?

    python tools/gpu_mcmc_time.py [--P 1000000,6000000] [--reps 50] [--rounds 5]

Per size: device-event time of  the kernel with 16-byte accesses (four Gaussians per lane),  the same kernel on buffers that are 4 bytes off a
16-byte boundary (one Gaussian per lane, scalar accesses),  gsr_scene.mcmc.inject_noise (torch.randn + the kernel),  upstream's chain of torch
ops (randn included, as it draws its own),  FusedAdam.step on the six tensors of the model -- the variants alternate round by round, the median
round is printed with the bytes each has to move (68 B per Gaussian for the noise pass, 28 B per parameter for Adam) over that time.  1 M
Gaussians are 68 MB, less than the 256 MiB of Infinity Cache: the second size shows the pass out of HBM."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting_amd"))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import diff_gaussian_rasterization as pkg  # noqa: E402
from gsr_optim import FusedAdam  # noqa: E402
from gsr_scene import mcmc  # noqa: E402
from gsr_scene.densify import quaternion_to_rotation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--P", default="1000000,6000000")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gpu_mcmc_time.py: no HIP device")
dev = torch.device("cuda:0")
lib = pkg._lib.load()
NOISE_SCALE, K, X0 = 5e5 * 1.6e-4, 100.0, 0.995


def upstream(xyz, scaling, rotation, opacity):
    """inject_noise_to_position of gsplat's ops (the expression of 3dgs-mcmc's train.py), in place on xyz."""
    opac = torch.sigmoid(opacity).flatten()
    L = quaternion_to_rotation(rotation) * torch.exp(scaling)[:, None, :]
    cov = torch.bmm(L, L.transpose(1, 2))
    noise = torch.randn_like(xyz) * (1 / (1 + torch.exp(-K * ((1 - opac) - X0)))).unsqueeze(-1) * NOISE_SCALE
    xyz.add_(torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


for P in [int(v) for v in args.P.split(",")]:
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    params = {k: nn.Parameter(torch.randn(s, device=dev, generator=g)) for k, s in shapes.items()}
    with torch.no_grad():
        params["scaling"].mul_(0.5).sub_(4.0)
    opt = FusedAdam([{"params": [params[k]], "lr": 1e-6, "name": k} for k in params], lr=1e-6, eps=1e-15)
    for p in params.values():
        p.grad = torch.randn_like(p) * 1e-3
    xi = torch.randn(P, 3, device=dev, generator=g)

    def off(t):      # a copy that starts 4 bytes past a 16-byte boundary
        buf = torch.empty(t.numel() + 4, device=dev)
        v = buf[1:1 + t.numel()]
        v.copy_(t.detach().reshape(-1))
        return v
    al = [params[k].detach() for k in ("xyz", "scaling", "rotation", "opacity")] + [xi]
    mis = [off(t) for t in al]
    assert all(t.data_ptr() % 16 == 0 for t in al) and all(t.data_ptr() % 16 == 4 for t in mis)
    stream = pkg._stream_ptr(dev)

    def kernel(bufs):
        pkg._lib.check(lib.gsr_mcmc_inject_noise(P, *[pkg._ptr(t) for t in bufs], 0, NOISE_SCALE, K, X0, stream), "gsr_mcmc_inject_noise")
    n_param = sum(p.numel() for p in params.values())
    variants = [("kernel, 4 Gaussians per lane (16-byte accesses)", lambda: kernel(al), 68 * P),
                ("kernel, 1 Gaussian per lane (scalar accesses)", lambda: kernel(mis), 68 * P),
                ("gsr_scene.mcmc.inject_noise (randn + kernel)", lambda: mcmc.inject_noise(opt, NOISE_SCALE), 68 * P),
                ("upstream's torch expression (randn included)", lambda: upstream(*al[:4]), 68 * P),
                ("FusedAdam.step, six tensors", opt.step, 28 * n_param)]
    with torch.no_grad():
        for _, fn, _ in variants:      # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, fn, _ in variants:
                times[name].append(timed(fn, args.reps))
    print(f"P = {P}: {args.rounds} rounds of {args.reps} calls, median round (min .. max)", flush=True)
    for name, _, nbytes in variants:
        t = statistics.median(times[name])
        print(f"  {name:52s} {t * 1e6:9.1f} us ({min(times[name]) * 1e6:.1f} .. {max(times[name]) * 1e6:.1f})   {nbytes / 1e6:8.1f} MB   {nbytes / t / 1e12:6.2f} TB/s",
              flush=True)
    del params, opt, xi, al, mis
    torch.cuda.empty_cache()
