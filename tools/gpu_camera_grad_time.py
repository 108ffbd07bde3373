"""Backward time at the bench frame (1 M Gaussians, 1920 x 1080, the fused [P,16,3] SH form with scales / rotations) with and without camera
gradients.  The per-Gaussian backward stage is read from the library's stage timers (gsr_profile_*), the whole backward from HIP events;
the two modes alternate, 30 measured frames each after 10 warm-up frames.  Writes the JSON to the path given as the first argument
(default: profiles/camera_grad_time.json).  Run it under its own `timeout`."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "gaussian-splatting_amd")]
import diff_gaussian_rasterization as pkg          # noqa: E402
from diff_gaussian_rasterization import _lib       # noqa: E402
import test_camera_grad_cpu as T                   # noqa: E402


def main():
    lib = _lib.load()
    sc = {k: v.cuda() for k, v in T.prep(T.scene(1_000_000, 31), "fused").items()}
    g = torch.Generator().manual_seed(7)
    wts = (torch.rand(3, 1080, 1920, generator=g).cuda(), torch.rand(1, 1080, 1920, generator=g).cuda())
    res = {True: [], False: []}
    stage = {True: [], False: []}
    n = 16
    ms = (C.c_float * n)()
    cnt = (C.c_int32 * n)()
    lib.gsr_profile_enable(1)
    for it in range(40):
        for cam_grad in (False, True):
            cam, leaves, loss, _ = T.render(pkg, sc, W=1920, H=1080, form="fused", cam_grad=cam_grad, device="cuda", wts=wts)
            torch.cuda.synchronize()
            lib.gsr_profile_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss.backward()
            e1.record()
            torch.cuda.synchronize()
            lib.gsr_profile_read(ms, cnt, n)
            if it >= 10:
                res[cam_grad].append(e0.elapsed_time(e1))
                stage[cam_grad].append([float(ms[k]) for k in range(n)])
    lib.gsr_profile_enable(0)
    med = lambda v: statistics.median(v)      # noqa: E731
    per_stage = {m: [med([s[k] for s in stage[m]]) for k in range(n)] for m in (False, True)}
    out = {"frame": "1 M Gaussians, 1920 x 1080, fused SH [P,16,3], scales/rotations, depth loss", "frames": len(res[True]),
           "backward_ms_median": {"without": med(res[False]), "with_camera_grad": med(res[True])},
           "stage_ms_median": {"without": per_stage[False], "with_camera_grad": per_stage[True]},
           "device": torch.cuda.get_device_name(0)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "camera_grad_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["backward_ms_median"]))
    print("stage ms without:", [round(x, 4) for x in per_stage[False]])
    print("stage ms with   :", [round(x, 4) for x in per_stage[True]])


if __name__ == "__main__":
    main()
