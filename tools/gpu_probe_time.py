"""Cost of the per-pixel probe (gsr_pixel_probe) at the bench frame (1 M Gaussians, 1920 x 1080, bench.py's scene, scales / rotations), next to the
tracking forward it reads the state of -- everything in one process, interleaved launch by launch, 30 measured launches after 10 warm-up launches, each
between two HIP events on the stream (outputs allocated once):
  probe            gsr_pixel_probe with all six outputs, threshold 0.5: one launch of probe_walk
  probe_ids_only   the same with median_id / top_id / count only (the picking use)
  forward          the tracking forward GaussianRasterizer.probe runs first when there is no render to hand (gsr_rasterize_forward with zero colours,
                   no_backward == 0): preprocess, sort, binning and the blend
  render           the forward's blend kernel alone (library stage timer): the kernel probe_walk has the structure of
Writes the JSON to the path given as the first argument (default: profiles/probe_time.json).  Run it under its own `timeout`."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gaussian-splatting_amd")]
import diff_gaussian_rasterization as pkg          # noqa: E402
from diff_gaussian_rasterization import _lib       # noqa: E402
from gsr_synth import make_camera, make_scene       # noqa: E402

WARMUP, MEASURED = 10, 30


def main():
    W, H, P = 1920, 1080, 1_000_000
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to("cuda")
    vm, pm, cp = cam.world_view_transform.cuda(), cam.full_proj_transform.cuda(), cam.camera_center.cuda()
    S = pkg.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3).cuda(), 1.0, vm, pm, 3, cp, False, False, False)
    rast = pkg.GaussianRasterizer(S)
    lib = _lib.load()
    device = sc.means3D.device
    f = lambda: torch.zeros(H, W, dtype=torch.float32, device=device)                  # noqa: E731
    i = lambda: torch.zeros(H, W, dtype=torch.int32, device=device)                    # noqa: E731
    out = pkg.PixelProbe(f(), f(), i(), i(), f(), i())
    rec_all = _lib.PixelProbeOut(*[t.data_ptr() for t in out], 0.5, 0)
    rec_ids = _lib.PixelProbeOut(None, None, out.median_id.data_ptr(), out.top_id.data_ptr(), None, out.count.data_ptr(), 0.5, 0)
    ms = {k: [] for k in ("probe", "probe_ids_only", "forward", "render")}
    event = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    stream = pkg._stream_ptr(device)
    instances = 0
    _lib.profile_enable(True)
    with torch.no_grad():
        for it in range(WARMUP + MEASURED):
            frame = {}
            torch.cuda.synchronize()
            _lib.profile_reset()
            e0, e1 = event(), event()
            e0.record()
            s, _, fwd, radii, _keep = rast._tracking_forward(sc.means3D, sc.opacities, sc.scales, sc.rotations, None)
            e1.record()
            torch.cuda.synchronize()
            frame["forward"] = e0.elapsed_time(e1)
            frame["render"] = _lib.profile_read()["render"]["ms"]
            instances = int(fwd.num_rendered)
            for key, rec in (("probe", rec_all), ("probe_ids_only", rec_ids)):
                e0, e1 = event(), event()
                e0.record()
                _lib.check(lib.gsr_pixel_probe(C.byref(s), P, instances, pkg._ptr(fwd.geom), pkg._ptr(fwd.binning), pkg._ptr(fwd.img), C.byref(rec),
                                               stream), "gsr_pixel_probe")
                e1.record()
                torch.cuda.synchronize()
                frame[key] = e0.elapsed_time(e1)
            if it >= WARMUP:
                for k, v in frame.items():
                    ms[k].append(v)
    _lib.profile_enable(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), scales/rotations, zero colours",
              "instances": instances, "launches": MEASURED, "device": torch.cuda.get_device_name(0),
              "contributions": int(out.count.sum()), "pixels_with_median": int((out.median_id >= 0).sum()),
              "ms_median": {k: round(v, 4) for k, v in med.items()},
              "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
              "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
              "probe_over_forward": round(med["probe"] / med["forward"], 4), "probe_over_render": round(med["probe"] / med["render"], 4)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probe_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
