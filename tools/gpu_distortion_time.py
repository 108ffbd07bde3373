"""Cost of the distortion loss on a rendered frame (gsr_distortion / gsr_distortion_backward) at the bench frame (1 M Gaussians, 1920 x 1080, bench.py's
scene, scales / rotations), next to the kernels it takes its frames from -- everything in one process, interleaved frame by frame, 20 measured frames
after 5 warm-up frames, each figure between two HIP events on the stream.  Per frame one tracking forward, then on its state:
  probe                 gsr_pixel_probe with all six outputs: the kernel distortion_map takes its frame from
  distortion_zM         gsr_distortion with the two saved planes, depth_mode M (0: z, 1: 1/z)
  distortion_z0_nosave  the same without the saved planes (a call that no backward follows)
  backward_zM           gsr_distortion_backward: the plan / flag launch, distortion_walk, the instance-record reduce
  geometry_C            gsr_render_features_backward_geometry with C = 3 and 4 channels: the walk distortion_walk takes its frame from, and the same reduce
  per_gaussian          the per-Gaussian backward that follows on the records (gsr_backward_preprocess in its colors_precomp form); it is the same call
                        after either walk
Also checks, on the last frame, that two calls give the same bits.
Writes the JSON to the path given as the first argument (default: profiles/distortion_time.json); a second argument is recorded as `label`.
Run it under its own `timeout`."""
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

WARMUP, MEASURED = 5, 20
CHANNELS = (3, 4)


def main():
    W, H, P = 1920, 1080, 1_000_000
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to("cuda")
    vm, pm, cp = cam.world_view_transform.cuda(), cam.full_proj_transform.cuda(), cam.camera_center.cuda()
    S = pkg.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3).cuda(), 1.0, vm, pm, 3, cp, False, False, False)
    rast = pkg.GaussianRasterizer(S)
    lib = _lib.load()
    device = sc.means3D.device
    g = torch.Generator().manual_seed(7)
    feats = {c: (torch.rand(P, c, generator=g) * 2.0 - 1.0).cuda() for c in CHANNELS}
    ups = {c: (torch.rand(c, H, W, generator=g) - 0.5).cuda() for c in CHANNELS}
    up = (torch.rand(H, W, generator=g) - 0.3).cuda()
    D = torch.zeros(H, W, device=device)
    saved = {m: torch.zeros(2, H, W, device=device) for m in (0, 1)}
    probe_out = [torch.zeros(H, W, dtype=t, device=device) for t in (torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.int32)]
    keys = ["forward", "probe", "distortion_z0", "distortion_z1", "distortion_z0_nosave", "backward_z0", "backward_z1", "per_gaussian"]
    keys += [f"geometry_{c}" for c in CHANNELS]
    ms = {k: [] for k in keys}
    event = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    stream = pkg._stream_ptr(device)
    scratch = None
    instances = 0

    def timed(frame, key, fn):
        e0, e1 = event(), event()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        frame[key] = e0.elapsed_time(e1)

    with torch.no_grad():
        for it in range(WARMUP + MEASURED):
            frame = {}
            torch.cuda.synchronize()
            state = {}

            def tracking():
                state["s"], _, state["fwd"], state["radii"], state["keep"] = rast._tracking_forward(sc.means3D, sc.opacities, sc.scales, sc.rotations, None)
            timed(frame, "forward", tracking)
            s, fwd = state["s"], state["fwd"]
            instances = int(fwd.num_rendered)
            st = (C.byref(s), P, instances, pkg._ptr(fwd.geom), pkg._ptr(fwd.binning), pkg._ptr(fwd.img))
            need = int(lib.gsr_backward_scratch_bytes(P, instances))
            if scratch is None or scratch.numel() < need:
                scratch = torch.empty(need * 9 // 8, dtype=torch.uint8, device=device)
            geo_frame = pkg._FeatureFrame(S, None, fwd, state["radii"], sc.means3D, sc.opacities, sc.scales, sc.rotations, None)
            rec = C.c_void_p(0)

            def records():
                off = int(rec.value) - scratch.data_ptr()
                return scratch[off:off + P * 48].view(torch.float32).view(P, 12)

            def forward(mode, save=True):
                out = _lib.DistortionOut(D.data_ptr(), saved[mode].data_ptr() if save else None, mode, 0)
                _lib.check(lib.gsr_distortion(*st, C.byref(out), stream), "gsr_distortion")

            def backward(mode):
                _lib.check(lib.gsr_distortion_backward(*st, pkg._ptr(up), pkg._ptr(saved[mode]), mode, pkg._ptr(scratch), C.byref(rec), stream),
                           "gsr_distortion_backward")

            def geometry(c):
                _lib.check(lib.gsr_render_features_backward_geometry(*st, pkg._ptr(feats[c]), pkg._ptr(ups[c]), c, pkg._ptr(scratch), C.byref(rec), stream),
                           "gsr_render_features_backward_geometry")

            def probe():
                out = _lib.PixelProbeOut(*[t.data_ptr() for t in probe_out], 0.5, 0)
                _lib.check(lib.gsr_pixel_probe(*st, C.byref(out), stream), "gsr_pixel_probe")

            timed(frame, "probe", probe)
            modes = (0, 1) if it % 2 == 0 else (1, 0)
            for m in modes:
                timed(frame, f"distortion_z{m}", lambda: forward(m))
            timed(frame, "distortion_z0_nosave", lambda: forward(0, False))
            for c in (CHANNELS if it % 2 == 0 else CHANNELS[::-1]):
                timed(frame, f"geometry_{c}", lambda: geometry(c))
            for m in modes:
                timed(frame, f"backward_z{m}", lambda: backward(m))
            timed(frame, "per_gaussian", lambda: pkg._geometry_from_records(geo_frame, records(), device))
            if it >= WARMUP:
                for k, v in frame.items():
                    ms[k].append(v)
        # two calls give the same bits
        forward(1)
        backward(1)
        a = (D.clone(), saved[1].clone(), records().clone())
        forward(1)
        backward(1)
        torch.cuda.synchronize()
        same = torch.equal(a[0], D) and torch.equal(a[1], saved[1]) and torch.equal(a[2], records())
        finite = bool(torch.isfinite(a[2]).all()) and float(a[2].abs().max()) > 0.0 and float(a[0].max()) > 0.0
    assert same and finite, (same, finite)
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), scales/rotations",
              "label": sys.argv[2] if len(sys.argv) > 2 else "product build", "library": os.path.relpath(_lib.lib_path(), ROOT),
              "instances": instances, "frames": MEASURED, "device": torch.cuda.get_device_name(0),
              "two_calls_equal_bits": same,
              "ms_median": {k: round(v, 4) for k, v in med.items()},
              "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
              "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
              "distortion_over_probe": round(med["distortion_z0"] / med["probe"], 4),
              "backward_over_geometry_3": round(med["backward_z0"] / med["geometry_3"], 4)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "distortion_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
