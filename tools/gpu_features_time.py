"""Cost of the N-channel feature render (gsr_render_features, gsr_render_features_backward) at the bench frame (1 M Gaussians, 1920 x 1080, bench.py's
scene, scales / rotations) for C = 3, 16 and 64, next to the route it replaces -- everything in one process, interleaved frame by frame, 20 measured
frames after 5 warm-up frames, each figure between two HIP events on the stream (outputs and scratch allocated once).  Per frame one tracking forward,
then on its state:
  probe                 gsr_pixel_probe with all six outputs: the kernel feature_walk has the structure of
  features_C            gsr_render_features: ceil(C / G) launches of feature_walk
  features_backward_C   gsr_render_features_backward: the zeroing of [P,C] and ceil(C / 4) x (flag memset, feature_grad_walk, feature_grad_reduce)
  route_C               what one had to do before: ceil(C / 3) x (gsr_rasterize_forward with three channels as colors_precomp, then gsr_backward_blend with
                        their upstream gradient) -- preprocess, sort, binning, blend, blend backward and its reduce every time
Also checks, on the last frame, that channel 0..2 of the C = 3 render equal the colour image of the route's forward within 1e-5.
Writes the JSON to the path given as the first argument (default: profiles/features_time.json); a second argument is recorded as `label` (the library a
tuning build was made with: GSR_LIB selects it, GSR_OUT / GSR_EXTRA_FLAGS="-DGSR_FEAT_G=..." of build.py make it).  Run it under its own `timeout`."""
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
CHANNELS = (3, 16, 64)


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
    outs = {c: torch.empty(c, H, W, device=device) for c in CHANNELS}
    grads = {c: torch.empty(P, c, device=device) for c in CHANNELS}
    triples = {c: [feats[c][:, k:k + 3].contiguous() if k + 3 <= c else torch.nn.functional.pad(feats[c][:, k:], (0, k + 3 - c)).contiguous()
                   for k in range(0, c, 3)] for c in CHANNELS}
    up3 = ups[3]
    f = lambda: torch.zeros(H, W, dtype=torch.float32, device=device)                  # noqa: E731
    i = lambda: torch.zeros(H, W, dtype=torch.int32, device=device)                    # noqa: E731
    probe_out = pkg.PixelProbe(f(), f(), i(), i(), f(), i())
    probe_rec = _lib.PixelProbeOut(*[t.data_ptr() for t in probe_out], 0.5, 0)
    color, invdepth, radii = torch.empty(3, H, W, device=device), torch.empty(1, H, W, device=device), torch.empty(P, dtype=torch.int32, device=device)
    keys = ["forward", "probe"] + [f"{k}_{c}" for c in CHANNELS for k in ("features", "features_backward", "route")]
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
                state["s"], _, state["fwd"], _, state["keep"] = rast._tracking_forward(sc.means3D, sc.opacities, sc.scales, sc.rotations, None)
            timed(frame, "forward", tracking)
            s, fwd = state["s"], state["fwd"]
            instances = int(fwd.num_rendered)
            st = (C.byref(s), P, instances, pkg._ptr(fwd.geom), pkg._ptr(fwd.binning), pkg._ptr(fwd.img))
            if scratch is None or scratch.numel() < lib.gsr_feature_grad_scratch_bytes(P, instances, 64):
                scratch = torch.empty(lib.gsr_feature_grad_scratch_bytes(P, instances, 64) * 9 // 8, dtype=torch.uint8, device=device)
            timed(frame, "probe", lambda: _lib.check(lib.gsr_pixel_probe(*st, C.byref(probe_rec), stream), "gsr_pixel_probe"))
            order = CHANNELS if it % 2 == 0 else CHANNELS[::-1]
            for c in order:
                timed(frame, f"features_{c}", lambda: _lib.check(lib.gsr_render_features(*st, pkg._ptr(feats[c]), c, pkg._ptr(outs[c]), stream),
                                                                 "gsr_render_features"))
                timed(frame, f"features_backward_{c}", lambda: _lib.check(lib.gsr_render_features_backward(
                    *st, pkg._ptr(ups[c]), c, pkg._ptr(scratch), pkg._ptr(grads[c]), stream), "gsr_render_features_backward"))

                def route():
                    for cols in triples[c]:
                        inputs = (sc.means3D, None, cols, sc.opacities, sc.scales, sc.rotations, None)
                        fw = pkg._rasterize_forward(s, P, 0, inputs, color, invdepth, radii, device)
                        pkg._backward_blend(s, P, fw, up3, None, device)
                timed(frame, f"route_{c}", route)
            if it >= WARMUP:
                for k, v in frame.items():
                    ms[k].append(v)
        # the two routes render the same image (the last route forward held channels 63.. of C = 64; redo the first triple of C = 3)
        pkg._rasterize_forward(s, P, 0, (sc.means3D, None, triples[3][0], sc.opacities, sc.scales, sc.rotations, None), color, invdepth, radii, device)
        _lib.check(lib.gsr_render_features(*st, pkg._ptr(feats[3]), 3, pkg._ptr(outs[3]), stream), "gsr_render_features")
        torch.cuda.synchronize()
        same = float((outs[3] - color).abs().max())
    assert same <= 1e-5, same
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), scales/rotations",
              "label": sys.argv[2] if len(sys.argv) > 2 else "product build", "library": os.path.relpath(_lib.lib_path(), ROOT),
              "instances": instances, "frames": MEASURED, "device": torch.cuda.get_device_name(0),
              "features_vs_colour_abs_max": same,
              "ms_median": {k: round(v, 4) for k, v in med.items()},
              "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
              "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
              "new_over_route": {str(c): round((med[f"features_{c}"] + med[f"features_backward_{c}"]) / med[f"route_{c}"], 4) for c in CHANNELS}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "features_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
