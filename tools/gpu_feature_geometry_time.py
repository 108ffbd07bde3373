"""Cost of the geometry / opacity gradients through the N-channel feature render (gsr_render_features_backward_geometry) at the bench frame (1 M Gaussians,
1920 x 1080, bench.py's scene, scales / rotations) for C = 3, 16 and 64, next to the route it replaces -- everything in one process, interleaved frame by
frame, 20 measured frames after 5 warm-up frames, each figure between two HIP events on the stream.  Per frame one tracking forward, then on its state:
  blend_backward        gsr_backward_blend with a three-channel upstream gradient: the kernel feature_geom_walk takes its frame from
  geometry_C            gsr_render_features_backward_geometry: the flag memset, one feature_geom_walk per channel group, the instance-record reduce
  geometry_C_orderK     the same with the launch order of the walks set to K (option bwd_heavy_first: 0 = tiles in index order, 2 = tiles by their
                        heaviest half, the library's default, 3 = every half tile on its own)
  per_gaussian_C        the per-Gaussian backward that follows on its records (gsr_backward_preprocess in its colors_precomp form)
  route_C               what one had to do before: ceil(C / 3) x (gsr_rasterize_forward with three channels as colors_precomp, then
                        gsr_rasterize_backward with their upstream gradient) -- preprocess, sort, binning, blend, blend backward, reduce, per-Gaussian
                        backward every time
Also checks, on the last frame, that the C = 3 records equal those of gsr_backward_blend on the same columns as colours within 1e-4 of the max per word.
Writes the JSON to the path given as the first argument (default: profiles/feature_geometry_time.json); a second argument is recorded as `label`.
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
CHANNELS = (3, 16, 64)
ORDERS = (0, 3)      # launch orders measured beside the default (2)


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
    triples = {c: [feats[c][:, k:k + 3].contiguous() if k + 3 <= c else torch.nn.functional.pad(feats[c][:, k:], (0, k + 3 - c)).contiguous()
                   for k in range(0, c, 3)] for c in CHANNELS}
    up3 = ups[3]
    color, invdepth, radii = torch.empty(3, H, W, device=device), torch.empty(1, H, W, device=device), torch.empty(P, dtype=torch.int32, device=device)
    route_grads, _ = pkg._gradients(P, device, True, False, None, False, True, True)
    keys = ["forward", "blend_backward"] + [f"{k}_{c}" for c in CHANNELS for k in ("geometry", "per_gaussian", "route")]
    keys += [f"geometry_{c}_order{k}" for c in CHANNELS for k in ORDERS]
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

            def records_of(c):
                _lib.check(lib.gsr_render_features_backward_geometry(*st, pkg._ptr(feats[c]), pkg._ptr(ups[c]), c, pkg._ptr(scratch), C.byref(rec), stream),
                           "gsr_render_features_backward_geometry")
                off = int(rec.value) - scratch.data_ptr()
                return scratch[off:off + P * 48].view(torch.float32).view(P, 12)

            timed(frame, "blend_backward", lambda: pkg._backward_blend(s, P, fwd, up3, None, device))
            order = CHANNELS if it % 2 == 0 else CHANNELS[::-1]
            for c in order:
                timed(frame, f"geometry_{c}", lambda: state.__setitem__("records", records_of(c)))
                for k in ORDERS:
                    _lib.set_option("bwd_heavy_first", k)
                    timed(frame, f"geometry_{c}_order{k}", lambda: records_of(c))
                _lib.set_option("bwd_heavy_first", 2)
                timed(frame, f"per_gaussian_{c}", lambda: pkg._geometry_from_records(geo_frame, state["records"], device))

                def route():
                    for cols in triples[c]:
                        inputs = (sc.means3D, None, cols, sc.opacities, sc.scales, sc.rotations, None)
                        fw = pkg._rasterize_forward(s, P, 0, inputs, color, invdepth, radii, device)
                        pkg._rasterize_backward(s, P, 0, inputs, radii, fw, up3, None, route_grads, device)
                timed(frame, f"route_{c}", route)
            if it >= WARMUP:
                for k, v in frame.items():
                    ms[k].append(v)
        # the two routes give the same records: C = 3 features as colours through gsr_backward_blend (bg = 0)
        fw = pkg._rasterize_forward(s, P, 0, (sc.means3D, None, triples[3][0], sc.opacities, sc.scales, sc.rotations, None), color, invdepth, radii, device)
        want = pkg._backward_blend(s, P, fw, up3, None, device).clone()
        st = (C.byref(s), P, int(fw.num_rendered), pkg._ptr(fw.geom), pkg._ptr(fw.binning), pkg._ptr(fw.img))
        got = records_of(3).clone()
        torch.cuda.synchronize()
        same = float(((got[:, :6] - want[:, :6]).abs().amax(dim=0) / want[:, :6].abs().amax(dim=0)).max())
    assert same <= 1e-4, same
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), scales/rotations",
              "label": sys.argv[2] if len(sys.argv) > 2 else "product build", "library": os.path.relpath(_lib.lib_path(), ROOT),
              "instances": instances, "frames": MEASURED, "device": torch.cuda.get_device_name(0),
              "records_vs_colour_blend_backward_rel_max": same,
              "ms_median": {k: round(v, 4) for k, v in med.items()},
              "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
              "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
              "geometry_3_over_blend_backward": round(med["geometry_3"] / med["blend_backward"], 4),
              "new_over_route": {str(c): round((med[f"geometry_{c}"] + med[f"per_gaussian_{c}"]) / med[f"route_{c}"], 4) for c in CHANNELS}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "feature_geometry_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
