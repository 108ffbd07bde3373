"""Cost of the absolute screen-space gradients (gsr_backward_blend_abs, gsr_absgrad_from_records) at the bench frame (1 M Gaussians, 1920 x 1080,
bench.py's scene, fused [P,16,3] SH with scales / rotations) -- everything in one process, interleaved frame by frame, 30 measured frames after 10
warm-up frames.  Per frame one training forward, then on its state, 5 back-to-back C calls each (scratch allocated once), the order of the two blend
backwards alternating from frame to frame:
  blend_off            gsr_backward_blend: HIP events around the calls, divided by 5 -- plan kernel, walk, the unit-based reduce chain
  blend_on             gsr_backward_blend_abs: the same with the walk's ABS instantiation and absgrad_reduce behind the reduce chain
  walk_off, walk_on    the walk kernel's share of the two (library stage timer render_bwd; includes the plan kernel)
  reduce_off, reduce_on  the reduce's share (library stage timer gather_bwd); reduce_on - reduce_off is absgrad_reduce
  from_records         gsr_absgrad_from_records (HIP events)
  absgrad_reduce_plus_from_records   (reduce_on - reduce_off) + from_records per frame
Also checks, on the last frame, that words 0..9 of the two record arrays are the same bits.
Writes the JSON to the path given as the first argument (default: profiles/absgrad_time.json).  Run it under its own `timeout`."""
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

REPEAT = 5


def main():
    W, H, P = 1920, 1080, 1_000_000
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to("cuda")
    g = torch.Generator().manual_seed(7)
    w_color = (torch.rand(3, H, W, generator=g) - 0.3).cuda()
    vm, pm, cp = cam.world_view_transform.cuda(), cam.full_proj_transform.cuda(), cam.camera_center.cuda()
    S = pkg.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3).cuda(), 1.0, vm, pm, 3, cp, False, False, False)
    rast = pkg.GaussianRasterizer(S)
    lib = _lib.load()
    scratch = {}
    abs_out = torch.empty(P, 3, device="cuda")
    keys = ("blend_off", "blend_on", "walk_off", "walk_on", "reduce_off", "reduce_on", "from_records", "absgrad_reduce_plus_from_records")
    ms = {k: [] for k in keys}
    instances, same_bits = 0, None
    _lib.profile_enable(True)
    event = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    for it in range(40):
        frame = {}
        leaves = [t.detach().clone().requires_grad_(True) for t in (sc.means3D, sc.opacities, sc.shs, sc.scales, sc.rotations)]
        color = rast(means3D=leaves[0], means2D=None, opacities=leaves[1], shs=leaves[2], scales=leaves[3], rotations=leaves[4])[0]
        ctx = pkg._rasterizer_nodes(color)[0]
        saved = ctx.saved_tensors
        instances = int(ctx.num_rendered)
        need = int(lib.gsr_backward_scratch_bytes(P, instances))
        for key in ("off", "on"):      # one scratch per variant: the records of both stay readable
            if key not in scratch or scratch[key].numel() < need:
                scratch[key] = torch.empty(int(need * 1.1), dtype=torch.uint8, device="cuda")
        keep: list = []
        s = pkg._make_settings(S, keep, None, bg_image=True)
        stream = pkg._stream_ptr(color.device)
        rec_ptr = {"off": C.c_void_p(0), "on": C.c_void_p(0)}
        state = (C.byref(s), P, instances, pkg._ptr(saved[8]), pkg._ptr(saved[9]), pkg._ptr(saved[10]), pkg._ptr(w_color), None)

        def blend(key):
            if key == "off":
                return lib.gsr_backward_blend(*state, pkg._ptr(scratch[key]), C.byref(rec_ptr[key]), stream)
            return lib.gsr_backward_blend_abs(*state, pkg._ptr(scratch[key]), C.byref(rec_ptr[key]), None, stream)

        for key in (("off", "on") if it % 2 == 0 else ("on", "off")):
            torch.cuda.synchronize()
            _lib.profile_reset()
            e0, e1 = event(), event()
            e0.record()
            for _ in range(REPEAT):
                _lib.check(blend(key), "blend backward " + key)
            e1.record()
            torch.cuda.synchronize()
            stages = _lib.profile_read()
            frame["blend_" + key] = e0.elapsed_time(e1) / REPEAT
            frame["walk_" + key] = stages["render_bwd"]["ms"] / REPEAT
            frame["reduce_" + key] = stages["gather_bwd"]["ms"] / REPEAT
        torch.cuda.synchronize()
        e0, e1 = event(), event()
        e0.record()
        for _ in range(REPEAT):
            _lib.check(lib.gsr_absgrad_from_records(C.byref(s), P, rec_ptr["on"], pkg._ptr(abs_out), stream), "gsr_absgrad_from_records")
        e1.record()
        torch.cuda.synchronize()
        frame["from_records"] = e0.elapsed_time(e1) / REPEAT
        frame["absgrad_reduce_plus_from_records"] = frame["reduce_on"] - frame["reduce_off"] + frame["from_records"]
        if it == 39:
            view = lambda key: scratch[key][int(rec_ptr[key].value) - scratch[key].data_ptr():][:P * 48].view(torch.float32).view(P, 12)      # noqa: E731
            same_bits = bool(torch.equal(view("on")[:, :10], view("off")[:, :10])) and float(view("off")[:, 10:].abs().max()) == 0.0
        if it >= 10:
            for k, v in frame.items():
                ms[k].append(v)
    _lib.profile_enable(False)
    result = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), fused SH [P,16,3], scales/rotations, colour loss only",
              "instances": instances, "frames": len(ms["blend_off"]), "device": torch.cuda.get_device_name(0),
              "rows_with_absgrad": int((abs_out[:, 0] > 0).sum()), "words_0_to_9_same_bits": same_bits,
              "ms_median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
              "ms_min": {k: round(min(v), 4) for k, v in ms.items()}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "absgrad_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
