"""Cost of the per-Gaussian blend-weight statistics (gsr_contribution_stats) at the bench frame (1 M Gaussians, 1920 x 1080, bench.py's scene, fused
[P,16,3] SH with scales / rotations), next to the kernels it sits beside and the route it replaces -- everything in one process, interleaved frame
by frame, 30 measured frames after 10 warm-up frames:
  stats / stats_weighted   gsr_contribution_stats on the training forward's state without / with pixel_weight: HIP events around 5 back-to-back C calls
                           (scratch and outputs allocated once), divided by 5 -- the flag clear, the walk and the reduce
  render                   the tracking forward blend of the training frame            (library stage timer)
  render_bwd, gather_bwd   the blend backward and its per-Gaussian reduce              (library stage timers)
  route_*                  what the statistics replace: a second forward with colors_precomp, only the colours requiring grad, and the backward of
                           sum E C_0, whose dL/dcolors[:,0] is weight_sum: HIP events around the forward and the backward, and their blend stages
Writes the JSON to the path given as the first argument (default: profiles/contrib_time.json).  Run it under its own `timeout`."""
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
    w_color, E = torch.rand(3, H, W, generator=g).cuda(), torch.rand(H, W, generator=g).cuda()
    colors = torch.rand(P, 3, generator=g).cuda()
    vm, pm, cp = cam.world_view_transform.cuda(), cam.full_proj_transform.cuda(), cam.camera_center.cuda()
    S = pkg.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3).cuda(), 1.0, vm, pm, 3, cp, False, False, False)
    rast = pkg.GaussianRasterizer(S)
    lib = _lib.load()
    out = pkg.ContributionStats(torch.empty(P, device="cuda"), torch.empty(P, device="cuda"), torch.empty(P, dtype=torch.int32, device="cuda"))
    rec = _lib.ContribOut(out.weight_sum.data_ptr(), out.weight_max.data_ptr(), out.pixel_count.data_ptr(), 0, 0)
    scratch = None
    ms = {k: [] for k in ("stats", "stats_weighted", "render", "render_bwd", "gather_bwd", "route_forward", "route_backward", "route_render",
                          "route_render_bwd", "route_gather_bwd")}
    instances = 0
    _lib.profile_enable(True)
    event = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    for it in range(40):
        frame = {}
        # ---- the training frame: forward, the statistics on its state, backward ----
        leaves = [t.detach().clone().requires_grad_(True) for t in (sc.means3D, sc.opacities, sc.shs, sc.scales, sc.rotations)]
        torch.cuda.synchronize()
        _lib.profile_reset()
        color = rast(means3D=leaves[0], means2D=None, opacities=leaves[1], shs=leaves[2], scales=leaves[3], rotations=leaves[4])[0]
        ctx = pkg._rasterizer_nodes(color)[0]
        saved = ctx.saved_tensors
        instances = int(ctx.num_rendered)
        if scratch is None or scratch.numel() < lib.gsr_contribution_scratch_bytes(P, instances):
            scratch = torch.empty(int(lib.gsr_contribution_scratch_bytes(P, instances) * 1.1), dtype=torch.uint8, device="cuda")
        keep: list = []
        s = pkg._make_settings(S, keep, None, bg_image=True)
        stream = pkg._stream_ptr(color.device)
        for key, weight in (("stats", None), ("stats_weighted", E)):
            torch.cuda.synchronize()
            e0, e1 = event(), event()
            e0.record()
            for _ in range(REPEAT):
                _lib.check(lib.gsr_contribution_stats(C.byref(s), P, instances, pkg._ptr(saved[8]), pkg._ptr(saved[9]), pkg._ptr(saved[10]),
                                                      pkg._ptr(weight), pkg._ptr(scratch), C.byref(rec), stream), "gsr_contribution_stats")
            e1.record()
            torch.cuda.synchronize()
            frame[key] = e0.elapsed_time(e1) / REPEAT
        (color * w_color).sum().backward()
        torch.cuda.synchronize()
        stages = _lib.profile_read()
        for k in ("render", "render_bwd", "gather_bwd"):
            frame[k] = stages[k]["ms"]
        # ---- the replaced route: a second forward with colors_precomp and the backward of sum E C_0 ----
        col = colors.clone().requires_grad_(True)
        torch.cuda.synchronize()
        _lib.profile_reset()
        e = [event() for _ in range(3)]
        e[0].record()
        c2 = rast(means3D=sc.means3D, means2D=None, opacities=sc.opacities, colors_precomp=col, scales=sc.scales, rotations=sc.rotations)[0]
        loss = (c2[0] * E).sum()
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        stages = _lib.profile_read()
        frame.update(route_forward=e[0].elapsed_time(e[1]), route_backward=e[1].elapsed_time(e[2]), route_render=stages["render"]["ms"],
                     route_render_bwd=stages["render_bwd"]["ms"], route_gather_bwd=stages["gather_bwd"]["ms"])
        if it >= 10:
            for k, v in frame.items():
                ms[k].append(v)
    _lib.profile_enable(False)
    result = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), fused SH [P,16,3], scales/rotations",
              "instances": instances, "frames": len(ms["stats"]), "device": torch.cuda.get_device_name(0),
              "contributing": int((out.pixel_count > 0).sum()),
              "ms_median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
              "ms_min": {k: round(min(v), 4) for k, v in ms.items()}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contrib_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
