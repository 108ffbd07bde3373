"""Cost of the alpha image and of the per-pixel / learnable background at the bench frame (1 M Gaussians, 1920 x 1080, bench.py's scene, fused
[P,16,3] SH with scales / rotations): the blend stages of the forward (`render`) and of the backward (`render_bwd`, which includes the
background-gradient kernels, and `gather_bwd`) from the library's stage timers (gsr_profile_*), the whole forward and backward from HIP events.
Four modes alternate frame by frame, 30 measured frames each after 10 warm-up frames:
  plain      GaussianRasterizer(settings), loss on color                      (the entry points of the reference's contract)
  alpha      return_alpha=True, loss on color and alpha
  bg_grad    return_alpha=True, loss on color and alpha, bg[3] requires grad
  bg_image   return_alpha=True, loss on color and alpha, bg[3,H,W] requires grad
Writes the JSON to the path given as the first argument (default: profiles/composite_time.json).  Run it under its own `timeout`."""
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

MODES = ("plain", "alpha", "bg_grad", "bg_image")
STAGES = ("render", "render_bwd", "gather_bwd")


def main():
    W, H, P = 1920, 1080, 1_000_000
    cam = make_camera(W, H)
    sc = make_scene(P, cam, seed=0, s_med=0.012).to("cuda")
    g = torch.Generator().manual_seed(7)
    w_color, w_alpha = torch.rand(3, H, W, generator=g).cuda(), torch.rand(1, H, W, generator=g).cuda()
    bg3, bg_img = torch.tensor([0.1, 0.0, 0.3]).cuda(), torch.rand(3, H, W, generator=g).cuda()
    vm, pm, cp = cam.world_view_transform.cuda(), cam.full_proj_transform.cuda(), cam.camera_center.cuda()
    ev = {m: {"forward": [], "backward": []} for m in MODES}
    st = {m: {k: [] for k in STAGES} for m in MODES}
    _lib.profile_enable(True)
    for it in range(40):
        for mode in MODES:
            leaves = [t.detach().clone().requires_grad_(True) for t in (sc.means3D, sc.opacities, sc.shs, sc.scales, sc.rotations)]
            bg = bg3 if mode in ("plain", "alpha") else (bg3 if mode == "bg_grad" else bg_img).clone().requires_grad_(True)
            S = pkg.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, bg, 1.0, vm, pm, 3, cp, False, False, False)
            rast = pkg.GaussianRasterizer(S) if mode == "plain" else pkg.GaussianRasterizer(S, return_alpha=True)
            torch.cuda.synchronize()
            _lib.profile_reset()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            out = rast(means3D=leaves[0], means2D=None, opacities=leaves[1], shs=leaves[2], scales=leaves[3], rotations=leaves[4])
            loss = (out[0] * w_color).sum() if mode == "plain" else (out[0] * w_color).sum() + (out[3] * w_alpha).sum()
            e[1].record()
            loss.backward()
            e[2].record()
            torch.cuda.synchronize()
            stages = _lib.profile_read()
            if it >= 10:
                ev[mode]["forward"].append(e[0].elapsed_time(e[1]))
                ev[mode]["backward"].append(e[1].elapsed_time(e[2]))
                for k in STAGES:
                    st[mode][k].append(stages[k]["ms"])
    _lib.profile_enable(False)
    med = statistics.median
    out = {"frame": "1 M Gaussians, 1920 x 1080, bench.py's scene (seed 0, s_med 0.012), fused SH [P,16,3], scales/rotations",
           "frames_per_mode": len(ev["plain"]["forward"]), "device": torch.cuda.get_device_name(0),
           "stage_ms_median": {m: {k: round(med(v), 4) for k, v in st[m].items()} for m in MODES},
           "stage_ms_min": {m: {k: round(min(v), 4) for k, v in st[m].items()} for m in MODES},
           "event_ms_median (includes the loss kernels)": {m: {k: round(med(v), 4) for k, v in ev[m].items()} for m in MODES}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "composite_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
