#!/usr/bin/env python
"""BASELINE.json configs[2] stand-in: the reference's FULL training loop (forward + loss + backward + density control +
optimizer), 30 000 iterations on its own schedule, on the drop-in packages of this repo.

    python tools/train_run.py [--iters 30000] [--P0 100000] [--P-target 1000000] [--cams 32] [--dense-adam]

What is mirrored from the reference (train.py:73-190, arguments/__init__.py:72-100, scene/gaussian_model.py):
  * a new camera every iteration, drawn without replacement from the training set (train.py:96-102) -- here `--cams`
    synthetic views of a synthetic target scene (no dataset ships with this repo; SURVEY.md 8(d) generator);
  * render through `GaussianRasterizer` in the separate-SH call form with `SparseGaussianAdam` (what the reference selects
    when the accelerated rasterizer is importable, train.py:37-41,180-183) or `--dense-adam` for the default optimizer;
  * loss 0.8 L1 + 0.2 (1 - SSIM) as one fused kernel pair (fused_ssim.fused_train_loss; train.py:119-126);
  * SH degree + 1 every 1000 iterations (train.py:92-94), exponential position learning-rate schedule
    (utils/general_utils.py:get_expon_lr_func; position_lr 1.6e-4 -> 1.6e-6 over 30 000 steps, scaled by the scene extent);
  * density statistics every iteration and clone / split / prune every 100 iterations from 500 to 15 000 with gradient
    threshold 0.0002, opacity floor 0.005, screen-size pruning after iteration 3000, opacity reset every 3000 iterations
    (train.py:160-174, arguments/__init__.py:91-95).
Beyond the reference, off by default: `--bilateral_grid`, gsplat's per-image appearance compensation (fused_bilagrid);
`--normal_consistency`, the depth-normal consistency regulariser of 2DGS (gsr_normals); `--mip_filter`, the 3D smoothing
filter and the antialiased rasterizer of Mip-Splatting (gsr_scene.mip).
Reported: iterations/s (whole run and per 5000-iteration window), the Gaussian count over time, peak device memory, the
largest R-sized scratch buffers.  One JSON line on stdout (also written to gpurun_out/train_run.json)."""
from __future__ import annotations

import argparse
import json
import math
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gaussian-splatting_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:get_expon_lr_func"""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0), 1))
    else:
        delay_rate = 1.0
    t = min(max(step / max_steps, 0), 1)
    return delay_rate * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30000)
    ap.add_argument("--P0", type=int, default=100_000)
    ap.add_argument("--P-target", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cams", type=int, default=32)
    ap.add_argument("--dense-adam", action="store_true")
    ap.add_argument("--extent", type=float, default=4.0, help="scene extent (cameras_extent of the reference)")
    ap.add_argument("--max-P", type=int, default=4_000_000, help="densification stops growing the set beyond this (memory guard)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--grad-threshold", type=float, default=0.0002, help="densify_grad_threshold (arguments/__init__.py:95)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--bilateral_grid", action="store_true",
                    help="per-camera appearance compensation (fused_bilagrid.BilateralGrid, 16 x 16 x 8): the rendered image is sliced through its "
                         "camera's grid before the loss, 10 tv_loss is added, the grids have their own gsr_optim.FusedAdam (lr 2e-3)")
    ap.add_argument("--normal_consistency", type=float, default=0.0, metavar="LAMBDA",
                    help="add LAMBDA * gsr_normals.normal_consistency_loss (2DGS uses 0.05): per-Gaussian normals and the view-space z rendered as "
                         "four feature channels with geometry gradients, depth = D / alpha, weight = the detached alpha; 0 (default) = off")
    ap.add_argument("--mip_filter", action="store_true",
                    help="Mip-Splatting: the 3D smoothing filter (gsr_scene.mip.compute_3d_filter over the training cameras at the start, after every "
                         "density-control step and every 100 iterations afterwards), the activations through gsr_scene.mip.filtered_activations, "
                         "antialiasing=True in the rasterizer's settings")
    ap.add_argument("--fuse-sh-step", action="store_true",
                    help="opt-in: the optimizer step of f_dc / f_rest is applied by the per-Gaussian backward kernel "
                         "(diff_gaussian_rasterization.fuse_sh_adam_into_backward); switched off on the iterations that densify, "
                         "where the reference's loop steps nothing")
    ap.add_argument("--save-state", default="", help="torch.save the model, the optimizer state and the loop's counters here at the end")
    ap.add_argument("--load-state", default="", help="continue from a --save-state file: the loop starts at the saved iteration + 1")
    ap.add_argument("--timeline", type=int, default=0,
                    help="after the loop: this many MORE iterations of the same loop (no density control) measured three ways -- wall clock per "
                         "iteration without any synchronisation, the library's per-stage HIP events, and torch events around the phases of "
                         "the iteration (activations + forward, loss, backward, statistics, optimizer) -- plus the host time each phase "
                         "takes to enqueue (VERDICT r05 weak #5: where does a 3 ms iteration of a grown scene go?)")
    a = ap.parse_args()

    from gsr_synth import look_at_camera, make_camera, make_scene
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, SparseGaussianAdam
    import diff_gaussian_rasterization as dgr
    from fused_ssim import fused_train_loss
    from gsr_normals import gaussian_normals, normal_consistency_loss
    from gsr_optim import FusedAdam
    from gsr_scene.densify import DensifyStats, densify_and_prune, reset_opacity

    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    random.seed(a.seed)
    torch.manual_seed(a.seed)
    W, H = a.width, a.height
    cam0 = make_camera(W, H)
    target = make_scene(a.P_target, cam0, seed=a.seed, s_med=0.012).to(dev)
    # training views: eyes on a small circle around the generating camera, all looking at the middle of the cloud
    cams = [cam0]
    for k in range(1, a.cams):
        ang = 2 * math.pi * k / max(1, a.cams - 1)
        r = 0.25 + 0.35 * ((k * 7) % 5) / 4.0
        cams.append(look_at_camera(W, H, (r * math.cos(ang), r * math.sin(ang), -0.2 * ((k % 3) - 1)), (0.0, 0.0, 7.0)))
    bg = torch.zeros(3, device=dev)

    # the reference's Camera objects keep their matrices on the device (scene/cameras.py): upload once, not per iteration
    _dev_cams = {}

    def settings(cam, deg, aa=False):
        c = _dev_cams.get(id(cam))
        if c is None:
            c = _dev_cams[id(cam)] = cam.to(dev)
        return GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, bg, 1.0, c.world_view_transform, c.full_proj_transform,
                                             deg, c.camera_center, False, False, aa)

    mip_cams = filter_3D = None
    if a.mip_filter:      # the camera records once (R = the view matrix's 3 x 3 block, T = its last row; centred principal point)
        from gsr_scene import mip
        mip_cams = torch.stack([torch.cat([cam.world_view_transform[:3, :3].reshape(-1), cam.world_view_transform[3, :3],
                                           torch.tensor([W / (2.0 * cam.tanfovx), H / (2.0 * cam.tanfovy), float(W), float(H)])])
                                for cam in cams]).to(dev)

    with torch.no_grad():
        gts = []
        for cam in cams:
            img = GaussianRasterizer(settings(cam, 3))(means3D=target.means3D, means2D=None, dc=target.shs[:, :1].contiguous(),
                                                       shs=target.shs[:, 1:].contiguous(), opacities=target.opacities,
                                                       scales=target.scales, rotations=target.rotations)[0]
            gts.append(img.clone())
    # initial model: a sparse, blurry subset of the target (the role of the SfM point cloud, scene/gaussian_model.py:147-173)
    step = max(1, a.P_target // a.P0)
    sub = slice(0, None, step)

    def par(t):
        return nn.Parameter(t.detach().clone().contiguous().requires_grad_(True))
    P0 = target.means3D[sub].shape[0]
    params = {"xyz": par(target.means3D[sub]), "f_dc": par(target.shs[sub, :1]), "f_rest": par(target.shs[sub, 1:] * 0.0),
              "opacity": par(torch.full((P0, 1), math.log(0.1 / 0.9), device=dev)),
              "scaling": par(torch.log(target.scales[sub] * 2.0)), "rotation": par(target.rotations[sub])}
    del target
    torch.cuda.empty_cache()
    ext = a.extent
    lrs = {"xyz": 0.00016 * ext, "f_dc": 0.0025, "f_rest": 0.0025 / 20.0, "opacity": 0.025, "scaling": 0.005, "rotation": 0.001}
    groups = [{"params": [params[k]], "lr": lrs[k], "name": k} for k in params]
    opt = FusedAdam(groups, lr=0.0, eps=1e-15) if a.dense_adam else SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    stats = DensifyStats.zeros(P0, dev)
    fusion = [None, None]          # handle, the f_rest tensor it was registered for

    def set_fusion(on):
        from diff_gaussian_rasterization import fuse_sh_adam_into_backward
        if fusion[0] is not None and (not on or fusion[1] is not params["f_rest"]):
            fusion[0].remove()
            fusion[0] = None
        if on and fusion[0] is None:
            fusion[0], fusion[1] = fuse_sh_adam_into_backward(opt, params["f_dc"], params["f_rest"]), params["f_rest"]
    deg = 0
    stack = []
    sizes, window_t, losses = [], [], []
    it0 = 1
    if a.load_state:
        st_ = torch.load(a.load_state, map_location=dev)
        params = {k: nn.Parameter(v.to(dev).contiguous().requires_grad_(True)) for k, v in st_["params"].items()}
        groups = [{"params": [params[k]], "lr": lrs[k], "name": k} for k in params]
        opt = FusedAdam(groups, lr=0.0, eps=1e-15) if a.dense_adam else SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
        for k, q in params.items():
            if k in st_["moments"]:
                m_, v_ = st_["moments"][k]
                opt.state[q] = {"step": (0 if a.dense_adam else torch.tensor(0.0)), "exp_avg": m_.to(dev).contiguous(), "exp_avg_sq": v_.to(dev).contiguous()}
                if a.dense_adam:
                    opt.state[q]["step"] = int(st_["it"])
        stats = DensifyStats.zeros(params["xyz"].shape[0], dev)
        deg, it0 = int(st_["deg"]), int(st_["it"]) + 1
        del st_
    bil = bil_opt = None
    if a.bilateral_grid:
        from fused_bilagrid import BilateralGrid
        bil = BilateralGrid(len(cams)).to(dev)
        bil_opt = FusedAdam([bil.grids], lr=2e-3, eps=1e-15)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t_start = t_win = time.perf_counter()
    for it in range(it0, a.iters + 1):
        lr_xyz = expon_lr(it, 0.00016 * ext, 0.0000016 * ext, 0, 0.01, 30000)
        for g in opt.param_groups:
            if g["name"] == "xyz":
                g["lr"] = lr_xyz
        if it % 1000 == 0 and deg < 3:
            deg += 1
        if not stack:
            stack = list(range(len(cams)))
        ci = stack.pop(random.randint(0, len(stack) - 1))
        P = params["xyz"].shape[0]
        if a.fuse_sh_step:      # (the tensors change at every densification; no fused step where the loop below replaces them)
            set_fusion(not (500 < it < 15000 and it % 100 == 0) and it < a.iters)
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        S = settings(cams[ci], deg, a.mip_filter)
        rot_act = torch.nn.functional.normalize(params["rotation"])
        if a.mip_filter:
            if filter_3D is None or (it >= 15000 and it % 100 == 0):      # start, after density control, every 100 once that has ended
                filter_3D = mip.compute_3d_filter(params["xyz"], mip_cams)
            scales_act, opacity_act = mip.filtered_activations(params["scaling"], params["opacity"], filter_3D)
        else:
            scales_act, opacity_act = torch.exp(params["scaling"]), torch.sigmoid(params["opacity"])
        out = (GaussianRasterizer(S, return_alpha=True) if a.normal_consistency > 0 else GaussianRasterizer(S))(
            means3D=params["xyz"], means2D=m2, dc=params["f_dc"], shs=params["f_rest"], opacities=opacity_act,
            scales=scales_act, rotations=rot_act)
        img, radii = out[0], out[1]
        gt = gts[ci]
        if bil is not None:
            loss = fused_train_loss(bil(img, ci), gt, 0.2) + 10.0 * bil.tv_loss()
        else:
            loss = fused_train_loss(img, gt, 0.2)          # train.py:119-126 as one fused kernel pair (L1 + SSIM + mix)
        if a.normal_consistency > 0:                       # the recipe on this frame's saved state
            alpha, vm = out[3], S.viewmatrix
            cols = torch.cat([gaussian_normals(scales_act, rot_act, params["xyz"], vm), (params["xyz"] @ vm[:3, 2] + vm[3, 2])[:, None]], dim=1)
            feat = dgr.render_features(img, cols, geometry=True)
            loss_n = normal_consistency_loss(feat[3] / alpha[0].clamp_min(1e-6), feat[:3], S.tanfovx, S.tanfovy, weight=alpha[0].detach())
            loss = loss + a.normal_consistency * loss_n
        loss.backward()
        with torch.no_grad():
            if it < 15000:
                stats.add(m2.grad, radii > 0, radii)
                if it > 500 and it % 100 == 0:
                    grow = params["xyz"].shape[0] < a.max_P
                    params, stats, _ = densify_and_prune(opt, stats, max_grad=a.grad_threshold if grow else 1e30, min_opacity=0.005, extent=ext,
                                                         max_screen_size=20 if it > 3000 else None, radii=radii)
                    filter_3D = None      # (--mip_filter: recomputed for the new set on the next iteration)
                if it % 3000 == 0:
                    params["opacity"] = reset_opacity(opt, 0.01)
            if it < a.iters:
                if a.dense_adam:
                    opt.step()
                else:
                    opt.step(radii > 0, radii.shape[0])
                opt.zero_grad(set_to_none=True)
                if bil_opt is not None:
                    bil_opt.step()
                    bil_opt.zero_grad(set_to_none=True)
        if it % 5000 == 0 or it == a.iters:
            torch.cuda.synchronize()
            now = time.perf_counter()
            window_t.append({"until_iter": it, "iters_per_s": round((5000 if it % 5000 == 0 else it % 5000) / (now - t_win), 2),
                             "P": int(params["xyz"].shape[0]), "loss": round(float(loss.detach()), 5),
                             "psnr_last_view": round(float(-10.0 * torch.log10(((img.detach() - gt) ** 2).mean().clamp_min(1e-12))), 2),
                             "num_rendered": int(dgr._last_R) if hasattr(dgr, "_last_R") else None,
                             "mem_allocated": int(torch.cuda.memory_allocated()), "mem_reserved": int(torch.cuda.memory_reserved())})
            t_win = now
        if it % 1000 == 0:
            sizes.append(int(params["xyz"].shape[0]))
    torch.cuda.synchronize()
    total = time.perf_counter() - t_start
    if a.save_state:
        torch.save({"params": {k: v.detach() for k, v in params.items()}, "it": a.iters, "deg": deg,
                    "moments": {k: (opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]) for k, q in params.items() if len(opt.state.get(q, {}))}},
                   a.save_state)
    timeline = None
    if a.timeline > 0:
        from diff_gaussian_rasterization import _lib

        def one_iteration(it, marks=None, host=None):
            """The loop body above without density control.  marks: list that receives torch events at the phase boundaries;
            host: dict that accumulates the host seconds each phase takes to ENQUEUE."""
            def mark(name, t0=[0.0]):      # noqa: B006
                now = time.perf_counter()
                if host is not None and name != "start":
                    host[name] = host.get(name, 0.0) + (now - t0[0])
                if marks is not None:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append((name, e))
                t0[0] = time.perf_counter()
            nonlocal stack
            if not stack:
                stack = list(range(len(cams)))
            ci = stack.pop(random.randint(0, len(stack) - 1))
            P = params["xyz"].shape[0]
            mark("start")
            m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
            img, radii, _ = GaussianRasterizer(settings(cams[ci], deg))(
                means3D=params["xyz"], means2D=m2, dc=params["f_dc"], shs=params["f_rest"], opacities=torch.sigmoid(params["opacity"]),
                scales=torch.exp(params["scaling"]), rotations=torch.nn.functional.normalize(params["rotation"]))
            mark("activations_forward")
            loss = fused_train_loss(img, gts[ci], 0.2)
            mark("loss")
            loss.backward()
            mark("backward")
            with torch.no_grad():
                stats.add(m2.grad, radii > 0, radii)
                mark("density_statistics")
                if a.dense_adam:
                    opt.step()
                else:
                    opt.step(radii > 0, radii.shape[0])
                opt.zero_grad(set_to_none=True)
                mark("optimizer")

        n = a.timeline
        for k in range(20):
            one_iteration(a.iters + k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            one_iteration(a.iters + k)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) / n * 1e3
        host = {}
        t0 = time.perf_counter()
        for k in range(n):
            one_iteration(a.iters + k, None, host)
        torch.cuda.synchronize()
        wall_host_pass_ms = (time.perf_counter() - t0) / n * 1e3
        _lib.profile_enable(True)
        _lib.profile_reset()
        for k in range(n):
            one_iteration(a.iters + k)
        torch.cuda.synchronize()
        stg = _lib.profile_read()
        _lib.profile_enable(False)
        # work counters of the two blend kernels (own pass: they slow the kernels): wave-steps per launch, heaviest wave
        _lib.profile_enable(False, counters=True)
        _lib.profile_counters(reset=True)
        nc_ = min(n, 20)
        for k in range(nc_):
            one_iteration(a.iters + k)
        torch.cuda.synchronize()
        ctr = _lib.profile_counters(reset=True)
        _lib.profile_enable(False)
        marks = []
        for k in range(n):
            one_iteration(a.iters + k, marks)
        torch.cuda.synchronize()
        phase = {}
        for (n0, e0), (n1, e1) in zip(marks[:-1], marks[1:]):
            key = n1 if n1 != "start" else "between_iterations"
            phase[key] = phase.get(key, 0.0) + e0.elapsed_time(e1)
        timeline = {"iterations": n, "P": int(params["xyz"].shape[0]), "num_rendered_last": int(dgr._last_R),
                    "wall_ms_per_iteration": round(wall_ms, 4), "iters_per_s": round(1e3 / wall_ms, 1),
                    "wall_ms_per_iteration_in_the_host_timing_pass": round(wall_host_pass_ms, 4),
                    "host_enqueue_ms_per_phase": {k: round(v / n * 1e3, 4) for k, v in host.items()},
                    "host_enqueue_ms_total": round(sum(host.values()) / n * 1e3, 4),
                    "gpu_ms_per_phase_torch_events": {k: round(v / n, 4) for k, v in phase.items()},
                    "gpu_ms_total_torch_events": round(sum(phase.values()) / n, 4),
                    "library_stage_ms": {k: round(v["ms"] / n, 4) for k, v in stg.items() if v["launches"]},
                    "blend_work_per_iteration": {"fwd_wave_steps": ctr["fwd_steps"] / nc_, "fwd_batches": ctr["fwd_batches"] / nc_, "bwd_wave_steps": ctr["bwd_steps"] / nc_,
                                                 "bwd_batches": ctr["bwd_batches"] / nc_, "fwd_max_wave_steps": ctr["fwd_max_wave_steps"], "bwd_max_wave_steps": ctr["bwd_max_wave_steps"],
                                                 "note": "a forward wave-step = one list entry blended by the 64 pixels of an 8x8 block; a backward wave-step = one entry x 128 pixels "
                                                         "(16x8 half tile); the bench frame (P 1 M, R 7.9 M) has 3.31 M / 1.85 M"},
                    "library_stage_launches_per_iteration": {k: round(v["launches"] / n, 2) for k, v in stg.items() if v["launches"]}}
        print("TIMELINE " + json.dumps(timeline), flush=True)
    n_run = a.iters - it0 + 1
    out = {"metric": "train iters/s, full loop (fwd + loss + bwd + density control + optimizer), reference schedule",
           "value": round(n_run / max(total, 1e-9), 2), "unit": "it/s", "iterations": n_run, "first_iteration": it0, "seconds": round(total, 2), "timeline": timeline,
           "config": {"workload": f"configs[2] stand-in: P0 {P0} -> densified, {W}x{H}, {len(cams)} synthetic views cycled without "
                                  f"replacement, target scene {a.P_target} Gaussians (SURVEY 8(d) generator, seed {a.seed})",
                      "optimizer": ("FusedAdam (dense)" if a.dense_adam else "SparseGaussianAdam + separate_sh call form") + (" + SH step inside backward (opt-in fusion)" if a.fuse_sh_step else "")
                                   + (" + per-camera bilateral grids 16x16x8 (slice before the loss, 10 tv_loss, FusedAdam lr 2e-3)" if a.bilateral_grid else "")
                                   + (f" + {a.normal_consistency:g} x depth-normal consistency (gsr_normals on a 4-channel feature render)" if a.normal_consistency > 0 else "")
                                   + (" + Mip-Splatting's 3D smoothing filter (gsr_scene.mip) and antialiasing" if a.mip_filter else ""),
                      "schedule": f"densify 500..15000 every 100 (grad {a.grad_threshold:g}, opacity 0.005, size 20 after 3000), opacity reset / 3000, "
                                  "SH degree +1 / 1000, position lr 1.6e-4 -> 1.6e-6 x extent", "extent": ext},
           "final_P": int(params["xyz"].shape[0]), "max_P": max(sizes + [P0]), "P_every_1000_iters": sizes,
           "windows": window_t, "peak_device_memory_bytes": int(torch.cuda.max_memory_allocated()),
           "scratch_bytes_last": {f"{k[0]}": int(v) for k, v in dgr._last_size.items()}, "max_num_rendered": int(dgr._max_R),
           "data": "synthetic", "dtype": "f32"}
    print(json.dumps(out), flush=True)
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        tag = ("dense" if a.dense_adam else "sparse") + a.tag
        json.dump(out, open(os.path.join(ROOT, "gpurun_out", f"train_run_{tag}.json"), "w"), indent=1)
    except Exception:
        pass


if __name__ == "__main__":
    main()
