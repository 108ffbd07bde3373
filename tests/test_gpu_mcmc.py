"""3DGS-MCMC density control on the MI355X: the two kernels of csrc/mcmc.hip against tests/mcmc_reference.py with the bars of tests/test_mcmc_cpu.py
(which runs the same source on the host), the grid-stride loop of the noise pass, run-to-run bits, and a short optimisation with gsr_scene.mcmc in the
loop (cap, relocation, noise)."""
import math

import numpy as np
import pytest
import torch

import mcmc_reference as MR
from helpers import make_camera, make_scene, oracle_settings
from test_gpu_parity import gpu_settings

pytestmark = pytest.mark.gpu

NOISE_SCALE = 0.8
DEV = "cuda:0"


def inject(case, xyz, activated=False, misalign=False, noise_scale=NOISE_SCALE):
    """gsr_mcmc_inject_noise on device copies of a case -> xyz afterwards, on the host.  misalign: every buffer starts 4 bytes past a 16-byte
    boundary (the scalar form of the kernel)."""
    import diff_gaussian_rasterization as pkg
    lib = pkg._lib.load()
    scaling, opacity = case["scaling"], case["opacity"]
    if activated:
        scaling, opacity = torch.exp(scaling.double()).float(), torch.sigmoid(opacity.double()).float()

    def put(t):
        t = t.reshape(-1).float()
        buf = torch.empty(t.numel() + 4, device=DEV)
        view = buf[1:1 + t.numel()] if misalign else buf[:t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 if misalign else 0)
        return view
    bufs = [put(t) for t in (xyz, scaling, case["rotation"], opacity, case["xi"])]
    P = int(xyz.shape[0])
    with torch.cuda.device(DEV):
        pkg._lib.check(lib.gsr_mcmc_inject_noise(P, *[pkg._ptr(b) for b in bufs], 1 if activated else 0, noise_scale, MR.GATE_K, MR.GATE_X0,
                                                 pkg._stream_ptr(torch.device(DEV))), "gsr_mcmc_inject_noise")
    return bufs[0].cpu().reshape(P, 3)


def check(case, got0, got_xyz, what, rows=None):
    sub = case if rows is None else {k: v[rows] for k, v in case.items()}
    d64 = MR.noise_delta(sub["scaling"], sub["rotation"], sub["opacity"], sub["xi"], NOISE_SCALE)
    bar = MR.noise_bar(sub["scaling"], sub["opacity"], sub["xi"], NOISE_SCALE)
    unit = MR.noise_unit(sub["scaling"], sub["opacity"], sub["xi"], NOISE_SCALE)
    got0 = got0 if rows is None else got0[rows]
    err = (got0.double() - d64).abs()
    print(f"[mcmc] gpu noise {what}: {len(d64)} rows, max error {float(((err - MR.DENORM32).clamp(min=0) / unit).max()):.2f} units (bar {MR.NOISE_C:g})", flush=True)
    assert bool((err <= bar).all()), (what, float((err / bar).max()))
    if got_xyz is not None:
        got_xyz = got_xyz if rows is None else got_xyz[rows]
        w32 = (sub["xyz"].double() + d64).float()
        ulp = (torch.nextafter(w32.abs(), torch.full_like(w32, math.inf)) - w32.abs()).double()
        assert bool(((got_xyz.double() - w32.double()).abs() <= ulp + bar).all()), what
    return bar


@pytest.mark.parametrize("P", [1, 3, 4, 5, 255, 1027])
def test_gpu_noise_kernel_is_upstreams_expression(P):
    case = MR.noise_case(P, seed=100 + P)
    zero = torch.zeros(P, 3)
    got = {}
    for activated in (False, True):
        for mis in (False, True):
            got[activated, mis] = inject(case, zero, activated, mis)
            bar = check(case, got[activated, mis], inject(case, case["xyz"], activated, mis), f"P={P} activated={activated} misaligned={mis}")
        assert torch.equal(got[activated, False].view(torch.int32), got[activated, True].view(torch.int32))
    assert bool(((got[False, False].double() - got[True, False].double()).abs() <= bar).all()), "activated 0 and 1 disagree"
    again = inject(case, zero)
    assert torch.equal(again.view(torch.int32), got[False, False].view(torch.int32)), "two runs with the same xi differ"


def test_gpu_noise_kernel_grid_stride_and_tail():
    """P just above 4 x 256 x the grid cap (2048 blocks): the grid-stride loop is taken once more by the first block, and three tail rows follow."""
    P = 4 * 256 * 2048 + 4 * 256 + 3
    case = MR.noise_case(P, seed=100 + P)
    got0 = inject(case, torch.zeros(P, 3))
    got = inject(case, case["xyz"])
    rows = torch.cat([torch.arange(4), torch.randint(0, P, (1000,), generator=torch.Generator().manual_seed(1)), torch.arange(P - 5, P)])
    check(case, got0, got, f"P={P}", rows)
    assert float(got0[4 * 256 * 2048:].abs().max()) > 1e-3 and float(got0[-3:].abs().max()) > 0      # the second trip and the tail did their work
    assert torch.equal(inject(case, case["xyz"]).view(torch.int32), got.view(torch.int32)), "two runs with the same xi differ"


@pytest.mark.parametrize("misalign", [False, True])
def test_gpu_noise_kernel_leaves_poisoned_rows_alone(misalign):
    P = 1027
    clean = MR.noise_case(P, seed=7)
    want = inject(clean, clean["xyz"], misalign=misalign)
    case = {k: v.clone() for k, v in clean.items()}
    rows = [0, 1, 2, 3, 6, 258, 513, 1020, 1024, 1025, 1026]
    for i, row in enumerate(rows):
        field, comp, value = MR.POISON[list(MR.POISON)[i % len(MR.POISON)]]
        if comp is None:
            case[field][row] = value
        else:
            case[field][row, comp] = value
    got = inject(case, case["xyz"], misalign=misalign)
    v = torch.tensor(rows)
    keep = torch.ones(P, dtype=torch.bool)
    keep[v] = False
    assert torch.equal(got[v].view(torch.int32), case["xyz"][v].view(torch.int32)), "a poisoned row moved"
    assert torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32)), "a clean row differs from the run without the poison"
    assert not torch.equal(want[v], clean["xyz"][v])


@pytest.mark.parametrize("n", [1, 255, 257])
def test_gpu_relocation_kernel_is_the_fp64_closed_form(n):
    from gsr_scene import mcmc
    o, s, r = MR.relocation_inputs(n, seed=n)
    if n == 1:
        o[0], r[0] = 0.3, 7
    got_o, got_s = mcmc.compute_relocation(torch.from_numpy(o).to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(r).to(DEV))
    assert got_o.is_cuda and got_o.shape == (n,) and got_s.shape == (n, 3)
    MR.check_relocation(got_o.cpu().numpy(), got_s.cpu().numpy(), *MR.relocation_expected(o, s, r), o, s)


def test_gpu_short_optimisation_with_mcmc_density_control():
    """train.py in miniature with the MCMC strategy: render, loss + opacity / scale regularisers, FusedAdam step, inject_noise every
    iteration, relocate + add_new every 50.  3 000 Gaussians grow by a tenth per call to the cap of 4 000 and stay there."""
    import torch.nn as nn
    from diff_gaussian_rasterization import GaussianRasterizer
    from gsr_optim import FusedAdam
    from gsr_scene import mcmc
    dev = torch.device(DEV)
    cam = make_camera(64, 64)
    target = make_scene(4000, cam, seed=21, s_med=0.06).to(dev)
    rast = GaussianRasterizer(gpu_settings(oracle_settings(cam), dev))
    kw0 = dict(colors_precomp=None, cov3D_precomp=None)
    with torch.no_grad():
        gt = rast(means3D=target.means3D, means2D=None, dc=target.shs[:, :1].contiguous(), shs=target.shs[:, 1:].contiguous(),
                  opacities=target.opacities, scales=target.scales, rotations=target.rotations, **kw0)[0]
    P0, cap = 3000, 4000
    mk = lambda t: nn.Parameter(t.detach().clone().contiguous().requires_grad_(True))      # noqa: E731
    opacity0 = torch.logit(target.opacities[:P0].clamp(0.05, 0.95))
    opacity0[::30] = math.log(0.0005 / 0.9995)      # a hundred Gaussians that are dead from the start
    params = {"xyz": mk(target.means3D[:P0]), "f_dc": mk(target.shs[:P0, :1]), "f_rest": mk(target.shs[:P0, 1:] * 0.0), "opacity": mk(opacity0),
              "scaling": mk(torch.log(target.scales[:P0] * 2.0)), "rotation": mk(target.rotations[:P0])}
    lrs = {"xyz": 1.6e-3, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 0.025, "scaling": 5e-3, "rotation": 1e-3}
    opt = FusedAdam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in params], lr=0.0, eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(3)
    losses, sizes, relocated = [], [P0], 0
    for it in range(1, 251):
        m2 = torch.zeros(params["xyz"].shape[0], 3, device=dev, requires_grad=True)
        img = rast(means3D=params["xyz"], means2D=m2, dc=params["f_dc"], shs=params["f_rest"], opacities=torch.sigmoid(params["opacity"]),
                   scales=torch.exp(params["scaling"]), rotations=torch.nn.functional.normalize(params["rotation"]), **kw0)[0]
        fit = (img - gt).abs().mean()
        loss = fit + 0.01 * torch.sigmoid(params["opacity"]).mean() + 0.01 * torch.exp(params["scaling"]).mean()
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        mcmc.inject_noise(opt, 5e4 * lrs["xyz"], generator=gen)
        losses.append(float(fit.detach()))
        if it % 50 == 0:
            dead = (torch.sigmoid(params["opacity"].detach()) <= 0.005).squeeze(-1)
            relocated += mcmc.relocate(opt, dead, min_opacity=0.005, generator=gen)
            assert float(torch.sigmoid(params["opacity"].detach()).min()) >= 0.005 * (1 - 1e-5), "a dead opacity survived the relocation"
            params = mcmc.add_new(opt, cap, growth=1.1, min_opacity=0.005, generator=gen)
            sizes.append(params["xyz"].shape[0])
            for k, p in params.items():
                st = opt.state[p]
                assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and p.is_contiguous() and p.shape[0] == sizes[-1], k
    print(f"[mcmc] sizes {sizes}, relocated {relocated}, loss {losses[0]:.4f} -> {np.mean(losses[-10:]):.4f}", flush=True)
    assert sizes == [3000, 3300, 3630, 3993, 4000, 4000], sizes            # reaches the cap, never exceeds it
    assert relocated >= 100
    assert all(bool(torch.isfinite(p).all()) for p in params.values())
    assert all(v == v for v in losses) and float(np.mean(losses[-10:])) < losses[0], (losses[0], losses[-10:])
