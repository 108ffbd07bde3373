"""The frame and the checks for the per-Gaussian instance-run reduce (csrc/gsr_reduce.h reduce_instance_runs in absgrad_reduce and
feature_grad_reduce<1|2|4>, and contrib_reduce's written-out copy of it), shared by tests/test_instance_runs_cpu.py (the SIMT build) and
tests/test_gpu_instance_runs.py (the MI355X).

The scenes of the other suites are at most 35 tiles large, so no Gaussian there owns a whole chunk of 64 instances: the reduce's fold path and its
skipped chunks never run.  This frame is 256 x 144 = 16 x 9 = 144 tiles with 300 Gaussians (300 % 64 = 44: the last wave has a tail), front to back:
  296 small ones (z in 2..6) touching a few tiles each: runs that cross chunk boundaries, the ordered path;
  one nearly transparent Gaussian over the whole frame (z = 7): 144 instances, all flagged -- the fold path with data;
  two opaque Gaussians over the whole frame (z = 8, 9; alpha is capped at 0.99, so T < 1e-4 needs two): the pixels terminate here;
  one more over the whole frame behind them (z = 10): 144 instances without a flag -- skipped chunks, and a visible Gaussian whose row stays zero.
A run of at least 127 instances contains a whole chunk wherever its wave's first chunk begins; frame_properties asserts that the frame has such runs
with and without contributions, on the host, from the oracle's tile counts and the reference's pixel_count.

Every entry point is held to the reference module it already has, with that module's bars and masks (tests/contrib_reference.py,
tests/absgrad_reference.py, tests/feature_reference.py), and is run twice and compared bit for bit.  Test infrastructure."""
import functools

import torch

from helpers import O, make_camera, make_scene
import absgrad_reference as AR
import contrib_reference as CR
import feature_reference as FR
import test_composite_cpu as T

W, H = 256, 144
N_SMALL = 296
WHOLE_CHUNK = 127      # instances from which a run holds a whole chunk of 64 whatever the chunk grid's phase
FEATURE_CHANNELS = (3, 8, 16, 20)      # slot records of 1, 2, 4, and 4 then 1 float4


@functools.lru_cache(maxsize=None)
def scene():
    cam = make_camera(W, H)
    sc = make_scene(N_SMALL + 4, cam, seed=5, s_med=0.05, overscan=1.0, z_min=2.0, z_max=6.0, sigma_log_scale=0.3)
    big = slice(N_SMALL, N_SMALL + 4)
    sc.means3D[big] = torch.tensor([[0.0, 0.0, 7.0], [0.0, 0.0, 8.0], [0.0, 0.0, 9.0], [0.0, 0.0, 10.0]])
    sc.scales[big] = torch.tensor([8.0, 60.0, 60.0, 60.0])[:, None].expand(4, 3)
    sc.rotations[big] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    sc.opacities[big] = torch.tensor([[0.05], [0.999], [0.999], [0.5]])
    return cam, sc


@functools.lru_cache(maxsize=None)
def oracle_aux():
    """aux (and settings) of the oracle's frame: computed once, shared by the tests, never modified."""
    cam, sc = scene()
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, False)
    with torch.no_grad():
        aux = O.rasterize(s=s0, want_fragile=True, return_aux=True, **T.call_kwargs(T.make_leaves(sc, "fused", grad=False), "fused", oracle=True))[3]
    return aux, s0


@functools.lru_cache(maxsize=None)
def frame_properties():
    """Asserts what the frame is for (module docstring) and that the reference alone stays within the share of fragile pixels its modules allow."""
    aux, s0 = oracle_aux()
    instances = aux["tiles_touched"]
    count = CR.reference(aux, s0, CR.mask_fragile(torch.ones(H, W), aux))["pixel_count"]
    P = instances.shape[0]
    assert P % 64 != 0
    assert int(((instances >= WHOLE_CHUNK) & (count > 0)).sum()) >= 1                # the fold path with data
    assert int(((instances >= WHOLE_CHUNK) & (count == 0)).sum()) >= 1               # skipped chunks, a visible Gaussian with a zero row
    small = instances[:N_SMALL]
    assert int((small > 0).sum()) > 200 and int(small.max()) < 64                    # the ordered path: short runs, many to a chunk
    # (the one input condition of all three reference modules: the same aux["fragile"] share under the same 1 % bar, which contrib_reference.check and
    # absgrad_reference.check assert again on every call)
    assert FR.check_input(aux) < 0.01
    return dict(P=P, instances=int(instances.sum()))


def render(pkg, device, return_alpha=False):
    cam, sc = scene()
    lv = T.make_leaves(sc, "fused", device)
    out, S = T.render_pkg(pkg, cam, lv, "fused", torch.zeros(3, device=device), return_alpha=return_alpha, device=device)
    return out, lv, S


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_contribution_stats(pkg, device, key):
    frame_properties()
    aux, s0 = oracle_aux()
    E = CR.mask_fragile(torch.rand(H, W, generator=torch.Generator().manual_seed(11)), aux)
    ref = CR.reference(aux, s0, E)
    out, _, _ = render(pkg, device)
    got, again = pkg.contribution_stats(out[0], E.to(device)), pkg.contribution_stats(out[0], E.to(device))
    plain, ones = pkg.contribution_stats(out[0]), pkg.contribution_stats(out[0], torch.ones(H, W, device=device))
    acc = pkg.contribution_stats(out[0], E.to(device))
    assert pkg.contribution_stats(out[0], E.to(device), into=acc) is acc
    CR.check(key, got, ref, aux)
    assert equal(got, again) and equal(plain, ones)
    whole = aux["tiles_touched"] >= WHOLE_CHUNK
    assert float(got.weight_sum[whole].max()) > 0.0 and int((got.pixel_count[whole] == 0).sum()) >= 1
    silent = got.pixel_count == 0
    assert float(got.weight_sum[silent].abs().max()) == 0.0 and float(got.weight_max[silent].max()) == 0.0
    assert torch.equal(acc.weight_sum, got.weight_sum + got.weight_sum) and torch.equal(acc.weight_max, got.weight_max)
    assert torch.equal(acc.pixel_count, got.pixel_count * 2)


def absgrad_pass(pkg, device, wC, wD):
    cam, sc = scene()
    lv = T.make_leaves(sc, "fused", device)
    m2d = torch.zeros(sc.P, 3, device=device, requires_grad=True)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3, device=device), device=device)
    out = pkg.GaussianRasterizer(S, absgrad=True)(**dict(T.call_kwargs(lv, "fused"), means2D=m2d))
    ((out[0] * wC.to(device)).sum() + (out[2] * wD.to(device)).sum()).backward()
    return m2d


def check_absgrad(pkg, device, key):
    frame_properties()
    aux, s0 = oracle_aux()
    g = torch.Generator().manual_seed(7)
    wC, wD = [AR.mask_fragile(torch.rand(n, H, W, generator=g) - 0.3, aux) for n in (3, 1)]
    ref = AR.reference(aux, s0, wC, wD)
    m2d, again = absgrad_pass(pkg, device, wC, wD), absgrad_pass(pkg, device, wC, wD)
    AR.check(key, m2d.absgrad, m2d.grad, ref, aux)
    assert torch.equal(m2d.absgrad, again.absgrad)
    whole = (aux["tiles_touched"] >= WHOLE_CHUNK).to(m2d.absgrad.device)
    assert float(m2d.absgrad[whole].sum(1).max()) > 0.0 and int((m2d.absgrad[whole].sum(1) == 0).sum()) >= 1


def feature_pass(pkg, rendered, f, grad_out):
    leaf = f.clone().requires_grad_(True)
    pkg.render_features(rendered, leaf).backward(grad_out)
    return leaf.grad


def check_feature_gradient(pkg, device, channels, key):
    frame_properties()
    aux, s0 = oracle_aux()
    g = torch.Generator().manual_seed(31)
    f = torch.rand(aux["means2D"].shape[0], channels, generator=g) * 2.0 - 1.0
    g_up = torch.stack([FR.mask_fragile(torch.rand(H, W, generator=g) - 0.5, aux) for _ in range(channels)])
    ref = FR.gradient(aux, s0, g_up)
    out, _, _ = render(pkg, device)
    got, again = feature_pass(pkg, out[0], f.to(device), g_up.to(device)), feature_pass(pkg, out[0], f.to(device), g_up.to(device))
    FR.check_gradient(key, got, ref, aux)
    assert torch.equal(got, again)
    whole = (aux["tiles_touched"] >= WHOLE_CHUNK).to(got.device)
    rows = got[whole].abs().sum(1)
    assert float(rows.max()) > 0.0 and int((rows == 0).sum()) >= 1
