"""Non-finite and out-of-range Gaussian parameters on the MI355X: the frames and the contract of tests/poison_frames.py through the shipped
operator (`GaussianRasterizer`, autograd) and `diff_gaussian_rasterization.debug.forward_with_views`, and what the training loop does with the
result (SparseGaussianAdam, gsr_density_stats, contribution_stats).  Every frame here has passed tests/test_poison_cpu.py, which runs the same
kernel source with guard bytes behind every buffer; the oracle runs once per frame and is shared."""
import functools

import pytest
import torch

import poison_frames as PF
import test_gpu_parity as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def oracle_of(kind, grad=False):
    """The oracle's frame of a kind (or "mixed"): computed once, shared, never modified."""
    frame = PF.build_mixed()[0] if kind == "mixed" else PF.build(kind).poisoned
    r = PF.run_oracle(frame, grad=grad)
    PF.guard_fragile_share(r[3])
    return r


def leaves_of(frame):
    L = {k: frame.field(k).detach().clone().to(DEV).requires_grad_(True) for k in frame.fields()}
    L["means2D"] = torch.zeros(frame.sc.P, 3, device=DEV, requires_grad=True)
    return L


def render(frame, L, return_alpha=False):
    from diff_gaussian_rasterization import GaussianRasterizer
    kw = {k: v for k, v in L.items() if k not in ("means3D", "means2D", "opacities")}
    return GaussianRasterizer(G.gpu_settings(PF.settings(), torch.device(DEV)), return_alpha=return_alpha)(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], **kw)


def run_gpu(frame, grad=True, no_backward=False):
    """-> (forward outputs and views, gradients by name) of one frame; the operator's image is the debug forward's bit for bit."""
    from diff_gaussian_rasterization.debug import forward_with_views
    d = {k: frame.field(k).to(DEV) for k in frame.fields()}
    out = forward_with_views(G.gpu_settings(PF.settings(), torch.device(DEV)), d["means3D"], d["opacities"], shs=d.get("shs"), colors_precomp=d.get("colors_precomp"),
                             scales=d.get("scales"), rotations=d.get("rotations"), cov3D_precomp=d.get("cov3D_precomp"), no_backward=no_backward)
    torch.cuda.synchronize()
    PF.check_structure(out)
    if not grad:
        return out, None
    L = leaves_of(frame)
    col, radii, invd = render(frame, L)
    wc, wd = PF.loss_weights()
    ((col * wc.to(DEV)).sum() + (invd * wd.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert PF.same_bits(col, out["color"]) and PF.same_bits(invd, out["invdepth"]) and torch.equal(radii, out["radii"])
    return out, {PF.GRAD_KEYS[k]: v.grad.detach().cpu() for k, v in L.items()}


@functools.lru_cache(maxsize=None)
def shared_run(which, form, victims=(), no_backward=False):
    """The clean frame of a call form, or its hidden frame for a victim set: run once, shared, never modified."""
    f = PF.clean(form)
    if which == "hidden":
        PF.hide(f, list(victims))
    return run_gpu(f, grad=not no_backward, no_backward=no_backward)


def g_frame(b, what):
    from diff_gaussian_rasterization import GaussianRasterizer
    form, v = PF.form_of(b.kind), tuple(b.victims)
    out, grads = run_gpu(b.poisoned)
    PF.check_equals_hidden(out, grads, *shared_run("hidden", form, v), b.victims)
    out_i, _ = run_gpu(b.poisoned, grad=False, no_backward=True)
    PF.check_equals_hidden(out_i, None, shared_run("hidden", form, v, True)[0], None, b.victims)
    s = PF.settings()
    vis = GaussianRasterizer(G.gpu_settings(s, torch.device(DEV))).markVisible(b.poisoned.sc.means3D.to(DEV)).cpu()
    if b.kind.field == "means3D":      # (markVisible sees positions only)
        assert not bool(vis[b.victims].any()), f"{what}: markVisible calls a victim visible"
    assert torch.equal(vis, PF.O.mark_visible(b.poisoned.sc.means3D, s.viewmatrix))
    return out, grads


@pytest.mark.parametrize("kind", PF.names("G"))
def test_geometry_poison_is_culled_and_leaves_the_hidden_frame(kind):
    out, _ = g_frame(PF.build(kind), kind)
    col, radii, invd, aux = oracle_of(kind)
    G.check_forward(PF.settings(), col, radii, invd, aux, out)


@pytest.mark.parametrize("name", list(PF.PLACEMENTS))
def test_structural_placements_of_culled_victims(name):
    out, grads = g_frame(PF.build_placement(name), name)
    if name == "every_gaussian":
        assert out["R"] == 0 and int(out["ranges"].abs().max()) == 0
        assert torch.equal(out["color"].cpu(), torch.tensor(PF.BG)[:, None, None].expand(3, PF.H, PF.W)) and float(out["invdepth"].abs().max()) == 0.0
        assert all(float(a.abs().max()) == 0.0 for a in grads.values())
    else:
        assert out["R"] > 0


@pytest.mark.parametrize("kind", PF.names("F"))
def test_odd_but_finite_parameters_are_ordinary_input(kind):
    col, radii, invd, aux, grads_o = oracle_of(kind, True)
    out, grads = run_gpu(PF.build(kind).poisoned)
    G.check_forward(PF.settings(), col, radii, invd, aux, out)
    PF.check_grads_against_oracle(grads, grads_o, what=kind)


@pytest.mark.parametrize("kind", PF.names("H"))
def test_huge_finite_splats_integers_and_finiteness(kind):
    b = PF.build(kind)
    f = b.poisoned
    with torch.no_grad():
        pre = PF.O.preprocess(f.sc.means3D, f.sc.opacities, PF.settings(), **f.oracle_kwargs())
        bins = PF.O.bin_and_sort(pre)
    out, grads = run_gpu(f)
    assert int(pre["tiles_touched"][b.victims].min()) == pre["grid"][0] * pre["grid"][1]
    assert torch.equal(out["radii"].cpu(), pre["radii"]) and torch.equal(out["tiles_touched"].cpu().long(), pre["tiles_touched"]) and out["R"] == int(bins["R"])
    assert torch.equal(out["point_list"].cpu().long(), bins["point_list"]) and torch.equal(out["ranges"].cpu().long(), bins["ranges"])
    assert bool(torch.isfinite(out["color"]).all()) and bool(torch.isfinite(out["invdepth"]).all())
    assert all(bool(torch.isfinite(a).all()) for a in grads.values())


@pytest.mark.parametrize("kind", PF.names("O"))
def test_non_finite_opacity_renders_with_alpha_099(kind):
    b = PF.build(kind)
    s, f, v = PF.settings(), b.poisoned, b.victims
    col, radii, invd, aux, grads_o = oracle_of(kind, True)
    out, grads = run_gpu(f)
    G.check_forward(s, col, radii, invd, aux, out)
    ref = PF.reference_rect(f)[v]
    assert torch.equal(out["tiles_touched"].cpu().long()[v], (ref[:, 2] - ref[:, 0]) * (ref[:, 3] - ref[:, 1]))
    clean_out = shared_run("clean", "sh")[0]
    assert float((out["color"] - clean_out["color"]).abs().max()) > 0.1, "the victims do not show"
    PF.check_grads_against_oracle(grads, grads_o, skip_rows=v, what=kind)
    PF.check_non_finite_rows_within(grads, v, kind)
    PF.check_same_outside(out, clean_out, PF.reference_tiles_of(f, v), kind)
    out_i, _ = run_gpu(f, grad=False, no_backward=True)
    G.check_forward(s, col, radii, invd, aux, out_i)
    assert PF.same_bits(out_i["color"], out["color"])


@pytest.mark.parametrize("kind", PF.names("C"))
def test_non_finite_colour_is_contained(kind):
    b = PF.build(kind)
    out, grads = run_gpu(b.poisoned)
    out_c, grads_c = shared_run("clean", PF.form_of(b.kind))
    col, radii, invd, aux = oracle_of(kind)
    if PF.check_colour_frame(kind, b, out, grads, out_c, grads_c, col, radii, invd, aux):
        G.check_forward(PF.settings(), col, radii, invd, aux, out)
        PF.check_grads_against_oracle(grads, oracle_of(kind, True)[4], skip_rows=b.victims, what=kind)
    out_i, _ = run_gpu(b.poisoned, grad=False, no_backward=True)
    assert PF.same_bits(out_i["color"], out["color"]) and PF.same_bits(out_i["invdepth"], out["invdepth"])


def test_mixed_frame_one_victim_of_every_kind():
    f, who = PF.build_mixed()
    col, radii, invd, aux, grads_o = oracle_of("mixed", True)
    out, grads = run_gpu(f)
    culled = [v for k, v in who.items() if PF.KIND[k].group == "G"]
    own = [v for k, v in who.items() if PF.KIND[k].group in "OC"]
    PF.check_culled(out, culled)
    binned = aux["rect"][[v for k, v in who.items() if PF.KIND[k].group == "C" and PF.KIND[k].value == PF.INF]]
    n_o, n_k = PF.check_image_with_non_finite(PF.settings(), col, radii, invd, aux, out, PF.tile_pixels(binned), "mixed")
    assert n_o > 0
    allowed = torch.unique(torch.cat([PF.listed_in(binned, out), torch.tensor(own)]))
    PF.check_non_finite_rows_within(grads, allowed, "mixed")
    PF.check_grads_against_oracle(grads, {k: torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0) for k, g in grads_o.items()}, skip_rows=allowed, what="mixed")
    for k in grads:
        assert float(grads[k][culled].abs().max()) == 0.0, f"mixed dL/d{k}: a culled victim's row is not zero"


# ---- what training does with a culled victim ----------------------------------------------------------------------------------------------
DOWNSTREAM = "scale_nan"


def test_sparse_adam_leaves_a_culled_victims_rows_alone():
    """SparseGaussianAdam.step(radii > 0, P) after the backward of a G frame: the victim's parameter row (its NaN included) and both moments keep
    their bits; the rows of visible Gaussians move."""
    from diff_gaussian_rasterization import SparseGaussianAdam
    b = PF.build(DOWNSTREAM)
    L = leaves_of(b.poisoned)
    names = [k for k in L if k != "means2D"]
    opt = SparseGaussianAdam([{"params": [L[k]], "lr": 1e-2, "name": k} for k in names], lr=1e-2, eps=1e-15)
    g = torch.Generator().manual_seed(3)
    for k in names:      # moments of an optimizer that has been running
        opt.state[L[k]] = {"step": torch.tensor(5.0), "exp_avg": torch.randn(L[k].shape, generator=g).to(DEV), "exp_avg_sq": torch.rand(L[k].shape, generator=g).to(DEV)}
    before = {k: (L[k].detach().clone(), opt.state[L[k]]["exp_avg"].clone(), opt.state[L[k]]["exp_avg_sq"].clone()) for k in names}
    col, radii, invd = render(b.poisoned, L)
    wc, wd = PF.loss_weights()
    ((col * wc.to(DEV)).sum() + (invd * wd.to(DEV)).sum()).backward()
    opt.step(radii > 0, PF.P)
    torch.cuda.synchronize()
    v = torch.tensor(b.victims, device=DEV)
    seen = torch.nonzero(radii > 0)[:, 0]
    assert int((radii[v] != 0).sum()) == 0 and len(seen) > 500
    for k in names:
        after = (L[k].detach(), opt.state[L[k]]["exp_avg"], opt.state[L[k]]["exp_avg_sq"])
        for a, a0, what in zip(after, before[k], ("parameter", "exp_avg", "exp_avg_sq")):
            assert PF.same_bits(a[v], a0[v]), f"{k}: the victim's {what} row changed"
            assert bool(torch.isfinite(a[seen]).all()), f"{k}: {what} of a visible Gaussian is not finite"
        assert not torch.equal(after[1][seen], before[k][1][seen]), f"{k}: the visible rows did not move"


def test_density_stats_leave_a_culled_victims_accumulators_alone():
    from gsr_scene.densify import DensifyStats
    b = PF.build(DOWNSTREAM)
    L = leaves_of(b.poisoned)
    col, radii, invd = render(b.poisoned, L)
    wc, _ = PF.loss_weights()
    (col * wc.to(DEV)).sum().backward()
    g = torch.Generator().manual_seed(4)
    st = DensifyStats(torch.rand(PF.P, 1, generator=g).to(DEV), torch.rand(PF.P, 1, generator=g).to(DEV).mul_(9).round_(), torch.rand(PF.P, generator=g).to(DEV))
    before = [t.clone() for t in (st.xyz_gradient_accum, st.denom, st.max_radii2D)]
    st.add(L["means2D"].grad, radii > 0, radii)
    torch.cuda.synchronize()
    v = torch.tensor(b.victims, device=DEV)
    for a, a0 in zip((st.xyz_gradient_accum, st.denom, st.max_radii2D), before):
        assert PF.same_bits(a[v], a0[v]) and bool(torch.isfinite(a).all())
    assert torch.equal(st.denom[radii > 0], before[1][radii > 0] + 1)


def test_contribution_stats_of_a_culled_victim_are_zero():
    """weight_sum = 0 and pixel_count = 0 for the victim, the hidden frame's bits for every other Gaussian."""
    import diff_gaussian_rasterization as pkg
    b = PF.build(DOWNSTREAM)
    E = torch.rand(PF.H, PF.W, generator=torch.Generator().manual_seed(6)).to(DEV)
    got, want = [pkg.contribution_stats(render(f, leaves_of(f))[0], E) for f in (b.poisoned, b.hidden)]
    torch.cuda.synchronize()
    v = torch.tensor(b.victims, device=DEV)
    assert float(got.weight_sum[v].abs().max()) == 0.0 and int(got.pixel_count[v].abs().max()) == 0 and float(got.weight_max[v].abs().max()) == 0.0
    assert all(PF.same_bits(x, y) for x, y in zip(got, want)) and int((got.pixel_count > 0).sum()) > 300
