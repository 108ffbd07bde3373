"""The differentiable alpha image and the per-pixel / learnable background (gsr_rasterize_forward_composite, gsr_backward_blend_composite,
include/gsr.h) through the shipped package on the CPU: the SIMT build of the whole library behind the package's own loader, as in
tests/test_simt_package_cpu.py.

The reference, without touching oracle/: the oracle detaches final_T and knows one constant, detached background, but it is linear in colour.
  * a differentiable oracle alpha is channel 0 of O.rasterize(..., colors_precomp = ones[P,3]) with bg = 0: the blend weights telescope to
    1 - T_final, termination included;
  * the oracle's image over any background B is color(bg = 0) + (1 - alpha_oracle) * B, differentiable in B too.
Bars: the image and gradient bars this project uses for the package on the CPU and on the GPU (tests/test_simt_package_cpu.py:73-88).  The
background gradient is held to what its definition gives: dL/dbg_image is the fp32 product final_T * dL/dC bit for bit, dL/dbg[3] is within
2^-23 * sum |T g| of the fp64 sum (exact products, fp64 accumulation, one rounding to fp32).

Test infrastructure: the product never loads the SIMT library."""
import ctypes as C
import os
import subprocess
import sys
from unittest import mock

import pytest
import torch

from helpers import O, make_camera, make_scene
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
from test_camera_grad_cpu import cov3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = [0.1, 0.0, 0.3]
FORMS = ["fused", "split", "precomp"]


def dense_scene(W=96, H=80, P=3000):      # mean alpha 0.78, 2.6 % of the pixels above 0.99, none empty
    cam = make_camera(W, H)
    return cam, make_scene(P, cam, seed=3, s_med=0.05)


def sparse_scene(W=96, H=80, P=400):      # 61 % of the pixels have no contributor: the blend backward's early exits
    cam = make_camera(W, H)
    return cam, make_scene(P, cam, seed=3, s_med=0.012)


def make_leaves(sc, form, device="cpu", grad=True):
    """The differentiable inputs of one call form, as leaves on `device`."""
    g = torch.Generator().manual_seed(21)
    t = dict(means=sc.means3D, opac=sc.opacities)
    if form == "precomp":
        t.update(colors=torch.rand(sc.P, 3, generator=g), cov=cov3d(sc.scales, sc.rotations))
    else:
        t.update(scales=sc.scales, rot=sc.rotations)
        if form == "split":
            t.update(dc=sc.shs[:, :1].contiguous(), rest=sc.shs[:, 1:].contiguous())
        else:
            t.update(shs=sc.shs)
    return {k: v.detach().clone().to(device).requires_grad_(grad) for k, v in t.items()}


def call_kwargs(lv, form, oracle=False):
    kw = dict(means3D=lv["means"], means2D=None, opacities=lv["opac"])
    if form == "precomp":
        kw.update(colors_precomp=lv["colors"], cov3D_precomp=lv["cov"])
    else:
        kw.update(scales=lv["scales"], rotations=lv["rot"])
        if form == "split" and not oracle:
            kw.update(dc=lv["dc"], shs=lv["rest"])
        elif form == "split":
            kw.update(shs=torch.cat([lv["dc"], lv["rest"]], dim=1))
        else:
            kw.update(shs=lv["shs"])
    return kw


def settings(S, cam, bg, aa=False, device="cpu", cam_grad=False):
    c = [t.detach().clone().to(device).requires_grad_(cam_grad) for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    return S(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, bg, 1.0, c[0], c[1], 3, c[2], False, False, aa)


def render_pkg(pkg, cam, lv, form, bg, aa=False, return_alpha=True, tile_rows=None, device="cpu", cam_grad=False):
    S = settings(pkg.GaussianRasterizationSettings, cam, bg, aa, device, cam_grad)
    rast = pkg.GaussianRasterizer(S, return_alpha=True) if return_alpha else pkg.GaussianRasterizer(S)
    if tile_rows is not None:
        rast.tile_rows = tile_rows
    return rast(**call_kwargs(lv, form)), S


def render_oracle(cam, lv, form, bg, aa=False):
    """The composed oracle of the module docstring -> (color, alpha, invdepth, aux of the colour render), differentiable in lv and bg."""
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, aa)
    kw = call_kwargs(lv, form, oracle=True)
    c0, radii, invd, aux = O.rasterize(s=s0, return_aux=True, **kw)
    kw1 = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
    a = O.rasterize(s=s0, colors_precomp=torch.ones(lv["means"].shape[0], 3), **kw1)[0][:1]
    B = bg if bg.dim() == 3 else bg[:, None, None]
    return c0 + (1.0 - a) * B, a, invd, aux


def weights(H, W, device="cpu", seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, H, W, generator=g).to(device) - 0.3 for n in (3, 1, 1)]      # colour, alpha, inverse depth


def loss_of(color, alpha, invd, w, parts="cad"):
    terms = []
    if "c" in parts:
        terms.append((color * w[0]).sum())
    if "a" in parts:
        terms.append((alpha * w[1]).sum())
    if "d" in parts:
        terms.append((invd * w[2]).sum())
    return sum(terms)


def image_bars(got, want, what):
    err = (got.detach().cpu() - want.detach()).abs().amax(0)
    frac, mx = float((err > 1e-5).float().mean()), float(err.max())
    print(f"[composite] {what}: share > 1e-5 = {frac:.5f}, max = {mx:.3e}", flush=True)
    assert frac < 0.01 and mx < 1.1 / 255.0, (what, frac, mx)


def grad_bars(got, want, what):
    """tests/test_simt_package_cpu.py:83-88: max < 2e-3 and 0.999-quantile < 1e-4 of max |grad| per tensor."""
    for k, a in want.items():
        b = got[k]
        if a is None:      # the oracle's loss does not reach this input at all
            assert b is None or float(b.abs().max()) == 0.0, (what, k)
            continue
        assert b is not None, f"{what}: {k}: no gradient from the package"
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        scale = float(a.abs().max())
        if scale == 0.0:
            assert float(b.abs().max()) == 0.0, (what, k)
            continue
        d = (a - b).abs() / scale
        mx, q = float(d.max()), float(torch.quantile(d.flatten()[:2_000_000], 0.999))
        print(f"[composite] {what}: {k}: max = {mx:.3e}, q0.999 = {q:.3e}", flush=True)
        assert mx < 2e-3 and q < 1e-4, (what, k, mx, q)


def final_T_of(pkg, out, P, H, W):
    """final_T [H,W] of the forward that produced `out`, through gsr_forward_views on the state the autograd node keeps."""
    from diff_gaussian_rasterization import _lib
    fn = out.grad_fn
    geom, binning, img = fn.saved_tensors[8:11]
    v = _lib.GsrForwardViews()
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    _lib.check(_lib.load().gsr_forward_views(P, C.c_int64(fn.num_rendered), W, H, ptr(geom), ptr(binning), ptr(img), C.byref(v)), "gsr_forward_views")
    off = int(v.final_T) - img.data_ptr()
    return img[off:off + H * W * 4].view(torch.float32).view(H, W).clone()


def bg_sum_bound(T, g, got, rows=None):
    """|dL/dbg[c] - fp64 sum of T g| <= 2^-23 sum |T g| per channel (rows: the band's pixel rows)."""
    T, g = T.detach().double().cpu(), g.detach().double().cpu()
    if rows is not None:
        T, g = T[rows[0]:rows[1]], g[:, rows[0]:rows[1]]
    prod = T[None] * g
    want, bound = prod.sum((1, 2)), prod.abs().sum((1, 2)) * 2.0 ** -23
    err = (got.detach().double().cpu() - want).abs()
    print(f"[composite] dL/dbg: err = {err.tolist()}, bound = {bound.tolist()}", flush=True)
    assert bool((err <= bound).all()), (err, bound)


# ---- 1. the alpha image ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_alpha_is_one_minus_final_T_and_leaves_the_other_outputs_alone(simt_lib, which):  # noqa: F811
    cam, sc = dense_scene() if which == "dense" else sparse_scene()
    bg = torch.tensor(BG)
    with package_on_the_cpu(simt_lib) as pkg:
        (color, radii, invd, alpha), _ = render_pkg(pkg, cam, make_leaves(sc, "fused"), "fused", bg)
        (color3, radii3, invd3), _ = render_pkg(pkg, cam, make_leaves(sc, "fused"), "fused", bg, return_alpha=False)
    lv = make_leaves(sc, "fused", grad=False)
    _, _, _, aux = O.rasterize(s=O.settings_from_camera(cam, bg, 3), return_aux=True, **call_kwargs(lv, "fused", oracle=True))
    assert alpha.shape == (1, cam.image_height, cam.image_width) and alpha.requires_grad
    image_bars(alpha, 1.0 - aux["final_T"][None], f"alpha ({which})")
    assert torch.equal(color, color3) and torch.equal(invd, invd3) and torch.equal(radii, radii3)
    empty = aux["n_contrib"] == 0
    assert (int(empty.sum()) == 0) if which == "dense" else (float(empty.float().mean()) > 0.4)
    assert torch.equal(alpha[0][empty], torch.zeros_like(alpha[0][empty]))


# ---- 2. gradients against the composed oracle --------------------------------------------------------------------------------------
def _both(simt_lib, cam, sc, form, aa, parts, bg_pkg=None, bg_ora=None):  # noqa: F811
    H, W = cam.image_height, cam.image_width
    w = weights(H, W)
    bg_pkg = torch.tensor(BG) if bg_pkg is None else bg_pkg
    bg_ora = torch.tensor(BG) if bg_ora is None else bg_ora
    lp, lo = make_leaves(sc, form), make_leaves(sc, form)
    with package_on_the_cpu(simt_lib) as pkg:
        (color, radii, invd, alpha), _ = render_pkg(pkg, cam, lp, form, bg_pkg, aa)
        loss_of(color, alpha, invd, w, parts).backward()
    co, ao, do, aux = render_oracle(cam, lo, form, bg_ora, aa)
    loss_of(co, ao, do, w, parts).backward()
    assert int((radii > 0).sum()) > 50
    return (color, alpha, invd, lp), (co, ao, do, lo), aux


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_gradients_of_a_colour_alpha_depth_loss_match_the_composed_oracle(simt_lib, form, aa):  # noqa: F811
    cam, sc = dense_scene()
    (color, alpha, invd, lp), (co, ao, do, lo), _ = _both(simt_lib, cam, sc, form, aa, "cad")
    image_bars(color, co, "color"), image_bars(alpha, ao, "alpha")
    grad_bars({k: v.grad for k, v in lp.items()}, {k: v.grad for k, v in lo.items()}, f"{form} aa={aa}")


@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_alpha_only_loss(simt_lib, which):  # noqa: F811
    """Only the alpha image reaches the loss: the colour gradient arrives as None, the blend backward runs on dL/dalpha alone."""
    cam, sc = dense_scene() if which == "dense" else sparse_scene()
    (_, _, _, lp), (_, _, _, lo), _ = _both(simt_lib, cam, sc, "fused", False, "a")
    assert float(lp["opac"].grad.abs().max()) > 0
    grad_bars({k: v.grad for k, v in lp.items()}, {k: v.grad for k, v in lo.items()}, f"alpha only ({which})")
    assert float(lp["shs"].grad.abs().max()) == 0.0      # alpha does not depend on colour


def test_colour_only_loss_with_return_alpha_is_the_plain_call_bit_for_bit(simt_lib):  # noqa: F811
    cam, sc = dense_scene()
    w = weights(cam.image_height, cam.image_width)
    grads = []
    with package_on_the_cpu(simt_lib) as pkg:
        for ra in (True, False):
            lv = make_leaves(sc, "split")
            out, _ = render_pkg(pkg, cam, lv, "split", torch.tensor(BG), return_alpha=ra)
            loss_of(out[0], None, out[2], w, "cd").backward()
            grads.append({k: v.grad for k, v in lv.items()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


# ---- 3. per-pixel and learnable background ---------------------------------------------------------------------------------------------
def _bg_image(H, W, seed=9):
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("which,W,H", [("dense", 96, 80), ("sparse", 90, 70)])
def test_per_pixel_background_image_and_its_gradient(simt_lib, which, W, H):  # noqa: F811
    """90 x 70 is not a multiple of 16 and most of its pixels have no contributor: dL/dbg_image = dL/dC there (T_final = 1)."""
    cam, sc = dense_scene(W, H) if which == "dense" else sparse_scene(W, H)
    w = weights(H, W)
    B = _bg_image(H, W)
    runs = []
    with package_on_the_cpu(simt_lib) as pkg:
        for _ in range(2):
            lv, bgp = make_leaves(sc, "fused"), B.clone().requires_grad_(True)
            (color, radii, invd, alpha), _ = render_pkg(pkg, cam, lv, "fused", bgp)
            T = final_T_of(pkg, color, sc.P, H, W)
            loss_of(color, alpha, invd, w, "cad").backward()
            runs.append((color, alpha, lv, bgp, T))
        (c0, _, _), _ = render_pkg(pkg, cam, make_leaves(sc, "fused", grad=False), "fused", torch.zeros(3), return_alpha=False)
    color, alpha, lv, bgp, T = runs[0]
    assert torch.equal(alpha[0], 1.0 - T)
    image_bars(color, c0 + T[None] * B, "color over bg_image vs color(bg=0) + T bg_image")
    lo, bgo = make_leaves(sc, "fused"), B.clone().requires_grad_(True)
    co, ao, do, aux = render_oracle(cam, lo, "fused", bgo)
    loss_of(co, ao, do, w, "cad").backward()
    image_bars(color, co, "color over bg_image vs the composed oracle")
    assert bgp.grad.shape == B.shape and torch.equal(bgp.grad, T[None] * w[0])      # the fp32 product, bit for bit
    empty = aux["n_contrib"] == 0
    if which == "sparse":
        assert float(empty.float().mean()) > 0.4 and torch.equal(bgp.grad[:, empty], w[0][:, empty])
    grad_bars({k: v.grad for k, v in lv.items()}, {k: v.grad for k, v in lo.items()}, f"bg_image ({which})")
    grad_bars({"bg": bgp.grad}, {"bg": bgo.grad}, f"dL/dbg_image ({which})")
    assert torch.equal(bgp.grad, runs[1][3].grad)
    for k in lv:
        assert torch.equal(lv[k].grad, runs[1][2][k].grad), k


@pytest.mark.parametrize("which,W,H", [("dense", 96, 80), ("sparse", 90, 70)])
def test_uniform_background_gradient(simt_lib, which, W, H):  # noqa: F811
    cam, sc = dense_scene(W, H) if which == "dense" else sparse_scene(W, H)
    w = weights(H, W)
    runs = []
    with package_on_the_cpu(simt_lib) as pkg:
        for ra in (True, False, False):      # the background gradient does not depend on return_alpha
            lv, bgp = make_leaves(sc, "precomp"), torch.tensor(BG, requires_grad=True)
            out, _ = render_pkg(pkg, cam, lv, "precomp", bgp, return_alpha=ra)
            T = final_T_of(pkg, out[0], sc.P, H, W)
            loss_of(out[0], None, out[2], w, "cd").backward()
            runs.append((lv, bgp, T))
        lv0 = make_leaves(sc, "precomp")
        out0, _ = render_pkg(pkg, cam, lv0, "precomp", torch.tensor(BG), return_alpha=False)
        loss_of(out0[0], None, out0[2], w, "cd").backward()
    lv, bgp, T = runs[0]
    assert bgp.grad is not None and bgp.grad.shape == (3,) and bgp.grad.dtype == torch.float32
    bg_sum_bound(T, w[0], bgp.grad)
    for other in runs[1:]:
        assert torch.equal(bgp.grad, other[1].grad)
    for k in lv:      # asking for the background's gradient leaves the Gaussians' alone
        assert torch.equal(lv[k].grad, lv0[k].grad), k


def test_background_gradient_is_independent_of_the_lane_schedule(simt_lib, tmp_path):  # noqa: F811
    """SIMT_SCHEDULE shuffles wave interleaving and workgroup order: dL/dbg, dL/dbg_image and alpha are the same bits (no float atomics)."""
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, torch\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {os.path.join(ROOT, 'gaussian-splatting_amd')!r}]\n"
        "import test_composite_cpu as T\n"
        "cam, sc = T.sparse_scene(90, 70)\n"
        "w = T.weights(70, 90)\n"
        "res = []\n"
        "with T.package_on_the_cpu(sys.argv[1]) as pkg:\n"
        "    for bg in (torch.tensor(T.BG), T._bg_image(70, 90)):\n"
        "        bg.requires_grad_(True)\n"
        "        lv = T.make_leaves(sc, 'fused')\n"
        "        (c, r, d, a), _ = T.render_pkg(pkg, cam, lv, 'fused', bg)\n"
        "        T.loss_of(c, a, d, w).backward()\n"
        "        res += [bg.grad, a.detach(), lv['opac'].grad]\n"
        "torch.save(res, sys.argv[2])\n")
    outs = []
    for k, sched in enumerate([None, "5", "11"]):
        env = dict(os.environ)
        env.pop("SIMT_SCHEDULE", None)
        if sched is not None:
            env["SIMT_SCHEDULE"] = sched
        out = tmp_path / f"g{k}.pt"
        subprocess.run([sys.executable, str(script), simt_lib, str(out)], check=True, env=env, cwd=ROOT, timeout=900)
        outs.append(torch.load(out))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


# ---- 4. edges and plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [False, True])
def test_empty_scene(simt_lib, image):  # noqa: F811
    """P == 0: alpha = 0, color = B, dL/dbg* = dL/dC."""
    cam, sc = sparse_scene(90, 70, 10)
    H, W = 70, 90
    w = weights(H, W)
    lv = {k: v.detach()[:0].clone().requires_grad_(True) for k, v in make_leaves(sc, "precomp").items()}
    bg = (_bg_image(H, W) if image else torch.tensor(BG)).requires_grad_(True)
    with package_on_the_cpu(simt_lib) as pkg:
        (color, radii, invd, alpha), _ = render_pkg(pkg, cam, lv, "precomp", bg)
        loss_of(color, alpha, invd, w).backward()
    assert torch.equal(alpha, torch.zeros(1, H, W)) and torch.equal(invd, torch.zeros(1, H, W)) and radii.numel() == 0
    assert torch.equal(color, bg.detach() if image else bg.detach()[:, None, None].expand(3, H, W))
    if image:
        assert torch.equal(bg.grad, w[0])
    else:
        bg_sum_bound(torch.ones(H, W), w[0], bg.grad)
    assert all(v.grad is not None and v.grad.numel() == 0 for v in lv.values())


@pytest.mark.parametrize("image", [False, True])
def test_band_of_tile_rows(simt_lib, image):  # noqa: F811
    """tile_rows = (1, 3): pixel rows 16 .. 47.  Outputs and dL/dbg_image are zero outside the band and the full frame's bits inside it; dL/dbg is
    the band's share."""
    cam, sc = dense_scene(96, 80, 1500)
    H, W, rows = 80, 96, (16, 48)
    w = weights(H, W)
    res = []
    with package_on_the_cpu(simt_lib) as pkg:
        for band in ((1, 3), None):
            lv = make_leaves(sc, "fused")
            bg = (_bg_image(H, W) if image else torch.tensor(BG)).requires_grad_(True)
            (color, radii, invd, alpha), _ = render_pkg(pkg, cam, lv, "fused", bg, tile_rows=band)
            T = final_T_of(pkg, color, sc.P, H, W)
            loss_of(color, alpha, invd, w).backward()
            res.append((color, alpha, bg, T))
    (cb, ab, bgb, Tb), (cf, af, bgf, Tf) = [(c.detach(), a.detach(), b, T) for c, a, b, T in res]
    inside = torch.zeros(H, dtype=torch.bool)
    inside[rows[0]:rows[1]] = True
    assert float(ab[0, ~inside].abs().max()) == 0.0 and float(cb[:, ~inside].abs().max()) == 0.0
    assert torch.equal(ab[:, inside], af[:, inside]) and torch.equal(cb[:, inside], cf[:, inside]) and float(ab.max()) > 0.5
    if image:
        assert float(bgb.grad[:, ~inside].abs().max()) == 0.0 and torch.equal(bgb.grad[:, inside], bgf.grad[:, inside])
        assert torch.equal(bgb.grad[:, inside], (Tf[None] * w[0])[:, inside])
    else:
        bg_sum_bound(Tf, w[0], bgb.grad, rows)
        assert not torch.equal(bgb.grad, bgf.grad)


def test_inference_build_writes_alpha(simt_lib):  # noqa: F811
    cam, sc = dense_scene(96, 80, 1500)
    with package_on_the_cpu(simt_lib) as pkg:
        with torch.no_grad():
            (c0, r0, d0, a0), _ = render_pkg(pkg, cam, make_leaves(sc, "fused", grad=False), "fused", torch.tensor(BG))
        (c1, r1, d1, a1), _ = render_pkg(pkg, cam, make_leaves(sc, "fused"), "fused", torch.tensor(BG))
    assert not a0.requires_grad and a0.grad_fn is None and a1.requires_grad
    assert torch.equal(a0, a1.detach()) and torch.equal(c0, c1.detach()) and 0.5 < float(a0.mean()) < 1.0


@pytest.mark.parametrize("shape", [(4,), (3, 1), (3, 80, 95), (1, 80, 96), (3, 80 * 96)])
def test_bad_background_shape_raises(simt_lib, shape):  # noqa: F811
    cam, sc = dense_scene(96, 80, 100)
    with package_on_the_cpu(simt_lib) as pkg:
        with pytest.raises(pkg.GsrError, match="raster_settings.bg must have shape"):
            render_pkg(pkg, cam, make_leaves(sc, "fused"), "fused", torch.zeros(shape))


def test_silhouette_loss_with_camera_gradients(simt_lib):  # noqa: F811
    """The motivating use: an alpha-only loss with the camera requiring grad.  Asking for the camera's gradient leaves the Gaussians' alone; the
    camera gradient is non-zero and reproducible."""
    cam, sc = dense_scene(96, 80, 1500)
    w = weights(80, 96)
    runs = []
    with package_on_the_cpu(simt_lib) as pkg:
        for cam_grad in (True, True, False):
            lv = make_leaves(sc, "fused")
            (color, radii, invd, alpha), S = render_pkg(pkg, cam, lv, "fused", torch.tensor(BG), cam_grad=cam_grad)
            loss_of(color, alpha, invd, w, "a").backward()
            runs.append((lv, (S.viewmatrix, S.projmatrix, S.campos)))
    (l1, c1), (l2, c2), (l3, c3) = runs
    for k in l1:
        assert torch.equal(l1[k].grad, l3[k].grad) and torch.equal(l1[k].grad, l2[k].grad), k
    for a, b in zip(c1, c2):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
    assert float(c1[0].grad.abs().max()) > 0 and float(c1[1].grad.abs().max()) > 0 and all(t.grad is None for t in c3)


def test_alpha_loss_with_the_fused_sh_adam_step(simt_lib):  # noqa: F811
    """fuse_sh_adam_into_backward combines with the composite blend backward: the two SH tensors are stepped in place exactly as with the plain
    blend backward followed by optimizer.step(), the other gradients are those of the unfused call."""
    cam, sc = dense_scene(96, 80, 1500)
    w = weights(80, 96)
    res = []
    with package_on_the_cpu(simt_lib) as pkg:
        for fuse in (True, False):
            lv = make_leaves(sc, "split")
            dc, rest = torch.nn.Parameter(lv.pop("dc").detach().clone()), torch.nn.Parameter(lv.pop("rest").detach().clone())
            lv.update(dc=dc, rest=rest)
            opt = torch.optim.Adam([{"params": [dc], "lr": 1e-2}, {"params": [rest], "lr": 1e-3}], eps=1e-15)
            handle = pkg.fuse_sh_adam_into_backward(opt, dc, rest) if fuse else None
            try:
                (color, radii, invd, alpha), _ = render_pkg(pkg, cam, lv, "split", torch.tensor(BG))
                loss_of(color, alpha, invd, w).backward()
                assert (dc.grad is None) == fuse
                opt.step()
            finally:
                if handle is not None:
                    handle.remove()
            res.append(lv)
    for k in ("means", "opac", "scales", "rot"):
        assert torch.equal(res[0][k].grad, res[1][k].grad), k
    for k in ("dc", "rest"):
        assert torch.allclose(res[0][k].detach(), res[1][k].detach(), rtol=0, atol=1e-6), k
        assert not torch.equal(res[0][k].detach(), make_leaves(sc, "split")[k].detach())


def test_default_call_does_not_touch_the_composite_entry_points(simt_lib):  # noqa: F811
    cam, sc = dense_scene(96, 80, 300)
    w = weights(80, 96)
    with package_on_the_cpu(simt_lib) as pkg:
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        calls = []
        real_f, real_b = lib.gsr_rasterize_forward_composite, lib.gsr_backward_blend_composite
        with mock.patch.object(lib, "gsr_rasterize_forward_composite", lambda *a: (calls.append("f"), real_f(*a))[1]), \
                mock.patch.object(lib, "gsr_backward_blend_composite", lambda *a: (calls.append("b"), real_b(*a))[1]):
            lv = make_leaves(sc, "fused")
            out, _ = render_pkg(pkg, cam, lv, "fused", torch.tensor(BG), return_alpha=False)
            assert len(out) == 3
            loss_of(out[0], None, out[2], w, "cd").backward()
            assert calls == []
            out, _ = render_pkg(pkg, cam, make_leaves(sc, "fused"), "fused", torch.tensor(BG))      # alpha returned but not used by the loss
            loss_of(out[0], None, out[2], w, "cd").backward()
            assert calls == ["f"]
            out, _ = render_pkg(pkg, cam, make_leaves(sc, "fused"), "fused", torch.tensor(BG))
            loss_of(*[out[i] for i in (0, 3, 2)], w).backward()
            assert calls == ["f", "f", "b"]


def test_composite_argument_validation_without_gpu():
    """The new entry points refuse a NULL `extra`, and dL_dbg without scratch, before any device work (tests/test_abi_cpu.py's style)."""
    from diff_gaussian_rasterization import _lib
    from diff_gaussian_rasterization._lib import GsrRasterSettings, RESIZE_FN, CompositeOut, CompositeGrads
    if not os.path.exists(_lib.lib_path()):      # (as the fixture of tests/test_abi_cpu.py: the product library, cross-compiled)
        import importlib.util
        spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(ROOT, "gaussian-splatting_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    lib = _lib.load()
    nr = C.c_int32(-1)
    cb = RESIZE_FN(lambda u, n: None)
    s = GsrRasterSettings()
    s.image_width, s.image_height = 64, 64
    fake = 0x1000
    s.bg = s.viewmatrix = s.projmatrix = s.campos = fake
    s.tanfovx = s.tanfovy = 0.5
    s.sh_degree = 3
    fwd = lambda extra: lib.gsr_rasterize_forward_composite(C.byref(s), 1, 16, fake, fake, None, fake, fake, fake, None, cb, None, cb, None, cb,      # noqa: E731
                                                            None, fake, None, fake, C.byref(nr), extra, None)
    assert fwd(None) == -1 and b"GsrCompositeOut" in lib.gsr_last_error()
    # with `extra` the call goes on to the usual checks: here the geometry callback that returns NULL
    assert fwd(C.byref(CompositeOut(None, None))) == -3
    rec = C.c_void_p(0)
    bwd = lambda extra: lib.gsr_backward_blend_composite(C.byref(s), 1, 0, fake, fake, fake, fake, None, fake, C.byref(rec), extra, None)      # noqa: E731
    assert bwd(None) == -1 and b"GsrCompositeGrads" in lib.gsr_last_error()
    assert bwd(C.byref(CompositeGrads(None, None, None, fake, None))) == -1 and b"scratch" in lib.gsr_last_error()
    assert bwd(C.byref(CompositeGrads(None, None, None, fake, fake + 4))) == -1 and b"aligned" in lib.gsr_last_error()
    s.image_width = 0
    assert bwd(C.byref(CompositeGrads(None, None, None, None, None))) == -1 and b"image size" in lib.gsr_last_error()
    assert lib.gsr_composite_grad_scratch_bytes(1920, 1080) >= 3 * 8 and lib.gsr_composite_grad_scratch_bytes(1920, 1080) % 8 == 0
    assert lib.gsr_composite_grad_scratch_bytes(0, 0) == 0 and lib.gsr_abi_version() == 4


def test_multi_gpu_renderers_take_the_constant_background_detached():
    """parallel.py: behaviour unchanged.  A background that requires grad enters the band renderer detached (like the camera), a per-pixel
    background is refused wherever the C ABI would read three floats of it, and so are the alpha output and the background gradient together with
    grad_sync."""
    import diff_gaussian_rasterization as pkg
    from diff_gaussian_rasterization import parallel
    eye = torch.eye(4)
    rs = pkg.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.tensor(BG, requires_grad=True), 1.0, eye, eye * 2, 0, torch.zeros(3), False, False)
    d = parallel._camera_detached(rs)
    assert not d.bg.requires_grad and torch.equal(d.bg, rs.bg)
    img = rs._replace(bg=torch.zeros(3, 8, 8))
    with pytest.raises(pkg.GsrError, match="single-GPU rasterizer only"):
        pkg._make_settings(img, [], (0, 1))      # what hip_render_packed / hip_render_segments / the sharded backward call
    pkg._make_settings(img, [], None, bg_image=True)
    with pytest.raises(pkg.GsrError, match=r"must have shape \[3\] or \[3, 8, 8\]"):
        pkg._make_settings(rs._replace(bg=torch.zeros(3, 8, 9)), [], None, bg_image=True)


def test_grad_sync_refuses_the_composite_features(simt_lib):  # noqa: F811
    cam, sc = dense_scene(96, 80, 100)
    with package_on_the_cpu(simt_lib) as pkg:
        lv = make_leaves(sc, "fused")
        S = settings(pkg.GaussianRasterizationSettings, cam, torch.tensor(BG))
        args = (lv["means"], None, lv["shs"], None, lv["opac"], lv["scales"], lv["rot"], None)
        with pytest.raises(pkg.GsrError, match="grad_sync"):
            pkg.rasterize_gaussians(*args, S, (0, 5), lambda rec: None, return_alpha=True)
        with pytest.raises(pkg.GsrError, match="grad_sync"):
            pkg.rasterize_gaussians(*args, S._replace(bg=torch.tensor(BG, requires_grad=True)), (0, 5), lambda rec: None)
        with pytest.raises(pkg.GsrError):
            pkg.rasterize_gaussians(*args, S._replace(bg=torch.zeros(3, 80, 96)), (0, 5), lambda rec: None)
        out = pkg.rasterize_gaussians(*args, S, (0, 5), lambda rec: None)
        assert len(out) == 3
