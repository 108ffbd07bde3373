"""Absolute screen-space gradients (gsr_backward_blend_abs, gsr_absgrad_from_records, `GaussianRasterizer(..., absgrad=True)`, `attach(absgrad=True)`)
through the shipped package on the CPU: the SIMT build of the whole library behind the package's own loader, as in tests/test_simt_package_cpu.py.
Reference and bars: tests/absgrad_reference.py.

Scenes (those of tests/test_contrib_cpu.py): 100 x 70 (partial tiles and partial half tiles on both axes) with 3000 Gaussians, s_med 0.05, opacity logits
raised by 3 -- lists over 128 entries, pixels that terminate, visible Gaussians that contribute nowhere --, its second view, and the sparse 96 x 80 frame
most of whose tiles are empty.

The cancellation case: the issue words it as "dL/dC antisymmetric about the centre" of one isotropic Gaussian on a pixel corner.  With an antisymmetric
dL/dC the per-pixel terms m (A dx + B dy) are SYMMETRIC (m and the offset both change sign) and nothing cancels; the terms are antisymmetric -- the case the
feature exists for, opposite per-pixel gradients under one Gaussian -- when dL/dC is symmetric about the centre.  The test uses that, with the issue's bound.

Test infrastructure: the product never loads the SIMT library."""
import functools
import types

import pytest
import torch

from helpers import O, look_at_camera, make_camera, make_scene
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import absgrad_reference as R
import contrib_reference as CR
import test_composite_cpu as T

W, H = 100, 70
CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def scene(which):
    if which == "sparse":
        return T.sparse_scene()
    if which == "corner":      # one isotropic Gaussian on the optical axis of a 32 x 32 frame: centre (15.5, 15.5), a pixel corner
        cam = make_camera(32, 32)
        sc = make_scene(1, cam, seed=1)
        sc.means3D = torch.tensor([[0.0, 0.0, 4.0]])
        sc.scales = torch.full((1, 3), 0.3)
        sc.rotations = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
        sc.opacities = torch.tensor([[0.8]])
        return cam, sc
    cam = make_camera(W, H) if which == "dense" else look_at_camera(W, H, (0.4, -0.3, -1.0), (0.0, 0.1, 4.0))
    sc = make_scene(3000, make_camera(W, H), seed=3, s_med=0.05)      # (the second view looks at the first view's scene)
    sc.opacities = CR.raise_opacity(sc.opacities)
    return cam, sc


def size(which):
    cam, _ = scene(which)
    return cam.image_height, cam.image_width


@functools.lru_cache(maxsize=None)
def oracle_aux(which, form="fused", aa=False, band=None):
    """aux (and settings) of the oracle's frame: computed once per configuration, shared by the tests, never modified."""
    cam, sc = scene(which)
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, aa)
    kw = T.call_kwargs(T.make_leaves(sc, form, grad=False), form, oracle=True)
    with torch.no_grad():
        if band is None:
            aux = O.rasterize(s=s0, want_fragile=True, return_aux=True, **kw)[3]
        else:
            aux = O.rasterize(s=s0, want_fragile=True, return_aux=True, tile_y0=band[0], tile_y1=band[1], **kw)[3]
    return aux, s0


def loss_weights(which, aux, seed=7):
    """(dL/dC [3,H,W], dL/dD [1,H,W], dL/dalpha-image [1,H,W]), zero at the fragile pixels."""
    h, w = size(which)
    g = torch.Generator().manual_seed(seed)
    return [R.mask_fragile(torch.rand(n, h, w, generator=g) - 0.3, aux) for n in (3, 1, 1)]


def oracle_means2D_grad(which, form, aa, wC, wD=None, wA=None, bg=None):
    """The oracle's own autograd gradient of means2D for the loss <color, wC> + <invdepth, wD> + <alpha, wA>, the colour over `bg` ([3,H,W]) composed as in
    tests/test_composite_cpu.py."""
    cam, sc = scene(which)
    lv = T.make_leaves(sc, form, grad=False)
    m2d = torch.zeros(sc.P, 3, requires_grad=True)
    s0 = O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, aa)
    kw = dict(T.call_kwargs(lv, form, oracle=True), means2D=m2d)
    color, _, invd = O.rasterize(s=s0, **kw)
    loss = (color * wC).sum()
    if wD is not None:
        loss = loss + (invd * wD).sum()
    if wA is not None or bg is not None:
        kw1 = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
        a = O.rasterize(s=s0, colors_precomp=torch.ones(sc.P, 3), **kw1)[0][:1]
        if bg is not None:
            loss = loss + ((1.0 - a) * bg * wC).sum()
        if wA is not None:
            loss = loss + (a * wA).sum()
    loss.backward()
    return m2d.grad


def run(pkg, which, form="fused", aa=False, absgrad=True, wC=None, wD=None, wA=None, bg=None, tile_rows=None, backward=True):
    """One render of the package with a means2D leaf and the backward of <color, wC> + <invdepth, wD> + <alpha, wA> -> (out, leaves incl. "m2d", settings)."""
    cam, sc = scene(which)
    lv = T.make_leaves(sc, form)
    lv["m2d"] = torch.zeros(sc.P, 3, requires_grad=True)
    S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3) if bg is None else bg, aa)
    rast = pkg.GaussianRasterizer(S, return_alpha=wA is not None, absgrad=absgrad)
    if tile_rows is not None:
        rast.tile_rows = tile_rows
    out = rast(**dict(T.call_kwargs(lv, form), means2D=lv["m2d"]))
    if backward:
        loss = (out[0] * wC).sum()
        if wD is not None:
            loss = loss + (out[2] * wD).sum()
        if wA is not None:
            loss = loss + (out[3] * wA).sum()
        loss.backward()
    return out, lv, S


def records(pkg, out, S, wC, wD, absgrad, tile_rows=None):
    """The [P,12] records of gsr_backward_blend / gsr_backward_blend_abs on the state the render's autograd node keeps (call before backward())."""
    fn = out[0].grad_fn
    saved = fn.saved_tensors
    geom, binning, img = saved[8:11]
    keep = []
    s = pkg._make_settings(S, keep, tile_rows, bg_image=True)
    rec = pkg._backward_blend(s, int(saved[0].shape[0]), pkg._Forward(geom, binning, img, fn.num_rendered), wC.contiguous(),
                              None if wD is None else wD.contiguous(), CPU, None, absgrad)
    return rec.clone()


def dominates(m2d, tol_rel=R.BAR):
    """absgrad + tol >= |grad| component-wise (a sum of absolute values against the absolute value of the sum)."""
    a, g = m2d.absgrad[:, :2].double(), m2d.grad[:, :2].double().abs()
    return bool((a + tol_rel * float(a.max()) >= g).all())


CONFIGS = [("dense", "fused", False, True), ("dense", "split", False, False), ("dense", "precomp", False, True), ("second", "fused", False, False),
           ("sparse", "fused", False, True), ("dense", "fused", True, True)]


@pytest.mark.parametrize("which,form,aa,depth", CONFIGS)
def test_absgrad_matches_the_reference(simt_lib, which, form, aa, depth):
    """Both SH forms and cov3D_precomp, antialiasing, with (HAS_DEPTH) and without an inverse-depth loss, three frames."""
    aux, s0 = oracle_aux(which, form, aa)
    wC, wD, _ = loss_weights(which, aux)
    wD = wD if depth else None
    ref = R.reference(aux, s0, wC, wD)
    R.check_signed(f"absgrad_cpu_reference_{which}_{form}_aa{int(aa)}_d{int(depth)}", ref, oracle_means2D_grad(which, form, aa, wC, wD))
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = run(pkg, which, form, aa, True, wC, wD)
    m2d = lv["m2d"]
    assert m2d.absgrad.shape == (aux["means2D"].shape[0], 3) and not m2d.absgrad.requires_grad
    nums = R.check(f"absgrad_cpu_{which}_{form}_aa{int(aa)}_d{int(depth)}", m2d.absgrad, m2d.grad, ref, aux)
    assert dominates(m2d)
    assert nums["cancellation"] < 0.9                     # the signed sums do cancel on these frames
    # zero rows: culled Gaussians and visible ones that contribute nowhere
    silent = ref["abs"].sum(1) == 0
    assert int((~(aux["radii"] > 0)).sum()) > 0 and int(((aux["radii"] > 0) & silent).sum()) > (20 if which == "dense" else 0)
    assert float(m2d.absgrad[silent].abs().max()) == 0.0
    if which == "dense" and not aa:
        assert int(aux["ranges"][:, 1].sub(aux["ranges"][:, 0]).max()) > 128      # lists of several batches (termination: tests/test_contrib_cpu.py)


def test_composite_terms(simt_lib):
    """return_alpha with a loss on the alpha image, over a per-pixel background: both reach m through T_final."""
    aux, s0 = oracle_aux("dense")
    wC, wD, wA = loss_weights("dense", aux)
    bg = torch.rand(3, H, W, generator=torch.Generator().manual_seed(9))
    ref = R.reference(aux, s0, wC, wD, wA, bg)
    plain = R.reference(aux, s0, wC, wD)
    R.check_signed("absgrad_cpu_reference_composite", ref, oracle_means2D_grad("dense", "fused", False, wC, wD, wA, bg))
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = run(pkg, "dense", wC=wC, wD=wD, wA=wA, bg=bg)
        out0, lv0, _ = run(pkg, "dense", absgrad=False, wC=wC, wD=wD, wA=wA, bg=bg)
    R.check("absgrad_cpu_composite", lv["m2d"].absgrad, lv["m2d"].grad, ref, aux)
    assert float((ref["abs"] - plain["abs"]).abs().max()) > 1e-3 * float(ref["abs"].max())      # the composite terms matter here
    for k in lv:
        assert torch.equal(lv[k].grad, lv0[k].grad), k
    assert not hasattr(lv0["m2d"], "absgrad") and dominates(lv["m2d"])


@pytest.mark.parametrize("depth", [False, True])
def test_on_and_off_agree_bit_for_bit_and_two_runs_agree(simt_lib, depth):
    aux, _ = oracle_aux("dense", "split")
    wC, wD, _ = loss_weights("dense", aux)
    wD = wD if depth else None
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv_on, S = run(pkg, "dense", "split", wC=wC, wD=wD, backward=False)
        rec_on, rec_off = records(pkg, out, S, wC, wD, True), records(pkg, out, S, wC, wD, False)
        loss = (out[0] * wC).sum()
        (loss if wD is None else loss + (out[2] * wD).sum()).backward()
        _, lv_off, _ = run(pkg, "dense", "split", absgrad=False, wC=wC, wD=wD)
        _, lv_again, _ = run(pkg, "dense", "split", wC=wC, wD=wD)
        from_rec = pkg._absgrad_from_records(pkg._make_settings(S, [], None, bg_image=True), rec_on.shape[0], rec_on, CPU)
    for k in lv_on:
        assert lv_on[k].grad is not None and torch.equal(lv_on[k].grad, lv_off[k].grad), k
        assert torch.equal(lv_on[k].grad, lv_again[k].grad), k
    assert torch.equal(rec_on[:, :10], rec_off[:, :10]) and float(rec_on[:, :10].abs().max()) > 0
    assert float(rec_off[:, 10:].abs().max()) == 0.0 and float(rec_on[:, 10:].min()) >= 0.0 and int((rec_on[:, 10] > 0).sum()) > 1000
    assert torch.equal(lv_on["m2d"].absgrad, lv_again["m2d"].absgrad) and torch.equal(lv_on["m2d"].absgrad, from_rec)
    assert torch.equal(from_rec[:, 0], rec_on[:, 10] * (0.5 * W)) and torch.equal(from_rec[:, 1], rec_on[:, 11] * (0.5 * H))
    assert not hasattr(lv_off["m2d"], "absgrad")
    if depth:
        assert float(rec_on[:, 9].abs().max()) > 0


def test_absgrad_is_overwritten_not_accumulated(simt_lib):
    aux, _ = oracle_aux("sparse")
    wC, _, _ = loss_weights("sparse", aux)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = run(pkg, "sparse", wC=wC, backward=False)
        (out[0] * wC).sum().backward(retain_graph=True)
        first, grad1 = lv["m2d"].absgrad, lv["m2d"].grad.clone()
        (out[0] * wC).sum().backward()
    assert lv["m2d"].absgrad is not first and torch.equal(lv["m2d"].absgrad, first) and float(first.max()) > 0
    assert torch.equal(lv["m2d"].grad, grad1 * 2)          # .grad accumulates as autograd does; .absgrad is the last backward's


def test_single_pixel_loss_pins_units_and_signs(simt_lib):
    """dL/dC is non-zero at one pixel: every Gaussian has one term, so absgrad = |grad| (summed moments against per-pixel products: 1e-5 of the maximum)."""
    aux, _ = oracle_aux("dense")
    ok = (~aux["fragile"]) & (aux["n_contrib"] > 20)
    ok[:, :10] = False
    y, x = [int(v) for v in ok.nonzero()[0]]
    wC = torch.zeros(3, H, W)
    wC[:, y, x] = torch.tensor([0.7, -0.4, 0.5])
    with package_on_the_cpu(simt_lib) as pkg:
        _, lv, _ = run(pkg, "dense", wC=wC)
    a, g = lv["m2d"].absgrad[:, :2].double(), lv["m2d"].grad[:, :2].double().abs()
    assert int((g.sum(1) > 0).sum()) > 10
    d = float((a - g).abs().max()) / float(g.max())
    R.parity_report("absgrad_cpu_single_pixel", abs_vs_grad_rel_max=d, gaussians=int((g.sum(1) > 0).sum()))
    assert d < R.BAR


def test_cancellation_under_one_gaussian(simt_lib):
    """One isotropic Gaussian centred on a pixel corner, dL/dC symmetric about its centre (module docstring): the per-pixel gradients cancel in pairs,
    |grad| < 1e-3 absgrad, and absgrad is the reference's."""
    aux, s0 = oracle_aux("corner", "precomp")
    assert torch.equal(aux["means2D"][0], torch.tensor([15.5, 15.5])) and float(aux["conic"][0, 1]) == 0.0 and aux["conic"][0, 0] == aux["conic"][0, 2]
    frag = aux["fragile"] | aux["fragile"].flip(0, 1)
    w = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(3)) - 0.3
    wC = w + w.flip(1, 2)
    wC[:, frag] = 0.0
    ref = R.reference(aux, s0, wC)
    w[:, frag] = 0.0      # (the reference is first validated on this frame with the generic weights)
    R.check_signed("absgrad_cpu_reference_corner", R.reference(aux, s0, w), oracle_means2D_grad("corner", "precomp", False, w))
    with package_on_the_cpu(simt_lib) as pkg:
        _, lv, _ = run(pkg, "corner", "precomp", wC=wC)
    a, g = lv["m2d"].absgrad[0, :2].double(), lv["m2d"].grad[0, :2].double().abs()
    R.parity_report("absgrad_cpu_cancellation", grad_over_absgrad_x=float(g[0] / a[0]), grad_over_absgrad_y=float(g[1] / a[1]))
    assert bool((g < 1e-3 * a).all()) and float(a.min()) > 0
    R.check("absgrad_cpu_corner", lv["m2d"].absgrad, None, ref, aux)


def test_bands_add_up(simt_lib):
    """The records of tile_rows (0, k) and (k, gy) add up to the full frame's (sums of non-negative terms over disjoint pixel sets): 1e-6 of the maximum."""
    aux, s0 = oracle_aux("dense")
    wC, wD, _ = loss_weights("dense", aux)
    k, gy = 2, (H + 15) // 16
    recs = []
    with package_on_the_cpu(simt_lib) as pkg:
        for band in (None, (0, k), (k, gy)):
            out, lv, S = run(pkg, "dense", wC=wC, wD=wD, tile_rows=band, backward=False)
            recs.append(records(pkg, out, S, wC, wD, True, band)[:, 10:].double())
            if band == (0, k):
                ((out[0] * wC).sum() + (out[2] * wD).sum()).backward()
                band_abs = lv["m2d"].absgrad
    full, lo, hi = recs
    d = float((lo + hi - full).abs().max()) / float(full.max())
    R.parity_report("absgrad_cpu_bands", sum_vs_full_rel_max=d)
    assert d < 1e-6 and float(lo.max()) > 0 and float(hi.max()) > 0 and int(((lo.sum(1) > 0) & (hi.sum(1) > 0)).sum()) > 20
    # ... and the band's contribution is the reference's for the band
    aux_b, _ = oracle_aux("dense", band=(0, k))
    ref = R.reference(aux_b, s0, wC, wD)
    d_band = float((band_abs[:, :2].double() - ref["abs"]).abs().max()) / float(ref["abs"].max())
    assert d_band < R.BAR, d_band


def test_empty_scene_and_error_cases(simt_lib):
    z3 = torch.zeros(0, 3)
    with package_on_the_cpu(simt_lib) as pkg:
        cam, sc = scene("dense")
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        rast = pkg.GaussianRasterizer(S, absgrad=True)
        m2d = torch.zeros(0, 3, requires_grad=True)
        out = rast(means3D=z3.clone().requires_grad_(True), means2D=m2d, opacities=torch.zeros(0, 1), colors_precomp=z3, scales=z3, rotations=torch.zeros(0, 4))
        out[0].sum().backward()
        assert m2d.absgrad.shape == (0, 3) and m2d.absgrad.dtype == torch.float32
        lv = T.make_leaves(sc, "fused")
        with pytest.raises(ValueError, match="absgrad=True needs a means2D"):
            rast(**T.call_kwargs(lv, "fused"))
        with pytest.raises(ValueError, match="absgrad=True needs a means2D"):
            rast(**dict(T.call_kwargs(lv, "fused"), means2D=torch.zeros(sc.P, 3)))
        args = (lv["means"], torch.zeros(sc.P, 3, requires_grad=True), lv["shs"], None, lv["opac"], lv["scales"], lv["rot"], None)
        with pytest.raises(RuntimeError, match="grad_sync") as err:
            pkg.rasterize_gaussians(*args, S, (0, 5), lambda rec: None, absgrad=True)
        assert isinstance(err.value, pkg.GsrError)
        assert len(pkg.rasterize_gaussians(*args, S, (0, 5), lambda rec: None)) == 3
        # a frame without a single instance (every Gaussian behind the camera): zero rows
        behind = (lv["means"].detach() * torch.tensor([1.0, 1.0, -1.0])).requires_grad_(True)
        m2 = torch.zeros(sc.P, 3, requires_grad=True)
        out = rast(means3D=behind, means2D=m2, opacities=lv["opac"], shs=lv["shs"], scales=lv["scales"], rotations=lv["rot"])
        out[0].sum().backward()
        assert m2.absgrad.shape == (sc.P, 3) and float(m2.absgrad.abs().max()) == 0.0


def test_c_level_argument_checks(simt_lib):
    import ctypes as C
    with package_on_the_cpu(simt_lib):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = _lib.GsrRasterSettings()
        s.image_width, s.image_height = 64, 64
        s.bg = s.viewmatrix = s.projmatrix = s.campos = 0x1000
        s.tanfovx = s.tanfovy = 0.5
        rec = C.c_void_p(0)
        assert lib.gsr_backward_blend_abs(C.byref(s), 0, 0, None, None, None, None, None, None, C.byref(rec), None, None) == 0      # P == 0, NULL extra
        assert lib.gsr_backward_blend_abs(C.byref(s), 4, 0, None, None, None, None, None, None, C.byref(rec), None, None) == -1
        assert b"NULL" in lib.gsr_last_error()
        assert lib.gsr_backward_blend_abs(None, 4, 0, None, None, None, None, None, None, C.byref(rec), None, None) == -1
        assert lib.gsr_absgrad_from_records(C.byref(s), 0, None, None, None) == 0
        assert lib.gsr_absgrad_from_records(C.byref(s), 4, None, None, None) == -1 and b"NULL" in lib.gsr_last_error()
        assert lib.gsr_absgrad_from_records(C.byref(s), 4, 0x1004, 0x1000, None) == -1 and b"aligned" in lib.gsr_last_error()
        assert lib.gsr_absgrad_from_records(C.byref(s), -1, 0x1000, 0x1000, None) == -1


def test_attach_feeds_absgrad_to_the_density_statistics():
    """A fake GaussianModel (the attributes attach() touches): xyz_gradient_accum grows by the norm of .absgrad, not of .grad."""
    from gsr_scene import densify
    P = 50
    g = torch.Generator().manual_seed(2)

    def model():
        return types.SimpleNamespace(optimizer=None, xyz_gradient_accum=torch.zeros(P, 1), denom=torch.zeros(P, 1), max_radii2D=torch.zeros(P))

    vsp = torch.zeros(P, 3, requires_grad=True)
    vsp.grad = torch.rand(P, 3, generator=g) - 0.5
    visible = torch.rand(P, generator=g) < 0.6
    on, off = densify.attach(model(), absgrad=True), densify.attach(model())
    with pytest.raises(RuntimeError, match=r"GaussianRasterizer\(raster_settings, absgrad=True\)"):
        on.add_densification_stats(vsp, visible)
    vsp.absgrad = vsp.grad.abs() * 3.0 + 1.0
    on.add_densification_stats(vsp, visible)
    off.add_densification_stats(vsp, visible)
    want = torch.zeros(P, 1)
    want[visible] = torch.norm(vsp.absgrad[visible, :2], dim=-1, keepdim=True)
    assert torch.equal(on.xyz_gradient_accum, want) and torch.equal(on.denom, visible.float()[:, None])
    assert torch.equal(off.denom, on.denom) and bool((off.xyz_gradient_accum[visible] < on.xyz_gradient_accum[visible]).all())
