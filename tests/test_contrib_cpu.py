"""Per-Gaussian blend-weight statistics (gsr_contribution_stats, `contribution_stats`, `GaussianRasterizer.contributions`) through the shipped package
on the CPU: the SIMT build of the whole library behind the package's own loader, as in tests/test_simt_package_cpu.py.  Reference and bars:
tests/contrib_reference.py.

Scenes: 100 x 70 (partial tiles and partial 8x8 blocks on both axes) with 3000 Gaussians, s_med 0.05, opacity logits raised by 3 -- a few percent of
the pixels terminate, the longest lists span several batches of 64, and some visible Gaussians contribute nowhere (the zero-row path); and the sparse
96 x 80 frame of tests/test_composite_cpu.py, most of whose tiles are empty (the early exits).

Test infrastructure: the product never loads the SIMT library."""
import ctypes as C
import functools

import pytest
import torch

from helpers import O, look_at_camera, make_camera, make_scene
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import contrib_reference as R
import test_composite_cpu as T

W, H = 100, 70


@functools.lru_cache(maxsize=None)
def scene(which):
    if which == "sparse":
        return T.sparse_scene()
    cam = make_camera(W, H) if which == "dense" else look_at_camera(W, H, (0.4, -0.3, -1.0), (0.0, 0.1, 4.0))
    sc = make_scene(3000, make_camera(W, H), seed=3, s_med=0.05)      # (the second view looks at the first view's scene)
    sc.opacities = R.raise_opacity(sc.opacities)
    return cam, sc


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


def weight(which, h, w, aux, seed=11):
    g = torch.Generator().manual_seed(seed)
    E = torch.rand(h, w, generator=g)
    if which == "masked":        # fragile pixels and a further random 10 % excluded
        E = R.mask_fragile(E, aux)
        E[torch.rand(h, w, generator=g) < 0.1] = 0.0
        return E
    if which == "signed":
        return R.mask_fragile(E - 0.3, aux)
    return R.mask_fragile(torch.ones(h, w), aux)


def render(pkg, which, form="fused", aa=False, tile_rows=None, return_alpha=False):
    cam, sc = scene(which)
    lv = T.make_leaves(sc, form)
    out, S = T.render_pkg(pkg, cam, lv, form, torch.zeros(3), aa, return_alpha=return_alpha, tile_rows=tile_rows)
    return out, lv, S


def standalone(pkg, S, lv, form, tile_rows=None, **kw):
    rast = pkg.GaussianRasterizer(S)
    if tile_rows is not None:
        rast.tile_rows = tile_rows
    geo = dict(cov3D_precomp=lv["cov"]) if form == "precomp" else dict(scales=lv["scales"], rotations=lv["rot"])
    return rast.contributions(lv["means"], lv["opac"], **geo, **kw)


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("form", ["fused", "precomp"])
@pytest.mark.parametrize("aa", [False, True])
def test_dense_frame_with_termination(simt_lib, form, aa):
    aux, s0 = oracle_aux("dense", form, aa)
    E = weight("masked", H, W, aux)
    ref = R.reference(aux, s0, E)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = render(pkg, "dense", form, aa)
        got = pkg.contribution_stats(out[0].clamp(0.0, 1.0), E)
        alone, radii = standalone(pkg, S, lv, form, pixel_weight=E[None])
    nums = R.check(f"contrib_cpu_dense_{form}_aa{int(aa)}", got, ref, aux)
    # termination and several batches of 64 are exercised (the antialiasing factor lowers every opacity: few pixels terminate there)
    assert nums["terminated_share"] > (0.001 if aa else 0.02) and nums["longest_list"] > 128
    visible = aux["radii"] > 0
    assert int((visible & (ref["pixel_count"] == 0)).sum()) > 20                # ... and the zero rows of visible Gaussians
    assert equal(got, alone) and torch.equal(radii, out[1])
    assert bool((radii[got.pixel_count > 0] > 0).all())


def test_sparse_frame(simt_lib):
    aux, s0 = oracle_aux("sparse")
    E = weight("ones", 80, 96, aux)
    ref = R.reference(aux, s0, E)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = render(pkg, "sparse")
        got = pkg.contribution_stats(out[0], E)
    R.check("contrib_cpu_sparse", got, ref, aux)
    assert float((aux["n_contrib"] == 0).float().mean()) > 0.3


def test_signed_weights(simt_lib):
    aux, s0 = oracle_aux("dense")
    E = weight("signed", H, W, aux)
    ref = R.reference(aux, s0, E)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = render(pkg, "dense")
        got = pkg.contribution_stats(out[0], E)
    R.check("contrib_cpu_signed", got, ref, aux, E_absmax=float(E.abs().max()))
    assert float(got.weight_sum.min()) < 0.0 and float(got.weight_max.min()) == 0.0
    assert bool(((got.weight_max == 0.0) & (got.weight_sum < 0.0) & (got.pixel_count > 0)).any())      # only negative pixels: the max ignores them


def test_no_weight_is_a_weight_of_ones_and_two_runs_agree(simt_lib):
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = render(pkg, "dense")
        a = pkg.contribution_stats(out[0])
        b = pkg.contribution_stats(out[0], torch.ones(H, W))
        c = pkg.contribution_stats(out[0] * 2.0)
        out2, _, _ = render(pkg, "dense")
        d = pkg.contribution_stats(out2[0])
    assert equal(a, b) and equal(a, c) and equal(a, d)
    assert int((a.pixel_count > 0).sum()) > 2000


def test_band(simt_lib):
    band = (1, 3)
    aux, s0 = oracle_aux("dense", band=band)
    full = R.reference(*oracle_aux("dense"))
    E = weight("masked", H, W, aux)
    ref = R.reference(aux, s0, E)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = render(pkg, "dense", tile_rows=band)
        got = pkg.contribution_stats(out[0], E)
        alone, _ = standalone(pkg, S, lv, "fused", tile_rows=band, pixel_weight=E)
    R.check("contrib_cpu_band", got, ref, aux)
    assert equal(got, alone)
    outside = (full["pixel_count"] > 0) & (ref["pixel_count"] == 0)
    assert int(outside.sum()) > 100
    assert float(got.weight_sum[outside].abs().max()) == 0.0 and float(got.weight_max[outside].max()) == 0.0 and int(got.pixel_count[outside].max()) == 0


def test_accumulate_over_two_views(simt_lib):
    with package_on_the_cpu(simt_lib) as pkg:
        out_a, _, _ = render(pkg, "dense")
        out_b, _, _ = render(pkg, "second")
        a, b = pkg.contribution_stats(out_a[0]), pkg.contribution_stats(out_b[0])
        acc = pkg.contribution_stats(out_a[0])
        back = pkg.contribution_stats(out_b[0], into=acc)
    assert back is acc
    assert int(((a.pixel_count > 0) & (b.pixel_count > 0)).sum()) > 500 and not torch.equal(a.pixel_count, b.pixel_count)
    assert torch.equal(acc.weight_sum, a.weight_sum + b.weight_sum)
    assert torch.equal(acc.weight_max, torch.maximum(a.weight_max, b.weight_max))
    assert torch.equal(acc.pixel_count, a.pixel_count + b.pixel_count)


def test_identities_against_the_product_itself(simt_lib):
    """With E = 1 the weights of a pixel telescope to its alpha; weight_sum is the colour gradient of sum E C_0."""
    g = torch.Generator().manual_seed(5)
    E = torch.rand(H, W, generator=g)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = render(pkg, "dense", "precomp", return_alpha=True)
        ones = pkg.contribution_stats(out[0])
        got = pkg.contribution_stats(out[0], E)
        (out[0][0] * E).sum().backward()
    alpha_total = float(out[3].detach().double().sum())
    assert abs(float(ones.weight_sum.double().sum()) - alpha_total) <= 1e-5 * alpha_total
    grad = lv["colors"].grad[:, 0].double()
    d = float((got.weight_sum.double() - grad).abs().max()) / float(grad.abs().max())
    R.parity_report("contrib_cpu_identities", sum_vs_alpha_rel=abs(float(ones.weight_sum.double().sum()) - alpha_total) / alpha_total, sum_vs_dcolor_rel_max=d)
    assert d < 1e-5
    assert bool((out[1][ones.pixel_count > 0] > 0).all())


def test_edge_and_error_cases(simt_lib):
    z3 = torch.zeros(0, 3)
    with package_on_the_cpu(simt_lib) as pkg:
        cam, sc = scene("dense")
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        rast = pkg.GaussianRasterizer(S)
        empty, radii = rast.contributions(z3, torch.zeros(0, 1), scales=z3, rotations=torch.zeros(0, 4))
        assert all(t.shape == (0,) for t in empty) and radii.shape == (0,)
        out, lv, _ = render(pkg, "dense")
        keepers = pkg.contribution_stats(out[0])
        before = tuple(t.clone() for t in keepers)
        # a frame without a single instance (every Gaussian behind the camera): zeros, or `into` left as it is
        behind = lv["means"].detach() * torch.tensor([1.0, 1.0, -1.0])
        nothing, _ = rast.contributions(behind, lv["opac"], scales=lv["scales"], rotations=lv["rot"])
        assert all(float(t.abs().max()) == 0.0 for t in nothing)
        rast.contributions(behind, lv["opac"], scales=lv["scales"], rotations=lv["rot"], into=keepers)
        assert equal(keepers, before)
        with pytest.raises(pkg.GsrError, match="no rasterizer call found"):
            pkg.contribution_stats(torch.rand(3, H, W, requires_grad=True) * 2.0)
        with pytest.raises(pkg.GsrError, match="no rasterizer call found"):
            pkg.contribution_stats(out[0].detach())
        out2, _, _ = render(pkg, "dense")
        with pytest.raises(pkg.GsrError, match="2 rasterizer calls"):
            pkg.contribution_stats(out[0] + out2[0])
        with pytest.raises(pkg.GsrError, match="pixel_weight must have shape"):
            pkg.contribution_stats(out[0], torch.ones(W, H))
        with pytest.raises(pkg.GsrError, match="pixel_weight must have shape"):
            pkg.contribution_stats(out[0], torch.ones(3, H, W))
        with pytest.raises(pkg.GsrError, match="into.pixel_count"):
            pkg.contribution_stats(out[0], into=pkg.ContributionStats(before[0], before[1], before[2].long()))
        out[0].sum().backward()
        with pytest.raises(pkg.GsrError, match="before backward"):
            pkg.contribution_stats(out[0])
        out3, _, _ = render(pkg, "dense")
        out3[0].sum().backward(retain_graph=True)
        assert equal(pkg.contribution_stats(out3[0]), before)


def test_c_level_argument_checks(simt_lib):
    with package_on_the_cpu(simt_lib):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = _lib.GsrRasterSettings()
        s.image_width, s.image_height = 64, 64
        s.bg = s.viewmatrix = s.projmatrix = s.campos = 0x1000
        s.tanfovx = s.tanfovy = 0.5
        assert lib.gsr_contribution_stats(C.byref(s), 10, 0, None, None, None, None, None, None, None) == -1
        assert b"GsrContribOut" in lib.gsr_last_error()
        rec = _lib.ContribOut(None, None, None, 0, 0)
        assert lib.gsr_contribution_stats(C.byref(s), 10, 5, 0x1000, 0x1000, 0x1000, None, None, C.byref(rec), None) == -1
        assert b"scratch" in lib.gsr_last_error()
        rec.accumulate = 2
        assert lib.gsr_contribution_stats(C.byref(s), 10, 0, None, None, None, None, None, C.byref(rec), None) == -1
        assert b"accumulate" in lib.gsr_last_error()
        assert lib.gsr_contribution_stats(None, 10, 0, None, None, None, None, None, C.byref(rec), None) == -1
        # four 16-byte slots and a flag word per instance, sized in 64 bits: past 2^31 bytes from 31.6 M instances on
        assert lib.gsr_contribution_scratch_bytes(1_000_000, 0) == 0
        assert lib.gsr_contribution_scratch_bytes(1_000_000, 8_000_000) >= 8_000_000 * 68
        assert lib.gsr_contribution_scratch_bytes(1_000_000, 40_000_000) >= 40_000_000 * 68 > 2 ** 31
        assert lib.gsr_contribution_scratch_bytes(10, 1000) % 128 == 0
