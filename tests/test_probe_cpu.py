"""Per-pixel probe (gsr_pixel_probe, `pixel_probe`, `GaussianRasterizer.probe`) through the shipped package on the CPU: the SIMT build of the whole library
behind the package's own loader, as in tests/test_contrib_cpu.py, whose scenes these are.  Reference and bars: tests/probe_reference.py.

Scenes: the dense 100 x 70 frame (partial tiles and partial 8x8 blocks on both axes, 3000 Gaussians, s_med 0.05, opacity logits raised by 3: terminating
pixels, lists over 128 entries) and the sparse 96 x 80 frame, most of whose pixels have no contributor.  None of its tiles has an empty range and only one
8x8 block has no contributor at all, so the two early exits that must still write the defaults are held to that on the isolated Gaussian of the
hand-computable frames as well (tests/probe_reference.py: most of its 4 x 3 tiles are empty).

Test infrastructure: the product never loads the SIMT library."""
import ctypes as C
import math

import pytest
import torch

from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import probe_reference as R
import test_composite_cpu as T
import test_contrib_cpu as TC

W, H = TC.W, TC.H
DEFAULTS = (0.0, 0.0, -1, -1, 0.0, 0)


def standalone(pkg, S, lv, form, tile_rows=None, **kw):
    rast = pkg.GaussianRasterizer(S)
    if tile_rows is not None:
        rast.tile_rows = tile_rows
    geo = dict(cov3D_precomp=lv["cov"]) if form == "precomp" else dict(scales=lv["scales"], rotations=lv["rot"])
    return rast.probe(lv["means"], lv["opac"], **geo, **kw)


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_scenes_meet_the_input_condition():
    """Reference alone: fragile plus near pixels are under 1 % of the frame for every configuration the tests below compare."""
    for which, form, aa in [("dense", f, a) for f in ("fused", "precomp") for a in (False, True)] + [("sparse", "fused", False)]:
        aux, s0 = TC.oracle_aux(which, form, aa)
        for t in (0.5, 0.9):
            share = R.input_condition(R.reference(aux, s0, t), aux)
            R.parity_report(f"probe_input_{which}_{form}_aa{int(aa)}_t{t}", fragile_or_near_share=share)
            assert share < 0.01, (which, form, aa, t, share)


@pytest.mark.parametrize("form", ["fused", "precomp"])
@pytest.mark.parametrize("aa", [False, True])
def test_dense_frame_with_termination(simt_lib, form, aa):
    aux, s0 = TC.oracle_aux("dense", form, aa)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "dense", form, aa)
        got = {t: pkg.pixel_probe(out[0].clamp(0.0, 1.0), t) for t in (0.5, 0.9)}
        default = pkg.pixel_probe(out[0])
        alone, radii = standalone(pkg, S, lv, form, threshold=0.9)
    for t in (0.5, 0.9):
        nums = R.check(f"probe_cpu_dense_{form}_aa{int(aa)}_t{t}", got[t], R.reference(aux, s0, t), aux)
        # termination and several batches of 64 are exercised (the antialiasing factor lowers every opacity: few pixels terminate there)
        assert nums["terminated_share"] > (0.001 if aa else 0.02) and nums["longest_list"] > 128
        assert nums["with_median"] > 1000
    assert equal(default, got[0.5]) and equal(alone, got[0.9]) and torch.equal(radii, out[1])
    # the threshold moves the median only
    assert all(torch.equal(got[0.5][i], got[0.9][i]) for i in (0, 3, 4, 5)) and not torch.equal(got[0.5].median_id, got[0.9].median_id)
    assert int((got[0.5].median_id != got[0.5].top_id).sum()) > 100


GARBAGE = ((7.5, torch.float32), (-3.25, torch.float32), (12345, torch.int32), (-777, torch.int32), (1e30, torch.float32), (99, torch.int32))


def through_the_c_abi(pkg, rendered, S, threshold=0.5):
    """gsr_pixel_probe on the state behind `rendered`, onto arrays prefilled with garbage; and once more with a single output (every one is optional)."""
    from diff_gaussian_rasterization import _lib
    st = pkg._saved_state(rendered, "pixel_probe", "probe")
    keep = []
    s = pkg._make_settings(S, keep, None, bg_image=True)
    shape = (int(S.image_height), int(S.image_width))
    raw = pkg.PixelProbe(*[torch.full(shape, v, dtype=dt) for v, dt in GARBAGE])
    only = torch.full(shape, 55, dtype=torch.int32)
    for rec in (_lib.PixelProbeOut(*[t.data_ptr() for t in raw], threshold, 0), _lib.PixelProbeOut(None, None, None, None, None, only.data_ptr(), threshold, 0)):
        assert _lib.load().gsr_pixel_probe(C.byref(s), st.P, st.fwd.num_rendered, pkg._ptr(st.fwd.geom), pkg._ptr(st.fwd.binning), pkg._ptr(st.fwd.img),
                                           C.byref(rec), None) == 0
    assert torch.equal(only, raw.count)
    return raw


def test_sparse_frame_and_every_pixel_is_written(simt_lib):
    """Through the C ABI onto arrays prefilled with garbage: pixels nobody contributes to hold exactly the defaults, 8x8 blocks without any contributor (the
    walk is skipped) included."""
    aux, s0 = TC.oracle_aux("sparse")
    ref = R.reference(aux, s0, 0.5)
    with package_on_the_cpu(simt_lib) as pkg:
        out, lv, S = TC.render(pkg, "sparse")
        got = pkg.pixel_probe(out[0])
        raw = through_the_c_abi(pkg, out[0], S)
    R.check("probe_cpu_sparse", got, ref, aux)
    assert equal(raw, got)
    empty = (aux["n_contrib"] == 0) & ~aux["fragile"]
    assert float(empty.float().mean()) > 0.3
    blocks = aux["n_contrib"].reshape(10, 8, 12, 8).amax(dim=(1, 3))
    assert int((blocks == 0).sum()) >= 1      # (a block whose largest n_contrib is 0; the next test has many)
    for t, v in zip(raw, DEFAULTS):
        assert bool((t[empty] == v).all())


def test_tiles_with_an_empty_range_are_written(simt_lib):
    """The isolated Gaussian of the hand-computable frames touches a few of the 4 x 3 tiles: the others have an empty range and still get the defaults."""
    cam, lv = R.hand_frame("isolated")
    s0 = TC.O.settings_from_camera(cam, torch.zeros(3), 3, 1.0, False)
    colors = torch.rand(2, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        aux = TC.O.rasterize(lv["means"], None, lv["opac"], s0, colors_precomp=colors, scales=lv["scales"], rotations=lv["rot"], return_aux=True)[3]
    ranges = aux["ranges"]
    empty_tiles = ranges[:, 1] == ranges[:, 0]
    assert 0 < int(empty_tiles.sum()) < 12
    # ... and in the tiles it touches, 8x8 blocks that nobody contributes to: the other way past the walk
    blocks = aux["n_contrib"].reshape(6, 8, 8, 8).amax(dim=(1, 3))
    assert int(((blocks == 0) & ~empty_tiles.reshape(3, 4).repeat_interleave(2, 0).repeat_interleave(2, 1)).sum()) > 0
    with package_on_the_cpu(simt_lib) as pkg:
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        out = pkg.GaussianRasterizer(S)(means3D=lv["means"].clone().requires_grad_(True), means2D=None, opacities=lv["opac"], colors_precomp=colors,
                                        scales=lv["scales"], rotations=lv["rot"])
        raw = through_the_c_abi(pkg, out[0], S)
        got = pkg.pixel_probe(out[0])
    assert equal(raw, got)
    for t in range(12):
        ty, tx = divmod(t, 4)
        if bool(empty_tiles[t]):
            for a, v in zip(raw, DEFAULTS):
                assert bool((a[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] == v).all())
    assert int(raw.top_id[R.HAND_PY, R.HAND_PX]) == 1


def test_hand_computable_frames(simt_lib):
    with package_on_the_cpu(simt_lib) as pkg:
        for which, check in (("isolated", R.check_isolated), ("layers", R.check_layers)):
            cam, lv = R.hand_frame(which)
            rast = pkg.GaussianRasterizer(T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3)))
            check(lambda t: rast.probe(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], threshold=t))


def test_counts_are_those_of_the_contribution_statistics_and_two_calls_agree(simt_lib):
    """An exact identity between two kernels: every (pixel, Gaussian) pair that contributes is counted once by each."""
    with package_on_the_cpu(simt_lib) as pkg:
        for which in ("dense", "sparse"):
            out, lv, S = TC.render(pkg, which)
            a = pkg.pixel_probe(out[0])
            stats = pkg.contribution_stats(out[0])
            b = pkg.pixel_probe(out[0] * 2.0)
            out2, _, _ = TC.render(pkg, which)
            c = pkg.pixel_probe(out2[0])
            assert int(a.count.sum()) == int(stats.pixel_count.sum()) > 0
            assert equal(a, b) and equal(a, c)
            # the Gaussians named by the id images contribute somewhere, and the top weight is at most the Gaussian's largest
            for ids in (a.top_id, a.median_id):
                assert bool((stats.pixel_count[ids[ids >= 0].long()] > 0).all())
            on = a.top_id >= 0
            assert bool((a.top_weight[on] <= stats.weight_max[a.top_id[on].long()]).all())


def test_band(simt_lib):
    band = (1, 3)
    aux, s0 = TC.oracle_aux("dense", band=band)
    with package_on_the_cpu(simt_lib) as pkg:
        full = pkg.pixel_probe(TC.render(pkg, "dense")[0][0], 0.9)
        out, lv, S = TC.render(pkg, "dense", tile_rows=band)
        got = pkg.pixel_probe(out[0], 0.9)
        alone, _ = standalone(pkg, S, lv, "fused", tile_rows=band, threshold=0.9)
    R.check("probe_cpu_band", got, R.reference(aux, s0, 0.9), aux)
    assert equal(got, alone)
    r0, r1 = band[0] * 16, band[1] * 16
    for g, f, v in zip(got, full, DEFAULTS):
        assert torch.equal(g[r0:r1], f[r0:r1])
        assert bool((g[:r0] == v).all()) and bool((g[r1:] == v).all())
    assert int((full.count[:r0] > 0).sum()) > 100 and int((full.count[r1:] > 0).sum()) > 100


def test_edge_and_error_cases(simt_lib):
    z3 = torch.zeros(0, 3)
    with package_on_the_cpu(simt_lib) as pkg:
        cam, sc = TC.scene("dense")
        S = T.settings(pkg.GaussianRasterizationSettings, cam, torch.zeros(3))
        rast = pkg.GaussianRasterizer(S)
        empty, radii = rast.probe(z3, torch.zeros(0, 1), scales=z3, rotations=torch.zeros(0, 4))
        assert radii.shape == (0,) and all(t.shape == (H, W) and bool((t == v).all()) for t, v in zip(empty, DEFAULTS))
        out, lv, _ = TC.render(pkg, "dense")
        before = pkg.pixel_probe(out[0])
        # a frame without a single instance (every Gaussian behind the camera)
        behind = lv["means"].detach() * torch.tensor([1.0, 1.0, -1.0])
        nothing, _ = rast.probe(behind, lv["opac"], scales=lv["scales"], rotations=lv["rot"])
        assert equal(nothing, empty)
        for bad in (0.0, 1.0, math.nan, -0.5, 1.5):
            with pytest.raises(pkg.GsrError, match="threshold"):
                pkg.pixel_probe(out[0], bad)
            with pytest.raises(pkg.GsrError, match="threshold"):
                rast.probe(lv["means"], lv["opac"], scales=lv["scales"], rotations=lv["rot"], threshold=bad)
        with pytest.raises(pkg.GsrError, match="no rasterizer call found"):
            pkg.pixel_probe(torch.rand(3, H, W, requires_grad=True) * 2.0)
        with pytest.raises(pkg.GsrError, match="no rasterizer call found"):
            pkg.pixel_probe(out[0].detach())
        out2, _, _ = TC.render(pkg, "dense")
        with pytest.raises(pkg.GsrError, match="2 rasterizer calls"):
            pkg.pixel_probe(out[0] + out2[0])
        out[0].sum().backward()
        with pytest.raises(pkg.GsrError, match="call pixel_probe before backward"):
            pkg.pixel_probe(out[0])
        out3, _, _ = TC.render(pkg, "dense")
        out3[0].sum().backward(retain_graph=True)
        assert equal(pkg.pixel_probe(out3[0]), before)
        assert {"PixelProbe", "pixel_probe"} <= set(pkg.__all__)
        assert not any(t.requires_grad for t in before)


def test_c_level_argument_checks(simt_lib):
    with package_on_the_cpu(simt_lib):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = _lib.GsrRasterSettings()
        s.image_width, s.image_height = 40, 40
        s.bg = s.viewmatrix = s.projmatrix = s.campos = 0x1000
        s.tanfovx = s.tanfovy = 0.5
        assert lib.gsr_pixel_probe(C.byref(s), 10, 0, None, None, None, None, None) == -1
        assert b"GsrPixelProbeOut" in lib.gsr_last_error()
        rec = _lib.PixelProbeOut(None, None, None, None, None, None, 0.5, 0)
        assert lib.gsr_pixel_probe(C.byref(s), 10, 5, None, 0x1000, 0x1000, C.byref(rec), None) == -1
        assert b"state buffers" in lib.gsr_last_error()
        assert lib.gsr_pixel_probe(C.byref(s), -1, 0, None, None, None, C.byref(rec), None) == -1
        assert lib.gsr_pixel_probe(C.byref(s), 10, -1, None, None, None, C.byref(rec), None) == -1
        assert lib.gsr_pixel_probe(None, 10, 0, None, None, None, C.byref(rec), None) == -1
        for bad in (0.0, 1.0, math.nan, -1.0, 2.0, math.inf):
            rec.threshold = bad
            assert lib.gsr_pixel_probe(C.byref(s), 10, 0, None, None, None, C.byref(rec), None) == -1
            assert b"threshold" in lib.gsr_last_error()
        # P == 0 / no instance: no state is needed, the defaults are written over the band and nowhere else
        for P, R_, band in ((0, 0, (0, 0)), (10, 0, (0, 0)), (0, 0, (1, 2))):
            arrays = [torch.full((40, 40), v, dtype=dt) for v, dt in
                      zip((7.5, -3.25, 12345, -777, 1e30, 99), (torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.int32))]
            garbage = [a.clone() for a in arrays]
            rec = _lib.PixelProbeOut(*[a.data_ptr() for a in arrays], 0.25, 0)
            s.tile_y0, s.tile_y1 = band
            assert lib.gsr_pixel_probe(C.byref(s), P, R_, None, None, None, C.byref(rec), None) == 0
            r0, r1 = (0, 40) if band == (0, 0) else (16, 32)
            for a, g, v in zip(arrays, garbage, DEFAULTS):
                assert bool((a[r0:r1] == v).all()) and torch.equal(a[:r0], g[:r0]) and torch.equal(a[r1:], g[r1:])
