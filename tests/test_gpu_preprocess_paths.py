"""The forward per-Gaussian kernel on the GPU: its hot instantiations (csrc/preprocess.hip GsrPreHot -- scales + rotations, a 16-coefficient SH
tensor fused or as dc / rest, a band of a quarter of the frame or more) against the generic one that `gsr_set_option("preprocess_generic", 1)`
forces, call form by call form: `torch.equal` on the image, the radii, the inverse depth, num_rendered and every array
`debug.forward_with_views` exposes; the gradients of one training-style call as well (the backward reads the forward's records).  The call
forms outside the hot set -- colors_precomp, cov3D_precomp, an SH tensor with M = 9, a band under a quarter of the frame -- must still take the
generic instantiation (test hook `debug_last_preprocess_path`: 1 generic, 2 hot) and are unchanged by the switch.
tests/test_simt_preprocess_paths_cpu.py is the same comparison of the kernel source on the CPU."""
import copy
import ctypes as C

import pytest
import torch

from helpers import O, make_camera, make_edge_scene, oracle_settings
from test_gpu_parity import gpu_settings

pytestmark = pytest.mark.gpu

GENERIC, HOT = 1, 2
DEV = "cuda:0"


def scene(P, W, H, seed=11):
    """P Gaussians of the edge scene (beyond the frustum, across the near plane, opacities under 1/255: culled lanes beside visible ones)."""
    cam = make_camera(W, H)
    sc = copy.copy(make_edge_scene(max(P, 8), cam, seed=seed))
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(sc, k, getattr(sc, k)[:P].contiguous())
    return cam, sc.to(DEV)


def forward(cam, sc, form, sh_degree=3, tile_rows=None):
    """debug.forward_with_views with the separate dc / rest form added (sh_dc of the settings record) -> {name: tensor}."""
    from diff_gaussian_rasterization import _f32c, _make_settings, _ptr, _rasterize_forward, _lib
    from diff_gaussian_rasterization.debug import _view
    lib = _lib.load()
    rs = gpu_settings(oracle_settings(cam, bg=torch.tensor([0.2, 0.4, 0.6]), sh_degree=sh_degree), torch.device(DEV))
    P, H, W = sc.P, int(rs.image_height), int(rs.image_width)
    shs, colors, scales, rotations, cov, dc, M = sc.shs, None, sc.scales, sc.rotations, None, None, 16
    if form == "split":
        dc, shs = sc.shs[:, :1].clone(), sc.shs[:, 1:].clone()      # (fresh allocations: 16-byte aligned, as the split form wants)
        assert dc.data_ptr() % 16 == 0 and shs.data_ptr() % 16 == 0
    elif form == "colors":
        shs, colors, M = None, torch.rand(P, 3, generator=torch.Generator().manual_seed(1)).to(DEV), 0
    elif form == "cov":
        cov, scales, rotations = O.compute_cov3d(sc.scales.cpu(), sc.rotations.cpu(), 1.0, torch.float32).to(DEV), None, None
    elif form == "m9":
        shs, M = sc.shs[:, :9].contiguous(), 9
    t = [_f32c(x) for x in (sc.means3D, shs, colors, sc.opacities, scales, rotations, cov)]
    keep = [dc]
    with torch.cuda.device(DEV):
        s = _make_settings(rs, keep, tile_rows, False)
        if dc is not None:
            s.sh_dc = dc.data_ptr()
        color = torch.zeros(3, H, W, dtype=torch.float32, device=DEV)
        invdepth = torch.zeros(1, H, W, dtype=torch.float32, device=DEV)
        radii = torch.empty(P, dtype=torch.int32, device=DEV)
        geom, binning, img, R = _rasterize_forward(s, P, M, t, color, invdepth, radii, torch.device(DEV), kinds=("state",) * 3)
        v = _lib.GsrForwardViews()
        _lib.check(lib.gsr_forward_views(P, R, W, H, _ptr(geom), _ptr(binning), _ptr(img), C.byref(v)), "gsr_forward_views")
        nt = ((W + 15) // 16) * ((H + 15) // 16)
        out = {"color": color, "invdepth": invdepth, "radii": radii, "R": torch.tensor([R]),
               "splats": _view(geom, v.splats, P * 64, torch.int32), "tiles_touched": _view(geom, v.tiles_touched, P * 4, torch.int32),
               "depth_order": _view(geom, v.depth_order, P * 4, torch.int32), "offsets": _view(geom, v.tile_scan, P * 4, torch.int32),
               "point_list": _view(binning, v.point_list, R * 4, torch.int32) if R > 0 else torch.empty(0, dtype=torch.int32),
               "ranges": _view(img, v.ranges, nt * 8, torch.int32), "final_T": _view(img, v.final_T, H * W * 4, torch.int32),
               "n_contrib": _view(img, v.n_contrib, H * W * 4, torch.int32)}
        out = {k: a.clone() for k, a in out.items()}
        if tile_rows is not None:      # the blend writes the band's pixel rows only: what lies outside is whatever the allocation held
            for k in ("final_T", "n_contrib"):
                out[k] = out[k].view(H, W)[tile_rows[0] * 16:min(tile_rows[1] * 16, H)].clone()
        torch.cuda.synchronize()
    return out


def took(path):
    from diff_gaussian_rasterization import _lib
    _lib.set_option("debug_last_preprocess_path", path)      # (raises GsrError when the most recent forward took the other one)


def both_ways(want_path, *args, **kw):
    from diff_gaussian_rasterization import _lib
    _lib.set_option("preprocess_generic", 0)
    auto = forward(*args, **kw)
    took(want_path)
    _lib.set_option("preprocess_generic", 1)
    try:
        forced = forward(*args, **kw)
        took(GENERIC)
    finally:
        _lib.set_option("preprocess_generic", 0)
    assert sorted(auto) == sorted(forced)
    for k in auto:
        assert torch.equal(auto[k], forced[k]), f"{k}: the two instantiations differ"
    return auto


@pytest.mark.parametrize("W,H", [(64, 48), (33, 17)])      # the second: no multiple of the 16 x 16 tile in either direction
@pytest.mark.parametrize("form", ["fused", "split"])
def test_hot_and_generic_instantiation_agree_bit_for_bit(form, W, H):
    for P in (1, 63, 64, 65, 255, 256, 257, 1000):      # the wave (64), workgroup (256) and last-block edges of the SH staging
        cam, sc = scene(P, W, H)
        out = both_ways(HOT, cam, sc, form)
        if P >= 255:
            assert int((out["radii"] > 0).sum()) > 0 and int((out["radii"] == 0).sum()) > 0, "the scene must mix visible and culled Gaussians"


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_hot_and_generic_instantiation_agree_at_every_sh_degree(degree):
    """sh_degree stays a run-time value of every instantiation."""
    for P, W, H in ((257, 64, 48), (1000, 33, 17)):
        cam, sc = scene(P, W, H)
        both_ways(HOT, cam, sc, "fused", sh_degree=degree)


def test_several_trips_of_the_grid_stride_loop_agree_bit_for_bit():
    """Every case above is one trip per wave.  preprocess_hot_grid = 2 makes the 1000 Gaussians two trips (the SH tile is reused), and a grid
    beyond the blocks (2040) is clamped to them."""
    from diff_gaussian_rasterization import _lib
    cam, sc = scene(1000, 64, 48)
    for form in ("fused", "split"):
        base = both_ways(HOT, cam, sc, form)
        for groups in (2, 2040):
            _lib.set_option("preprocess_hot_grid", groups)
            try:
                out = forward(cam, sc, form)
            finally:
                _lib.set_option("preprocess_hot_grid", 0)
            took(HOT)
            for k in base:
                assert torch.equal(base[k], out[k]), (form, groups, k)


def test_a_wide_band_is_hot_and_a_band_under_a_quarter_of_the_frame_stays_generic():
    """(tile_y1 - tile_y0) * 4 >= gy is the launcher's band test.  48 x 96 pixels = 6 tile rows: rows [1, 3) are a third of the frame, row
    [2, 3) a sixth (the 64 x 48 and 33 x 17 frames have 3 and 2 tile rows: no band of theirs is under a quarter)."""
    cam, sc = scene(1000, 48, 96)
    both_ways(HOT, cam, sc, "fused", tile_rows=(1, 3))
    both_ways(GENERIC, cam, sc, "fused", tile_rows=(2, 3))
    both_ways(GENERIC, cam, sc, "split", tile_rows=(2, 3))


@pytest.mark.parametrize("form,degree", [("colors", 3), ("cov", 3), ("m9", 2)])
def test_other_call_forms_still_take_the_generic_instantiation(form, degree):
    for P, W, H in ((257, 64, 48), (1000, 33, 17)):
        cam, sc = scene(P, W, H)
        both_ways(GENERIC, cam, sc, form, sh_degree=degree)


@pytest.mark.parametrize("form", ["fused", "split"])
def test_gradients_of_the_two_instantiations_agree_bit_for_bit(form):
    from diff_gaussian_rasterization import GaussianRasterizer, _lib
    cam, sc = scene(1000, 64, 48)
    rs = gpu_settings(oracle_settings(cam, bg=torch.tensor([0.2, 0.4, 0.6])), torch.device(DEV))
    g = torch.Generator().manual_seed(5)
    wc, wd = torch.randn(3, 48, 64, generator=g).to(DEV), torch.randn(1, 48, 64, generator=g).to(DEV)

    def run(generic, want):
        _lib.set_option("preprocess_generic", generic)
        try:
            L = {k: getattr(sc, k).detach().clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
            if form == "split":
                L["dc"], L["shs"] = (t.clone().requires_grad_(True) for t in (sc.shs[:, :1], sc.shs[:, 1:]))
            else:
                L["shs"] = sc.shs.detach().clone().requires_grad_(True)
            L["means2D"] = torch.zeros(sc.P, 3, device=DEV, requires_grad=True)
            col, radii, invd = GaussianRasterizer(raster_settings=rs)(**L)
            took(want)
            ((col * wc).sum() + (invd * wd).sum()).backward()
            torch.cuda.synchronize()
        finally:
            _lib.set_option("preprocess_generic", 0)
        return col.detach(), radii, invd.detach(), {k: t.grad for k, t in L.items()}

    a, b = run(0, HOT), run(1, GENERIC)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert a[3][k] is not None and torch.equal(a[3][k], b[3][k]), f"dL/d{k} differs"
    assert float(a[3]["shs"].abs().max()) > 0 and float(a[3]["means3D"].abs().max()) > 0
