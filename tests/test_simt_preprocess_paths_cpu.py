"""The forward per-Gaussian kernel has one body and several compile-time call forms (csrc/preprocess.hip GsrPreForm): the launcher picks a
"hot" instantiation for scales + rotations, a 16-coefficient SH tensor (fused or dc / rest) and a band of a quarter of the frame or more, and
the generic one -- every condition tested at run time, the only form before -- for everything else.  `gsr_set_option("preprocess_generic", 1)`
forces the generic one.  Here, without a GPU: the whole library compiled for the host against the SIMT shim (tests/simt_build.build_library),
called through the C ABI as tests/test_simt_abi_cpu.py does; every call form runs both ways on the same small scene and EVERY array the forward
leaves -- image, inverse depth, radii, R, the 64-byte splat records, tiles_touched, depth order, tile scan, sorted point list, tile ranges,
final_T, n_contrib -- is compared byte for byte.  Which instantiation a call took is read back through the test hook
`debug_last_preprocess_path` (1 generic, 2 hot).  tests/test_gpu_preprocess_paths.py is the same comparison of the gfx950 code.

Test infrastructure: a checker of the kernel SOURCE; the product has no CPU path."""
import copy
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

from helpers import O, make_camera, make_edge_scene, oracle_settings
import test_simt_abi_cpu as A

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

GENERIC, HOT = 1, 2


@pytest.fixture(scope="module")
def lib():
    from simt_build import build_library
    h = C.CDLL(build_library())
    h.gsr_last_error.restype = C.c_char_p
    yield h
    h.gsr_set_option(b"preprocess_generic", 0)


def scene(P, W, H, seed=11):
    """P Gaussians of the edge scene (overscan beyond the frustum, depths across the near plane, opacities below 1/255: culled lanes next to
    visible ones in every wave) in front of a W x H camera."""
    cam = make_camera(W, H)
    sc = make_edge_scene(max(P, 8), cam, seed=seed)
    sc = copy.copy(sc)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(sc, k, getattr(sc, k)[:P].contiguous())
    return cam, sc


def aligned(a):
    """A copy of `a` at a 64-byte aligned address (the split SH form wants 16-byte aligned tensors; numpy promises that for no small array)."""
    raw = np.zeros(a.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    out = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def forward(lib, cam, sc, form, sh_degree=3, tile_rows=None):
    """One gsr_rasterize_forward in call form `form` -> {name: numpy array}, everything the forward leaves."""
    s = oracle_settings(cam, bg=torch.tensor([0.2, 0.4, 0.6]), sh_degree=sh_degree)
    keep = []
    rs = A.settings_of(s, keep, tile_rows)
    H, W, P = int(s.image_height), int(s.image_width), sc.P
    a = dict(means3D=A.f32(sc.means3D), opacities=A.f32(sc.opacities), scales=A.f32(sc.scales), rotations=A.f32(sc.rotations), shs=A.f32(sc.shs),
             colors=None, cov=None)
    M = 16
    if form == "split":
        dc = aligned(a["shs"][:, :1])
        a["shs"] = aligned(a["shs"][:, 1:])
        keep.append(dc)
        rs.sh_dc = A.ptr(dc).value
    elif form == "colors":
        a["shs"], a["colors"], M = None, A.f32(torch.rand(P, 3, generator=torch.Generator().manual_seed(1))), 0
    elif form == "cov":
        a["cov"] = A.f32(O.compute_cov3d(sc.scales, sc.rotations, 1.0, torch.float32))
        a["scales"] = a["rotations"] = None
    elif form == "m9":
        a["shs"], M = np.ascontiguousarray(a["shs"][:, :9]), 9
    (color, color_s), (invd, invd_s), (radii, radii_s) = A.guarded((3, H, W), np.float32), A.guarded((1, H, W), np.float32), A.guarded(P, np.int32)
    geom, binning, img = A.Buffer(), A.Buffer(), A.Buffer()
    nr = C.c_int32(0)
    rc = lib.gsr_rasterize_forward(C.byref(rs), P, M, A.ptr(a["means3D"]), A.ptr(a["shs"]), A.ptr(a["colors"]), A.ptr(a["opacities"]), A.ptr(a["scales"]),
                                   A.ptr(a["rotations"]), A.ptr(a["cov"]), geom.cb, None, binning.cb, None, img.cb, None, A.ptr(color), A.ptr(invd), A.ptr(radii),
                                   C.byref(nr), None)
    assert rc == 0, lib.gsr_last_error()
    A.guards_intact([("color", color_s), ("invdepth", invd_s), ("radii", radii_s), ("geom", geom.a), ("binning", binning.a), ("image state", img.a)])
    R = int(nr.value)
    v = A.Views()
    assert lib.gsr_forward_views(P, C.c_int64(R), W, H, A.ptr(geom.a), A.ptr(binning.a), A.ptr(img.a), C.byref(v)) == 0, lib.gsr_last_error()
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    out = {"color": color, "invdepth": invd, "radii": radii, "R": np.array([R]),
           "splats": geom.view(v.splats, P * 64, np.uint32).copy(), "tiles_touched": geom.view(v.tiles_touched, P * 4, np.int32).copy(),
           "depth_order": geom.view(v.depth_order, P * 4, np.int32).copy(), "tile_scan": geom.view(v.tile_scan, P * 4, np.int32).copy(),
           "point_list": binning.view(v.point_list, R * 4, np.int32).copy() if R else np.zeros(0, np.int32),
           "ranges": img.view(v.ranges, nt * 8, np.int32).copy(), "final_T": img.view(v.final_T, H * W * 4, np.uint32).copy(),
           "n_contrib": img.view(v.n_contrib, H * W * 4, np.int32).copy()}
    return out


def both_ways(lib, want_path, *args, **kw):
    """The call as the launcher decides it (must take `want_path`) and with preprocess_generic = 1: the same bytes in every array."""
    assert lib.gsr_set_option(b"preprocess_generic", 0) == 0
    auto = forward(lib, *args, **kw)
    assert lib.gsr_set_option(b"debug_last_preprocess_path", want_path) == 0, lib.gsr_last_error()
    assert lib.gsr_set_option(b"preprocess_generic", 1) == 0
    try:
        forced = forward(lib, *args, **kw)
        assert lib.gsr_set_option(b"debug_last_preprocess_path", GENERIC) == 0, lib.gsr_last_error()
    finally:
        lib.gsr_set_option(b"preprocess_generic", 0)
    assert sorted(auto) == sorted(forced)
    for k in auto:
        assert auto[k].tobytes() == forced[k].tobytes(), f"{k}: the two instantiations differ"
    return auto


SIZES = [(64, 48), (33, 17)]      # the second: no multiple of the 16 x 16 tile in either direction


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000])      # the wave (64), workgroup (256) and last-block edges of the SH staging
def test_hot_and_generic_instantiation_leave_the_same_bytes_fused_sh(lib, P, W, H):
    cam, sc = scene(P, W, H)
    out = both_ways(lib, HOT, cam, sc, "fused")
    if P >= 255:
        assert int((out["radii"] > 0).sum()) > 0 and int((out["radii"] == 0).sum()) > 0, "the scene must mix visible and culled Gaussians"


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_hot_and_generic_instantiation_leave_the_same_bytes_lower_sh_degrees(lib, degree):
    """sh_degree stays a run-time value of every instantiation (degree 3 is the case above)."""
    cam, sc = scene(257, 64, 48)
    both_ways(lib, HOT, cam, sc, "fused", sh_degree=degree)


@pytest.mark.parametrize("P,W,H", [(1, 33, 17), (65, 64, 48), (257, 33, 17), (1000, 64, 48)])
def test_hot_and_generic_instantiation_leave_the_same_bytes_separate_dc_and_rest(lib, P, W, H):
    cam, sc = scene(P, W, H)
    both_ways(lib, HOT, cam, sc, "split")


def test_a_wide_band_is_hot_and_a_band_under_a_quarter_of_the_frame_stays_generic(lib):
    """(tile_y1 - tile_y0) * 4 >= gy is the launcher's band test.  48 x 96 pixels = 6 tile rows: rows [1, 3) are a third of the frame, row
    [2, 3) a sixth (the 64 x 48 and 33 x 17 frames have 3 and 2 tile rows: no band of theirs is under a quarter)."""
    cam, sc = scene(257, 48, 96)
    both_ways(lib, HOT, cam, sc, "fused", tile_rows=(1, 3))
    both_ways(lib, GENERIC, cam, sc, "fused", tile_rows=(2, 3))
    both_ways(lib, GENERIC, cam, sc, "split", tile_rows=(2, 3))


@pytest.mark.parametrize("form,degree", [("colors", 3), ("cov", 3), ("m9", 2)])
def test_other_call_forms_still_take_the_generic_instantiation(lib, form, degree):
    cam, sc = scene(257, 64, 48)
    both_ways(lib, GENERIC, cam, sc, form, sh_degree=degree)


def test_the_switches_refuse_what_they_do_not_know(lib):
    assert lib.gsr_set_option(b"preprocess_generic", 2) != 0 and lib.gsr_set_option(b"preprocess_hot_grid", 2048) != 0
    assert lib.gsr_set_option(b"debug_last_preprocess_path", 0) != 0
    cam, sc = scene(300, 64, 48)
    base = forward(lib, cam, sc, "fused")
    for groups in (1, 2, 2040):      # any grid is the same frame (the trips are grid-stride); more workgroups than blocks are not launched
        assert lib.gsr_set_option(b"preprocess_hot_grid", groups) == 0
        try:
            out = forward(lib, cam, sc, "fused")
        finally:
            lib.gsr_set_option(b"preprocess_hot_grid", 0)
        assert lib.gsr_set_option(b"debug_last_preprocess_path", HOT) == 0
        for k in base:
            assert base[k].tobytes() == out[k].tobytes(), (groups, k)
