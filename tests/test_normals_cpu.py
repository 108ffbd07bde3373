"""The normal-consistency regulariser without a GPU: tests/normals_reference.py pinned to cases worked out by hand, then the kernels of
csrc/normals.hip -- compiled for the host with the whole library (tests/simt) and called through the C ABI on guarded numpy buffers, and through
the gsr_normals package on the CPU -- against that reference.  Bars and input makers: tests/normals_reference.py."""
import ctypes as C
import math
import shutil

import numpy as np
import pytest
import torch

import normals_reference as NR
from test_mcmc_cpu import Guarded
from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# no interior; no interior; a single interior pixel; one ragged tile; one tile with ragged rows and a halo on the y axis; 3 x 5 tiles, ragged
IMAGE_SHAPES = [(1, 1), (2, 5), (3, 3), (5, 9), (37, 53), (70, 150)]
GAUSSIAN_SIZES = [0, 1, 63, 64, 65, 5000]
TX, TY = NR.TANFOV


def bits(t):
    return t.view(torch.int32)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------------
def test_reference_fronto_parallel_plane_faces_the_camera():
    nd = NR.depth_to_normal(torch.full((7, 9), 3.0, dtype=torch.float64), TX, TY)
    want = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)[:, None, None].expand(3, 5, 7)
    assert float((nd[:, 1:-1, 1:-1] - want).abs().max()) <= 1e-15
    border = torch.ones(7, 9, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert float(nd[:, border].abs().max()) == 0.0


@pytest.mark.parametrize("angles", [(0.3, 0.0), (-0.5, 0.0), (0.25, -0.35)])
def test_reference_tilted_plane_gives_the_analytic_normal(angles):
    """The plane through (0, 0, z0) with unit normal m = Ry(a) Rx(b) (0, 0, -1): a ray (rx, ry, 1) z meets it at z = m_z z0 / <m, (rx, ry, 1)>;
    differences of points of a plane lie in the plane, so every interior normal is m."""
    a, b = angles
    m = torch.tensor([-math.sin(a) * math.cos(b), math.sin(b), -math.cos(a) * math.cos(b)], dtype=torch.float64)
    H, W, z0 = 21, 33, 4.0
    rx = (((2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1) * TX)[None, :]
    ry = (((2 * torch.arange(H, dtype=torch.float64) + 1) / H - 1) * TY)[:, None]
    depth = m[2] * z0 / (m[0] * rx + m[1] * ry + m[2])
    assert float(depth.min()) > 0
    nd = NR.depth_to_normal(depth, TX, TY)[:, 1:-1, 1:-1]
    assert float((nd - m[:, None, None]).abs().max()) <= 1e-12
    # and the loss of the plane's own normal map is the share of border pixels
    loss = NR.normal_consistency_loss(depth, m[:, None, None].expand(3, H, W).contiguous(), TX, TY)
    assert float(loss) == pytest.approx(1.0 - (H - 2) * (W - 2) / (H * W), abs=1e-12)


def test_reference_flat_gaussian_faces_the_camera():
    s = torch.tensor([[1.0, 1.0, 0.1]], dtype=torch.float64)
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    eye = torch.eye(4, dtype=torch.float64)
    n = NR.gaussian_normals(s, q, torch.tensor([[0.0, 0.0, 5.0]], dtype=torch.float64), eye)
    assert torch.equal(n, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64))
    n = NR.gaussian_normals(s, q, torch.tensor([[0.0, 0.0, -5.0]], dtype=torch.float64), eye)
    assert torch.equal(n, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64))
    # lowest index on ties; the quaternion as given: |q| = 2 scales R's off-diagonal part, the normal is that column normalised
    ties = torch.tensor([[0.2, 0.2, 0.5], [0.5, 0.2, 0.2], [0.3, 0.3, 0.3], [0.5, 0.5, 0.1]], dtype=torch.float64)
    assert NR.smallest_axis(ties).tolist() == [0, 1, 0, 2]
    q2 = torch.tensor([[2.0, 0.0, 0.0, 0.0]], dtype=torch.float64)      # R = diag(1, 1, 1) for (w, 0, 0, 0) of any length
    assert torch.equal(NR.gaussian_normals(s, q2, torch.tensor([[0.0, 0.0, 5.0]], dtype=torch.float64), eye), torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64))


@pytest.mark.parametrize("shape", IMAGE_SHAPES + [(270, 480)])
def test_depth_maker_is_well_conditioned_everywhere(shape):
    H, W = shape
    if H < 3 or W < 3:
        return
    c = NR.conditioning(NR.make_depth(H, W, seed=H + W), TX, TY)
    print(f"[normals] conditioning {shape}: min |c| / (|du| |dv|) = {float(c.min()):.3f}", flush=True)
    assert float(c.min()) >= 0.05
    d = NR.make_depth(H, W, seed=H + W)
    assert 3.4 <= float(d.min()) and float(d.max()) <= 4.6


def test_sign_exemption_stays_under_its_cap():
    for P in GAUSSIAN_SIZES:
        _, _, compared = NR.gaussian_reference(P)
        exempt = int((~compared).sum())
        print(f"[normals] P {P}: {exempt} rows exempt (|n . p| / |p| < {NR.SIGN_EXEMPT:g})", flush=True)
        assert exempt <= NR.SIGN_EXEMPT_MAX * P


def test_no_bar_is_above_the_cap_that_rejects_the_textbook_form():
    """Differencing back-projected points in fp32 (2DGS's depth_to_normal) must miss the bar of the normal map at 270 x 480, where the
    difference form written in fp32 torch passes it: the cap is what tells the two apart."""
    assert max(NR.BARS.values()) <= 2e-6
    H, W = 270, 480
    depth = NR.make_depth(H, W, H + W)
    want = NR.depth_to_normal(depth.double(), TX, TY)
    nx = (((2 * torch.arange(W, dtype=torch.float32) + 1) / W - 1) * TX)[None, :]
    ny = (((2 * torch.arange(H, dtype=torch.float32) + 1) / H - 1) * TY)[:, None]
    pts = torch.stack([nx * depth, ny * depth, depth])
    c = torch.cross(pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1], pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2], dim=0)
    textbook = float((c / c.norm(dim=0, keepdim=True) - want[:, 1:-1, 1:-1]).abs().max())
    ours = float((NR.depth_to_normal(depth, TX, TY) - want).abs().max())
    print(f"[normals] 270 x 480 in fp32 torch: textbook form {textbook:.2e}, difference form {ours:.2e} (bar {NR.BARS['depth_normals']:.1e})", flush=True)
    assert textbook > NR.BARS["depth_normals"] >= ours


# ---- the kernels through the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(simt_lib):  # noqa: F811
    h = C.CDLL(simt_lib)
    h.gsr_last_error.restype = C.c_char_p
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    h.gsr_gaussian_normals.argtypes = [i] + [vp] * 6
    h.gsr_gaussian_normals_backward.argtypes = [i] + [vp] * 7
    h.gsr_depth_normals.argtypes = [i, i, f, f] + [vp] * 3
    h.gsr_depth_normals_backward.argtypes = [i, i, f, f] + [vp] * 4
    h.gsr_normal_loss_partial_count.restype, h.gsr_normal_loss_partial_count.argtypes = C.c_int64, [i, i]
    h.gsr_normal_loss.argtypes = [i, i, f, f] + [vp] * 6
    h.gsr_normal_loss_backward.argtypes = [i, i, f, f] + [vp] * 7
    return h


def unwritten(buf, t):
    return np.array_equal(buf.a.view(np.int32), t.numpy().view(np.int32))


def run_depth_normals(lib, depth, dL=None, offset=0):
    """-> Nd [3,H,W], dL/ddepth [H,W] (None without dL).  Every buffer is guarded; offset 4: base pointers 4 bytes off a 64-byte boundary."""
    H, W = depth.shape
    bz, bo = Guarded(depth.numpy(), offset), Guarded(np.full((3, H, W), 7.0, np.float32), offset)
    assert lib.gsr_depth_normals(H, W, TX, TY, bz.ptr, bo.ptr, None) == 0, lib.gsr_last_error()
    bufs, ddepth = [bz, bo], None
    if dL is not None:
        bd, bg = Guarded(dL.numpy(), offset), Guarded(np.full((H, W), 7.0, np.float32), offset)
        assert lib.gsr_depth_normals_backward(H, W, TX, TY, bz.ptr, bd.ptr, bg.ptr, None) == 0, lib.gsr_last_error()
        assert unwritten(bd, dL), "an input was written"
        bufs += [bd, bg]
        ddepth = torch.from_numpy(bg.a.copy())
    assert all(b.intact() for b in bufs), "the bytes around a buffer were overwritten"
    assert unwritten(bz, depth), "an input was written"
    return torch.from_numpy(bo.a.copy()), ddepth


def run_loss(lib, depth, normals, weight, dL_dloss=1.75, want="nd", offset=0):
    """-> loss (float32 scalar tensor), dL/dnormals, dL/ddepth (None where not in `want`)."""
    H, W = depth.shape
    count = lib.gsr_normal_loss_partial_count(H, W)
    assert count >= 1
    bz, bn = Guarded(depth.numpy(), offset), Guarded(normals.numpy(), offset)
    bw = Guarded(weight.numpy(), offset) if weight is not None else None
    bp, bl = Guarded(np.full(count, np.nan, np.float64)), Guarded(np.full(1, 7.0, np.float32), offset)
    bs = Guarded(np.full(1, dL_dloss, np.float32), offset)
    bgn = Guarded(np.full((3, H, W), 7.0, np.float32), offset) if "n" in want else None
    bgd = Guarded(np.full((H, W), 7.0, np.float32), offset) if "d" in want else None
    wp = bw.ptr if bw else None
    assert lib.gsr_normal_loss(H, W, TX, TY, bz.ptr, bn.ptr, wp, bp.ptr, bl.ptr, None) == 0, lib.gsr_last_error()
    assert lib.gsr_normal_loss_backward(H, W, TX, TY, bz.ptr, bn.ptr, wp, bs.ptr, bgn.ptr if bgn else None, bgd.ptr if bgd else None, None) == 0, \
        lib.gsr_last_error()
    assert all(b.intact() for b in (bz, bn, bw, bp, bl, bs, bgn, bgd) if b is not None), "the bytes around a buffer were overwritten"
    assert unwritten(bz, depth) and unwritten(bn, normals) and (bw is None or unwritten(bw, weight)), "an input was written"
    return (torch.from_numpy(bl.a.copy())[0], torch.from_numpy(bgn.a.copy()) if bgn else None, torch.from_numpy(bgd.a.copy()) if bgd else None)


def run_gaussians(lib, s, q, m, vm, dL=None, offset=0):
    P = s.shape[0]
    bs, bq, bm, bv = (Guarded(t.numpy(), offset) for t in (s, q, m, vm))
    bo = Guarded(np.full((P, 3), 7.0, np.float32), offset)
    assert lib.gsr_gaussian_normals(P, bs.ptr, bq.ptr, bm.ptr, bv.ptr, bo.ptr, None) == 0, lib.gsr_last_error()
    bufs, drot = [bs, bq, bm, bv, bo], None
    if dL is not None:
        bd, bg = Guarded(dL.numpy(), offset), Guarded(np.full((P, 4), 7.0, np.float32), offset)
        assert lib.gsr_gaussian_normals_backward(P, bs.ptr, bq.ptr, bm.ptr, bv.ptr, bd.ptr, bg.ptr, None) == 0, lib.gsr_last_error()
        bufs += [bd, bg]
        drot = torch.from_numpy(bg.a.copy())
    assert all(b.intact() for b in bufs), "the bytes around a buffer were overwritten"
    assert unwritten(bs, s) and unwritten(bq, q) and unwritten(bm, m) and unwritten(bv, vm), "an input was written"
    return torch.from_numpy(bo.a.copy()), drot


def compare_image(what, nd, ddepth_map, loss, gn, gz, H, W, seed, weighted):
    r_nd, r_dmap, r_loss, r_gz, r_gn = NR.image_reference(H, W, seed, weighted)
    return NR.check(what, {
        "Nd": (NR.rel_max(nd, r_nd) if r_nd.abs().max() > 0 else float(nd.abs().max()), "depth_normals"),
        "ddepth(map)": (NR.rel_max(ddepth_map, r_dmap), "depth_grad"),
        "loss": (abs(float(loss) - r_loss) / r_loss, "loss"),
        "ddepth(loss)": (NR.rel_max(gz, r_gz), "depth_grad"),
        "dnormals": (NR.rel_max(gn, r_gn), "normal_grad")})


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", IMAGE_SHAPES)
def test_image_kernels_are_the_reference(lib, shape, weighted):
    H, W = shape
    seed = H + W
    depth, normals, weight, dL = NR.image_case(H, W, seed, weighted)
    nd, dmap = run_depth_normals(lib, depth, dL)
    loss, gn, gz = run_loss(lib, depth, normals, weight)
    compare_image(f"host {shape} weight {weighted}", nd, dmap, loss, gn, gz, H, W, seed, weighted)
    if H < 3 or W < 3:
        assert float(loss) == 1.0 and float(nd.abs().max()) == 0.0 and float(gn.abs().max()) == 0.0 and float(gz.abs().max()) == 0.0
        assert float(dmap.abs().max()) == 0.0
    # one gradient alone: the same bits of that gradient; a second run: the same bits of everything
    loss_n, gn_only, none = run_loss(lib, depth, normals, weight, want="n")
    assert none is None and torch.equal(bits(gn_only), bits(gn)) and torch.equal(bits(loss_n), bits(loss))
    _, none, gz_only = run_loss(lib, depth, normals, weight, want="d")
    assert none is None and torch.equal(bits(gz_only), bits(gz))
    nd2, dmap2 = run_depth_normals(lib, depth, dL)
    assert torch.equal(bits(nd2), bits(nd)) and torch.equal(bits(dmap2), bits(dmap))
    run_loss(lib, depth, normals, weight, want="")      # no gradient asked for: nothing happens, nothing is touched


def test_image_kernels_with_base_pointers_off_alignment(lib):
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    nd, dmap = run_depth_normals(lib, depth, dL, offset=4)
    loss, gn, gz = run_loss(lib, depth, normals, weight, offset=4)
    compare_image("host offset 4", nd, dmap, loss, gn, gz, H, W, H + W, True)
    nd0, dmap0 = run_depth_normals(lib, depth, dL)
    loss0, gn0, gz0 = run_loss(lib, depth, normals, weight)
    assert torch.equal(bits(nd), bits(nd0)) and torch.equal(bits(dmap), bits(dmap0)) and torch.equal(bits(loss), bits(loss0))
    assert torch.equal(bits(gn), bits(gn0)) and torch.equal(bits(gz), bits(gz0))


def compare_gaussians(what, n, drot, P, seed=0):
    r_n, r_dq, compared = NR.gaussian_reference(P, seed)
    if P == 0:
        return {}
    return NR.check(what, {"n": (float((n.double() - r_n)[compared].abs().max()), "gaussian_normals"),
                           "drot": (float((drot.double() - r_dq)[compared].abs().max() / r_dq.abs().max()), "rotation_grad")})


@pytest.mark.parametrize("P", GAUSSIAN_SIZES)
def test_gaussian_kernels_are_the_reference(lib, P):
    s, q, m, vm, dL = NR.make_gaussians(P)
    n, drot = run_gaussians(lib, s, q, m, vm, dL)
    assert n.shape == (P, 3) and drot.shape == (P, 4)
    compare_gaussians(f"host P {P}", n, drot, P)
    if P >= 64:
        # the rows with NaN / inf in an input are zero rows, forward and backward; the others (the zero quaternion's too) are unit normals
        assert float(n[6:15].abs().max()) == 0.0 and float(drot[6:15].abs().max()) == 0.0
        rest = torch.cat([n[:6], n[15:]])
        assert float((rest.norm(dim=1) - 1).abs().max()) <= 1e-6
        assert float(n[5, 2]) > 0 and NR.smallest_axis(s[:5]).tolist() == [0, 0, 1, 0, 2]      # behind the camera: away from +z
    n4, drot4 = run_gaussians(lib, s, q, m, vm, dL, offset=4)
    assert torch.equal(bits(n4), bits(n)) and torch.equal(bits(drot4), bits(drot))


# ---- the non-finite contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [math.nan, math.inf, 0.0, -1.0])
def test_poisoned_depths_stay_in_their_neighbourhood(lib, poison):
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    nd, dmap = run_depth_normals(lib, depth, dL)
    loss, gn, gz = run_loss(lib, depth, normals, weight)
    spots = [(0, 0), (0, 20), (17, 29), (H - 1, W - 2), (16, 51)]      # a corner, two edges, the interior, next to the right edge
    bad = depth.clone()
    for y, x in spots:
        bad[y, x] = poison
    nd_b, dmap_b = run_depth_normals(lib, bad, dL)
    loss_b, gn_b, gz_b = run_loss(lib, bad, normals, weight)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    dist = torch.stack([(yy - y).abs() + (xx - x).abs() for y, x in spots]).amin(0)
    near1, near2 = dist <= 1, dist <= 2
    assert torch.equal(bits(nd_b)[:, ~near1], bits(nd)[:, ~near1]) and float(nd_b[:, near1].abs().max()) == 0.0
    assert torch.equal(bits(gn_b)[:, ~near1], bits(gn)[:, ~near1]) and float(gn_b[:, near1].abs().max()) == 0.0
    assert torch.equal(bits(dmap_b)[~near2], bits(dmap)[~near2]) and torch.equal(bits(gz_b)[~near2], bits(gz)[~near2])
    for t in (nd_b, dmap_b, gn_b, gz_b, loss_b):
        assert bool(torch.isfinite(t).all())
    assert not torch.equal(bits(dmap_b)[near2], bits(dmap)[near2])


def test_nan_normals_where_nothing_is_compared(lib):
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    depth = depth.clone()
    depth[20, 30] = math.nan      # an invalid stencil in the interior as well
    nd, _ = run_depth_normals(lib, depth)
    off = (nd == 0).all(0) | (weight == 0)
    assert int(off.sum()) > 2 * (H + W) - 4 + 5 and bool((weight == 0)[1:-1, 1:-1].any())
    zeros, nans = normals.clone(), normals.clone()
    zeros[:, off] = 0.0
    nans[:, off] = math.nan
    a, b = run_loss(lib, depth, zeros, weight), run_loss(lib, depth, nans, weight)
    for x, y in zip(a, b):
        assert bool(torch.isfinite(y).all()) and torch.equal(bits(x), bits(y))
    assert float(b[1][:, off].abs().max()) == 0.0
    # the same through the map's backward: a NaN incoming gradient at a pixel whose Nd is zero goes nowhere
    dLn = dL.clone()
    dLn[:, (nd == 0).all(0)] = math.nan
    _, g0 = run_depth_normals(lib, depth, dL)
    _, g1 = run_depth_normals(lib, depth, dLn)
    assert bool(torch.isfinite(g1).all()) and torch.equal(bits(g0), bits(g1))


def test_invalid_arguments_are_refused_before_any_launch(lib):
    H, W = 5, 9
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    bz, bn, bd = Guarded(depth.numpy()), Guarded(normals.numpy()), Guarded(dL.numpy())
    out, gz = Guarded(np.full((3, H, W), 7.0, np.float32)), Guarded(np.full((H, W), 7.0, np.float32))
    part, loss, one = Guarded(np.full(4, 7.0, np.float64)), Guarded(np.full(1, 7.0, np.float32)), Guarded(np.ones(1, np.float32))
    for h, w, tx, ty in ((0, W, TX, TY), (H, 0, TX, TY), (-1, W, TX, TY), (H, W, 0.0, TY), (H, W, TX, -1.0), (H, W, math.nan, TY), (H, W, TX, math.inf),
                         (1 << 16, 1 << 16, TX, TY)):
        assert lib.gsr_depth_normals(h, w, tx, ty, bz.ptr, out.ptr, None) < 0 and lib.gsr_last_error(), (h, w, tx, ty)
        assert lib.gsr_depth_normals_backward(h, w, tx, ty, bz.ptr, bd.ptr, gz.ptr, None) < 0
        assert lib.gsr_normal_loss(h, w, tx, ty, bz.ptr, bn.ptr, None, part.ptr, loss.ptr, None) < 0
        assert lib.gsr_normal_loss_backward(h, w, tx, ty, bz.ptr, bn.ptr, None, one.ptr, out.ptr, gz.ptr, None) < 0
    assert lib.gsr_normal_loss_partial_count(0, 5) == 0 and lib.gsr_normal_loss_partial_count(1 << 16, 1 << 16) == 0
    assert lib.gsr_normal_loss_partial_count(H, W) == 1 and lib.gsr_normal_loss_partial_count(70, 150) == 15
    assert lib.gsr_depth_normals(H, W, TX, TY, None, out.ptr, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_depth_normals(H, W, TX, TY, bz.ptr, None, None) == -1
    assert lib.gsr_depth_normals_backward(H, W, TX, TY, bz.ptr, None, gz.ptr, None) == -1
    assert lib.gsr_normal_loss(H, W, TX, TY, bz.ptr, None, None, part.ptr, loss.ptr, None) == -1
    assert lib.gsr_normal_loss(H, W, TX, TY, bz.ptr, bn.ptr, None, None, loss.ptr, None) == -1
    assert lib.gsr_normal_loss_backward(H, W, TX, TY, bz.ptr, bn.ptr, None, None, out.ptr, gz.ptr, None) == -1
    s, q, m, vm, dLn = NR.make_gaussians(1)
    bs, bq, bm, bv = (Guarded(t.numpy()) for t in (s, q, m, vm))
    n = Guarded(np.full((1, 3), 7.0, np.float32))
    assert lib.gsr_gaussian_normals(-1, bs.ptr, bq.ptr, bm.ptr, bv.ptr, n.ptr, None) == -1
    assert lib.gsr_gaussian_normals(1, bs.ptr, None, bm.ptr, bv.ptr, n.ptr, None) == -1 and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_gaussian_normals(0, None, None, None, None, None, None) == 0      # P == 0: a no-op
    assert lib.gsr_gaussian_normals_backward(0, None, None, None, None, None, None, None) == 0
    assert all(bool((b.a == 7.0).all()) and b.intact() for b in (out, gz, part, loss, n))


# ---- through the package on the CPU -----------------------------------------------------------------------------------------------------------
def test_package_on_the_host_build(simt_lib, lib):  # noqa: F811
    import gsr_normals as GN
    from diff_gaussian_rasterization import GsrError
    H, W = 37, 53
    depth, normals, weight, dL = NR.image_case(H, W, H + W, True)
    s, q, m, vm, dLn = NR.make_gaussians(65)
    with package_on_the_cpu(simt_lib):
        z = depth.clone().requires_grad_(True)
        nd = GN.depth_to_normal(z, TX, TY)
        nd.backward(dL)
        want_nd, want_dmap = run_depth_normals(lib, depth, dL)
        assert torch.equal(bits(nd.detach()), bits(want_nd)) and torch.equal(bits(z.grad), bits(want_dmap))
        z, n = depth.clone().requires_grad_(True), normals.clone().requires_grad_(True)
        loss = GN.normal_consistency_loss(z, n, TX, TY, weight=weight)
        (1.75 * loss).backward()
        want_loss, want_gn, want_gz = run_loss(lib, depth, normals, weight, dL_dloss=1.75)
        assert loss.dim() == 0 and torch.equal(bits(loss.detach()), bits(want_loss))
        assert torch.equal(bits(n.grad), bits(want_gn)) and torch.equal(bits(z.grad), bits(want_gz))
        # each gradient only when it is asked for, without a weight as well
        z2 = depth.clone().requires_grad_(True)
        GN.normal_consistency_loss(z2, normals, TX, TY).backward()
        _, _, gz1 = run_loss(lib, depth, normals, None, dL_dloss=1.0, want="d")
        assert torch.equal(bits(z2.grad), bits(gz1))
        n2 = normals.clone().requires_grad_(True)
        GN.normal_consistency_loss(depth, n2, TX, TY, weight).backward()
        _, gn1, _ = run_loss(lib, depth, normals, weight, dL_dloss=1.0, want="n")
        assert torch.equal(bits(n2.grad), bits(gn1))
        # per-Gaussian: the gradient reaches rotations alone
        leaves = [t.clone().requires_grad_(True) for t in (s, q, m)]
        out = GN.gaussian_normals(leaves[0], leaves[1], leaves[2], vm)
        out.backward(dLn)
        want_n, want_drot = run_gaussians(lib, s, q, m, vm, dLn)
        assert torch.equal(bits(out.detach()), bits(want_n)) and torch.equal(bits(leaves[1].grad), bits(want_drot))
        assert leaves[0].grad is None and leaves[2].grad is None
        assert GN.gaussian_normals(s[:0], q[:0], m[:0], vm).shape == (0, 3)
        for call, msg in ((lambda: GN.depth_to_normal(depth[None], TX, TY), r"\(1, 37, 53\)"),
                          (lambda: GN.depth_to_normal(depth.double(), TX, TY), "float64"),
                          (lambda: GN.depth_to_normal(depth, 0.0, TY), "positive"),
                          (lambda: GN.depth_to_normal(depth, TX, -0.5), "positive"),
                          (lambda: GN.depth_to_normal(depth[:0], TX, TY), "empty"),
                          (lambda: GN.normal_consistency_loss(depth, normals[:2], TX, TY), r"\(2, 37, 53\)"),
                          (lambda: GN.normal_consistency_loss(depth, normals[:, :, :-1], TX, TY), r"\(3, 37, 52\)"),
                          (lambda: GN.normal_consistency_loss(depth, normals, TX, TY, weight[None]), r"\(1, 37, 53\)"),
                          (lambda: GN.normal_consistency_loss(depth, normals, math.nan, TY), "positive"),
                          (lambda: GN.normal_consistency_loss(depth.tolist(), normals, TX, TY), "list"),
                          (lambda: GN.gaussian_normals(s, q[:, :3], m, vm), r"\(65, 3\)"),
                          (lambda: GN.gaussian_normals(s, q, m[:64], vm), r"\(64, 3\)"),
                          (lambda: GN.gaussian_normals(s, q, m, vm[:3]), r"\(3, 4\)"),
                          (lambda: GN.gaussian_normals(s.half(), q, m, vm), "float16")):
            with pytest.raises(GsrError, match=msg):
                call()
    with pytest.raises(GsrError, match="must live on a HIP device"):      # the product has no CPU path
        GN.depth_to_normal(depth, TX, TY)
    meta = torch.empty(H, W, device="meta")
    with package_on_the_cpu(simt_lib):
        with pytest.raises(GsrError, match="normals on cpu"):      # mismatched devices
            GN.normal_consistency_loss(meta, normals, TX, TY)
