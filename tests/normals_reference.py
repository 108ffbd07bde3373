"""Per-Gaussian normals, the normals of a depth map and the normal-consistency loss, restated in torch on the CPU (fp64 unless the inputs
say otherwise), gradients by autograd.  include/gsr.h states the semantics; tests/test_normals_cpu.py pins this file to cases worked out by
hand and the kernels of csrc/normals.hip to this file; tests/test_gpu_normals.py does the latter on the device.

NUMERICS CONTRACT.  Pixel (x, y) has nx = (2 x + 1) / W - 1, ny = (2 y + 1) / H - 1 and the point p = (nx tanfovx z, ny tanfovy z, z) -- the
rasterizer's pixel centres (pix = ((ndc + 1) W - 1) / 2, centred principal point).  For an interior pixel (1 <= x <= W - 2, 1 <= y <= H - 2):
    dz = z(x+1, y) - z(x-1, y), sz = their sum;  dz' = z(x, y+1) - z(x, y-1), sz' = their sum
    du = (tanfovx (nx dz + (2 / W) sz),  ny tanfovy dz,  dz)
    dv = (nx tanfovx dz',  tanfovy (ny dz' + (2 / H) sz'),  dz')
    c = dv x du,   Nd = c / |c|                         (a fronto-parallel plane: (0, 0, -1); normals face the camera, 2DGS's orientation)
The depth differences are formed BEFORE any multiplication by the ray.  Nd = 0 at border pixels, where any of the five stencil depths (centre
included) is not a finite positive number, and where |c| is zero or not finite.  The gradient of the normalisation is (g - N <N, g>) / |c|;
validity, the border, the index k of the smallest scale and the sign of a Gaussian's normal carry none.
    loss = (1 / (H W)) sum_p [1 - w(p) <normals(p), Nd(p)>];  a pixel with Nd = 0 or w = 0 contributes exactly 1 whatever `normals` holds.

Per-Gaussian: k = the index of the smallest scale, the LOWEST index on exact ties (explicit comparisons below, not argmin); a = column k of
R(q), q as given; v = the view matrix's rotation applied to a; n = v / |v|, negated when <n, view-space mean> > 0; rows with a non-finite
input or |v| zero / non-finite are zero.

BARS.  Each bar is 4 x the largest error of the HOST build of the kernel source (tests/test_normals_cpu.py prints them; -ffp-contract=off)
against this file in fp64 over all shapes of the CPU test, the margin covering contraction and libm differences of the device build, and no
bar goes above 2e-6 -- which is what rejects differencing back-projected points (in fp32 torch on this file's depths: 2.8e-6 at 270 x 480, 2.0e-5 at
1080 x 1920, where the difference form stays at 1.0e-7 and 1.1e-7; tests/test_normals_cpu.py re-measures the first pair).  Normals and gradients are relative to
the largest reference magnitude of the tensor, the loss is relative.  No pixel is exempt.  Gaussian rows are exempt only where the fp64
|n . p| / |p| < 1e-4 (the sign is ambiguous there), at most 0.1 % of the rows."""
import functools
import math

import torch

TANFOV = (0.7, 0.45)
CAP = 2e-6
# the largest error of the host build over IMAGE_SHAPES / GAUSSIAN_SIZES of tests/test_normals_cpu.py (printed there as "[normals] ...")
MEASURED = {
    "depth_normals": 1.43e-7,     # |Nd - reference| (max |reference| is 1); at 70 x 150
    "depth_grad": 2.92e-7,        # dL/ddepth of depth_to_normal (1.85e-7) and of the loss (2.92e-7), relative to max |reference|
    "loss": 4.54e-8,              # relative; at 5 x 9
    "normal_grad": 2.03e-7,       # dL/dnormals of the loss, relative to max |reference|
    "gaussian_normals": 1.61e-7,  # |n - reference|; at P = 5000
    "rotation_grad": 2.64e-7,     # dL/drotations, relative to max |reference|; at P = 5000
}
BARS = {k: min(4.0 * v, CAP) for k, v in MEASURED.items()}
SIGN_EXEMPT = 1e-4
SIGN_EXEMPT_MAX = 0.001


# ---- the three functions --------------------------------------------------------------------------------------------------------------------------
def smallest_axis(scales):
    """[P] long: the index of the smallest scale, the lowest index on exact ties (NaN compares false and never wins)."""
    s0, s1, s2 = scales.unbind(1)
    k = torch.zeros(scales.shape[0], dtype=torch.long, device=scales.device)
    smin = s0
    take1 = s1 < smin
    k = torch.where(take1, torch.ones_like(k), k)
    smin = torch.where(take1, s1, smin)
    return torch.where(s2 < smin, torch.full_like(k, 2), k)


def rotation_matrix(q):
    """[P,3,3]: R(q) of the quaternion as given (w first), the matrix of csrc/gsr_math.h; not normalised."""
    r, x, y, z = q.unbind(1)
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
            [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
            [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]
    return torch.stack([torch.stack(row, dim=1) for row in rows], dim=1)


def gaussian_normals(scales, rotations, means3D, viewmatrix, return_margin=False):
    """-> [P,3] in the dtype of the inputs; differentiable in `rotations`.  return_margin: also |n . p| / |p| per row (inf on zero rows)."""
    finite = torch.isfinite(scales).all(1) & torch.isfinite(rotations).all(1) & torch.isfinite(means3D).all(1)
    dev = scales.device
    one = torch.ones((), dtype=scales.dtype, device=dev)
    q = torch.where(finite[:, None], rotations, torch.tensor([1.0, 0, 0, 0], dtype=rotations.dtype, device=dev).expand_as(rotations))
    s = torch.where(finite[:, None], scales.detach(), one)
    m = torch.where(finite[:, None], means3D.detach(), one)
    k = smallest_axis(s)
    a = rotation_matrix(q)[torch.arange(q.shape[0], device=dev), :, k]      # column k
    vm = viewmatrix.detach()
    v = a @ vm[:3, :3]                                            # v_i = sum_j vm[4 j + i] a_j
    p = m @ vm[:3, :3] + vm[3, :3]
    length = v.norm(dim=1)
    ok = finite & (length > 0) & torch.isfinite(length) & torch.isfinite(p).all(1)
    v = torch.where(ok[:, None], v, torch.tensor([0.0, 0, 1.0], dtype=v.dtype, device=dev).expand_as(v))
    n = v / v.norm(dim=1, keepdim=True)
    side = (n.detach() * p).sum(1)
    n = torch.where((side > 0)[:, None], -n, n)
    n = torch.where(ok[:, None], n, torch.zeros_like(n))
    if return_margin:
        margin = torch.where(ok, side.abs() / p.norm(dim=1), torch.full_like(side, math.inf))
        return n, margin
    return n


def _stencil(depth):
    """The five depths of every interior pixel with invalid depths replaced by 1, and the validity of the stencil."""
    good = torch.isfinite(depth) & (depth > 0)
    z = torch.where(good, depth, torch.ones_like(depth))
    c, l, r, u, d = z[1:-1, 1:-1], z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
    ok = good[1:-1, 1:-1] & good[1:-1, :-2] & good[1:-1, 2:] & good[:-2, 1:-1] & good[2:, 1:-1]
    return c, l, r, u, d, ok


def tangents(depth, tanfovx, tanfovy):
    """du, dv [3,H-2,W-2] of the interior pixels (the literal statement of the contract) and the validity of their stencils."""
    H, W = depth.shape
    dt, dev = depth.dtype, depth.device
    nx = ((2 * torch.arange(1, W - 1, dtype=dt, device=dev) + 1) / W - 1)[None, :]
    ny = ((2 * torch.arange(1, H - 1, dtype=dt, device=dev) + 1) / H - 1)[:, None]
    _, l, r, u, d, ok = _stencil(depth)
    dz, sz, dzy, szy = r - l, r + l, d - u, d + u
    du = torch.stack([tanfovx * (nx * dz + (2.0 / W) * sz), ny * tanfovy * dz, dz])
    dv = torch.stack([nx * tanfovx * dzy, tanfovy * (ny * dzy + (2.0 / H) * szy), dzy])
    return du, dv, ok


def depth_to_normal(depth, tanfovx, tanfovy):
    """depth [H,W] -> [3,H,W] in the dtype of depth; differentiable in depth."""
    H, W = depth.shape
    if H < 3 or W < 3:
        return torch.zeros(3, H, W, dtype=depth.dtype, device=depth.device)      # (every pixel is border)
    du, dv, ok = tangents(depth, tanfovx, tanfovy)
    c = torch.cross(dv, du, dim=0)
    length = c.norm(dim=0)
    ok = ok & (length > 0) & torch.isfinite(length)
    c = torch.where(ok[None], c, torch.tensor([0.0, 0, -1.0], dtype=c.dtype, device=c.device)[:, None, None].expand_as(c))
    n = torch.where(ok[None], c / c.norm(dim=0, keepdim=True), torch.zeros_like(c))
    return torch.nn.functional.pad(n, (1, 1, 1, 1))


def normal_consistency_loss(depth, normals, tanfovx, tanfovy, weight=None):
    """-> 0-dim; differentiable in depth and normals; weight is a constant."""
    nd = depth_to_normal(depth, tanfovx, tanfovy)
    w = torch.ones_like(depth) if weight is None else weight.detach()
    on = (nd.detach() != 0).any(0) & (w != 0)
    n = torch.where(on[None], normals, torch.zeros_like(normals))
    dot = torch.where(on, w * (n * nd).sum(0), torch.zeros_like(w))
    return (1.0 - dot).mean()


def conditioning(depth, tanfovx, tanfovy):
    """|c| / (|du| |dv|) of the interior pixels (fp64): the sine of the angle between the two tangents."""
    du, dv, _ = tangents(depth.double(), tanfovx, tanfovy)
    return torch.cross(dv, du, dim=0).norm(dim=0) / (du.norm(dim=0) * dv.norm(dim=0))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def make_depth(H, W, seed):
    """[H,W] fp32: a tilted plane around z = 4 plus a sinusoidal bump of amplitude 0.15 (4 +- 0.5 over the frame)."""
    g = torch.Generator().manual_seed(seed)
    a, b, ph = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1).tolist()
    u = ((torch.arange(W, dtype=torch.float64) + 0.5) / W * 2 - 1)[None, :]
    v = ((torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1)[:, None]
    z = 4.0 + 0.2 * a * u + 0.15 * b * v + 0.15 * torch.sin(2.2 * u + 3.0 * ph) * torch.cos(1.7 * v - ph)
    return z.float().contiguous()


@functools.lru_cache(maxsize=None)
def image_case(H, W, seed, weighted=True):
    """depth [H,W], normals [3,H,W] (near unit length), weight [H,W] in [0, 1] with exact zeros (None if not weighted), dL/dNd [3,H,W]; fp32.
    Shared between tests: treat as read-only."""
    g = torch.Generator().manual_seed(1000 + seed)
    depth = make_depth(H, W, seed)
    normals = torch.randn(3, H, W, generator=g)
    normals = (normals / normals.norm(dim=0, keepdim=True) * (0.8 + 0.4 * torch.rand(H, W, generator=g))).contiguous()
    weight = None
    if weighted:
        weight = torch.rand(H, W, generator=g)
        weight[torch.rand(H, W, generator=g) < 0.1] = 0.0
        weight = weight.contiguous()
    dL = torch.randn(3, H, W, generator=g).contiguous()
    return depth, normals, weight, dL


@functools.lru_cache(maxsize=None)
def image_reference(H, W, seed, weighted=True, dL_dloss=1.75):
    """fp64: Nd, dL/ddepth of <Nd, dL>, loss, dL/ddepth and dL/dnormals of dL_dloss * loss."""
    depth, normals, weight, dL = image_case(H, W, seed, weighted)
    tx, ty = TANFOV
    z = depth.double().requires_grad_(True)
    nd = depth_to_normal(z, tx, ty)
    ddepth_map = torch.autograd.grad((nd * dL.double()).sum(), z, allow_unused=True)[0] if nd.requires_grad else None
    if ddepth_map is None:
        ddepth_map = torch.zeros_like(z)
    z2, n2 = depth.double().requires_grad_(True), normals.double().requires_grad_(True)
    loss = normal_consistency_loss(z2, n2, tx, ty, None if weight is None else weight.double())
    gz, gn = torch.autograd.grad(dL_dloss * loss, (z2, n2), allow_unused=True)
    gz = torch.zeros_like(z2) if gz is None else gz
    gn = torch.zeros_like(n2) if gn is None else gn
    return nd.detach(), ddepth_map.detach(), float(loss.detach()), gz.detach(), gn.detach()


def view_matrix(seed=0):
    """[4,4] fp32 in the rasterizer's layout (the transposed world-to-camera matrix): a rotation of 0.4 rad about a skew axis, a small shift."""
    axis = torch.tensor([0.3, 1.0, -0.2], dtype=torch.float64)
    axis = axis / axis.norm()
    ang = 0.4 + 0.1 * seed
    K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = R
    w2c[:3, 3] = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
    return w2c.t().contiguous().float()


DESIGNED_ROWS = 16      # rows 0..15 of make_gaussians when P >= 64


@functools.lru_cache(maxsize=None)
def make_gaussians(P, seed=0):
    """scales [P,3], rotations [P,4], means3D [P,3], viewmatrix [4,4], dL/dn [P,3]; fp32; read-only.  Random unit quaternions, every 7th row
    scaled by 0.5 or 2; means around (0, 0, 5) in view space; log-normal scales.  With P >= 64 the first DESIGNED_ROWS rows are: exact two-way
    ties (0..2: which pair ties for the minimum), an exact three-way tie (3), a tie that is not the minimum (4), a mean behind the camera
    (5), NaN / +inf / -inf in each input (6..14), a zero quaternion (15: R(0) is the identity, a valid row)."""
    g = torch.Generator().manual_seed(77 + seed)
    vm = view_matrix(seed)
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    q[3::7] *= 0.5
    q[5::7] *= 2.0
    s = torch.exp(torch.randn(P, 3, generator=g) * 0.6 - 3.0)
    view = torch.randn(P, 3, generator=g) * torch.tensor([1.5, 1.0, 1.0]) + torch.tensor([0.0, 0.0, 5.0])
    w2c = vm.double().t()
    m = ((view.double() - w2c[:3, 3]) @ w2c[:3, :3]).float()      # world = R^T (view - t)
    if P >= 64:
        s[0] = torch.tensor([0.02, 0.02, 0.05]); s[1] = torch.tensor([0.02, 0.05, 0.02]); s[2] = torch.tensor([0.05, 0.02, 0.02])
        s[3] = torch.tensor([0.03, 0.03, 0.03]); s[4] = torch.tensor([0.05, 0.05, 0.01])
        m[5] = ((torch.tensor([0.3, -0.2, -5.0], dtype=torch.float64) - w2c[:3, 3]) @ w2c[:3, :3]).float()
        s[6, 1] = math.nan; s[7, 0] = math.inf; s[8, 2] = -math.inf
        q[9, 0] = math.nan; q[10, 3] = math.inf; q[11, 2] = -math.inf
        m[12, 0] = math.nan; m[13, 1] = math.inf; m[14, 2] = -math.inf
        q[15] = 0.0
    dL = torch.randn(P, 3, generator=g)
    return s.contiguous(), q.contiguous(), m.contiguous(), vm, dL.contiguous()


@functools.lru_cache(maxsize=None)
def gaussian_reference(P, seed=0):
    """fp64: normals [P,3], dL/drotations [P,4], the rows that are compared [P] bool."""
    s, q, m, vm, dL = make_gaussians(P, seed)
    q64 = q.double().requires_grad_(True)
    n, margin = gaussian_normals(s.double(), q64, m.double(), vm.double(), return_margin=True)
    (dq,) = torch.autograd.grad((n * dL.double()).sum(), q64) if P else (torch.zeros(0, 4, dtype=torch.float64),)
    dq = torch.where(torch.isfinite(dq), dq, torch.zeros_like(dq))      # (rows whose own q is non-finite: the contract says zero)
    return n.detach(), dq, margin >= SIGN_EXEMPT


# ---- comparisons: print every figure, then assert ---------------------------------------------------------------------------------------------------
def rel_max(got, want):
    """max |got - want| / max |want| (absolute when the reference is all zero)."""
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    return float((got.double() - want).abs().max()) / (scale if scale > 0 else 1.0)


def check(what, figures):
    """figures: {name: (error, bar key)}"""
    print(f"[normals] {what}: " + ", ".join(f"{k} {e:.2e} (bar {BARS[b]:.1e})" for k, (e, b) in figures.items()), flush=True)
    for k, (e, b) in figures.items():
        assert e <= BARS[b], (what, k, e, BARS[b])
    return {k: e for k, (e, _) in figures.items()}
