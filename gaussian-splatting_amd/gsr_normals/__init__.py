"""Normal-consistency regulariser of 2DGS / GOF / RaDe-GS / PGSR on the MI355X: per-Gaussian normals, the normals of a depth map and the fused
loss  (1 / (H W)) sum_p [1 - w(p) <normals(p), Nd(p)>]  as HIP kernels (csrc/normals.hip, gsr_gaussian_normals / gsr_depth_normals /
gsr_normal_loss and their backwards).

    gaussian_normals(scales[P,3], rotations[P,4], means3D[P,3], viewmatrix[4,4]) -> [P,3]      camera space, facing the camera
    depth_to_normal(depth[H,W], tanfovx, tanfovy) -> [3,H,W]
    normal_consistency_loss(depth[H,W], normals[3,H,W], tanfovx, tanfovy, weight=None) -> 0-dim tensor

include/gsr.h states the numerics contract (the difference form of the depth normals, which stays at a few 1e-7 of error at every resolution
where differencing back-projected points does not), INTEGRATION.md 3k the contract for borders and non-finite pixels.  Normals are planar
[3,H,W], the layout of a feature render.  No floating-point atomics: two runs give the same bits.  There is no CPU fallback.

The recipe, on ONE rasterizer call with return_alpha=True (INTEGRATION.md 3g for the feature render and its `z` column):

    rast = GaussianRasterizer(settings, return_alpha=True)
    color, radii, invdepth, alpha = rast(means3D=xyz, means2D=screen, opacities=opac, shs=shs, scales=s, rotations=q)
    n = gaussian_normals(s, q, xyz, settings.viewmatrix)                                      # [P,3]
    z = (xyz @ settings.viewmatrix[:3, 2] + settings.viewmatrix[3, 2])[:, None]               # the z column of 3g
    F = render_features(color, torch.cat([n, z], dim=1), geometry=True)                       # [4,H,W]: Nr = F[:3], D = F[3]
    depth = F[3] / alpha[0].clamp_min(1e-6)
    loss = normal_consistency_loss(depth, F[:3], settings.tanfovx, settings.tanfovy, weight=alpha[0].detach())

Gradients reach `rotations` through both the normals and the render, `means3D`, `scales` and `opacities` through the render."""
from __future__ import annotations

import math

import torch

import diff_gaussian_rasterization as _pkg
from diff_gaussian_rasterization import _lib

__all__ = ["gaussian_normals", "depth_to_normal", "normal_consistency_loss", "GaussianNormals", "DepthToNormal", "NormalConsistencyLoss"]


def _check(what: str, name: str, t, shape, like=None) -> None:
    """`t` is a float32 tensor on a HIP device whose shape matches `shape` (None: any size) -- and lives where `like` does."""
    ok = torch.is_tensor(t) and t.dim() == len(shape) and t.dtype == torch.float32 and all(s is None or s == d for s, d in zip(shape, t.shape))
    if not ok:
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        raise _lib.GsrError(f"{what}: {name} must be a float32 tensor of shape {want}, got "
                            f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} {getattr(t, 'dtype', '')}")
    _pkg._require_cuda(t, name)
    if like is not None and t.device != like.device:
        raise _lib.GsrError(f"{what}: {name} on {t.device}, the first tensor on {like.device}")


def _tanfov(what: str, tanfovx, tanfovy):
    tx, ty = float(tanfovx), float(tanfovy)
    if not (tx > 0.0 and ty > 0.0 and math.isfinite(tx) and math.isfinite(ty)):
        raise _lib.GsrError(f"{what}: tanfovx and tanfovy must be positive and finite, got {tx}, {ty}")
    return tx, ty


class GaussianNormals(torch.autograd.Function):
    """gsr_gaussian_normals / gsr_gaussian_normals_backward: the gradient goes to `rotations` only; nothing is saved but the inputs."""

    @staticmethod
    def forward(ctx, scales, rotations, means3D, viewmatrix):
        what = "gaussian_normals"
        _check(what, "scales", scales, (None, 3))
        P = scales.shape[0]
        _check(what, "rotations", rotations, (P, 4), scales)
        _check(what, "means3D", means3D, (P, 3), scales)
        _check(what, "viewmatrix", viewmatrix, (4, 4), scales)
        s, q, m, vm = (t.detach().contiguous() for t in (scales, rotations, means3D, viewmatrix))
        out = torch.empty((P, 3), dtype=torch.float32, device=s.device)
        lib = _lib.load()
        with torch.cuda.device(s.device):
            _lib.check(lib.gsr_gaussian_normals(P, _pkg._ptr(s), _pkg._ptr(q), _pkg._ptr(m), _pkg._ptr(vm), _pkg._ptr(out),
                                                _pkg._stream_ptr(s.device)), f"gsr_gaussian_normals (P {P})")
        ctx.save_for_backward(s, q, m, vm)
        return out

    @staticmethod
    def backward(ctx, dL_dnormals):
        s, q, m, vm = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        P = s.shape[0]
        g = dL_dnormals.contiguous().float()
        out = torch.empty((P, 4), dtype=torch.float32, device=s.device)
        lib = _lib.load()
        with torch.cuda.device(s.device):
            _lib.check(lib.gsr_gaussian_normals_backward(P, _pkg._ptr(s), _pkg._ptr(q), _pkg._ptr(m), _pkg._ptr(vm), _pkg._ptr(g), _pkg._ptr(out),
                                                         _pkg._stream_ptr(s.device)), "gsr_gaussian_normals_backward")
        return None, out, None, None


class DepthToNormal(torch.autograd.Function):
    """gsr_depth_normals / gsr_depth_normals_backward."""

    @staticmethod
    def forward(ctx, depth, tanfovx, tanfovy):
        what = "depth_to_normal"
        _check(what, "depth", depth, (None, None))
        if depth.numel() == 0:
            raise _lib.GsrError(f"{what}: empty depth of shape {tuple(depth.shape)}")
        tx, ty = _tanfov(what, tanfovx, tanfovy)
        z = depth.detach().contiguous()
        H, W = z.shape
        out = torch.empty((3, H, W), dtype=torch.float32, device=z.device)
        lib = _lib.load()
        with torch.cuda.device(z.device):
            _lib.check(lib.gsr_depth_normals(H, W, tx, ty, _pkg._ptr(z), _pkg._ptr(out), _pkg._stream_ptr(z.device)),
                       f"gsr_depth_normals (depth {tuple(z.shape)})")
        ctx.save_for_backward(z)
        ctx.tanfov = (tx, ty)
        return out

    @staticmethod
    def backward(ctx, dL_dnormals):
        (z,) = ctx.saved_tensors
        H, W = z.shape
        g = dL_dnormals.contiguous().float()
        out = torch.empty_like(z)
        lib = _lib.load()
        with torch.cuda.device(z.device):
            _lib.check(lib.gsr_depth_normals_backward(H, W, ctx.tanfov[0], ctx.tanfov[1], _pkg._ptr(z), _pkg._ptr(g), _pkg._ptr(out),
                                                      _pkg._stream_ptr(z.device)), "gsr_depth_normals_backward")
        return out, None, None


class NormalConsistencyLoss(torch.autograd.Function):
    """gsr_normal_loss / gsr_normal_loss_backward: ONE backward launch writes the gradients that are asked for -- dL/ddepth and dL/dnormals
    together, or either alone with the same bits."""

    @staticmethod
    def forward(ctx, depth, normals, tanfovx, tanfovy, weight):
        what = "normal_consistency_loss"
        _check(what, "depth", depth, (None, None))
        if depth.numel() == 0:
            raise _lib.GsrError(f"{what}: empty depth of shape {tuple(depth.shape)}")
        H, W = depth.shape
        _check(what, "normals", normals, (3, H, W), depth)
        if weight is not None:
            _check(what, "weight", weight, (H, W), depth)
        tx, ty = _tanfov(what, tanfovx, tanfovy)
        z, n = depth.detach().contiguous(), normals.detach().contiguous()
        w = None if weight is None else weight.detach().contiguous()
        lib = _lib.load()
        count = int(lib.gsr_normal_loss_partial_count(H, W))
        if count <= 0:
            raise _lib.GsrError(f"{what}: unsupported image size {H} x {W}")
        partials = torch.empty(count, dtype=torch.float64, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        with torch.cuda.device(z.device):
            _lib.check(lib.gsr_normal_loss(H, W, tx, ty, _pkg._ptr(z), _pkg._ptr(n), _pkg._ptr(w), _pkg._ptr(partials), _pkg._ptr(loss),
                                           _pkg._stream_ptr(z.device)), f"gsr_normal_loss (depth {tuple(z.shape)})")
        ctx.save_for_backward(z, n, w)
        ctx.tanfov = (tx, ty)
        return loss

    @staticmethod
    def backward(ctx, dL_dloss):
        z, n, w = ctx.saved_tensors
        H, W = z.shape
        g = dL_dloss.contiguous().float().reshape(1)          # dL/dloss as one device scalar
        d_depth = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        d_normals = torch.empty_like(n) if ctx.needs_input_grad[1] else None
        if d_depth is not None or d_normals is not None:
            lib = _lib.load()
            with torch.cuda.device(z.device):
                _lib.check(lib.gsr_normal_loss_backward(H, W, ctx.tanfov[0], ctx.tanfov[1], _pkg._ptr(z), _pkg._ptr(n), _pkg._ptr(w), _pkg._ptr(g),
                                                        _pkg._ptr(d_normals), _pkg._ptr(d_depth), _pkg._stream_ptr(z.device)),
                           "gsr_normal_loss_backward")
        return d_depth, d_normals, None, None, None


def gaussian_normals(scales: torch.Tensor, rotations: torch.Tensor, means3D: torch.Tensor, viewmatrix: torch.Tensor) -> torch.Tensor:
    """Camera-space normals [P,3] of P Gaussians: the axis of the smallest (activated) scale -- lowest index on ties -- taken from R(q) of the
    quaternion as given, rotated by the view matrix of the rasterizer's settings, normalised and turned to face the camera.  Differentiable in
    `rotations` only; the camera is a constant on this path.  Rows with a non-finite input come out as zeros."""
    return GaussianNormals.apply(scales, rotations, means3D, viewmatrix)


def depth_to_normal(depth: torch.Tensor, tanfovx: float, tanfovy: float) -> torch.Tensor:
    """Normals [3,H,W] of the depth map depth[H,W] (camera-space z per pixel), facing the camera: (0, 0, -1) on a fronto-parallel plane.
    Zero at the border and wherever a depth of the five-point stencil is not a finite positive number.  Differentiable in `depth`."""
    return DepthToNormal.apply(depth, tanfovx, tanfovy)


def normal_consistency_loss(depth: torch.Tensor, normals: torch.Tensor, tanfovx: float, tanfovy: float, weight: torch.Tensor = None) -> torch.Tensor:
    """mean over the pixels of 1 - weight <normals, depth_to_normal(depth)> -> 0-dim tensor, the depth normals never written to memory.
    `weight` [H,W] is a constant (pass the detached alpha); `normals` is used as it comes -- normalise a rendered normal map in torch first if
    the cosine is wanted.  Differentiable in `depth` and `normals`, each gradient computed only when asked for.  See the module docstring
    for the end-to-end recipe."""
    return NormalConsistencyLoss.apply(depth, normals, tanfovx, tanfovy, weight)
