"""The 3D smoothing filter of Mip-Splatting next to the operator (Yu et al., CVPR 2024; Gaussian Opacity Fields and RaDe-GS train with it too):
every Gaussian is low-passed in world space to the finest sampling rate any training camera sees it at.  The 2D half of the paper is
`antialiasing=True` of the rasterizer's settings.

    pack_cameras(cameras, device) -> [C,16]                               the camera records of the sweep
    compute_3d_filter(means3D, cameras, return_seen=False) -> [P,1]       upstream's GaussianModel.compute_3D_filter
    filtered_activations(raw_scales, raw_opacity, filter_3D)              get_scaling_with_3D_filter / get_opacity_with_3D_filter, differentiable
    fuse(raw_scales, raw_opacity, filter_3D)                              the filter folded into raw parameters, for save_ply

Both hot pieces are native (csrc/mip.hip): the sweep is ONE kernel over all cameras (gsr_mip_filter_3d; upstream: a Python loop
with ~20 torch kernels per camera), the activations are one streaming pass each way (gsr_mip_activations / _backward; upstream: a dozen torch
kernels forward and twice that backward).  include/gsr.h states the semantics, the numerics contract of the opacity factor and the two
departures from upstream; INTEGRATION.md 3l the recipe.  There is no CPU fallback.

    filter_3D = gsr_scene.mip.compute_3d_filter(gaussians._xyz, train_cameras)        # at the start, after every densification, every 100
    ...                                                                               # iterations once densification has ended
    scales, opacity = gsr_scene.mip.filtered_activations(gaussians._scaling, gaussians._opacity, filter_3D)
    rasterizer(..., scales=scales, opacities=opacity)                                 # settings: antialiasing=True"""
from __future__ import annotations

import math
from typing import Tuple

import torch

_EPS32 = float(torch.finfo(torch.float32).eps)
RECORD = 16      # floats per camera: R[9] row-major, T[3] (cam = xyz R + T), focal_x, focal_y, width, height


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


def _check(what: str, name: str, t, shape, like=None) -> None:
    pkg = _pkg()
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32:
        raise pkg.GsrError(f"{what}: {name} must be a float32 tensor of shape {tuple(shape)}, got "
                           f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} {getattr(t, 'dtype', '')}")
    pkg._require_cuda(t, name)
    if like is not None and t.device != like.device:
        raise pkg.GsrError(f"{what}: {name} on {t.device}, the first tensor on {like.device}")


def pack_cameras(cameras, device) -> torch.Tensor:
    """[C,16] float32 on `device` from camera objects with `R`, `T` (cam = xyz R + T, the reference's Camera.R / Camera.T), `image_width`,
    `image_height` and either `focal_x` / `focal_y` (Mip-Splatting's camera) or `FoVx` / `FoVy` (the reference's: focal = W / (2 tan(FoV / 2))).
    A tensor that is packed already passes through (moved to `device`)."""
    pkg = _pkg()
    if torch.is_tensor(cameras):
        if cameras.dim() != 2 or cameras.shape[1] != RECORD or cameras.shape[0] < 1:
            raise pkg.GsrError(f"pack_cameras: packed cameras must be [C,{RECORD}] with C >= 1, got {tuple(cameras.shape)}")
        return cameras.to(device=device, dtype=torch.float32).contiguous()
    rows = []
    for i, cam in enumerate(cameras):
        try:
            R = torch.as_tensor(cam.R, dtype=torch.float64).reshape(9)
            T = torch.as_tensor(cam.T, dtype=torch.float64).reshape(3)
            W, H = float(cam.image_width), float(cam.image_height)
            if hasattr(cam, "focal_x") and hasattr(cam, "focal_y"):
                fx, fy = float(cam.focal_x), float(cam.focal_y)
            else:
                fx, fy = W / (2.0 * math.tan(float(cam.FoVx) / 2.0)), H / (2.0 * math.tan(float(cam.FoVy) / 2.0))
        except AttributeError as e:
            raise pkg.GsrError(f"pack_cameras: camera {i} needs R, T, image_width, image_height and focal_x / focal_y or FoVx / FoVy ({e})")
        rows.append(torch.cat([R, T, torch.tensor([fx, fy, W, H], dtype=torch.float64)]))
    if not rows:
        raise pkg.GsrError("pack_cameras: at least one camera is needed")
    return torch.stack(rows).to(device=device, dtype=torch.float32).contiguous()


@torch.no_grad()
def compute_3d_filter(means3D: torch.Tensor, cameras, return_seen: bool = False):
    """Upstream's compute_3D_filter in one call: filter_3D [P,1] = (the smallest view depth over the cameras that see the Gaussian -- z > 0.2,
    projection inside the screen enlarged by 15 % -- or, for a Gaussian no camera sees, the largest such depth of the scene) / max focal_x *
    sqrt(0.2).  `cameras`: camera objects or a packed [C,16] tensor (pack_cameras; pack once and reuse it).  return_seen: also upstream's
    valid_points [P] bool.  No host synchronisation.  Nothing seen at all leaves the distance at 100000 (upstream raises); a non-finite mean
    is unseen and changes nobody else's value."""
    pkg = _pkg()
    if not torch.is_tensor(means3D) or means3D.dim() != 2 or means3D.shape[1] != 3 or means3D.dtype != torch.float32:
        raise pkg.GsrError(f"compute_3d_filter: means3D must be a float32 tensor of shape [P,3], got "
                           f"{tuple(means3D.shape) if torch.is_tensor(means3D) else type(means3D).__name__} {getattr(means3D, 'dtype', '')}")
    pkg._require_cuda(means3D, "means3D")
    xyz = means3D.detach().contiguous()
    cams = pack_cameras(cameras, xyz.device)
    P, C = int(xyz.shape[0]), int(cams.shape[0])
    out = torch.empty(P, dtype=torch.float32, device=xyz.device)
    seen = torch.empty(P, dtype=torch.uint8, device=xyz.device) if return_seen else None
    lib = pkg._lib.load()
    scratch = torch.empty(int(lib.gsr_mip_filter_scratch_bytes(P)), dtype=torch.uint8, device=xyz.device)
    with torch.cuda.device(xyz.device):
        pkg._lib.check(lib.gsr_mip_filter_3d(P, pkg._ptr(xyz), C, pkg._ptr(cams), pkg._ptr(out), pkg._ptr(seen), pkg._ptr(scratch),
                                             pkg._stream_ptr(xyz.device)), f"gsr_mip_filter_3d (P {P}, C {C})")
    out = out.reshape(P, 1)
    return (out, seen.bool()) if return_seen else out


class FilteredActivations(torch.autograd.Function):
    """gsr_mip_activations / gsr_mip_activations_backward; nothing is saved but the inputs, filter_3D gets no gradient (a buffer upstream)."""

    @staticmethod
    def forward(ctx, raw_scales, raw_opacity, filter_3D):
        pkg = _pkg()
        what = "filtered_activations"
        if not torch.is_tensor(raw_scales) or raw_scales.dim() != 2:
            raise pkg.GsrError(f"{what}: raw_scales must be a float32 tensor of shape [P,3]")
        P = int(raw_scales.shape[0])
        _check(what, "raw_scales", raw_scales, (P, 3))
        _check(what, "raw_opacity", raw_opacity, (P, 1), raw_scales)
        _check(what, "filter_3D", filter_3D, (P, 1), raw_scales)
        rs, ro, f = (t.detach().contiguous() for t in (raw_scales, raw_opacity, filter_3D))
        scales = torch.empty((P, 3), dtype=torch.float32, device=rs.device)
        opacity = torch.empty((P, 1), dtype=torch.float32, device=rs.device)
        lib = pkg._lib.load()
        with torch.cuda.device(rs.device):
            pkg._lib.check(lib.gsr_mip_activations(P, pkg._ptr(rs), pkg._ptr(ro), pkg._ptr(f), pkg._ptr(scales), pkg._ptr(opacity),
                                                   pkg._stream_ptr(rs.device)), f"gsr_mip_activations (P {P})")
        ctx.save_for_backward(rs, ro, f)
        ctx.set_materialize_grads(False)      # an output nobody used arrives as None and goes to the kernel as NULL
        return scales, opacity

    @staticmethod
    def backward(ctx, dL_dscales, dL_dopacity):
        pkg = _pkg()
        rs, ro, f = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        P = int(rs.shape[0])
        if dL_dscales is None and dL_dopacity is None:
            return torch.zeros_like(rs), torch.zeros_like(ro), None
        gs = None if dL_dscales is None else dL_dscales.contiguous().float()
        go = None if dL_dopacity is None else dL_dopacity.contiguous().float()
        d_rs, d_ro = torch.empty_like(rs), torch.empty_like(ro)
        lib = pkg._lib.load()
        with torch.cuda.device(rs.device):
            pkg._lib.check(lib.gsr_mip_activations_backward(P, pkg._ptr(rs), pkg._ptr(ro), pkg._ptr(f), pkg._ptr(gs), pkg._ptr(go), pkg._ptr(d_rs),
                                                            pkg._ptr(d_ro), pkg._stream_ptr(rs.device)), "gsr_mip_activations_backward")
        return d_rs, d_ro, None


def filtered_activations(raw_scales: torch.Tensor, raw_opacity: torch.Tensor, filter_3D: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scales [P,3], opacity [P,1]) = (sqrt(exp(raw_scales)^2 + f^2), sigmoid(raw_opacity) prod_i s_i / s'_i) from the raw parameters
    ([P,3] log scales, [P,1] logits) and filter_3D [P,1]: what upstream's get_scaling_with_3D_filter and get_opacity_with_3D_filter hand to
    the rasterizer, one HIP pass forward and one backward.  Differentiable in the two raw tensors; filter_3D is a constant.  A row with a
    non-finite raw value keeps the damage to itself and gets zero gradients."""
    return FilteredActivations.apply(raw_scales, raw_opacity, filter_3D)


@torch.no_grad()
def fuse(raw_scales: torch.Tensor, raw_opacity: torch.Tensor, filter_3D: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Upstream's get_scaling_n_opacity_with_3D_filter followed by log / logit: raw parameters whose PLAIN activations (exp, sigmoid) are the
    filtered values -- what save_ply writes so that a viewer without the filter shows the trained scene.  The opacity is clamped to
    [0, 1 - eps] before the logit (as gsr_scene.mcmc): a fully opaque Gaussian stays finite."""
    scales, opacity = filtered_activations(raw_scales.detach(), raw_opacity.detach(), filter_3D.detach())
    return torch.log(scales), torch.logit(opacity.clamp(max=1.0 - _EPS32))
