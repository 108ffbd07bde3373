"""MI355X counterpart of gsplat's `lib_bilagrid` / `fused_bilagrid` (per-image appearance compensation by a bilateral grid,
"Bilateral Guided Radiance Field Processing"): slicing, its backward and the total-variation regulariser as HIP kernels.

    slice_image(grids[N,12,L,Gh,Gw], image[3,H,W], idx) -> [3,H,W]      grid `idx` applied to one image
    total_variation_loss(grids[N,12,L,Gh,Gw]) -> 0-dim tensor
    BilateralGrid(num, grid_X=16, grid_Y=16, grid_W=8)                  nn.Module holding `grids`: forward(image, idx), tv_loss()

A grid holds one 3x4 affine colour map per vertex (channel 4 i + j = entry (i, j), j over r, g, b, 1); a pixel samples it trilinearly at its
position and its luminance 0.299 r + 0.587 g + 0.114 b, with the conventions of torch's grid_sample(align_corners=True, padding_mode="border")
(include/gsr.h states them in full, INTEGRATION.md 3j the contract for non-finite pixels).  LAYOUT: images are this project's planar
[3,H,W], the rasterizer's output as it comes -- gsplat's module takes [..., H, W, 3] pixels and an explicit coordinate grid; here the
coordinates are the pixel centres and are not an input.  The backward uses no floating-point atomics: two runs give the same bits.
All compute is in libgsr_hip.so (gsr_bilagrid_*, csrc/bilagrid.hip); there is no CPU fallback."""
from __future__ import annotations

import torch
import torch.nn as nn

import diff_gaussian_rasterization as _pkg
from diff_gaussian_rasterization import _lib

__all__ = ["slice_image", "total_variation_loss", "BilateralGrid", "SliceImage", "TotalVariation"]


def _check_grids(what: str, grids) -> None:
    if not torch.is_tensor(grids) or grids.dim() != 5 or grids.shape[1] != 12 or grids.dtype != torch.float32:
        raise _lib.GsrError(f"{what}: grids must be a float32 tensor of shape [N,12,L,Gh,Gw], got "
                            f"{tuple(grids.shape) if torch.is_tensor(grids) else type(grids).__name__} {getattr(grids, 'dtype', '')}")
    if grids.shape[0] < 1:
        raise _lib.GsrError(f"{what}: no grid in a tensor of shape {tuple(grids.shape)}")
    _pkg._require_cuda(grids, "grids")


class SliceImage(torch.autograd.Function):
    """out = grid `idx` of `grids` applied to `image`.  The gradient of `grids` is a zero-filled tensor of its shape with slice `idx` written
    by the kernel; the gradient of `image` is computed only when it is asked for."""

    @staticmethod
    def forward(ctx, grids, image, idx):
        _check_grids("slice_image", grids)
        if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32 or image.numel() == 0:
            raise _lib.GsrError(f"slice_image: image must be a non-empty float32 tensor of shape [3,H,W], got "
                                f"{tuple(image.shape) if torch.is_tensor(image) else type(image).__name__} {getattr(image, 'dtype', '')}")
        _pkg._require_cuda(image, "image")
        if image.device != grids.device:
            raise _lib.GsrError(f"slice_image: image on {image.device}, grids on {grids.device}")
        idx = int(idx)
        if not 0 <= idx < grids.shape[0]:
            raise _lib.GsrError(f"slice_image: idx {idx} outside the {grids.shape[0]} grids of a tensor of shape {tuple(grids.shape)}")
        grid = grids.detach()[idx].contiguous()
        img = image.detach().contiguous()
        _, H, W = img.shape
        L, Gh, Gw = grid.shape[1:]
        out = torch.empty_like(img)
        lib = _lib.load()
        with torch.cuda.device(img.device):
            _lib.check(lib.gsr_bilagrid_slice(H, W, L, Gh, Gw, _pkg._ptr(grid), _pkg._ptr(img), _pkg._ptr(out), _pkg._stream_ptr(img.device)),
                       f"gsr_bilagrid_slice (image {tuple(img.shape)}, grids {tuple(grids.shape)})")
        ctx.save_for_backward(grid, img)
        ctx.grids_shape, ctx.idx = tuple(grids.shape), idx
        return out

    @staticmethod
    def backward(ctx, dL_dout):
        lib = _lib.load()
        grid, img = ctx.saved_tensors
        _, H, W = img.shape
        L, Gh, Gw = grid.shape[1:]
        g = dL_dout.contiguous().float()
        d_grids = torch.zeros(ctx.grids_shape, dtype=torch.float32, device=img.device)
        d_img = torch.empty_like(img) if ctx.needs_input_grad[1] else None
        nbytes = int(lib.gsr_bilagrid_scratch_bytes(H, W, L, Gh, Gw))
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=img.device)
        with torch.cuda.device(img.device):
            _lib.check(lib.gsr_bilagrid_slice_backward(H, W, L, Gh, Gw, _pkg._ptr(grid), _pkg._ptr(img), _pkg._ptr(g), _pkg._ptr(d_grids[ctx.idx]),
                                                       _pkg._ptr(d_img), _pkg._ptr(scratch), nbytes, _pkg._stream_ptr(img.device)),
                       "gsr_bilagrid_slice_backward")
        return (d_grids if ctx.needs_input_grad[0] else None), d_img, None


class TotalVariation(torch.autograd.Function):
    """(1 / N) sum over the three grid axes of the mean squared forward difference (gsr_bilagrid_tv / gsr_bilagrid_tv_backward)."""

    @staticmethod
    def forward(ctx, grids):
        _check_grids("total_variation_loss", grids)
        lib = _lib.load()
        x = grids.detach().contiguous()
        N, _, L, Gh, Gw = x.shape
        count = int(lib.gsr_bilagrid_tv_partial_count(N, L, Gh, Gw))
        if count <= 0:
            raise _lib.GsrError(f"total_variation_loss: unsupported grid sizes in a tensor of shape {tuple(x.shape)} (L, Gh, Gw must be 2..64)")
        partials = torch.empty(count, dtype=torch.float64, device=x.device)
        tv = torch.empty((), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.gsr_bilagrid_tv(N, L, Gh, Gw, _pkg._ptr(x), _pkg._ptr(partials), _pkg._ptr(tv), _pkg._stream_ptr(x.device)),
                       f"gsr_bilagrid_tv (grids {tuple(x.shape)})")
        ctx.save_for_backward(x)
        return tv

    @staticmethod
    def backward(ctx, dL_dtv):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        N, _, L, Gh, Gw = x.shape
        g = dL_dtv.contiguous().float().reshape(1)          # dL/dtv as one device scalar
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.gsr_bilagrid_tv_backward(N, L, Gh, Gw, _pkg._ptr(x), _pkg._ptr(g), _pkg._ptr(out), _pkg._stream_ptr(x.device)),
                       "gsr_bilagrid_tv_backward")
        return out


def slice_image(grids: torch.Tensor, image: torch.Tensor, idx: int) -> torch.Tensor:
    """Grid `idx` of grids[N,12,L,Gh,Gw] applied to the planar image[3,H,W] -> [3,H,W].  Differentiable in `grids` and `image`."""
    return SliceImage.apply(grids, image, idx)


def total_variation_loss(grids: torch.Tensor) -> torch.Tensor:
    """Total variation of grids[N,12,L,Gh,Gw] (gsplat's `total_variation_loss`) -> 0-dim tensor; exactly 0 on identity grids."""
    return TotalVariation.apply(grids)


class BilateralGrid(nn.Module):
    """`num` bilateral grids of grid_X x grid_Y vertices over the image and grid_W over the luminance, initialised to the identity map
    (gsplat's `BilateralGrid`: the same parameter name, sizes and `tv_loss`).  LAYOUT: `forward(image, idx)` takes a planar [3,H,W] image
    and the index of its grid and samples at the pixel centres -- gsplat's forward takes (grid_xy[..., 2], rgb[..., 3], idx)."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        self.grid_width, self.grid_height, self.grid_guidance = int(grid_X), int(grid_Y), int(grid_W)
        eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float32)
        self.grids = nn.Parameter(eye.view(1, 12, 1, 1, 1).repeat(int(num), 1, self.grid_guidance, self.grid_height, self.grid_width).contiguous())

    def forward(self, image: torch.Tensor, idx: int) -> torch.Tensor:
        return slice_image(self.grids, image, idx)

    def tv_loss(self) -> torch.Tensor:
        return total_variation_loss(self.grids)
