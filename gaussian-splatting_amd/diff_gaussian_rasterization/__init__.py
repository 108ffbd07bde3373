"""MI355X-native drop-in for the reference's `diff_gaussian_rasterization` package.

Exports exactly what gaussian_renderer/__init__.py:14 imports -- `GaussianRasterizationSettings` and
`GaussianRasterizer` -- with the same constructor fields (gaussian_renderer/__init__.py:36-50), the same
keyword call (gaussian_renderer/__init__.py:102-110), the same 3-tuple return `(color[3,H,W], radii[P],
invdepth[1,H,W])` and the same autograd contract (gradients to means3D, means2D (NDC-scaled dummy, read at
scene/gaussian_model.py:472), shs / colors_precomp, opacities, scales, rotations / cov3D_precomp).

It also exports `SparseGaussianAdam` (train.py:37-41, scene/gaussian_model.py:24-27), which makes the reference
use the "separate_sh" call form -- `rasterizer(dc=features_dc, shs=features_rest, ...)`,
gaussian_renderer/__init__.py:82-100 -- supported here without concatenating the two tensors.
All compute goes through the C ABI of libgsr_hip.so (include/gsr.h, hand-written gfx950 HIP kernels); there is no
CPU or eager-PyTorch fallback -- a missing library raises.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import GsrError, GsrRasterSettings, RESIZE_FN  # noqa: F401

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "SparseGaussianAdam", "rasterize_gaussians", "GsrError",
           "ContributionStats", "contribution_stats", "PixelProbe", "pixel_probe", "render_features"]


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    antialiasing: bool = False


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _bucket(nbytes: int) -> int:
    """Round a scratch size up to one of 8 sizes per octave (<= 12.5 % slack)."""
    nbytes = int(nbytes)
    if nbytes <= (1 << 20):
        return nbytes
    step = 1 << (nbytes.bit_length() - 4)
    return (nbytes + step - 1) // step * step


_last_size: dict = {}
_last_R = 0          # num_rendered of the most recent forward (diagnostics: tools/train_run.py)
_max_R = 0


def _sized(kind: str, device, nbytes: int) -> int:
    """Allocation size for an R-sized scratch buffer (binning state, backward scratch).  R changes by a fraction of a
    percent from frame to frame as the Gaussians move; handing the caching allocator a different size every iteration
    makes it hipMalloc a fresh block now and then, which costs tens of ms on ROCm (seen as one-off 75 ms stalls in
    bench.py's train legs whenever the size crossed a rounding boundary).  So sizes are sticky: the last size of this
    kind is reused while it fits (and is not more than twice too big); when it does not, the new size jumps 12.5 %
    ahead of the need and is rounded to 8 steps per octave -- a training run re-allocates once per ~12 % growth."""
    nbytes = int(nbytes)
    key = (kind, getattr(device, "index", None))
    last = _last_size.get(key, 0)
    if nbytes <= last <= 2 * max(nbytes, 1 << 20):
        return last
    new = _bucket(nbytes + nbytes // 8)
    _last_size[key] = new
    if last > (64 << 20):
        # the size class of a large scratch buffer changed (densification grew the set): blocks of the old class would stay in
        # torch's caching allocator for ever -- a 30 000-iteration run that grew 100 k -> 1.4 M Gaussians ended with 12 GB
        # reserved against 1 GB allocated.  They are handed back at the start of the next forward.
        global _trim_pending
        _trim_pending = True
    return new


_trim_pending = False


def _trim_cache_if_pending():
    global _trim_pending
    if _trim_pending:
        _trim_pending = False
        torch.cuda.empty_cache()


class _Buffer:
    """A growable uint8 device tensor handed to the library through a resize callback (the reference's
    resizeFunctional lambda).  The callback closes over a one-element list, NOT over the _Buffer: a closure that referenced
    `self` would form a reference cycle (self -> ctypes callback -> closure -> self) that only the cyclic garbage collector
    breaks -- and it does not see device memory pressure: a 30 000-iteration training run of round 1's version accumulated
    > 100 GB of dead scratch buffers between collections."""

    def __init__(self, device, kind: str = "state"):
        holder = [torch.empty(0, dtype=torch.uint8, device=device)]
        self._holder = holder

        def _resize(_user, nbytes):
            if holder[0].numel() < nbytes:
                holder[0] = torch.empty(_sized(kind, device, nbytes), dtype=torch.uint8, device=device)
            return holder[0].data_ptr()

        self.cb = RESIZE_FN(_resize)

    @property
    def t(self) -> torch.Tensor:
        return self._holder[0]


def _make_settings(rs: GaussianRasterizationSettings, keep: list, tile_rows, no_backward: bool = False, bg_image: bool = False) -> GsrRasterSettings:
    """`bg_image`: the caller hands rs.bg to the composite entry points as a per-pixel image [3,H,W] as well (the single-GPU autograd function);
    everywhere else -- the multi-GPU renderers included -- the C ABI reads three floats, so any other shape than [3] is refused."""
    H, W = int(rs.image_height), int(rs.image_width)
    if tuple(rs.bg.shape) != (3,) and not (bg_image and tuple(rs.bg.shape) == (3, H, W)):
        raise GsrError(f"raster_settings.bg must have shape [3]" + (f" or [3, {H}, {W}] (image_height, image_width)" if bg_image else
                       " here (a per-pixel background [3,H,W] is supported by the single-GPU rasterizer only)") + f", got {list(rs.bg.shape)}")
    dev_t = [_f32c(rs.bg), _f32c(rs.viewmatrix), _f32c(rs.projmatrix), _f32c(rs.campos)]
    keep.extend(dev_t)
    s = GsrRasterSettings()
    s.image_height = int(rs.image_height)
    s.image_width = int(rs.image_width)
    s.tanfovx = float(rs.tanfovx)
    s.tanfovy = float(rs.tanfovy)
    s.bg = dev_t[0].data_ptr()
    s.scale_modifier = float(rs.scale_modifier)
    s.viewmatrix = dev_t[1].data_ptr()
    s.projmatrix = dev_t[2].data_ptr()
    s.sh_degree = int(rs.sh_degree)
    s.campos = dev_t[3].data_ptr()
    s.prefiltered = int(bool(rs.prefiltered))
    s.debug = int(bool(rs.debug))
    s.antialiasing = int(bool(rs.antialiasing))
    s.no_backward = int(bool(no_backward))
    if tile_rows is None:
        s.tile_y0, s.tile_y1 = 0, 0
    elif int(tile_rows[1]) <= int(tile_rows[0]):
        # empty band (a rank that owns no tile rows): (0, 0) would mean "all rows" in the C ABI, so hand over a
        # band past the last row, which the library clamps to an empty one
        s.tile_y0 = s.tile_y1 = 1 << 20
    else:
        s.tile_y0, s.tile_y1 = int(tile_rows[0]), int(tile_rows[1])
    return s


def _stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise GsrError(f"{name} must live on a HIP device ('cuda'); the MI355X rasterizer has no CPU path")


# ---- one function per native operation of the rasterizer.  `s` is a _make_settings record (the caller keeps its tensors alive); the
# caller holds torch.cuda.device(device).  Tensors are passed as they are: None where the C ABI takes NULL. --------------------------------
class _Forward(NamedTuple):
    """What a forward leaves for its blend backward: the three scratch buffers and R (num_rendered)."""
    geom: torch.Tensor
    binning: torch.Tensor
    img: torch.Tensor
    num_rendered: int


def _rasterize_forward(s, P, M, inputs, color, invdepth, radii, device, kinds=("geom", "binning", "image"), extra=None) -> _Forward:
    """gsr_rasterize_forward, or with a _lib.CompositeOut `extra` (alpha image, per-pixel background) gsr_rasterize_forward_composite.
    inputs = (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp); `kinds` are the _Buffer kinds of the geometry,
    binning and image buffers."""
    lib = _lib.load()
    geom, binning, img = (_Buffer(device, k) for k in kinds)
    nr = C.c_int32(0)
    args = (C.byref(s), P, M, *[_ptr(t) for t in inputs], geom.cb, None, binning.cb, None, img.cb, None, _ptr(color), _ptr(invdepth),
            _ptr(radii), C.byref(nr))
    if extra is None:
        _lib.check(lib.gsr_rasterize_forward(*args, _stream_ptr(device)), "gsr_rasterize_forward")
    else:
        _lib.check(lib.gsr_rasterize_forward_composite(*args, C.byref(extra), _stream_ptr(device)), "gsr_rasterize_forward_composite")
    return _Forward(geom.t, binning.t, img.t, int(nr.value))


def _rasterize_records(entry: str, s, lead, records, device):
    """gsr_rasterize_from_splats / _from_packed / _from_segments (`entry`): bins and blends projected records in the settings' band.
    `lead` is what the entry point takes between the settings and the records: (P,) or (n_segments, capacity).
    -> (color[3,H,W], invdepth[1,H,W], _Forward), zeros outside the band."""
    lib = _lib.load()
    color = torch.zeros(3, s.image_height, s.image_width, dtype=torch.float32, device=device)
    invdepth = torch.zeros(1, s.image_height, s.image_width, dtype=torch.float32, device=device)
    geom, binning, img = _Buffer(device, "geom"), _Buffer(device, "binning"), _Buffer(device, "image")
    nr = C.c_int32(0)
    args = (C.byref(s), *lead, _ptr(records), geom.cb, None, binning.cb, None, img.cb, None, _ptr(color), _ptr(invdepth), C.byref(nr),
            _stream_ptr(device))
    if entry == "gsr_rasterize_from_splats":
        rc = lib.gsr_rasterize_from_splats(*args)
    elif entry == "gsr_rasterize_from_packed":
        rc = lib.gsr_rasterize_from_packed(*args)
    else:
        rc = lib.gsr_rasterize_from_segments(*args)
    _lib.check(rc, entry)
    return color, invdepth, _Forward(geom.t, binning.t, img.t, int(nr.value))


def _preprocess_shard(raster_settings, tile_rows, keep: list, rows, means3D, sh, opacities, scales, rotations, dc, what: str):
    """gsr_preprocess_forward on one shard of Gaussians (the multi-GPU modes; split SH only in degree-3 storage).
    -> (settings, records, radii[P], M, (means3D, sh, opacities, scales, rotations, dc) as passed to the kernels).  The settings
    (band `tile_rows`, dc) serve the caller's next calls; their tensors live in `keep`.  records: [P,16], or [rows,16] whose rows
    past the shard are zero (records without tiles) when `rows` is given."""
    lib = _lib.load()
    _require_cuda(means3D, "means3D")
    device = means3D.device
    P = int(means3D.shape[0])
    m_c, sh_c, op_c, sc_c, rot_c, dc_c = (_f32c(t) for t in (means3D, sh, opacities, scales, rotations, dc))
    M = int(sh_c.shape[1]) + (1 if dc_c is not None else 0)
    if dc_c is not None and (M != 16 or dc_c.data_ptr() % 16 or sh_c.data_ptr() % 16):
        raise GsrError(f"{what}: the split SH form needs degree-3 storage (dc[P,1,3] + shs[P,15,3])")
    with torch.cuda.device(device):
        s = _make_settings(raster_settings, keep, tile_rows, False)
        if dc_c is not None:
            s.sh_dc = dc_c.data_ptr()
        if rows is None:
            records = torch.empty(P, 16, dtype=torch.float32, device=device)
        else:
            records = torch.zeros(int(rows), 16, dtype=torch.float32, device=device)
        radii = torch.empty(P, dtype=torch.int32, device=device)
        scratch = torch.empty(_sized("geom_shard", device, lib.gsr_geometry_bytes(P)), dtype=torch.uint8, device=device)
        _lib.check(lib.gsr_preprocess_forward(C.byref(s), P, M, _ptr(m_c), _ptr(sh_c), None, _ptr(op_c), _ptr(sc_c), _ptr(rot_c), None,
                                              _ptr(scratch), _ptr(radii), _ptr(records), _stream_ptr(device)), "gsr_preprocess_forward")
    return s, records, radii, M, (m_c, sh_c, op_c, sc_c, rot_c, dc_c)


def _backward_scratch(lib, P, num_rendered, device) -> torch.Tensor:
    return torch.empty(_sized("bwd", device, lib.gsr_backward_scratch_bytes(P, num_rendered)), dtype=torch.uint8, device=device)


def _backward_blend(s, P, fwd: _Forward, g_color, g_depth, device, extra=None, absgrad: bool = False) -> Optional[torch.Tensor]:
    """gsr_backward_blend, or with a _lib.CompositeGrads `extra` (alpha-image gradient, per-pixel background, background gradient)
    gsr_backward_blend_composite -> the per-Gaussian 48-byte gradient records [P,12], a view into the backward scratch (None for P == 0,
    where only the composite call has anything to write: the background gradient).  `absgrad`: gsr_backward_blend_abs (`extra` or not) --
    the same records with the absolute screen-space gradient sums in words 10, 11."""
    lib = _lib.load()
    scratch = _backward_scratch(lib, P, fwd.num_rendered, device)
    rec_ptr = C.c_void_p(0)
    args = (C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), _ptr(g_color), _ptr(g_depth), _ptr(scratch),
            C.byref(rec_ptr))
    if absgrad:
        _lib.check(lib.gsr_backward_blend_abs(*args, None if extra is None else C.byref(extra), _stream_ptr(device)), "gsr_backward_blend_abs")
    elif extra is None:
        _lib.check(lib.gsr_backward_blend(*args, _stream_ptr(device)), "gsr_backward_blend")
    else:
        _lib.check(lib.gsr_backward_blend_composite(*args, C.byref(extra), _stream_ptr(device)), "gsr_backward_blend_composite")
    if P == 0:
        return None
    off = int(rec_ptr.value) - scratch.data_ptr()
    return scratch[off:off + P * 48].view(torch.float32).view(P, 12)


def _absgrad_from_records(s, P, records, device) -> torch.Tensor:
    """gsr_absgrad_from_records: words 10, 11 of the [P,12] records of an `absgrad` blend backward -> means2D_abs[P,3], the units and layout of
    dL_dmeans2D."""
    out = torch.empty(P, 3, dtype=torch.float32, device=device)
    if P > 0:
        _lib.check(_lib.load().gsr_absgrad_from_records(C.byref(s), P, _ptr(records), _ptr(out), _stream_ptr(device)), "gsr_absgrad_from_records")
    return out


def _gradients(P, device, colors: bool, cov3D: bool, sh_rows, dc: bool, scales: bool, rotations: bool):
    """The per-Gaussian backward's outputs in the order of include/gsr.h -- [dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D,
    dL_dcov3D, dL_dsh, dL_dscales, dL_drotations] -- and dL_d(sh_dc); the flags (sh_rows: rows of dL_dsh per Gaussian) say which of the
    optional ones exist (None otherwise)."""
    f = dict(dtype=torch.float32, device=device)
    opt = lambda on, *shape: torch.empty(P, *shape, **f) if on else None      # noqa: E731
    grads = [torch.empty(P, 3, **f), opt(colors, 3), torch.empty(P, 1, **f), torch.empty(P, 3, **f), opt(cov3D, 6),
             opt(sh_rows is not None, sh_rows, 3), opt(scales, 3), opt(rotations, 4)]
    return grads, opt(dc, 1, 3)


def _backward_preprocess(s, P, M, inputs, radii, geom, records, grads, device, extra=None) -> None:
    """The per-Gaussian backward from the [P,12] records: gsr_backward_preprocess, or with a _lib.CameraGrads `extra`
    gsr_backward_preprocess_camera, or with a _lib.ShAdam gsr_backward_preprocess_sh_adam (which writes no colour or SH gradient: it
    steps the two SH tensors in place).  inputs = (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp),
    grads as _gradients returns them."""
    lib = _lib.load()
    st = _stream_ptr(device)
    if isinstance(extra, _lib.ShAdam):
        m, sh, _, op, sc, rot, cov = inputs
        dm2, _, dop, dm3, dcov, _, dsc, drot = grads
        _lib.check(lib.gsr_backward_preprocess_sh_adam(C.byref(s), P, M, _ptr(m), _ptr(sh), _ptr(op), _ptr(sc), _ptr(rot), _ptr(cov),
                                                       _ptr(radii), _ptr(geom), _ptr(records), _ptr(dm2), _ptr(dop), _ptr(dm3),
                                                       _ptr(dcov), _ptr(dsc), _ptr(drot), C.byref(extra), st),
                   "gsr_backward_preprocess_sh_adam")
        return
    args = (C.byref(s), P, M, *[_ptr(t) for t in inputs], _ptr(radii), _ptr(geom), _ptr(records), *[_ptr(g) for g in grads])
    if extra is None:
        _lib.check(lib.gsr_backward_preprocess(*args, st), "gsr_backward_preprocess")
    else:
        _lib.check(lib.gsr_backward_preprocess_camera(*args, C.byref(extra), st), "gsr_backward_preprocess_camera")


def _rasterize_backward(s, P, M, inputs, radii, fwd: _Forward, g_color, g_depth, grads, device) -> None:
    """gsr_rasterize_backward: blend backward and per-Gaussian backward in one call (arguments as _backward_preprocess)."""
    lib = _lib.load()
    scratch = _backward_scratch(lib, P, fwd.num_rendered, device)
    _lib.check(lib.gsr_rasterize_backward(C.byref(s), P, M, fwd.num_rendered, *[_ptr(t) for t in inputs], _ptr(radii), _ptr(fwd.geom),
                                          _ptr(fwd.binning), _ptr(fwd.img), _ptr(g_color), _ptr(g_depth), *[_ptr(g) for g in grads],
                                          _ptr(scratch), None, _stream_ptr(device)), "gsr_rasterize_backward")


class ContributionStats(NamedTuple):
    """Per-Gaussian blend-weight statistics of one or more forwards (include/gsr.h gsr_contribution_stats): with w = alpha * T, the
    forward's blend weight, and a per-pixel weight E: weight_sum[P] = sum_p E w, weight_max[P] = max(0, max_p E w) (float32) and
    pixel_count[P] = pixels with E != 0 the Gaussian was blended into (int32)."""
    weight_sum: torch.Tensor
    weight_max: torch.Tensor
    pixel_count: torch.Tensor


def _pixel_weight(pixel_weight, H: int, W: int, device) -> Optional[torch.Tensor]:
    if pixel_weight is None:
        return None
    if tuple(pixel_weight.shape) not in ((H, W), (1, H, W)):
        raise GsrError(f"pixel_weight must have shape [{H}, {W}] or [1, {H}, {W}] (image_height, image_width), got {list(pixel_weight.shape)}")
    if pixel_weight.device != device:
        raise GsrError(f"pixel_weight lives on {pixel_weight.device}, the rendered state on {device}")
    return _f32c(pixel_weight.detach())


def _contribution_stats(s, P, fwd: _Forward, pixel_weight, into: Optional[ContributionStats], device) -> ContributionStats:
    """gsr_contribution_stats on the state a tracking forward left: fresh arrays, or `into` combined in place."""
    lib = _lib.load()
    if into is None:
        out = ContributionStats(torch.empty(P, dtype=torch.float32, device=device), torch.empty(P, dtype=torch.float32, device=device),
                                torch.empty(P, dtype=torch.int32, device=device))
    else:
        out = into
        for t, dt, name in zip(out, (torch.float32, torch.float32, torch.int32), ContributionStats._fields):
            if tuple(t.shape) != (P,) or t.dtype != dt or t.device != device or not t.is_contiguous():
                raise GsrError(f"into.{name} must be a contiguous {dt} tensor of shape [{P}] on {device}")
    scratch = torch.empty(_sized("contrib", device, lib.gsr_contribution_scratch_bytes(P, fwd.num_rendered)), dtype=torch.uint8, device=device)
    rec = _lib.ContribOut(out.weight_sum.data_ptr(), out.weight_max.data_ptr(), out.pixel_count.data_ptr(), 0 if into is None else 1, 0)
    _lib.check(lib.gsr_contribution_stats(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), _ptr(pixel_weight),
                                          _ptr(scratch), C.byref(rec), _stream_ptr(device)), "gsr_contribution_stats")
    return out


def _rasterizer_nodes(t: torch.Tensor) -> list:
    """The _RasterizeGaussians nodes of the autograd graph behind `t` (the node of an autograd.Function is its ctx)."""
    found, seen, stack = [], set(), [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if isinstance(fn, _RasterizeGaussians._backward_cls):
            found.append(fn)
            continue      # (what fed the rasterizer is not a render of it)
        stack.extend(f for f, _ in fn.next_functions)
    return found


class _SavedState(NamedTuple):
    """What a read-only entry point needs of the one rasterizer call behind a tensor (_saved_state)."""
    settings: GaussianRasterizationSettings
    tile_rows: Optional[Tuple[int, int]]
    P: int
    fwd: _Forward
    device: torch.device
    node: object = None      # the _RasterizeGaussians node itself (render_features(geometry=True): its inputs and per-Gaussian state)


def _saved_state(rendered, who: str, standalone: str) -> _SavedState:
    """The state that the ONE _RasterizeGaussians node behind `rendered` keeps for its backward; GsrError for no node, several nodes, a node of the
    multi-GPU renderers or freed state.  `who` / `standalone` name the caller and its no_grad counterpart in the messages."""
    nodes = _rasterizer_nodes(rendered) if isinstance(rendered, torch.Tensor) else []
    if len(nodes) != 1:
        raise GsrError(("no rasterizer call found behind `rendered`: it must be computed from a GaussianRasterizer output with gradients enabled "
                        f"(under torch.no_grad() use GaussianRasterizer.{standalone})") if not nodes else
                       f"`rendered` depends on {len(nodes)} rasterizer calls: pass a tensor computed from exactly one")
    ctx = nodes[0]
    if ctx.grad_sync is not None:
        raise GsrError(f"{who} does not support the multi-GPU renderers (a rasterizer call with grad_sync)")
    try:
        saved = ctx.saved_tensors
    except RuntimeError as e:
        raise GsrError(f"the rasterizer call's state has been freed: call {who} before backward(), or use retain_graph=True") from e
    means3D, geom, binning, img = saved[0], saved[8], saved[9], saved[10]
    return _SavedState(ctx.raster_settings, ctx.tile_rows, int(means3D.shape[0]), _Forward(geom, binning, img, ctx.num_rendered), means3D.device, ctx)


def contribution_stats(rendered: torch.Tensor, pixel_weight: Optional[torch.Tensor] = None,
                       into: Optional[ContributionStats] = None) -> ContributionStats:
    """What every Gaussian gave to a frame that has ALREADY been rendered (no reference counterpart): `rendered` is any tensor computed
    from one rasterizer call's outputs with gradients enabled -- the reference's `render(...)["render"]`, after exposure and clamp --
    and the statistics are read from the state that call keeps for its backward: no second forward, no backward.  Call it BEFORE
    `backward()` frees that state (or use `retain_graph=True`).  `pixel_weight` [H,W] or [1,H,W] weights the pixels (a per-pixel error,
    a mask: pixels with weight 0 are excluded); None is 1 everywhere.  `into` (a ContributionStats of an earlier call) is combined in
    place -- sum + frame, max(max, frame), count + frame -- and returned, so scores over many views build up without torch ops.
    With `tile_rows` the statistics are the band's.  Nothing here is differentiable; two calls give the same bits."""
    st = _saved_state(rendered, "contribution_stats", "contributions")
    rs = st.settings
    pw = _pixel_weight(pixel_weight, int(rs.image_height), int(rs.image_width), st.device)
    keep: list = []
    with torch.no_grad(), torch.cuda.device(st.device):
        s = _make_settings(rs, keep, st.tile_rows, bg_image=True)
        return _contribution_stats(s, st.P, st.fwd, pw, into, st.device)


class PixelProbe(NamedTuple):
    """Per-pixel probe of one forward (include/gsr.h gsr_pixel_probe), every field [H,W]: with w = alpha * T the blend weight of a contributor at
    view-space depth z, front to back: expected_depth = sum w z (float32, not normalised: divide by alpha), median_depth / median_id = z and Gaussian
    index of the first contributor behind which transmittance is < threshold (0.0 / -1: none), top_id / top_weight = index and w of the contributor
    with the largest w (-1 / 0.0: none; the nearest wins ties), count = contributors (ids and count int32)."""
    expected_depth: torch.Tensor
    median_depth: torch.Tensor
    median_id: torch.Tensor
    top_id: torch.Tensor
    top_weight: torch.Tensor
    count: torch.Tensor


def _pixel_probe(s, P, fwd: _Forward, threshold: float, H: int, W: int, device) -> PixelProbe:
    """gsr_pixel_probe on the state a tracking forward left.  The arrays are allocated with the defaults: with `tile_rows` the library leaves
    pixels outside the band untouched."""
    lib = _lib.load()
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise GsrError(f"threshold must be inside (0, 1), got {threshold}")
    f = lambda: torch.zeros(H, W, dtype=torch.float32, device=device)                        # noqa: E731
    i = lambda v: torch.full((H, W), v, dtype=torch.int32, device=device)                   # noqa: E731
    out = PixelProbe(f(), f(), i(-1), i(-1), f(), i(0))
    rec = _lib.PixelProbeOut(*[t.data_ptr() for t in out], threshold, 0)
    _lib.check(lib.gsr_pixel_probe(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), C.byref(rec),
                                   _stream_ptr(device)), "gsr_pixel_probe")
    return out


def pixel_probe(rendered: torch.Tensor, threshold: float = 0.5) -> PixelProbe:
    """What a frame that has ALREADY been rendered means for every pixel (no reference counterpart): median / expected depth, the Gaussian under the
    pixel, the number of blended Gaussians -- a PixelProbe.  `rendered` and the state it is read from are `contribution_stats`'s: any tensor computed
    from one rasterizer call's outputs with gradients enabled, before `backward()` frees the state (or with `retain_graph=True`); no second forward.
    `threshold` in (0, 1) is the transmittance that defines median_depth / median_id (0.5: the median).  With `tile_rows`, pixels outside the band
    hold the defaults (0, -1).  Nothing here is differentiable; two calls give the same bits."""
    st = _saved_state(rendered, "pixel_probe", "probe")
    rs = st.settings
    keep: list = []
    with torch.no_grad(), torch.cuda.device(st.device):
        s = _make_settings(rs, keep, st.tile_rows, bg_image=True)
        return _pixel_probe(s, st.P, st.fwd, threshold, int(rs.image_height), int(rs.image_width), st.device)


MAX_FEATURE_CHANNELS = 1024      # GSR_MAX_FEATURE_CHANNELS of include/gsr.h


def _feature_rows(features, P: int, device) -> torch.Tensor:
    """`features` as the C ABI takes it: [P,C] float32 contiguous on the state's device, 1 <= C <= MAX_FEATURE_CHANNELS."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2:
        raise GsrError(f"features must be a tensor of shape [P, C], got {list(features.shape) if isinstance(features, torch.Tensor) else type(features)}")
    if int(features.shape[0]) != P:
        raise GsrError(f"features has {int(features.shape[0])} rows, the rendered state {P} Gaussians")
    if not 1 <= int(features.shape[1]) <= MAX_FEATURE_CHANNELS:
        raise GsrError(f"features must have between 1 and {MAX_FEATURE_CHANNELS} channels, got {int(features.shape[1])}")
    if features.device != device:
        raise GsrError(f"features lives on {features.device}, the rendered state on {device}")
    return features


class _RenderFeatures(torch.autograd.Function):
    """F[C,H,W] = sum_g w f[g] on the state of a finished tracking forward (gsr_render_features), differentiable in `features` only
    (gsr_render_features_backward).  It keeps its OWN references to the three state tensors, so its backward does not depend on the frame's
    graph; without a gradient to compute it keeps nothing."""

    @staticmethod
    def forward(ctx, features, geom, binning, img, num_rendered, raster_settings, tile_rows):
        P, Cn = int(features.shape[0]), int(features.shape[1])
        out = _features_forward(features, _Forward(geom, binning, img, num_rendered), raster_settings, tile_rows)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(geom, binning, img)
            ctx.num_rendered, ctx.raster_settings, ctx.tile_rows, ctx.shape, ctx.dtype = num_rendered, raster_settings, tile_rows, (P, Cn), features.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        geom, binning, img = ctx.saved_tensors
        grad = _features_backward(grad_out, ctx.shape, _Forward(geom, binning, img, ctx.num_rendered), ctx.raster_settings, ctx.tile_rows)
        return grad.to(ctx.dtype), None, None, None, None, None, None


def _features_forward(features, fwd: _Forward, raster_settings, tile_rows) -> torch.Tensor:
    """gsr_render_features on the state a tracking forward left -> F[C,H,W] (fp32)."""
    lib = _lib.load()
    device = features.device
    P, Cn = int(features.shape[0]), int(features.shape[1])
    H, W = int(raster_settings.image_height), int(raster_settings.image_width)
    f = _f32c(features.detach())
    out = torch.zeros(Cn, H, W, dtype=torch.float32, device=device)      # (with `tile_rows` the library leaves pixels outside the band untouched)
    keep: list = []
    with torch.cuda.device(device):
        s = _make_settings(raster_settings, keep, tile_rows, bg_image=True)
        _lib.check(lib.gsr_render_features(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), _ptr(f), Cn, _ptr(out),
                                           _stream_ptr(device)), "gsr_render_features")
    return out


def _features_backward(grad_out, shape, fwd: _Forward, raster_settings, tile_rows) -> torch.Tensor:
    """gsr_render_features_backward -> dL/dfeatures [P,C] (fp32)."""
    lib = _lib.load()
    P, Cn = shape
    device = grad_out.device
    g = _f32c(grad_out)
    grad = torch.empty(P, Cn, dtype=torch.float32, device=device)
    keep: list = []
    with torch.cuda.device(device):
        s = _make_settings(raster_settings, keep, tile_rows, bg_image=True)
        scratch = torch.empty(_sized("contrib", device, lib.gsr_feature_grad_scratch_bytes(P, fwd.num_rendered, Cn)), dtype=torch.uint8, device=device)
        _lib.check(lib.gsr_render_features_backward(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), _ptr(g), Cn,
                                                    _ptr(scratch), _ptr(grad), _stream_ptr(device)), "gsr_render_features_backward")
    return grad


class _FeatureFrame(NamedTuple):
    """The frame a feature render with geometry gradients stands on: the state of its tracking forward and the per-Gaussian inputs of that forward as
    the C ABI took them (fp32, contiguous; None where the call had none)."""
    settings: GaussianRasterizationSettings
    tile_rows: Optional[Tuple[int, int]]
    fwd: _Forward
    radii: torch.Tensor
    means3D: torch.Tensor
    opacities: torch.Tensor
    scales: Optional[torch.Tensor]
    rotations: Optional[torch.Tensor]
    cov3D: Optional[torch.Tensor]


def _feature_geometry_records(frame: _FeatureFrame, features, grad_out) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """gsr_render_features_backward_geometry -> (the [P,12] records, a view into the scratch returned beside it; None for P == 0)."""
    lib = _lib.load()
    device = grad_out.device
    P, Cn = int(features.shape[0]), int(features.shape[1])
    fwd = frame.fwd
    keep: list = []
    s = _make_settings(frame.settings, keep, frame.tile_rows, bg_image=True)
    scratch = _backward_scratch(lib, P, fwd.num_rendered, device)
    rec_ptr = C.c_void_p(0)
    _lib.check(lib.gsr_render_features_backward_geometry(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img),
                                                         _ptr(features), _ptr(grad_out), Cn, _ptr(scratch), C.byref(rec_ptr), _stream_ptr(device)),
               "gsr_render_features_backward_geometry")
    if P == 0:
        return None, scratch
    off = int(rec_ptr.value) - scratch.data_ptr()
    return scratch[off:off + P * 48].view(torch.float32).view(P, 12), scratch


def _geometry_from_records(frame: _FeatureFrame, records, device):
    """The per-Gaussian backward on records whose colour words are zero, in its `colors_precomp` form with a zero colour tensor: no [P,M,3] SH
    gradient is allocated or written.  -> _gradients' list."""
    P = int(frame.means3D.shape[0])
    grads, _ = _gradients(P, device, True, frame.cov3D is not None, None, False, frame.scales is not None, frame.rotations is not None)
    keep: list = []
    s = _make_settings(frame.settings, keep, frame.tile_rows, bg_image=True)
    inputs = (frame.means3D, None, torch.zeros(P, 3, dtype=torch.float32, device=device), frame.opacities, frame.scales, frame.rotations, frame.cov3D)
    _backward_preprocess(s, P, 0, inputs, frame.radii, frame.fwd.geom, records, grads, device)
    return grads


class _RenderFeaturesGeometry(torch.autograd.Function):
    """_RenderFeatures that is also differentiable in the geometry of its frame: inputs are `features` and the caller's own means3D, means2D, opacities,
    scales, rotations, cov3D_precomp (None where the rasterizer call had none).  F has _RenderFeatures' bits.  The backward runs
    gsr_render_features_backward for `features`, and for the geometry gsr_render_features_backward_geometry followed by the per-Gaussian backward
    (gsr_backward_preprocess); what nobody needs is not computed.  The camera is a constant on this path."""

    @staticmethod
    def forward(ctx, features, means3D, means2D, opacities, scales, rotations, cov3D, frame: _FeatureFrame):
        out = _features_forward(features, frame.fwd, frame.settings, frame.tile_rows)
        if any(ctx.needs_input_grad[:7]):
            ctx.frame = frame
            ctx.features = _f32c(features.detach()) if any(ctx.needs_input_grad[1:7]) else None
            ctx.shape, ctx.dtype = (int(features.shape[0]), int(features.shape[1])), features.dtype
            ctx.meta = tuple(None if t is None else (tuple(t.shape), t.dtype) for t in (means3D, means2D, opacities, scales, rotations, cov3D))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        frame = ctx.frame
        device = grad_out.device
        need = ctx.needs_input_grad
        g = _f32c(grad_out)
        d_features = None
        if need[0]:
            d_features = _features_backward(g, ctx.shape, frame.fwd, frame.settings, frame.tile_rows).to(ctx.dtype)
        out = [None] * 6
        if any(need[1:7]) and ctx.shape[0] > 0:
            with torch.cuda.device(device):
                records, _scratch = _feature_geometry_records(frame, ctx.features, g)
                dm2, _, dop, dm3, dcov, _, dsc, drot = _geometry_from_records(frame, records, device)
            for k, t in enumerate((dm3, dm2, dop, dsc, drot, dcov)):
                if need[1 + k] and ctx.meta[k] is not None and t is not None:
                    out[k] = t.view(ctx.meta[k][0]).to(ctx.meta[k][1])
        elif any(need[1:7]):
            out = [None if (m is None or not need[1 + k]) else torch.zeros(m[0], dtype=m[1], device=device) for k, m in enumerate(ctx.meta)]
        return (d_features, *out, None)


def _geometry_frame(st: _SavedState) -> Tuple[_FeatureFrame, tuple]:
    """(the frame behind a rasterizer call as _RenderFeaturesGeometry takes it, the caller's own geometry tensors of that call)."""
    saved = st.node.saved_tensors
    has_sh, has_col, has_sc, has_rot, has_cov = st.node.flags
    frame = _FeatureFrame(st.settings, st.tile_rows, st.fwd, saved[7], saved[0], saved[3], saved[4] if has_sc else None, saved[5] if has_rot else None,
                          saved[6] if has_cov else None)
    return frame, st.node.geom_inputs


def render_features(rendered: torch.Tensor, features: torch.Tensor, geometry: bool = False) -> torch.Tensor:
    """-> F[C,H,W] = sum_g w_gp features[g,c]: N-channel per-Gaussian features (language / semantic fields, distillation heads, label votes) blended
    with the weights w = alpha * T of a frame that has ALREADY been rendered (no reference counterpart; include/gsr.h gsr_render_features).
    `rendered` and the state it is read from are `contribution_stats`'s: any tensor computed from one rasterizer call's outputs with gradients
    enabled, before that call's `backward()` frees the state (or with `retain_graph=True`); no second forward, whatever C is.  `features` is
    [P,C], 1 <= C <= 1024.  There is NO background term and no normalisation: compose with the alpha image of `return_alpha=True`.
    With `geometry=False` (the default) differentiable in `features` ONLY: geometry and opacity are constants of the frame already rendered, so
    no gradient reaches means3D, scales, rotations or opacities through F.  With `geometry=True` (joint training of a field and its geometry,
    depth / normal supervision through a rendered z or normal column; include/gsr.h gsr_render_features_backward_geometry) F has the same bits
    and its backward also delivers gradients to the tensors that were PASSED TO THE RASTERIZER CALL behind `rendered` -- means3D, opacities,
    scales + rotations or cov3D_precomp, and means2D if it was passed (so the feature loss counts in the densification statistics) -- which
    autograd adds to what the colour loss delivers.  The camera stays a constant on this path: no gradient reaches viewmatrix / projmatrix /
    campos through F.  The backward keeps its own references to the state: it still runs after the frame's own `backward()`.  Rows of Gaussians
    that contribute nowhere never reach the image (they may hold anything) and get exact zero gradients.  With `tile_rows`, pixels outside the
    band are 0 and the gradients are the band's.  Two calls give the same bits, and channel c of F and of dL/dfeatures has the bits of a call on
    column c alone."""
    st = _saved_state(rendered, "render_features", "features")
    features = _feature_rows(features, st.P, st.device)
    if not geometry:
        return _RenderFeatures.apply(features, st.fwd.geom, st.fwd.binning, st.fwd.img, st.fwd.num_rendered, st.settings, st.tile_rows)
    frame, (means3D, means2D, opacities, scales, rotations, cov3D) = _geometry_frame(st)
    return _RenderFeaturesGeometry.apply(features, means3D, means2D, opacities, scales, rotations, cov3D, frame)


def _distortion_forward(frame: _FeatureFrame, depth_mode: int, want_saved: bool, device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """gsr_distortion on the state a tracking forward left -> (D[H,W], saved[2,H,W] or None), fp32."""
    lib = _lib.load()
    rs, fwd = frame.settings, frame.fwd
    H, W = int(rs.image_height), int(rs.image_width)
    P = int(frame.means3D.shape[0])
    out = torch.zeros(H, W, dtype=torch.float32, device=device)      # (with `tile_rows` the library leaves pixels outside the band untouched)
    saved = torch.zeros(2, H, W, dtype=torch.float32, device=device) if want_saved else None
    keep: list = []
    with torch.cuda.device(device):
        s = _make_settings(rs, keep, frame.tile_rows, bg_image=True)
        rec = _lib.DistortionOut(out.data_ptr(), saved.data_ptr() if want_saved else None, depth_mode, 0)
        _lib.check(lib.gsr_distortion(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), C.byref(rec),
                                      _stream_ptr(device)), "gsr_distortion")
    return out, saved


def _distortion_records(frame: _FeatureFrame, grad_out, saved, depth_mode: int) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """gsr_distortion_backward -> (the [P,12] records, a view into the scratch returned beside it; None for P == 0)."""
    lib = _lib.load()
    device = grad_out.device
    P = int(frame.means3D.shape[0])
    fwd = frame.fwd
    keep: list = []
    s = _make_settings(frame.settings, keep, frame.tile_rows, bg_image=True)
    scratch = _backward_scratch(lib, P, fwd.num_rendered, device)
    rec_ptr = C.c_void_p(0)
    _lib.check(lib.gsr_distortion_backward(C.byref(s), P, fwd.num_rendered, _ptr(fwd.geom), _ptr(fwd.binning), _ptr(fwd.img), _ptr(grad_out),
                                           _ptr(saved), depth_mode, _ptr(scratch), C.byref(rec_ptr), _stream_ptr(device)),
               "gsr_distortion_backward")
    if P == 0:
        return None, scratch
    off = int(rec_ptr.value) - scratch.data_ptr()
    return scratch[off:off + P * 48].view(torch.float32).view(P, 12), scratch


class _Distortion(torch.autograd.Function):
    """D[H,W] of gsr_distortion on a frame's state, differentiable in the caller's own means3D, means2D, opacities, scales, rotations, cov3D_precomp
    (None where the rasterizer call had none): the backward runs gsr_distortion_backward followed by the per-Gaussian backward
    (gsr_backward_preprocess).  It keeps its own references to the state (the frame) and the forward's two planes of totals; without a gradient to
    compute neither is kept nor are the planes allocated.  The camera is a constant on this path."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D, frame: _FeatureFrame, depth_mode: int):
        device = frame.means3D.device
        need = any(ctx.needs_input_grad[:6])
        out, saved = _distortion_forward(frame, depth_mode, need, device)
        if need:
            ctx.frame, ctx.saved, ctx.depth_mode = frame, saved, depth_mode
            ctx.meta = tuple(None if t is None else (tuple(t.shape), t.dtype) for t in (means3D, means2D, opacities, scales, rotations, cov3D))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        frame = ctx.frame
        device = grad_out.device
        need = ctx.needs_input_grad
        g = _f32c(grad_out)
        out = [None] * 6
        if int(frame.means3D.shape[0]) > 0:
            with torch.cuda.device(device):
                records, _scratch = _distortion_records(frame, g, ctx.saved, ctx.depth_mode)
                dm2, _, dop, dm3, dcov, _, dsc, drot = _geometry_from_records(frame, records, device)
            for k, t in enumerate((dm3, dm2, dop, dsc, drot, dcov)):
                if need[k] and ctx.meta[k] is not None and t is not None:
                    out[k] = t.view(ctx.meta[k][0]).to(ctx.meta[k][1])
        else:
            out = [None if (m is None or not need[k]) else torch.zeros(m[0], dtype=m[1], device=device) for k, m in enumerate(ctx.meta)]
        return (*out, None, None)


def distortion_map(rendered: torch.Tensor, inverse_depth: bool = False) -> torch.Tensor:
    """-> D[H,W] = sum_i sum_j w_i w_j |t_i - t_j| over the contributors of every pixel of a frame that has ALREADY been rendered: the Mip-NeRF 360
    distortion loss of 2DGS / GOF / RaDe-GS (no reference counterpart; include/gsr.h gsr_distortion), which keeps the mass of a ray in one place and
    removes floaters and semi-transparent shells.  w = alpha * T are the frame's blend weights, t the Gaussian's view-space depth z or, with
    `inverse_depth=True`, 1/z (the bounded choice for unbounded scenes).  NOT normalised: divide by the square of the alpha image of
    `return_alpha=True` for the normalised form.  `rendered` and the state it is read from are `render_features`'s: any tensor computed from one
    rasterizer call's outputs with gradients enabled, before that call's `backward()` frees the state (or with `retain_graph=True`); no second
    forward.  D is differentiable in the tensors that were PASSED TO THE RASTERIZER CALL behind `rendered` -- means3D (its depth included),
    opacities, scales + rotations or cov3D_precomp, and means2D if it was passed -- which autograd adds to what the colour loss delivers; the camera
    is a constant on this path.  The backward keeps its own references to the state: it still runs after the frame's own `backward()`.  When no
    input needs a gradient nothing is kept.  With `tile_rows`, pixels outside the band are 0 and the gradients are the band's.  Two calls give the
    same bits.  For the depth map itself see `pixel_probe` / the inverse-depth image."""
    st = _saved_state(rendered, "distortion_map", "distortion")
    frame, (means3D, means2D, opacities, scales, rotations, cov3D) = _geometry_frame(st)
    return _Distortion.apply(means3D, means2D, opacities, scales, rotations, cov3D, frame, 1 if inverse_depth else 0)


def _mark_visible(points: torch.Tensor, name: str, viewmatrix, projmatrix) -> torch.Tensor:
    """gsr_mark_visible -> bool[P]: in front of the near plane (the reference's checkFrustum with prefiltered = False)."""
    lib = _lib.load()
    _require_cuda(points, name)
    with torch.no_grad(), torch.cuda.device(points.device):
        pos, vm, pm = _f32c(points), _f32c(viewmatrix), _f32c(projmatrix)
        present = torch.empty(pos.shape[0], dtype=torch.uint8, device=pos.device)
        _lib.check(lib.gsr_mark_visible(int(pos.shape[0]), _ptr(pos), _ptr(vm), _ptr(pm), _ptr(present), _stream_ptr(pos.device)),
                   "gsr_mark_visible")
    return present.bool()


# ---- opt-in: the Adam step of the two SH tensors inside the backward (gsr_backward_preprocess_sh_adam) --------------------------
_SH_ADAM = {}      # id(rest parameter) -> _ShAdamFusion


class _ShAdamFusion:
    """Registered by `fuse_sh_adam_into_backward`.  While it is active, a rasterizer call in the reference's separate_sh form whose
    `dc=` / `shs=` arguments ARE the two registered leaf parameters does not return their gradients from backward: the per-Gaussian
    backward kernel applies the optimizer's update to them in place (and to the optimizer's moments), bit for bit what
    `optimizer.step()` would have done with the gradient, which therefore never travels to HBM and back.  `optimizer.step()`
    afterwards skips the two tensors (their .grad is None) and steps the rest as usual."""

    def __init__(self, optimizer, dc, rest):
        import weakref
        self.optimizer, self.dc, self.rest = optimizer, weakref.ref(dc), weakref.ref(rest)
        self.sparse = isinstance(optimizer, SparseGaussianAdam)
        self.key = id(rest)

    def matches(self, dc, rest):
        return self.dc() is dc and self.rest() is rest

    def remove(self):
        _SH_ADAM.pop(self.key, None)

    def _group(self, param):
        for g in self.optimizer.param_groups:
            if any(q is param for q in g["params"]):
                return g
        raise GsrError("fused SH Adam: the parameter is not in the optimizer any more (re-register after densification)")

    def arm(self):
        """Moments (created on first use), hyper-parameters and -- dense Adam -- the incremented step counts as a _lib.ShAdam."""
        dc, rest = self.dc(), self.rest()      # (the Parameter objects: the optimizer's state is keyed by them)
        if dc is None or rest is None:
            raise GsrError("fused SH Adam: a registered parameter no longer exists")
        st = []
        for q in (dc, rest):
            s_ = self.optimizer.state[q]
            if len(s_) == 0:
                s_["step"] = torch.tensor(0.0, dtype=torch.float32) if self.sparse else 0
                s_["exp_avg"] = torch.zeros_like(q, memory_format=torch.contiguous_format)
                s_["exp_avg_sq"] = torch.zeros_like(q, memory_format=torch.contiguous_format)
            if not self.sparse:
                s_["step"] = int(s_["step"]) + 1
            st.append(s_)
        g_dc, g_rest = self._group(dc), self._group(rest)
        b1, b2 = (0.9, 0.999) if self.sparse else g_rest["betas"]
        if not self.sparse and tuple(g_dc["betas"]) != tuple(g_rest["betas"]) or g_dc["eps"] != g_rest["eps"]:
            raise GsrError("fused SH Adam: the two SH parameter groups must share betas and eps")
        return _lib.ShAdam(st[0]["exp_avg"].data_ptr(), st[0]["exp_avg_sq"].data_ptr(), st[1]["exp_avg"].data_ptr(),
                           st[1]["exp_avg_sq"].data_ptr(), float(g_dc["lr"]), float(g_rest["lr"]), float(b1), float(b2),
                           float(g_rest["eps"]), 0 if self.sparse else int(st[0]["step"]), 0 if self.sparse else int(st[1]["step"]),
                           1 if self.sparse else 0, 0)


def fuse_sh_adam_into_backward(optimizer, dc_param, rest_param):
    """OPT-IN (no reference counterpart): from now on `loss.backward()` applies `optimizer`'s step to `dc_param` ([P,1,3]) and
    `rest_param` ([P,15,3]) itself when they reach the rasterizer as `dc=` / `shs=` (gaussian_renderer/__init__.py:82-100,
    separate_sh).  `optimizer` is a `SparseGaussianAdam` (rows with radii > 0, as `step(radii > 0, N)` would) or a
    `gsr_optim.FusedAdam` / `torch.optim.Adam`-configured optimizer (every row).  One backward per step; call `.remove()` on the
    returned handle -- or register the new parameters -- when densification replaces the tensors."""
    ent = _ShAdamFusion(optimizer, dc_param, rest_param)
    _SH_ADAM[ent.key] = ent
    return ent


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, tile_rows, grad_sync, dc, viewmatrix=None, projmatrix=None, campos=None, bg=None, return_alpha=False,
                absgrad=False):
        # viewmatrix / projmatrix / campos / bg: raster_settings' own tensors, passed again so that autograd sees them (camera gradients,
        # gsr_backward_preprocess_camera; background gradient, gsr_backward_blend_composite).  The kernels read them from raster_settings.
        _lib.load()      # (a missing library is reported before anything else)
        _require_cuda(means3D, "means3D")
        _trim_cache_if_pending()
        device = means3D.device
        P = int(means3D.shape[0])
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        means3D_c, sh_c, col_c = _f32c(means3D), _f32c(sh), _f32c(colors_precomp)
        op_c, sc_c, rot_c, cov_c = _f32c(opacities), _f32c(scales), _f32c(rotations), _f32c(cov3Ds_precomp)
        dc_c = _f32c(dc)
        # split form: dc[P,1,3] + sh[P,M-1,3].  The kernels take it natively for degree-3 storage (M == 16).  A model
        # with max_sh_degree 0 has an empty `sh`: the DC tensor then IS the fused [P,1,3] record ("as_sh").  Other small
        # records (M = 4, 9) or unaligned views are concatenated like the reference's own get_features
        # (scene/gaussian_model.py:121-125) and the gradient is split again in backward ("cat").
        ctx.dc_mode = "none"
        if dc_c is not None:
            if sh_c is None or sh_c.numel() == 0 or sh_c.shape[1] == 0:
                ctx.dc_mode = "as_sh"
                sh_c, dc_c = dc_c.view(P, 1, 3), None
            elif sh_c.shape[1] + 1 != 16 or dc_c.data_ptr() % 16 or sh_c.data_ptr() % 16:
                ctx.dc_mode = "cat"
                sh_c, dc_c = torch.cat([dc_c.view(P, 1, 3), sh_c], dim=1), None
            else:
                ctx.dc_mode = "split"
        M = int(sh_c.shape[1]) if sh_c is not None and sh_c.dim() == 3 else 0
        if dc_c is not None:
            M += 1
        # background: [3] (the reference's form) or a per-pixel image [3,H,W]; either may require grad (passed again as `bg`)
        bg_c = _f32c(raster_settings.bg)
        ctx.bg_image = bg_c.dim() == 3      # (the shape itself is checked by _make_settings)
        ctx.bg_grad = bool(len(ctx.needs_input_grad) > 15 and ctx.needs_input_grad[15])
        if grad_sync is not None and (ctx.bg_image or ctx.bg_grad or return_alpha):
            raise GsrError("the alpha image, a per-pixel background and the background gradient are not supported together with grad_sync "
                           "(multi-GPU renderers): detach / broadcast the background and call without return_alpha")
        # absgrad: the backward also leaves sum over pixels of |per-pixel dL/dmeans2D| in means2D.absgrad (gsr_backward_blend_abs)
        ctx.absgrad = bool(absgrad)
        if ctx.absgrad and (means2D is None or not means2D.requires_grad):      # (the tensor's own flag: a render under no_grad is fine)
            raise ValueError("absgrad=True needs a means2D tensor that requires grad (the reference's screenspace_points): the backward "
                             "leaves the absolute gradient in its .absgrad attribute")
        if ctx.absgrad and grad_sync is not None:
            raise GsrError("absgrad is not supported together with grad_sync (multi-GPU renderers): use the single-GPU rasterizer for it")
        ctx.means2D_ref = means2D if ctx.absgrad else None      # the caller's own tensor: backward sets its .absgrad
        # the caller's own geometry tensors (the saved ones are converted copies when an fp32 / contiguity conversion happened):
        # render_features(geometry=True) sends its gradients to these
        ctx.geom_inputs = (means3D, means2D, opacities, scales, rotations, cov3Ds_precomp)
        # the composite entry point only when something beyond the reference's contract is asked for
        composite = bool(return_alpha) or ctx.bg_image or ctx.bg_grad
        keep: list = []
        with torch.cuda.device(device):
            # inside autograd.Function.forward grad mode is off; needs_input_grad tells whether a backward can follow
            ctx.camera_grad = any(ctx.needs_input_grad[12:15])
            no_backward = not (any(ctx.needs_input_grad[:8]) or ctx.needs_input_grad[11] or ctx.camera_grad or ctx.bg_grad)
            s = _make_settings(raster_settings, keep, tile_rows, no_backward, bg_image=grad_sync is None)
            if dc_c is not None:
                s.sh_dc = dc_c.data_ptr()
            color = torch.empty(3, H, W, dtype=torch.float32, device=device)
            invdepth = torch.empty(1, H, W, dtype=torch.float32, device=device)
            alpha = torch.empty(1, H, W, dtype=torch.float32, device=device) if return_alpha else None
            if tile_rows is not None:   # rows outside the band are not written by the kernels
                color.zero_()
                invdepth.zero_()
                if alpha is not None:
                    alpha.zero_()
            extra = _lib.CompositeOut(alpha.data_ptr() if alpha is not None else None, bg_c.data_ptr() if ctx.bg_image else None) if composite else None
            radii = torch.empty(P, dtype=torch.int32, device=device)
            cpu_args = _cpu_copy((means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                  raster_settings)) if raster_settings.debug else None
            try:
                fwd = _rasterize_forward(s, P, M, (means3D_c, sh_c, col_c, op_c, sc_c, rot_c, cov_c), color, invdepth, radii, device, extra=extra)
            except Exception:
                if cpu_args is not None:
                    torch.save(cpu_args, "snapshot_fw.dump")
                    print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise
        ctx.raster_settings = raster_settings
        ctx.tile_rows = tile_rows
        ctx.grad_sync = grad_sync
        ctx.num_rendered = fwd.num_rendered
        global _last_R, _max_R
        _last_R = ctx.num_rendered
        _max_R = max(_max_R, _last_R)
        ctx.M = M
        ctx.op_shape = tuple(opacities.shape)
        ctx.has_means2D = means2D is not None
        ctx.flags = (sh_c is not None, colors_precomp is not None, scales is not None, rotations is not None,
                     cov3Ds_precomp is not None)
        ctx.has_dc = dc_c is not None
        ctx.sh_adam = None
        if ctx.dc_mode == "split" and grad_sync is None and colors_precomp is None and _SH_ADAM:
            ent = _SH_ADAM.get(id(sh))
            if ent is not None and ent.matches(dc, sh) and sh_c is sh and dc_c is dc and sh.requires_grad and dc.requires_grad:
                ctx.sh_adam = ent
        if ctx.sh_adam is not None and ctx.camera_grad:
            raise GsrError("camera gradients (viewmatrix / projmatrix / campos requiring grad) cannot be combined with the SH Adam step "
                           "fused into the backward (fuse_sh_adam_into_backward): remove the fusion or detach the camera tensors")
        ctx.cam_meta = tuple((t.shape, t.dtype) if t is not None else None for t in (viewmatrix, projmatrix, campos))
        ctx.bg_meta = (bg.shape, bg.dtype) if bg is not None else None
        ctx.return_alpha = bool(return_alpha)
        ctx.sh_given = sh is not None
        ctx.dc_shape = tuple(dc.shape) if dc is not None else None
        ctx.save_for_backward(means3D_c, sh_c if sh_c is not None else means3D_c.new_empty(0),
                              col_c if col_c is not None else means3D_c.new_empty(0), op_c,
                              sc_c if sc_c is not None else means3D_c.new_empty(0),
                              rot_c if rot_c is not None else means3D_c.new_empty(0),
                              cov_c if cov_c is not None else means3D_c.new_empty(0),
                              radii, fwd.geom, fwd.binning, fwd.img,
                              dc_c if dc_c is not None else means3D_c.new_empty(0),
                              bg_c if ctx.bg_image else means3D_c.new_empty(0))
        ctx.mark_non_differentiable(radii)
        # an output nobody differentiates through (the inverse-depth image unless depth supervision is on, train.py:130-137)
        # arrives in backward as None instead of a materialised zero image: the blend backward then runs its build without
        # the 1/depth terms ("skip the invdepth terms when it is all-zero / None")
        ctx.set_materialize_grads(False)
        if return_alpha:
            return color, radii, invdepth, alpha
        return color, radii, invdepth

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_out_depth, grad_out_alpha=None):
        lib = _lib.load()
        (means3D, sh, col, op, sc, rot, cov, radii, geom, binning, img, dc, bg_img) = ctx.saved_tensors
        if grad_out_color is None:          # only the inverse-depth and / or the alpha image was used
            rs_ = ctx.raster_settings
            grad_out_color = torch.zeros(3, int(rs_.image_height), int(rs_.image_width), dtype=torch.float32, device=means3D.device)
        has_sh, has_col, has_sc, has_rot, has_cov = ctx.flags
        rs = ctx.raster_settings
        device = means3D.device
        P = int(means3D.shape[0])
        M = ctx.M
        has_dc = ctx.has_dc
        fused_adam = ctx.sh_adam if (ctx.sh_adam is not None and _SH_ADAM.get(ctx.sh_adam.key) is ctx.sh_adam) else None
        # (intermediates of the kernel unless they are inputs' grads: dL_dcolors, dL_dcov3D)
        grads, dL_ddc = _gradients(P, device, has_col, has_cov, (M - 1 if has_dc else M) if (has_sh and fused_adam is None) else None,
                                   has_dc and fused_adam is None, has_sc, has_rot)
        cam_out = cam_scratch = None
        if ctx.camera_grad:      # [16] view, [16] projection, [3] campos (64-byte offsets), fp32
            cam_out = torch.zeros(48, dtype=torch.float32, device=device)
            cam_scratch = torch.empty(max(int(lib.gsr_camera_grad_scratch_bytes(P)), 8), dtype=torch.uint8, device=device)
        # the composite blend backward only when the loss reaches the alpha image, the background is per pixel or its gradient is wanted:
        # a colour / depth loss over a constant background runs what it ran before return_alpha existed
        comp = dL_dbg = g_alpha = comp_scratch = None
        if grad_out_alpha is not None or ctx.bg_image or ctx.bg_grad:
            H, W = int(rs.image_height), int(rs.image_width)
            g_alpha = _f32c(grad_out_alpha)
            if ctx.bg_grad:      # [3,H,W] products, or their sums [3] with the reduction's scratch
                dL_dbg = torch.empty((3, H, W) if ctx.bg_image else (3,), dtype=torch.float32, device=device)
                if not ctx.bg_image:
                    comp_scratch = torch.empty(max(int(lib.gsr_composite_grad_scratch_bytes(W, H)), 8), dtype=torch.uint8, device=device)
            comp = _lib.CompositeGrads(_ptr(g_alpha), _ptr(bg_img) if ctx.bg_image else None,
                                       _ptr(dL_dbg) if ctx.bg_image else None, None if ctx.bg_image else _ptr(dL_dbg), _ptr(comp_scratch))
        g_color = _f32c(grad_out_color)
        keep: list = []
        if P == 0 and ctx.bg_grad:      # no Gaussian: T_final = 1 everywhere, the forward kept no state
            with torch.cuda.device(device):
                _backward_blend(_make_settings(rs, keep, ctx.tile_rows, bg_image=True), 0, _Forward(None, None, None, 0), g_color, None, device, comp)
        if P > 0:
            g_depth = _f32c(grad_out_depth)
            with torch.cuda.device(device):
                s = _make_settings(rs, keep, ctx.tile_rows, bg_image=ctx.bg_image)
                if has_dc:
                    s.sh_dc = dc.data_ptr()
                    s.dL_dsh_dc = dL_ddc.data_ptr() if dL_ddc is not None else None
                inputs = (means3D, sh if has_sh else None, col if has_col else None, op, sc if has_sc else None, rot if has_rot else None,
                          cov if has_cov else None)
                fwd = _Forward(geom, binning, img, ctx.num_rendered)
                cpu_args = _cpu_copy((means3D, radii, col, sc, rot, cov, sh, grad_out_color, rs)) if rs.debug else None
                try:
                    if fused_adam is None and not ctx.camera_grad and ctx.grad_sync is None and comp is None and not ctx.absgrad:
                        _rasterize_backward(s, P, M, inputs, radii, fwd, g_color, g_depth, grads, device)
                    else:
                        # blend backward -> (multi-GPU: sum of the 48-byte per-Gaussian records across ranks, parallel.py) -> the
                        # per-Gaussian backward that also sums the camera gradient, or steps the two SH tensors in place
                        records = _backward_blend(s, P, fwd, g_color, g_depth, device, comp, ctx.absgrad)
                        if ctx.grad_sync is not None:
                            ctx.grad_sync(records)
                        if ctx.absgrad:      # gsplat's convention: overwritten by every backward, never accumulated
                            ctx.means2D_ref.absgrad = _absgrad_from_records(s, P, records, device)
                        if fused_adam is not None:
                            extra = fused_adam.arm()
                        elif ctx.camera_grad:
                            extra = _lib.CameraGrads(cam_out.data_ptr(), cam_out.data_ptr() + 64, cam_out.data_ptr() + 128,
                                                     cam_scratch.data_ptr())
                        else:
                            extra = None
                        _backward_preprocess(s, P, M, inputs, radii, geom, records, grads, device, extra)
                except Exception:
                    if cpu_args is not None:
                        torch.save(cpu_args, "snapshot_bw.dump")
                        print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                    raise
        if ctx.absgrad and P == 0:
            ctx.means2D_ref.absgrad = torch.zeros(0, 3, dtype=torch.float32, device=device)
        dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drot = grads
        dL_dopacity = dL_dopacity.view(ctx.op_shape)
        if ctx.dc_mode == "as_sh":      # the DC tensor travelled as the fused [P,1,3] form
            dL_ddc = dL_dsh.view(ctx.dc_shape)
            dL_dsh = dL_dsh.new_zeros(P, 0, 3) if ctx.sh_given else None
        elif ctx.dc_mode == "cat":
            dL_ddc = dL_dsh[:, :1].reshape(ctx.dc_shape)
            dL_dsh = dL_dsh[:, 1:]
        elif has_dc and dL_ddc is not None:
            dL_ddc = dL_ddc.view(ctx.dc_shape)
        cam_grads = (None, None, None)
        if ctx.camera_grad:
            cam_grads = tuple(None if (meta is None or not ctx.needs_input_grad[12 + k]) else
                              cam_out[16 * k:16 * k + (3 if k == 2 else 16)].reshape(meta[0]).to(meta[1])
                              for k, meta in enumerate(ctx.cam_meta))
        if dL_dbg is not None:
            dL_dbg = dL_dbg.reshape(ctx.bg_meta[0]).to(ctx.bg_meta[1])
        return (dL_dmeans3D, dL_dmeans2D if ctx.has_means2D else None, dL_dsh, dL_dcolors if has_col else None, dL_dopacity, dL_dscales, dL_drot,
                dL_dcov3D if has_cov else None, None, None, None, dL_ddc) + cam_grads + (dL_dbg, None, None)


def _cpu_copy(args):
    return tuple(a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, tile_rows: Optional[Tuple[int, int]] = None, grad_sync=None, dc=None, return_alpha: bool = False,
                        absgrad: bool = False):
    """Functional form.  `grad_sync(records[P,12])`, if given, is called between the blend backward and the
    per-Gaussian backward (multi-GPU: all-reduce of the 48-byte gradient records, parallel.py).
    `tile_rows=(y0, y1)` (extension) restricts binning + blending to that
    band of 16-pixel tile rows; pixels outside the band come back as zeros.  `dc` (the reference's separate_sh
    form): SH coefficient 0 as [P,1,3]; `sh` then holds coefficients 1.. as [P,M-1,3].
    Camera gradients (no reference counterpart): when raster_settings.viewmatrix / projmatrix / campos require grad, backward
    returns their gradients too (include/gsr.h gsr_backward_preprocess_camera; with `tile_rows`, the band's contribution).
    Alpha image and background (no reference counterpart, include/gsr.h gsr_rasterize_forward_composite): `return_alpha=True` returns
    `(color, radii, invdepth, alpha)` with the differentiable accumulated opacity alpha[1,H,W] = 1 - T_final.  raster_settings.bg may be
    [3] or a per-pixel image [3,H,W]; when it requires grad, backward returns its gradient (with `tile_rows`, the band's contribution).
    Not available with `grad_sync` (GsrError).
    Absolute screen-space gradients (no reference counterpart, include/gsr.h gsr_backward_blend_abs; AbsGS, gsplat's `absgrad`):
    with `absgrad=True` every backward also sets `means2D.absgrad`, a fresh [P,3] fp32 tensor (overwritten, never accumulated) =
    (0.5 W sum_p |dL/dpx per pixel|, 0.5 H sum_p |dL/dpy per pixel|, 0) -- the units and layout of means2D.grad, whose signed sums
    cancel under a large Gaussian over fine detail.  Every gradient is the bits of the same call with absgrad=False.  means2D must
    require grad (ValueError); not available with `grad_sync` (GsrError); with `tile_rows`, the band's contribution."""
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, tile_rows, grad_sync, dc, raster_settings.viewmatrix,
                                     raster_settings.projmatrix, raster_settings.campos, raster_settings.bg, bool(return_alpha), bool(absgrad))


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings, return_alpha: bool = False, absgrad: bool = False):
        """`return_alpha=True` (opt-in, no reference counterpart): the call returns `(color, radii, invdepth, alpha)`, alpha[1,H,W] being the
        differentiable accumulated opacity 1 - T_final (rasterize_gaussians).  `absgrad=True` (opt-in, no reference counterpart): every
        backward also sets `means2D.absgrad`, the absolute screen-space gradient of AbsGS (rasterize_gaussians)."""
        super().__init__()
        self.raster_settings = raster_settings
        self.return_alpha = bool(return_alpha)
        self.absgrad = bool(absgrad)

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """bool[P]: in front of the near plane (the reference's mark_visible / checkFrustum)."""
        return _mark_visible(positions, "positions", self.raster_settings.viewmatrix, self.raster_settings.projmatrix)

    def forward(self, means3D, means2D, opacities, dc=None, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if dc is not None and shs is None:
            raise Exception('dc (SH coefficient 0) was given without shs (the remaining coefficients)!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, getattr(self, "tile_rows", None), None, dc, self.return_alpha, self.absgrad)


    def _tracking_forward(self, means3D, opacities, scales, rotations, cov3D_precomp):
        """-> (settings, P, _Forward, radii, keep): a tracking forward with zero colours (call it under no_grad and the device guard); honours
        `tile_rows`.  `keep` holds what the settings point to."""
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        rs = self.raster_settings
        device, P = means3D.device, int(means3D.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        keep: list = []
        s = _make_settings(rs, keep, getattr(self, "tile_rows", None), no_backward=False, bg_image=True)
        inputs = (_f32c(means3D.detach()), None, torch.zeros(P, 3, dtype=torch.float32, device=device), _f32c(opacities.detach()),
                  _f32c(scales.detach()) if scales is not None else None, _f32c(rotations.detach()) if rotations is not None else None,
                  _f32c(cov3D_precomp.detach()) if cov3D_precomp is not None else None)
        color = torch.empty(3, H, W, dtype=torch.float32, device=device)
        invdepth = torch.empty(1, H, W, dtype=torch.float32, device=device)
        radii = torch.empty(P, dtype=torch.int32, device=device)
        return s, P, _rasterize_forward(s, P, 0, inputs, color, invdepth, radii, device), radii, keep

    def contributions(self, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, pixel_weight=None,
                      into: Optional[ContributionStats] = None):
        """-> (ContributionStats, radii[P]): the statistics of `contribution_stats` for this camera without a render of one's own to hand
        (no reference counterpart): runs a tracking forward with zero colours under no_grad, honours `tile_rows`, keeps nothing."""
        _lib.load()
        _require_cuda(means3D, "means3D")
        rs = self.raster_settings
        device = means3D.device
        pw = _pixel_weight(pixel_weight, int(rs.image_height), int(rs.image_width), device)
        with torch.no_grad(), torch.cuda.device(device):
            s, P, fwd, radii, _keep = self._tracking_forward(means3D, opacities, scales, rotations, cov3D_precomp)
            return _contribution_stats(s, P, fwd, pw, into, device), radii

    def probe(self, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, threshold: float = 0.5):
        """-> (PixelProbe, radii[P]): the per-pixel probe of `pixel_probe` for this camera without a render of one's own to hand (no reference
        counterpart): runs a tracking forward with zero colours under no_grad, honours `tile_rows`, keeps nothing."""
        _lib.load()
        _require_cuda(means3D, "means3D")
        rs = self.raster_settings
        device = means3D.device
        with torch.no_grad(), torch.cuda.device(device):
            s, P, fwd, radii, _keep = self._tracking_forward(means3D, opacities, scales, rotations, cov3D_precomp)
            return _pixel_probe(s, P, fwd, threshold, int(rs.image_height), int(rs.image_width), device), radii

    def features(self, means3D, opacities, features, scales=None, rotations=None, cov3D_precomp=None, geometry: bool = False):
        """-> (F[C,H,W], radii[P]): `render_features` for this camera without a render of one's own to hand (no reference counterpart): runs a
        tracking forward with zero colours under no_grad, honours `tile_rows`, then blends `features` [P,C] with its weights.  Differentiable in
        `features` only: no gradient reaches the geometry or the opacities through F -- unless `geometry=True`, which makes F (same bits)
        differentiable in means3D, opacities and scales + rotations / cov3D_precomp as well (`render_features`)."""
        _lib.load()
        _require_cuda(means3D, "means3D")
        device = means3D.device
        features = _feature_rows(features, int(means3D.shape[0]), device)
        tile_rows = getattr(self, "tile_rows", None)
        with torch.no_grad(), torch.cuda.device(device):
            _s, _P, fwd, radii, _keep = self._tracking_forward(means3D, opacities, scales, rotations, cov3D_precomp)
        if not geometry:
            return _RenderFeatures.apply(features, fwd.geom, fwd.binning, fwd.img, fwd.num_rendered, self.raster_settings, tile_rows), radii
        c = lambda t: _f32c(t.detach()) if t is not None else None      # noqa: E731  (what the tracking forward read)
        frame = _FeatureFrame(self.raster_settings, tile_rows, fwd, radii, c(means3D), c(opacities), c(scales), c(rotations), c(cov3D_precomp))
        return _RenderFeaturesGeometry.apply(features, means3D, None, opacities, scales, rotations, cov3D_precomp, frame), radii

    def distortion(self, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, inverse_depth: bool = False):
        """-> (D[H,W], radii[P]): `distortion_map` for this camera without a render of one's own to hand (no reference counterpart): runs a tracking
        forward with zero colours under no_grad, honours `tile_rows`, then the distortion loss on its state, differentiable in means3D, opacities and
        scales + rotations / cov3D_precomp."""
        _lib.load()
        _require_cuda(means3D, "means3D")
        device = means3D.device
        tile_rows = getattr(self, "tile_rows", None)
        with torch.no_grad(), torch.cuda.device(device):
            _s, _P, fwd, radii, _keep = self._tracking_forward(means3D, opacities, scales, rotations, cov3D_precomp)
        c = lambda t: _f32c(t.detach()) if t is not None else None      # noqa: E731  (what the tracking forward read)
        frame = _FeatureFrame(self.raster_settings, tile_rows, fwd, radii, c(means3D), c(opacities), c(scales), c(rotations), c(cov3D_precomp))
        return _Distortion.apply(means3D, None, opacities, scales, rotations, cov3D_precomp, frame, 1 if inverse_depth else 0), radii


class SparseGaussianAdam(torch.optim.Adam):
    """`SparseGaussianAdam(params, lr, eps).step(visibility, N)` (scene/gaussian_model.py:194-196, train.py:180-183):
    Adam that updates only the rows of Gaussians that were visible in this iteration; parameter and both moments of the
    others stay untouched.  One fused HIP launch for all parameter groups (gsr_sparse_adam_step_multi; round 5 -- one launch per group before).  State layout
    (`step`, `exp_avg`, `exp_avg_sq`) is torch.optim.Adam's, so the optimizer-state surgery of
    scene/gaussian_model.py:316-405 (prune / cat / replace) works unchanged.
    [RECALLED -- the accelerated rasterizer's source is not vendored] betas are fixed at (0.9, 0.999) and there is no
    bias correction; parity for this class is unpinned."""

    def __init__(self, params, lr, eps):
        super().__init__(params=params, lr=lr, eps=eps)

    @torch.no_grad()
    def step(self, visibility, N):
        lib = _lib.load()
        N = int(N)
        vis = visibility.reshape(-1)
        if vis.dtype == torch.bool:
            vis = vis.contiguous().view(torch.uint8)      # a bool tensor IS one byte per element: no conversion kernel
        elif vis.dtype != torch.uint8:
            vis = vis.to(torch.uint8)
        vis = vis.contiguous()
        by_device: dict = {}      # device -> [(param, grad, state, M, lr, eps)]: ONE launch per device (gsr_sparse_adam_step_multi)
        for group in self.param_groups:
            lr, eps = group["lr"], group["eps"]
            assert len(group["params"]) == 1, "more than one tensor in group"
            param = group["params"][0]
            if param.grad is None:
                continue
            _require_cuda(param, "parameter")
            if param.dtype != torch.float32 or not param.is_contiguous():
                raise GsrError("SparseGaussianAdam needs contiguous fp32 parameters")
            state = self.state[param]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
            M = param.numel() // N if N > 0 else 0
            if N > 0 and (param.numel() != N * M or vis.numel() != N):
                raise GsrError(f"parameter of {param.numel()} elements / visibility of {vis.numel()} do not match N = {N}")
            g = param.grad if param.grad.is_contiguous() else param.grad.contiguous()
            by_device.setdefault(param.device, []).append((param, g, state, M, float(lr), float(eps)))
        for dev, items in by_device.items():
            arr = (_lib.SparseAdamTensor * len(items))()
            for k, (param, g, state, M, lr, eps) in enumerate(items):
                arr[k] = _lib.SparseAdamTensor(param.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), M, lr, eps)
            with torch.cuda.device(dev):
                _lib.check(lib.gsr_sparse_adam_step_multi(arr, len(items), _ptr(vis), N, 0.9, 0.999, _stream_ptr(dev)), "gsr_sparse_adam_step_multi")
