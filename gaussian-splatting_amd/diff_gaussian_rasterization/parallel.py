"""Sharding of the rasterizer across the GPUs of one node (net-new: the reference has no
multi-GPU code).  None of these entry points returns camera gradients: viewmatrix / projmatrix / campos enter them
detached, whatever their requires_grad (the single-process rasterize_gaussians(tile_rows=...) returns a band's share).  One process per GPU, torch.distributed (backend "nccl" = RCCL over xGMI on ROCm, "gloo" in the CPU
tests).  Three modes:

A. TWO-AXIS (training; `render_two_axis`, SURVEY 8(e) as specified)
  * Gaussian axis: rank g owns P/G Gaussians -- parameters, optimizer state, the per-Gaussian forward
    (gsr_preprocess_forward) and backward (gsr_backward_preprocess) -- nothing of size O(59 P) ever crosses ranks;
  * pixel axis: rank g owns a contiguous band of 16-pixel tile ROWS [y0_g, y1_g), balanced by the per-row instance
    counts (BandPlan), and runs binning + blending on it (gsr_rasterize_from_splats, gsr_backward_blend);
  * forward : all-gather of the 64-byte splat records, then ONE all-gather of the rendered strips;
  * backward: the blend backward yields per-Gaussian 48-byte gradient records for ALL Gaussians from the own band;
    reduce-scatter (sum) hands every rank the totals of its own shard.

B. REPLICATED PARAMETERS, BANDS ONLY (forward-only rendering; `render_sharded`, bench.py's forward metric)
  * every rank holds all parameters and runs the HBM-streaming preprocess on all P (SH colours are evaluated only for
    Gaussians that touch the rank's band): for a forward-only frame re-running the preprocess (0.085 ms at 1 M) is
    cheaper than all-gathering 64 MB of records and takes one collective off the critical path;
  * forward: ONE all_gather of the rendered strips (asynchronous form: gather_strips_async, frames pipelined);
  * backward (optional): ONE all_reduce of the [P,12] records, per-Gaussian backward replicated.

C. GAUSSIAN-SHARDED WITH A DESTINATION-TARGETED EXCHANGE (round 3; `render_gaussian_sharded`, bench.py --gpus N)
  * as A, but a projected splat travels only to the ranks whose band its tile rectangle touches: per-band stable
    compaction into 48-byte packed records (gsr_route_count / gsr_route_pack), ONE variable-size all-to-all
    (all_to_all_single) instead of the all-gather of every record, and the receiving rank bins + blends
    (gsr_rasterize_from_packed) only the Gaussians of its band -- depth sort, scan, emission and tile sort shrink with
    the band, which the replicated / all-gathered forms A and B cannot do;
  * backward: blend backward on the received set -> the reverse all-to-all of the 48-byte gradient rows ->
    gsr_route_return adds them into the shard's [P,12] record (band order, no atomics) -> per-Gaussian backward;
  * exact form: the G x G count matrix (all-gather of G counters) is read back by the host to size the variable all-to-all;
  * FIXED-CAPACITY form (round 4, `set_exchange_mode("fixed")`): every (source, band) pair owns a segment of capacity + 1 rows
    with the count in a header row, so the all-to-all has equal splits and NO count travels to the host.  The capacity is
    learned from exact frames (largest entry of the count matrix x slack -- the same number on every rank); whether any segment
    overflowed is all-reduced on the device and reaches the host with the frame's R read-back, which the frame has anyway; an
    overflowing frame is repeated in the exact form by every rank and raises the capacity (ExchangePolicy).

The band renderer / the two stages are injectable, so the index math and the collectives are tested on CPU with gloo
and the oracle (tests/test_parallel_gloo.py); `hip_band_renderer` and `_TwoAxisHip` are the product's.
"""
from __future__ import annotations

import ctypes as C
import sys
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import _lib
from . import (_Forward, _backward_blend, _backward_preprocess, _f32c, _gradients, _make_settings, _preprocess_shard, _ptr,
               _rasterize_records, rasterize_gaussians)

_pkg = sys.modules[__package__]      # (`_stream_ptr` is looked up on the package at call time, like its own code does)

TILE = 16


@dataclass
class BandPlan:
    """Contiguous tile-row bands, one per rank (bands may be empty)."""
    bounds: List[int]            # len = world+1, bounds[g]..bounds[g+1]

    @staticmethod
    def uniform(n_rows: int, world: int) -> "BandPlan":
        return BandPlan([(n_rows * g) // world for g in range(world + 1)])

    @staticmethod
    def balanced(row_cost: Sequence[float], world: int) -> "BandPlan":
        """Split rows so that every band carries ~1/world of the total cost (prefix-sum cut points)."""
        n = len(row_cost)
        total = float(sum(row_cost))
        if total <= 0 or world == 1:
            return BandPlan.uniform(n, world)
        cum = [0.0]
        for c in row_cost:
            cum.append(cum[-1] + float(c))
        bounds = [0]
        for g in range(1, world):
            target = total * g / world
            r = bounds[-1]
            while r < n and cum[r + 1] <= target:
                r += 1
            # r = last cut with cum[r] <= target; take the nearer of r / r+1
            if r < n and (cum[r + 1] - target) < (target - cum[r]):
                r += 1
            bounds.append(max(r, bounds[-1]))
        bounds.append(n)
        return BandPlan(bounds)

    def band(self, rank: int) -> Tuple[int, int]:
        return self.bounds[rank], self.bounds[rank + 1]

    def pixel_rows(self, rank: int, H: int) -> Tuple[int, int]:
        y0, y1 = self.band(rank)
        return min(y0 * TILE, H), min(y1 * TILE, H)


def _world(group) -> int:
    return dist.get_world_size(group) if dist.is_initialized() else 1


class StripGather:
    """An all-gather of image strips in flight (gather_strips_async).  wait() returns the full [C,H,W] image."""

    def __init__(self, local, recv, rows, work):
        self._local, self._recv, self._rows, self._work = local, recv, rows, work

    def wait(self) -> torch.Tensor:
        if self._work is None:
            return self._local
        self._work.wait()          # RCCL: the current stream waits for the collective; the host does not block
        recv, rows = self._recv, self._rows
        # one concatenation instead of one copy per rank; padding rows of the shorter strips are dropped
        full = torch.cat([recv[g, :, : gb - ga] for g, (ga, gb) in enumerate(rows)], dim=1)
        self._work = None
        self._local = full
        return full


_exact_strips_default: Optional[bool] = None      # None: exact sizes iff the backend is "nccl"; set by set_exact_strips()


def set_exact_strips(flag: Optional[bool]) -> None:
    """Force the padded (False) or the exact-size (True) strip all-gather, e.g. after probe_collectives() found that the
    backend refuses all_gather with unequal tensors."""
    global _exact_strips_default
    _exact_strips_default = flag


class _StripGatherList:
    """Exact-size form of StripGather: one receive buffer per rank (dist.all_gather with unequal sizes)."""

    def __init__(self, bufs, rows, work):
        self._bufs, self._rows, self._work, self._full = bufs, rows, work, None

    def wait(self) -> torch.Tensor:
        if self._full is None:
            self._work.wait()
            self._full = torch.cat(self._bufs, dim=1)
            self._work = None
        return self._full


def gather_strips_async(local: torch.Tensor, plan: BandPlan, H: int, group=None, exact: Optional[bool] = None):
    """local: [C,H,W] with only this rank's rows valid.  Starts ONE all-gather of the strips and returns a handle with
    .wait(); the collective runs on the backend's own stream, so work enqueued afterwards (the next frame's
    rasterization) overlaps it.  Strips have different heights under a balanced plan: with RCCL (`exact`, default on
    for backend "nccl") every strip travels at its exact size (all_gather with unequal tensors = grouped broadcasts);
    otherwise -- gloo, or if the exact form is refused -- strips are padded to the tallest band."""
    world = _world(group)
    if world == 1:
        return StripGather(local, None, None, None)
    rank = dist.get_rank(group)
    C, _, W = local.shape
    rows = [plan.pixel_rows(g, H) for g in range(world)]
    heights = [b - a for a, b in rows]
    a, b = rows[rank]
    if exact is None:
        exact = _exact_strips_default if _exact_strips_default is not None else dist.get_backend(group) == "nccl"
    if exact and len(set(heights)) > 1 and min(heights) > 0:
        # No per-rank fallback here: a rank that fell back to the padded collective while its peers issued the
        # exact one would hang the job, and an asynchronous RCCL failure is not raised at the call site anyway.  Which form is
        # used is decided ONCE and collectively -- probe_collectives() tries the unequal all_gather on every rank and
        # all-reduces the outcome, the caller then calls set_exact_strips() -- and an error in the chosen form propagates.
        bufs = [local.new_empty(C, h, W) for h in heights]
        work = dist.all_gather(bufs, local[:, a:b].contiguous(), group=group, async_op=True)
        return _StripGatherList(bufs, rows, work)
    hmax = max(1, max(heights))
    send = local.new_empty(C, hmax, W)          # padding rows are never read back
    send[:, : b - a] = local[:, a:b]
    recv = local.new_empty(world, C, hmax, W)
    work = dist.all_gather_into_tensor(recv.view(-1), send.view(-1), group=group, async_op=True)   # flat: concat semantics on every backend
    return StripGather(local, recv, rows, work)


def gather_strips(local: torch.Tensor, plan: BandPlan, H: int, group=None) -> torch.Tensor:
    """Blocking form: the full [C,H,W] image on every rank."""
    return gather_strips_async(local, plan, H, group).wait()


class _GatherStrips(torch.autograd.Function):
    """forward: all_gather the strips; backward: keep only the own band's rows of dL/dpixel (the other rows belong
    to other ranks, which receive the same upstream gradient because the loss is computed replicated)."""

    @staticmethod
    def forward(ctx, local, plan, H, group):
        ctx.rows = plan.pixel_rows(dist.get_rank(group) if dist.is_initialized() else 0, H)
        return gather_strips(local, plan, H, group)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.rows
        out = torch.zeros_like(g)
        out[:, a:b] = g[:, a:b]
        return out, None, None, None


def render_sharded(render_band: Callable, inputs: Sequence, plan: BandPlan, group=None, reduce: str = "params"):
    """render_band(inputs, (y0, y1)) -> (color[3,H,W], radii[P], invdepth[1,H,W]) with only the band's rows valid
    (zeros elsewhere), differentiable w.r.t. the tensor inputs.  Returns the full image / radii / inverse depth on
    every rank.  reduce="params": the parameter gradients are summed across ranks by hooks on `inputs`;
    reduce="records": the band renderer sums its own per-Gaussian records (hip_band_renderer)."""
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    world = _world(group)
    if reduce == "params" and world > 1:
        def _mk(t):
            def _hook(g):
                g = g.contiguous().clone()
                dist.all_reduce(g, op=dist.ReduceOp.SUM, group=group)
                return g
            return _hook
        hooked = []
        for t in inputs:
            if isinstance(t, torch.Tensor) and t.requires_grad:
                v = t.view_as(t)          # non-leaf alias so that the hook fires once per backward of this render
                v.register_hook(_mk(v))
                hooked.append(v)
            else:
                hooked.append(t)
        inputs = hooked
    color, radii, invdepth = render_band(inputs, plan.band(rank))
    H = color.shape[1]
    both = _GatherStrips.apply(torch.cat([color, invdepth], dim=0), plan, H, group)
    return both[:3], radii, both[3:4]


def _camera_detached(raster_settings):
    """The multi-GPU forms return no camera and no background gradient: viewmatrix / projmatrix / campos / bg enter them detached (a
    per-band partial gradient without an all-reduce would be wrong, and summing it is out of scope).  They take the constant
    background [3] only: a per-pixel image [3,H,W] is refused (GsrError, _make_settings), and there is no alpha output."""
    t = {k: getattr(raster_settings, k) for k in ("viewmatrix", "projmatrix", "campos", "bg")}
    if not any(isinstance(v, torch.Tensor) and v.requires_grad for v in t.values()):
        return raster_settings
    return raster_settings._replace(**{k: v.detach() for k, v in t.items()})


def hip_band_renderer(raster_settings, group=None):
    """The product's band renderer: inputs = (means3D, shs, opacities, scales, rotations); the per-Gaussian 2-D
    gradient records are all-reduced between the blend backward and the per-Gaussian backward.  The camera tensors enter
    detached: no camera gradient (as every multi-GPU entry point of this module)."""
    raster_settings = _camera_detached(raster_settings)

    def _sync(records: torch.Tensor):
        if _world(group) > 1:
            dist.all_reduce(records, op=dist.ReduceOp.SUM, group=group)

    def _render(inputs, rows):
        m, sh, o, s_, r_ = inputs
        return rasterize_gaussians(m, None, sh, None, o, s_, r_, None, raster_settings, rows, _sync)

    return _render


def row_costs_from_ranges(ranges: torch.Tensor, gx: int, gy: int, group=None, banded: bool = True) -> List[float]:
    """Per tile-row instance counts for re-balancing.  With banded=True `ranges` [gx*gy,2] holds valid entries only
    for this rank's band (zeros elsewhere), so a SUM all_reduce yields the global per-row histogram."""
    cnt = (ranges[:, 1] - ranges[:, 0]).to(torch.float32).view(gy, gx).sum(dim=1)
    if banded and _world(group) > 1:
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
    # every row also costs a fixed amount (pixels to write)
    return (cnt + 256.0 * gx * 0.05).tolist()


# ------------------------------------------------------------------------------------------------------------------
# Two-axis sharding: Gaussian axis for the per-Gaussian stages, pixel axis for binning + blending.
# ------------------------------------------------------------------------------------------------------------------
def padded_shard_size(P_local: int, group=None) -> int:
    """Rows every rank contributes to the record all-gather: the largest shard, so that all_gather_into_tensor /
    reduce_scatter_tensor see equal chunks (smaller shards pad with zero rows = records without tiles)."""
    if _world(group) == 1:
        return int(P_local)
    t = torch.tensor([int(P_local)], dtype=torch.int64)
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return int(t.item())


class _AllGatherRows(torch.autograd.Function):
    """[P_pad, k] per rank -> [world * P_pad, k] on every rank; backward = reduce-scatter (sum) of the gradient rows.
    The generic (autograd) form of the record exchange -- the CPU oracle path of the gloo tests uses it; the HIP path
    (_TwoAxisHip) issues the same two collectives around its fused kernels."""

    @staticmethod
    def forward(ctx, rows, group):
        ctx.group = group
        world = _world(group)
        if world == 1:
            return rows
        out = rows.new_empty(world * rows.shape[0], *rows.shape[1:])
        dist.all_gather_into_tensor(out.view(-1), rows.contiguous().view(-1), group=group)
        return out

    @staticmethod
    def backward(ctx, g):
        world = _world(ctx.group)
        if world == 1:
            return g, None
        g = g.contiguous()
        out = g.new_empty(g.shape[0] // world, *g.shape[1:])
        if dist.get_backend(ctx.group) == "gloo":      # gloo has no reduce_scatter: all-reduce + slice (tests only)
            dist.all_reduce(g, op=dist.ReduceOp.SUM, group=ctx.group)
            r = dist.get_rank(ctx.group)
            out.copy_(g[r * out.shape[0]:(r + 1) * out.shape[0]])
        else:
            dist.reduce_scatter_tensor(out.view(-1), g.view(-1), op=dist.ReduceOp.SUM, group=ctx.group)
        return out, None


def all_gather_rows(rows: torch.Tensor, group=None) -> torch.Tensor:
    return _AllGatherRows.apply(rows, group)


def _reduce_scatter_rows(full: torch.Tensor, out: torch.Tensor, group) -> None:
    """out[P_pad, k] <- sum over ranks of full[rank * P_pad : (rank + 1) * P_pad]."""
    world = _world(group)
    if world == 1:
        out.copy_(full)
    elif dist.get_backend(group) == "gloo":
        tmp = full.clone()
        dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=group)
        r = dist.get_rank(group)
        out.copy_(tmp[r * out.shape[0]:(r + 1) * out.shape[0]])
    else:
        dist.reduce_scatter_tensor(out.view(-1), full.view(-1), op=dist.ReduceOp.SUM, group=group)


class _TwoAxisHip(torch.autograd.Function):
    """The product's two-axis renderer for one rank: local shard of Gaussians in, the rank's band of the image out.
    forward : gsr_preprocess_forward (shard) -> all-gather of 64-byte records -> gsr_rasterize_from_splats (band)
    backward: gsr_backward_blend (band; records of all Gaussians) -> reduce-scatter of 48-byte records ->
              gsr_backward_preprocess (shard)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, opacities, scales, rotations, raster_settings, band, P_pad, group, dc):
        world = _world(group)
        keep: list = []
        s, records, radii, M, (m_c, sh_c, op_c, sc_c, rot_c, dc_c) = _preprocess_shard(
            raster_settings, band, keep, int(P_pad), means3D, sh, opacities, scales, rotations, dc, "two-axis renderer")
        device = m_c.device
        with torch.cuda.device(device):
            if world > 1:
                all_records = torch.empty(world * int(P_pad), 16, dtype=torch.float32, device=device)
                dist.all_gather_into_tensor(all_records.view(-1), records.view(-1), group=group)
            else:
                all_records = records
            P_all = int(all_records.shape[0])
            color, invdepth, fwd = _rasterize_records("gsr_rasterize_from_splats", s, (P_all,), all_records, device)
        ctx.raster_settings, ctx.band, ctx.group, ctx.P_pad, ctx.P_all, ctx.M = raster_settings, band, group, int(P_pad), P_all, M
        ctx.num_rendered = fwd.num_rendered
        ctx.has_means2D = means2D is not None
        ctx.has_dc = dc_c is not None
        ctx.op_shape = tuple(opacities.shape)
        ctx.dc_shape = tuple(dc.shape) if dc is not None else None
        ctx.save_for_backward(m_c, sh_c, op_c, sc_c, rot_c, radii, fwd.geom, fwd.binning, fwd.img,
                              dc_c if dc_c is not None else m_c.new_empty(0))
        ctx.mark_non_differentiable(radii)
        return color, radii, invdepth

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth):
        m, sh, op, sc, rot, radii, geom, binning, img, dc = ctx.saved_tensors
        device = m.device
        P, P_pad, P_all, M = int(m.shape[0]), ctx.P_pad, ctx.P_all, ctx.M
        grads, d_dc = _gradients(P, device, True, True, M - 1 if ctx.has_dc else M, ctx.has_dc, True, True)
        keep: list = []
        with torch.cuda.device(device):
            s = _make_settings(ctx.raster_settings, keep, ctx.band)
            if ctx.has_dc:
                s.sh_dc, s.dL_dsh_dc = dc.data_ptr(), d_dc.data_ptr()
            full = _backward_blend(s, P_all, _Forward(geom, binning, img, ctx.num_rendered), _f32c(g_color), _f32c(g_depth), device)
            mine = torch.empty(P_pad, 12, dtype=torch.float32, device=device)
            _reduce_scatter_rows(full, mine, ctx.group)
            if P > 0:
                _backward_preprocess(s, P, M, (m, sh, None, op, sc, rot, None), radii, None, mine, grads, device)
        d_m2, _, d_op, d_m3, _, d_sh, d_sc, d_rot = grads
        return (d_m3, d_m2 if ctx.has_means2D else None, d_sh, d_op.view(ctx.op_shape), d_sc, d_rot, None, None, None, None,
                d_dc.view(ctx.dc_shape) if ctx.has_dc else None)


def render_two_axis(raster_settings, means3D, sh, opacities, scales, rotations, plan: BandPlan, P_pad: Optional[int] = None,
                    group=None, means2D=None, dc=None):
    """Two-axis sharded render of one frame: this rank's shard of Gaussians in, the FULL image (strips all-gathered)
    out.  Returns (color[3,H,W], radii[P_local], invdepth[1,H,W]); gradients flow to the rank's own shard only."""
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if P_pad is None:
        P_pad = padded_shard_size(means3D.shape[0], group)
    color, radii, invdepth = _TwoAxisHip.apply(means3D, means2D, sh, opacities, scales, rotations, raster_settings,
                                               plan.band(rank), P_pad, group, dc)
    H = color.shape[1]
    both = _GatherStrips.apply(torch.cat([color, invdepth], dim=0), plan, H, group)
    return both[:3], radii, both[3:4]


# ------------------------------------------------------------------------------------------------------------------
# C. Gaussian-sharded rendering with a destination-targeted exchange of packed splat records (round 3)
# ------------------------------------------------------------------------------------------------------------------
PACKED_WORDS = 12      # 48-byte packed record: x, y, conA, conB | conC, opacity, r, g | b, depth, rect.x bits, rect.y bits


def exchange_counts(counts: torch.Tensor, group=None) -> Tuple[List[int], List[int]]:
    """counts[G] (this rank's records per destination band, on the collective's device) -> (send_counts, recv_counts) as
    Python lists: ONE all-gather of the G counters gives every rank the G x G matrix, and its read-back is the single host
    sync of a Gaussian-sharded frame (all_to_all_single needs the split sizes on the host)."""
    mat = exchange_count_matrix(counts, group)
    rank = dist.get_rank(group) if _world(group) > 1 else 0
    return mat[rank].tolist(), mat[:, rank].tolist()


def exchange_count_matrix(counts: torch.Tensor, group=None) -> torch.Tensor:
    """counts[G] on the collective's device -> the world x G matrix of all ranks' counts as a host int64 tensor (identical on
    every rank): one all-gather + the read-back that is the exact form's host synchronisation."""
    world = _world(group)
    c = counts.to(torch.int64).contiguous()
    if world == 1:
        return c.view(1, -1).cpu()
    mat = torch.empty(world * c.numel(), dtype=torch.int64, device=c.device)
    dist.all_gather_into_tensor(mat, c, group=group)
    return mat.view(world, -1).cpu()


class ExchangePolicy:
    """How mode C moves the packed records.  Every rank of the group must hold the same settings; the state below evolves
    identically on all of them because it only depends on all-gathered / all-reduced quantities.
      mode "exact": count matrix read back by the host, variable-size all-to-all (round 3)
      mode "fixed": fixed-capacity segments with the count in a header row, equal-split all-to-all, no host read-back of counts.
                    Frames run exact until a capacity is known (and again after every overflow)."""

    def __init__(self, mode: str = "exact", slack: float = 1.25, granule: int = 256):
        if mode not in ("exact", "fixed"):
            raise ValueError("exchange mode must be 'exact' or 'fixed'")
        self.mode, self.slack, self.granule = mode, float(slack), int(granule)
        self.capacity: Optional[int] = None      # record rows per (source, band) segment
        self.frames_exact = self.frames_fixed = self.overflows = 0

    def observe(self, max_count: int) -> None:
        """max_count = the largest entry of the count matrix of an exact frame.  The capacity only grows (the envelope over the
        cameras seen so far)."""
        need = -(-int(max_count * self.slack + 1) // self.granule) * self.granule
        self.capacity = max(self.capacity or 0, need, self.granule)

    def use_fixed(self) -> bool:
        return self.mode == "fixed" and self.capacity is not None


_policies: dict = {}


def set_exchange_mode(mode: str, group=None, slack: float = 1.25, granule: int = 256) -> ExchangePolicy:
    """Select the exchange form of mode C for a process group (call on every rank with the same arguments)."""
    _policies[group] = ExchangePolicy(mode, slack, granule)
    return _policies[group]


def exchange_policy(group=None) -> ExchangePolicy:
    if group not in _policies:
        _policies[group] = ExchangePolicy()
    return _policies[group]


def all_to_all_equal(send: torch.Tensor, group=None, async_op: bool = False):
    """send[world * n, ...] -> recv of the same shape: block g of `send` goes to rank g, block g of `recv` came from rank g.
    Returns (recv, work)."""
    world = _world(group)
    if world == 1:
        return send, None
    send = send.contiguous()
    recv = torch.empty_like(send)
    if send.is_cuda and dist.get_backend(group) == "gloo":      # CPU-test backend with device tensors, see all_to_all_rows
        r_cpu = torch.empty(recv.shape, dtype=recv.dtype)
        dist.all_to_all_single(r_cpu, send.cpu(), group=group)
        recv.copy_(r_cpu)
        return recv, None
    work = dist.all_to_all_single(recv, send, group=group, async_op=async_op)
    return recv, (work if async_op else None)


def any_rank_flag(flag: torch.Tensor, group=None) -> torch.Tensor:
    """flag int32[1] on the collective's device -> max over the ranks, same device; no host synchronisation with RCCL."""
    if _world(group) == 1:
        return flag
    if flag.is_cuda and dist.get_backend(group) == "gloo":
        f = flag.cpu()
        dist.all_reduce(f, op=dist.ReduceOp.MAX, group=group)
        return f.to(flag.device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
    return flag


_flag_ring: dict = {}


class _HostFlag:
    """The pinned overflow flag of one frame + the event recorded behind its device-to-host copy.  Reading it (`flag[0]`) first waits for that
    event (the R read-back that normally orders the read lives on the stream handed to the library -- which is torch's current stream
    today, but the read must not depend on that)."""

    def __init__(self, t: torch.Tensor, event=None):
        self.t, self.event = t, event

    def __getitem__(self, i):
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        return self.t[i]


def _pinned_flag(device) -> torch.Tensor:
    """A pinned host int32[1] from a small per-device ring (several frames may be in flight)."""
    ring = _flag_ring.setdefault(device, {"bufs": [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(8)], "next": 0})
    t = ring["bufs"][ring["next"] % 8]
    ring["next"] += 1
    return t


# ---- torch restatement of the fixed-capacity layout (CPU tests; the HIP kernels are checked against it on the GPU) ----
def pack_fixed_torch(rows: torch.Tensor, counts: Sequence[int], capacity: int) -> torch.Tensor:
    """rows[sum(counts), K] grouped by band -> [G * (capacity + 1), K]: per band a header row (column 0 = the count, column 1 =
    the capacity, as VALUES -- the HIP form stores the same two numbers as integer bits) + the first min(count, capacity) rows;
    unused rows are zero."""
    G, K = len(counts), rows.shape[1]
    out = rows.new_zeros(G * (capacity + 1), K)
    pos = 0
    for b, c in enumerate(counts):
        base = b * (capacity + 1)
        out[base, 0], out[base, 1] = float(c), float(capacity)
        n = min(int(c), capacity)
        out[base + 1:base + 1 + n] = rows[pos:pos + n]
        pos += int(c)
    return out


def unpack_fixed_torch(segs: torch.Tensor, n_segments: int, capacity: int) -> Tuple[torch.Tensor, List[int]]:
    """Inverse on the receiver: ([sum(min(count, capacity)), K] rows in segment order, the header counts)."""
    parts, counts = [], []
    for s_ in range(n_segments):
        base = s_ * (capacity + 1)
        c = int(segs[base, 0].item())
        counts.append(c)
        parts.append(segs[base + 1:base + 1 + min(c, capacity)])
    return (torch.cat(parts, dim=0) if parts else segs[:0]), counts


class _ExchangeRowsFixed(torch.autograd.Function):
    """Differentiable fixed-capacity exchange of rows (the oracle path of the gloo tests): pack -> equal-split all-to-all -> unpack;
    backward = the same exchange in reverse with the gradient rows in the same layout."""

    @staticmethod
    def forward(ctx, rows, counts, capacity, group):
        world = _world(group)
        recv_segs, _ = all_to_all_equal(pack_fixed_torch(rows.detach(), counts, capacity), group)
        recv, rcounts = unpack_fixed_torch(recv_segs, world, capacity)
        ctx.meta = ([min(int(c), capacity) for c in counts], [min(c, capacity) for c in rcounts], capacity, group, int(rows.shape[0]),
                    [int(c) for c in counts])
        return recv.clone()

    @staticmethod
    def backward(ctx, g):
        kept, rkept, capacity, group, n_rows, counts = ctx.meta
        back_segs, _ = all_to_all_equal(pack_fixed_torch(g.contiguous(), rkept, capacity), group)
        out = g.new_zeros(n_rows, g.shape[1])
        pos = 0
        for b, (c, k) in enumerate(zip(counts, kept)):
            base = b * (capacity + 1)
            out[pos:pos + k] = back_segs[base + 1:base + 1 + k]
            pos += c
        return out, None, None, None


def exchange_rows_fixed(rows: torch.Tensor, counts: Sequence[int], capacity: int, group=None) -> Tuple[torch.Tensor, bool]:
    """-> (received rows, overflow anywhere in the group).  On overflow the received set is incomplete: repeat the frame exactly."""
    flag = torch.tensor([1 if max([int(c) for c in counts] + [0]) > capacity else 0], dtype=torch.int32, device=rows.device)
    flag = any_rank_flag(flag, group)
    return _ExchangeRowsFixed.apply(rows, [int(c) for c in counts], int(capacity), group), bool(int(flag.item()))


def all_to_all_rows(send: torch.Tensor, send_counts: Sequence[int], recv_counts: Sequence[int], group=None, async_op: bool = False):
    """send[sum(send_counts), K] rows grouped by destination -> recv[sum(recv_counts), K] rows grouped by source rank.
    Returns (recv, work) -- work is None unless async_op."""
    world = _world(group)
    recv = send.new_empty(int(sum(recv_counts)), *send.shape[1:])
    if world == 1:
        recv.copy_(send)
        return recv, None
    if send.is_cuda and dist.get_backend(group) == "gloo":
        # CPU-test backend with device tensors (tests/: two ranks sharing one GPU over gloo): gloo's all-to-all takes host
        # tensors only, so the rows are staged through host memory.  RCCL ("nccl") takes the device tensors directly.
        r_cpu = torch.empty(recv.shape, dtype=recv.dtype)
        dist.all_to_all_single(r_cpu, send.contiguous().cpu(), [int(c) for c in recv_counts], [int(c) for c in send_counts], group=group)
        recv.copy_(r_cpu)
        return recv, None
    work = dist.all_to_all_single(recv, send.contiguous(), [int(c) for c in recv_counts], [int(c) for c in send_counts],
                                  group=group, async_op=async_op)
    return recv, (work if async_op else None)


class _ExchangeRows(torch.autograd.Function):
    """Differentiable all_to_all_rows (the oracle path of the gloo tests; the HIP path issues the same two collectives
    around its fused kernels): backward = the reverse all-to-all of the gradient rows."""

    @staticmethod
    def forward(ctx, send, send_counts, recv_counts, group):
        ctx.meta = (list(send_counts), list(recv_counts), group)
        return all_to_all_rows(send, send_counts, recv_counts, group)[0]

    @staticmethod
    def backward(ctx, g):
        send_counts, recv_counts, group = ctx.meta
        return all_to_all_rows(g.contiguous(), recv_counts, send_counts, group)[0], None, None, None


def exchange_rows(send: torch.Tensor, send_counts, recv_counts, group=None) -> torch.Tensor:
    return _ExchangeRows.apply(send, send_counts, recv_counts, group)


def route_plan_torch(miny: torch.Tensor, maxy: torch.Tensor, tiles: torch.Tensor, bounds: Sequence[int]):
    """Reference semantics of gsr_route_count / gsr_route_pack in torch (CPU tests; checked against the HIP kernels on the
    GPU): a record goes to band b iff it has tiles and its tile rows [miny, maxy) intersect [bounds[b], bounds[b+1]).
    Returns (send_index int64 -- Gaussian indices grouped by band, ascending inside a band -- , counts list)."""
    idx, counts = [], []
    for b in range(len(bounds) - 1):
        m = (tiles > 0) & (miny.clamp_min(bounds[b]) < maxy.clamp_max(bounds[b + 1]))      # (an empty band receives nothing)
        sel = torch.nonzero(m, as_tuple=False).flatten()
        idx.append(sel)
        counts.append(int(sel.numel()))
    return (torch.cat(idx) if idx else miny.new_zeros(0, dtype=torch.int64)), counts


def _i32_array(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def _i64_array(vals):
    return (C.c_int64 * len(vals))(*[int(v) for v in vals])


def hip_preprocess_shard(raster_settings, means3D, sh, opacities, scales, rotations, dc=None):
    """gsr_preprocess_forward on this rank's shard: (records[P,16], radii[P], M, contiguous inputs)."""
    _, records, radii, M, inputs = _preprocess_shard(raster_settings, None, [], None, means3D, sh, opacities, scales, rotations, dc,
                                                     "sharded renderer")
    return records, radii, M, inputs


def hip_route_count(records: torch.Tensor, bounds: Sequence[int]):
    """gsr_route_count: (counts int32[G] on the device, scratch) -- no host sync."""
    lib = _lib.load()
    device = records.device
    P, G = int(records.shape[0]), len(bounds) - 1
    with torch.cuda.device(device):
        scratch = torch.empty(max(128, lib.gsr_route_scratch_bytes(P, G)), dtype=torch.uint8, device=device)
        counts = torch.empty(G, dtype=torch.int32, device=device)
        _lib.check(lib.gsr_route_count(P, _ptr(records), G, _i32_array(bounds), _ptr(scratch), _ptr(counts), _pkg._stream_ptr(device)),
                   "gsr_route_count")
    return counts, scratch


def hip_route_pack(records: torch.Tensor, bounds: Sequence[int], send_counts: Sequence[int], scratch: torch.Tensor):
    """gsr_route_pack: (packed[sum,12], send_ids int32[sum], offsets list of G+1)."""
    lib = _lib.load()
    device = records.device
    P, G = int(records.shape[0]), len(bounds) - 1
    offsets = [0]
    for c in send_counts:
        offsets.append(offsets[-1] + int(c))
    with torch.cuda.device(device):
        packed = torch.empty(offsets[-1], PACKED_WORDS, dtype=torch.float32, device=device)
        send_ids = torch.empty(offsets[-1], dtype=torch.int32, device=device)
        _lib.check(lib.gsr_route_pack(P, _ptr(records), G, _i32_array(bounds), _i64_array(offsets), _ptr(scratch), _ptr(packed),
                                      _ptr(send_ids), _pkg._stream_ptr(device)), "gsr_route_pack")
    return packed, send_ids, offsets


def hip_route_pack_fixed(records: torch.Tensor, bounds: Sequence[int], capacity: int, scratch: torch.Tensor, counts: torch.Tensor):
    """gsr_route_pack_fixed: (segments[G * (capacity + 1), 12], send_ids int32[G * (capacity + 1)]) -- no host knowledge of the counts."""
    lib = _lib.load()
    device = records.device
    P, G = int(records.shape[0]), len(bounds) - 1
    rows = G * (int(capacity) + 1)
    with torch.cuda.device(device):
        packed = torch.empty(rows, PACKED_WORDS, dtype=torch.float32, device=device)
        send_ids = torch.empty(rows, dtype=torch.int32, device=device)
        _lib.check(lib.gsr_route_pack_fixed(P, _ptr(records), G, _i32_array(bounds), int(capacity), _ptr(scratch), _ptr(counts),
                                            _ptr(packed), _ptr(send_ids), _pkg._stream_ptr(device)), "gsr_route_pack_fixed")
    return packed, send_ids


def hip_render_segments(raster_settings, band, segs: torch.Tensor, n_segments: int, capacity: int, no_backward: bool):
    """gsr_rasterize_from_segments on this rank's band (see hip_render_packed); the state's Gaussian count is
    n_segments * (capacity + 1)."""
    keep: list = []
    with torch.cuda.device(segs.device):
        s = _make_settings(raster_settings, keep, band, no_backward)
        return _rasterize_records("gsr_rasterize_from_segments", s, (int(n_segments), int(capacity)), segs, segs.device)


def _fixed_exchange_forward(records, bounds, counts, rscratch, policy: ExchangePolicy, group, async_op: bool = False):
    """The fixed-capacity exchange of one frame: -> (received segments, send_ids, overflow flag (_HostFlag), work, packed send buffer).
    The flag's copy to pinned memory is queued on the current stream ahead of the ingest kernel that publishes R, so it has normally
    arrived when the frame's R read-back returns; `flag[0]` waits for the event recorded behind the copy in any case."""
    cap = int(policy.capacity)
    packed, send_ids = hip_route_pack_fixed(records, bounds, cap, rscratch, counts)
    flag = any_rank_flag((counts.to(torch.int64) > cap).any().to(torch.int32).reshape(1), group)
    pinned = _pinned_flag(records.device)
    pinned.copy_(flag, non_blocking=True)
    event = None
    if flag.is_cuda:
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(flag.device))
    recv, work = all_to_all_equal(packed, group, async_op=async_op)
    return recv, send_ids, _HostFlag(pinned, event), work, packed


def hip_render_packed(raster_settings, band, recv: torch.Tensor, no_backward: bool):
    """gsr_rasterize_from_packed on this rank's band: (color[3,H,W], invdepth[1,H,W], state) with only the band's rows
    written (zeros elsewhere); state = (geom, binning, img, num_rendered) for gsr_backward_blend."""
    keep: list = []
    with torch.cuda.device(recv.device):
        s = _make_settings(raster_settings, keep, band, no_backward)
        return _rasterize_records("gsr_rasterize_from_packed", s, (int(recv.shape[0]),), recv, recv.device)


class _GaussianShardedHip(torch.autograd.Function):
    """Mode C for one rank: local shard of Gaussians in, the rank's band of the image out (see the module docstring)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, opacities, scales, rotations, raster_settings, plan, group, dc):
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        bounds = list(plan.bounds)
        records, radii, M, (m_c, sh_c, op_c, sc_c, rot_c, dc_c) = hip_preprocess_shard(raster_settings, means3D, sh, opacities,
                                                                                      scales, rotations, dc)
        counts, rscratch = hip_route_count(records, bounds)
        no_backward = not (any(ctx.needs_input_grad[:6]) or ctx.needs_input_grad[9])
        policy = exchange_policy(group)
        G = len(bounds) - 1
        done = False
        if policy.use_fixed():
            # fixed-capacity segments: no count reaches the host; the overflow flag arrives with the R read-back inside the render call
            cap = int(policy.capacity)
            recv, send_ids, host_flag, _, _ = _fixed_exchange_forward(records, bounds, counts, rscratch, policy, group)
            color, invdepth, (geom, binning, img, nr) = hip_render_segments(raster_settings, plan.band(rank), recv, G, cap, no_backward)
            if int(host_flag[0]) == 0:
                policy.frames_fixed += 1
                ctx.fixed_capacity = cap
                ctx.send_counts = ctx.recv_counts = None
                ctx.offsets = [b * (cap + 1) for b in range(G + 1)]
                done = True
            else:
                policy.overflows += 1      # every rank sees the same flag: all repeat the frame in the exact form
        if not done:
            mat = exchange_count_matrix(counts, group)                               # the exact frame's host sync
            policy.observe(int(mat.max()) if mat.numel() else 0)
            policy.frames_exact += 1
            send_counts, recv_counts = mat[rank].tolist(), mat[:, rank].tolist()
            packed, send_ids, offsets = hip_route_pack(records, bounds, send_counts, rscratch)
            recv, _ = all_to_all_rows(packed, send_counts, recv_counts, group)
            color, invdepth, (geom, binning, img, nr) = hip_render_packed(raster_settings, plan.band(rank), recv, no_backward)
            ctx.fixed_capacity = None
            ctx.send_counts, ctx.recv_counts, ctx.offsets = send_counts, recv_counts, offsets
        ctx.raster_settings, ctx.band, ctx.group, ctx.M = raster_settings, plan.band(rank), group, M
        ctx.P_recv, ctx.num_rendered = int(recv.shape[0]), nr
        ctx.has_means2D, ctx.has_dc = means2D is not None, dc_c is not None
        ctx.op_shape = tuple(opacities.shape)
        ctx.dc_shape = tuple(dc.shape) if dc is not None else None
        ctx.save_for_backward(m_c, sh_c, op_c, sc_c, rot_c, radii, geom, binning, img, send_ids,
                              dc_c if dc_c is not None else m_c.new_empty(0))
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return color, radii, invdepth

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth):
        m, sh, op, sc, rot, radii, geom, binning, img, send_ids, dc = ctx.saved_tensors
        device = m.device
        P, P_recv, M = int(m.shape[0]), ctx.P_recv, ctx.M
        rs = ctx.raster_settings
        f = dict(dtype=torch.float32, device=device)
        if g_color is None:
            g_color = torch.zeros(3, int(rs.image_height), int(rs.image_width), **f)
        grads, d_dc = _gradients(P, device, True, True, M - 1 if ctx.has_dc else M, ctx.has_dc, True, True)
        keep: list = []
        with torch.cuda.device(device):
            s = _make_settings(rs, keep, ctx.band)
            if ctx.has_dc:
                s.sh_dc, s.dL_dsh_dc = dc.data_ptr(), d_dc.data_ptr()
            if P_recv > 0:
                full = _backward_blend(s, P_recv, _Forward(geom, binning, img, ctx.num_rendered), _f32c(g_color), _f32c(g_depth), device)
            else:
                full = torch.empty(0, 12, **f)
            if ctx.fixed_capacity is not None:      # same layout back: block g of the gradient rows belongs to rank g
                returned, _ = all_to_all_equal(full, ctx.group)
            else:
                returned, _ = all_to_all_rows(full, ctx.recv_counts, ctx.send_counts, ctx.group)      # rows back to their owners
            if P > 0:
                mine = torch.empty(P, 12, **f)
                _lib.check(_lib.load().gsr_route_return(P, len(ctx.offsets) - 1, _i64_array(ctx.offsets), _ptr(send_ids), _ptr(returned),
                                                        _ptr(mine), _pkg._stream_ptr(device)), "gsr_route_return")
                _backward_preprocess(s, P, M, (m, sh, None, op, sc, rot, None), radii, None, mine, grads, device)
        d_m2, _, d_op, d_m3, _, d_sh, d_sc, d_rot = grads
        return (d_m3, d_m2 if ctx.has_means2D else None, d_sh, d_op.view(ctx.op_shape), d_sc, d_rot, None, None, None,
                d_dc.view(ctx.dc_shape) if ctx.has_dc else None)


def render_gaussian_sharded(raster_settings, means3D, sh, opacities, scales, rotations, plan: BandPlan, group=None,
                            means2D=None, dc=None, gather_invdepth: bool = True):
    """Mode C render of one frame: this rank's shard of Gaussians in, the FULL image (strips all-gathered) out.  Shards must
    be contiguous index ranges in rank order (ties in depth resolve by global index, as on one GPU).  Returns
    (color[3,H,W], radii[P_local], invdepth[1,H,W]); gradients flow to the rank's own shard only.
    gather_invdepth=False: only the colour strips are gathered (invdepth then holds this rank's band only) -- what a
    training step without depth supervision needs; the blend backward then runs its build without the 1/depth terms."""
    color, radii, invdepth = _GaussianShardedHip.apply(means3D, means2D, sh, opacities, scales, rotations, raster_settings,
                                                       plan, group, dc)
    H = color.shape[1]
    if gather_invdepth:
        both = _GatherStrips.apply(torch.cat([color, invdepth], dim=0), plan, H, group)
        return both[:3], radii, both[3:4]
    return _GatherStrips.apply(color, plan, H, group), radii, invdepth


class ShardedFrame:
    """A forward-only mode-C frame in flight (bench.py's pipelined forward): begin() has projected, routed and launched the
    all-to-all; finish() waits for it, renders the band and launches the strip all-gather."""
    __slots__ = ("rs", "plan", "group", "recv", "work", "radii", "keep", "fixed", "flag", "inputs")


def sharded_forward_begin(raster_settings, means3D, sh, opacities, scales, rotations, plan: BandPlan, group=None, dc=None) -> ShardedFrame:
    fr = ShardedFrame()
    with torch.no_grad():
        records, radii, _, keep = hip_preprocess_shard(raster_settings, means3D, sh, opacities, scales, rotations, dc)
        bounds = list(plan.bounds)
        counts, rscratch = hip_route_count(records, bounds)
        policy = exchange_policy(group)
        fr.fixed, fr.flag = None, None
        if policy.use_fixed():
            fr.recv, _, fr.flag, fr.work, packed = _fixed_exchange_forward(records, bounds, counts, rscratch, policy, group, async_op=True)
            fr.fixed = int(policy.capacity)
            fr.inputs = (means3D, sh, opacities, scales, rotations, dc)      # (an overflowing frame is repeated in the exact form)
        else:
            mat = exchange_count_matrix(counts, group)
            policy.observe(int(mat.max()) if mat.numel() else 0)
            policy.frames_exact += 1
            rank = dist.get_rank(group) if dist.is_initialized() else 0
            send_counts, recv_counts = mat[rank].tolist(), mat[:, rank].tolist()
            packed, _, _ = hip_route_pack(records, bounds, send_counts, rscratch)
            fr.recv, fr.work = all_to_all_rows(packed, send_counts, recv_counts, group, async_op=True)
        fr.keep = (packed, records)      # alive until the collective has read them
    fr.rs, fr.plan, fr.group, fr.radii = raster_settings, plan, group, radii
    return fr


def sharded_forward_finish(fr: ShardedFrame):
    """-> handle with .wait() -> full colour image [3,H,W] on every rank."""
    rank = dist.get_rank(fr.group) if dist.is_initialized() else 0
    with torch.no_grad():
        if fr.work is not None:
            fr.work.wait()
        if fr.fixed is not None:
            policy = exchange_policy(fr.group)
            color, _, _ = hip_render_segments(fr.rs, fr.plan.band(rank), fr.recv, len(fr.plan.bounds) - 1, fr.fixed, True)
            if int(fr.flag[0]) != 0:      # a segment overflowed somewhere (every rank reads the same flag): exact form, larger capacity
                policy.overflows += 1
                cap, policy.capacity = policy.capacity, None
                redo = sharded_forward_begin(fr.rs, *fr.inputs[:5], fr.plan, fr.group, fr.inputs[5])
                policy.capacity = max(policy.capacity or 0, cap)
                fr.inputs = None
                return sharded_forward_finish(redo)
            policy.frames_fixed += 1
            fr.inputs = None
        else:
            color, _, _ = hip_render_packed(fr.rs, fr.plan.band(rank), fr.recv, True)
        fr.keep = None
        return gather_strips_async(color, fr.plan, int(fr.rs.image_height), fr.group)


def probe_collectives(group=None, device=None) -> dict:
    """First contact with the collective backend (RCCL has never run before the driver's multi-GPU bench: VERDICT r02 weak #8):
    one tiny instance of every collective the renderers use, each in its own try / except, so that a caller can pick a mode
    that works and REPORT what failed instead of dying inside a frame.  Returns {"backend", "all_reduce", "all_gather",
    "all_to_all_single", "all_gather_uneven", "reduce_scatter", "errors": {name: message}}."""
    out = {"backend": None, "all_reduce": False, "all_gather": False, "all_to_all_single": False, "all_gather_uneven": False,
           "reduce_scatter": False, "errors": {}}
    world = _world(group)
    if world == 1:
        return out
    rank = dist.get_rank(group)
    out["backend"] = dist.get_backend(group)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if out["backend"] == "nccl" else torch.device("cpu")

    def attempt(name, fn):
        try:
            fn()
            if device.type == "cuda":
                torch.cuda.synchronize(device)
            out[name] = True
        except Exception as ex:          # noqa: BLE001 -- the message is the result
            out["errors"][name] = repr(ex)[:300]

    def _all_reduce():
        t = torch.ones(4, device=device)
        dist.all_reduce(t, group=group)
        assert float(t[0]) == world

    def _all_gather():
        t = torch.full((8,), float(rank), device=device)
        o = torch.empty(8 * world, device=device)
        dist.all_gather_into_tensor(o, t, group=group)
        assert float(o[-1]) == world - 1

    def _a2a():
        send_counts = [1 + ((rank + d) % 3) for d in range(world)]
        recv_counts = [1 + ((r + rank) % 3) for r in range(world)]
        send = torch.full((sum(send_counts), PACKED_WORDS), float(rank), device=device)
        recv, _ = all_to_all_rows(send, send_counts, recv_counts, group)
        assert recv.shape[0] == sum(recv_counts) and float(recv[-1, 0]) == world - 1

    def _uneven():
        bufs = [torch.empty(r + 1, 4, device=device) for r in range(world)]
        dist.all_gather(bufs, torch.full((rank + 1, 4), float(rank), device=device), group=group)
        assert float(bufs[-1][0, 0]) == world - 1

    def _reduce_scatter():
        if out["backend"] == "gloo":
            raise RuntimeError("gloo has no reduce_scatter (the callers use all_reduce + slice)")
        full = torch.ones(world * 4, device=device)
        o = torch.empty(4, device=device)
        dist.reduce_scatter_tensor(o, full, group=group)
        assert float(o[0]) == world

    attempt("all_reduce", _all_reduce)
    attempt("all_gather", _all_gather)
    attempt("all_to_all_single", _a2a)
    attempt("all_gather_uneven", _uneven)
    attempt("reduce_scatter", _reduce_scatter)
    # every rank must come to the SAME verdict (a collective that failed on one rank only is unusable for all): the outcomes
    # are min-reduced, so that mode and strip-gather form are chosen identically everywhere
    names = ("all_gather", "all_to_all_single", "all_gather_uneven", "reduce_scatter")
    if out["all_reduce"]:
        try:
            v = torch.tensor([1.0 if out[n] else 0.0 for n in names], device=device)
            dist.all_reduce(v, op=dist.ReduceOp.MIN, group=group)
            for n, ok in zip(names, v.tolist()):
                if out[n] and ok == 0.0:
                    out["errors"][n] = "failed on another rank"
                out[n] = bool(ok)
        except Exception as ex:          # noqa: BLE001
            out["errors"]["agreement"] = repr(ex)[:300]
    return out
