// Fixed-order reductions shared by the kernels that must give the same bits in two runs (device only): the per-Gaussian reduce over the runs of
// instance records that a walk kernel leaves behind (absgrad.hip, features.hip), and the fp64
// sum over the 256 threads of a workgroup (normals.hip, bilagrid.hip).  One definition each of what must never drift apart between their users:
// the tail lane of the depth order, and the order in which every path adds.  The rule of gsr_blend.h holds here too: each piece compiles to the
// code it replaced, kernel by kernel, or is not shared for that kernel.
// TWO KERNELS KEEP A WRITTEN-OUT COPY of reduce_instance_runs because it compiled to other code there: contrib_reduce (contrib.hip) and
// feature_grad_reduce<2> (features.hip).  A change to the frame below is a change to those two as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsrw {

// ------------------------------------------------------------------------------------------------
// The instance-run reduce.  In emission (= depth) order a Gaussian's instances are contiguous: Gaussian j of the depth order owns the instances
// [offsets[j - 1], offsets[j]).  One wave64 per 64 consecutive Gaussians of the depth order streams their instances 64 at a time (lane = instance:
// the coalesced flag words one chunk ahead, then whatever Ops::load reads of the flagged slots), and every Gaussian lane takes its own instances
// of the chunk in ascending (emission) order from the values parked in LDS.  A chunk that belongs to one Gaussian entirely (a splat over hundreds
// of tiles) is folded over the wave instead and taken once -- which chunks those are depends on the frame only, so two runs add in the same order.
// A chunk without a flag is skipped.  Lanes past the last Gaussian read Gaussian P - 1 and own nothing.  No atomics.
//
// Ops (per kernel; it holds the lane's accumulator and the LDS table the kernel declared):
//     Value                      what one instance contributes
//     Value load(f, k)           the value of instance k, whose flag word is f (byte q != 0: slot q has a record), its slots combined in slot order
//     void  fold_take(v, own)    v combined over the 64 lanes (the same total in every lane); the lanes with `own` take the total
//     void  take(const Value&)   accumulator <- accumulator combined with the value
//     void  park(lane, v)        the lane's value into LDS
//     Value parked(i)            ... and the value of lane i back
// store(g): called once by every lane that owns a non-empty run, g its Gaussian -- the kernel's own store, written at the call (`accumulate`, scales
// and channel tests stay with their kernels).
// Two forms that read better are not used because they compile to other code, against the rule above: returning (g, owns) and testing it in the
// kernel inverts the loop's closing branch in every kernel; fold and take as two calls merge feature_grad_reduce's per-float4 takes into one region.
// Known cost: a wave whose 64 Gaussians hold one very large splat streams all its chunks alone (the tail the blend backward's unit-based reduce was
// built to avoid); chunks without flags -- most of such a splat -- cost one coalesced flag read each.
// ------------------------------------------------------------------------------------------------
template <class Ops, class Store>
__device__ __forceinline__ void reduce_instance_runs(int P, const uint32_t* order, const uint32_t* offsets, const uint32_t* flags, Ops& ops, Store store) {
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t jc = j < P ? j : (int64_t)P - 1;
    const uint32_t incl = offsets[jc];
    uint32_t excl = jc > 0 ? offsets[jc - 1] : 0u;
    if (j >= P) excl = incl;                      // (lanes past the last Gaussian own nothing)
    const uint32_t g = order[jc];
    const uint32_t c_begin = (uint32_t)__builtin_amdgcn_readlane((int)excl, 0);
    const uint32_t c_end = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    auto load_flags = [&](uint32_t c) -> uint32_t {
        const int64_t k = (int64_t)c + lane;
        return (c < c_end && k < (int64_t)c_end) ? flags[k] : 0u;
    };
    uint32_t f_next = load_flags(c_begin);
    for (uint32_t c = c_begin; c < c_end; c += 64) {
        const uint32_t f = f_next;
        f_next = load_flags(c + 64);
        if (__ballot(f != 0u) == 0ull) continue;      // nobody contributed through these 64 instances (hidden behind nearer ones)
        typename Ops::Value v = ops.load(f, (int64_t)c + lane);
        // a chunk inside one Gaussian's run: fold (the same total in every lane); else the owners take their instances in order
        const uint32_t lo = max(excl, c), hi = min(incl, c + 64u);
        const bool own_all = lo < hi && hi - lo == 64u;
        if (__ballot(own_all) != 0ull) {
            ops.fold_take(v, own_all);
            continue;
        }
        ops.park(lane, v);
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lo; i < hi; ++i) ops.take(ops.parked(i - c));
        __builtin_amdgcn_wave_barrier();
    }
    if (j < P && incl > excl) store(g);
}

// ------------------------------------------------------------------------------------------------
// fp64 sum over the 256 threads of a workgroup in a fixed order (a tree over LDS, s: 256 doubles); the total in thread 0.
// (bg_grad_kernel / bg_grad_finish of render_bwd.hip run the same tree three values wide, one barrier per level, and keep it written out: see there.)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_f64(double v, double* s) {
    const int tid = (int)threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s[tid] += s[tid + h];
        __syncthreads();
    }
    return s[0];
}
// The one-workgroup kernel body behind a kernel that left one fp64 partial per workgroup: thread t adds partials t, t + 256, ... in that order, the
// tree, one rounding: out[0] = (float)(sum / divisor).  (x / 1.0 is x: a caller without a divisor passes the literal and the division is gone.)
__device__ __forceinline__ void block_sum_partials_f64(int n, const double* __restrict__ partials, double divisor, float* __restrict__ out, double* s) {
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += 256) acc += partials[i];
    const double sum = block_sum_f64(acc, s);
    if (threadIdx.x == 0) out[0] = (float)(sum / divisor);
}

}  // namespace gsrw
