// Absolute screen-space gradients (gsr_backward_blend_abs / gsr_absgrad_from_records, include/gsr.h; the densification signal of AbsGS,
// gsplat's `absgrad`): for every Gaussian g, over the pixels p at which the blend backward takes it (list position < n_contrib, power <= 0,
// alpha >= 1/255), with m_gp = opacity G dL/dalpha_gp (the backward's own m) and (dx, dy) = mean2D - p,
//     abs_x[g] = sum_p |m_gp (A dx + B dy)|,   abs_y[g] = sum_p |m_gp (C dy + B dx)|
// -- the sum of the absolute values of the per-pixel terms whose signed sums are words 0, 1 of the [P,12] records.  The per-pixel terms exist
// only inside the walk kernel (render_bwd.hip, render_bwd_half<*, true>): it leaves, per (half tile, instance), the two sums in words 10, 11 of
// the instance record in log2 units (the conic as the walk holds it: -log2(e) times the sums above).
//
// Two kernels here, NO atomics, every sum in a fixed association order -> two runs give the same bits:
//
//  absgrad_reduce        the structure of contrib_reduce (contrib.hip).  In emission (= depth) order a Gaussian's instances are contiguous.  One wave
//                        per 64 consecutive Gaussians of the depth order streams their instances 64 at a time (lane = instance: coalesced flag words one
//                        chunk ahead, then only the third float4 of the flagged slot records, the up to GSR_BWD_SLOTS of an instance added in slot
//                        order), parks the per-instance pair in LDS, and every Gaussian lane adds its own instances of the chunk in ascending
//                        (emission) order.  A chunk that belongs to one Gaussian entirely is folded by a butterfly instead -- which chunks those are
//                        depends on the frame only.  A chunk without a flag is skipped.  The finished pair times 1 / log2(e) goes to words 10, 11 of
//                        splat_grads[g] (pixel units, like words 0, 1); rows of Gaussians without instances keep the zeros of the launcher of
//                        bwd_reduce_units, after which this kernel runs on the same stream.  The unit-based reduce chain is not touched.
//  absgrad_from_records  element-wise: means2D_abs[g] = (0.5 W abs_x, 0.5 H abs_y, 0), the units and layout of dL_dmeans2D.
// Known cost: a wave of the reduce whose 64 Gaussians hold one very large splat streams all its chunks alone (the tail the blend backward's
// unit-based reduce was built to avoid); chunks without flags -- most of such a splat -- cost one coalesced flag read each.
#include "gsr_internal.h"

namespace {

constexpr float LN2 = 0.6931471805599453f;      // 1 / log2(e): the walk's sums are in log2 units (gsr_blend.h conic_*_to_log2)

__global__ void __launch_bounds__(64)
absgrad_reduce(int P, int64_t R, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
               const float4* __restrict__ inst_grads /*[GSR_BWD_SLOTS][R] records of 3 float4*/, const uint32_t* __restrict__ flags,
               float* __restrict__ splat_grads /*[P,12]*/) {
    __shared__ float s_x[64];
    __shared__ float s_y[64];
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t jc = j < P ? j : (int64_t)P - 1;
    const uint32_t incl = offsets[jc];
    uint32_t excl = jc > 0 ? offsets[jc - 1] : 0u;
    if (j >= P) excl = incl;                      // (lanes past the last Gaussian own nothing)
    const uint32_t g = order[jc];
    const uint32_t c_begin = (uint32_t)__builtin_amdgcn_readlane((int)excl, 0);
    const uint32_t c_end = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    float acc_x = 0.0f, acc_y = 0.0f;
    auto load_flags = [&](uint32_t c) -> uint32_t {
        const int64_t k = (int64_t)c + lane;
        return (c < c_end && k < (int64_t)c_end) ? flags[k] : 0u;
    };
    uint32_t f_next = load_flags(c_begin);
    for (uint32_t c = c_begin; c < c_end; c += 64) {
        const uint32_t f = f_next;
        f_next = load_flags(c + 64);
        if (__ballot(f != 0u) == 0ull) continue;      // nobody took these 64 instances (hidden behind nearer ones)
        const int64_t k = (int64_t)c + lane;
        float4 rec[GSR_BWD_SLOTS];
#pragma unroll
        for (int q = 0; q < GSR_BWD_SLOTS; ++q) {
            rec[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((f >> (8 * q)) & 0xFFu) rec[q] = inst_grads[((int64_t)q * R + k) * 3 + 2];
        }
        float x = rec[0].z, y = rec[0].w;
#pragma unroll
        for (int q = 1; q < GSR_BWD_SLOTS; ++q) {      // the half tiles of the instance's tile, in slot order (a missing slot adds zeros)
            x += rec[q].z;
            y += rec[q].w;
        }
        // a chunk inside one Gaussian's run: butterfly (the same total in every lane); else the owners add their instances in order
        const uint32_t lo = max(excl, c), hi = min(incl, c + 64u);
        const bool own_all = lo < hi && hi - lo == 64u;
        if (__ballot(own_all) != 0ull) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                x += __shfl_xor(x, off, 64);
                y += __shfl_xor(y, off, 64);
            }
            if (own_all) { acc_x += x; acc_y += y; }
            continue;
        }
        s_x[lane] = x; s_y[lane] = y;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lo; i < hi; ++i) {
            acc_x += s_x[i - c];
            acc_y += s_y[i - c];
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (j < P && incl > excl)
        *reinterpret_cast<float2*>(splat_grads + (int64_t)g * 12 + 10) = make_float2(LN2 * acc_x, LN2 * acc_y);
}

__global__ void __launch_bounds__(256)
absgrad_from_records(int P, float half_w, float half_h, const float* __restrict__ splat_grads /*[P,12]*/, float* __restrict__ means2D_abs /*[P,3]*/) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
        const float2 a = *reinterpret_cast<const float2*>(splat_grads + i * 12 + 10);
        means2D_abs[i * 3 + 0] = a.x * half_w;
        means2D_abs[i * 3 + 1] = a.y * half_h;
        means2D_abs[i * 3 + 2] = 0.f;
    }
}

}  // namespace

void gsr_launch_absgrad_reduce(int P, int64_t R, const GsrSavedFrame& f, const float* inst_grads, const uint32_t* inst_flag, float* splat_grads,
                               hipStream_t st) {
    if (P <= 0 || R <= 0) return;
    hipLaunchKernelGGL(absgrad_reduce, dim3((P + 63) / 64), dim3(64), 0, st, P, R, f.order, f.offsets, reinterpret_cast<const float4*>(inst_grads),
                       inst_flag, splat_grads);
}

void gsr_launch_absgrad_from_records(int P, int W, int H, const float* splat_grads, float* means2D_abs, hipStream_t st) {
    if (P <= 0) return;
    int64_t nb = ((int64_t)P + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(absgrad_from_records, dim3((int)nb), dim3(256), 0, st, P, 0.5f * (float)W, 0.5f * (float)H, splat_grads, means2D_abs);
}
