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
//  absgrad_reduce        the instance-run reduce of gsr_reduce.h (reduce_instance_runs, described there with its known cost) over AbsgradOps: only the
//                        third float4 of the flagged slot records is read, the up to GSR_BWD_SLOTS of an instance added in slot order.  The finished
//                        pair times 1 / log2(e) goes to words 10, 11 of splat_grads[g] (pixel units, like words 0, 1); rows of Gaussians without
//                        instances keep the zeros of the launcher of bwd_reduce_units, after which this kernel runs on the same stream.  The
//                        unit-based reduce chain is not touched.
//  absgrad_from_records  element-wise: means2D_abs[g] = (0.5 W abs_x, 0.5 H abs_y, 0), the units and layout of dL_dmeans2D.
#include "gsr_internal.h"
#include "gsr_reduce.h"

namespace {

constexpr float LN2 = 0.6931471805599453f;      // 1 / log2(e): the walk's sums are in log2 units (gsr_blend.h conic_*_to_log2)

// what absgrad_reduce does with an instance (gsr_reduce.h reduce_instance_runs): words 10, 11 of the records of its half tiles
struct AbsgradOps {
    typedef float2 Value;
    const float4* __restrict__ inst_grads;
    int64_t R;
    float* s_x; float* s_y;      // LDS, 64 each
    float acc_x = 0.0f, acc_y = 0.0f;
    __device__ __forceinline__ Value load(uint32_t f, int64_t k) const {
        float4 rec[GSR_BWD_SLOTS];
#pragma unroll
        for (int q = 0; q < GSR_BWD_SLOTS; ++q) {
            rec[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((f >> (8 * q)) & 0xFFu) rec[q] = inst_grads[((int64_t)q * R + k) * 3 + 2];      // (only the third float4 of a record)
        }
        float x = rec[0].z, y = rec[0].w;
#pragma unroll
        for (int q = 1; q < GSR_BWD_SLOTS; ++q) {      // the half tiles of the instance's tile, in slot order (a missing slot adds zeros)
            x += rec[q].z;
            y += rec[q].w;
        }
        return make_float2(x, y);
    }
    __device__ __forceinline__ void fold_take(Value v, bool own_all) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v.x += __shfl_xor(v.x, off, 64);
            v.y += __shfl_xor(v.y, off, 64);
        }
        if (own_all) take(v);
    }
    __device__ __forceinline__ void take(const Value& v) { acc_x += v.x; acc_y += v.y; }
    __device__ __forceinline__ void park(int lane, const Value& v) const { s_x[lane] = v.x; s_y[lane] = v.y; }
    __device__ __forceinline__ Value parked(uint32_t i) const { return make_float2(s_x[i], s_y[i]); }
};

__global__ void __launch_bounds__(64)
absgrad_reduce(int P, int64_t R, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
               const float4* __restrict__ inst_grads /*[GSR_BWD_SLOTS][R] records of 3 float4*/, const uint32_t* __restrict__ flags,
               float* __restrict__ splat_grads /*[P,12]*/) {
    __shared__ float s_x[64];
    __shared__ float s_y[64];
    AbsgradOps ops{inst_grads, R, s_x, s_y};
    gsrw::reduce_instance_runs(P, order, offsets, flags, ops, [&](uint32_t g) {
        *reinterpret_cast<float2*>(splat_grads + (int64_t)g * 12 + 10) = make_float2(LN2 * ops.acc_x, LN2 * ops.acc_y);
    });
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
