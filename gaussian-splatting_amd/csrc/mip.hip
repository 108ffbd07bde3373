// 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024; also trained with by Gaussian Opacity Fields and RaDe-GS): the two native pieces,
// DESIGN.md 5.12.  The 2D half of the paper is antialiasing=True of the rasterizer (csrc/gsr_math.h).
//
// mip_sweep -- upstream's compute_3D_filter, a Python loop over the training cameras with ~20 torch kernels per turn, as ONE kernel: a lane owns
// kSweepItems Gaussians, reads their means once and walks all C camera records, which sit at wave-uniform addresses and arrive by scalar loads.
// Per (Gaussian, camera) pair: three 3-term dot products as explicit fmaf chains (the same roundings on the device and in the host build, whatever
// the contraction flag), the depth test z > 0.2, and the screen test with the division traded for comparisons,
//     -0.15 W <= x / z fx + W / 2 <= 1.15 W    <=>    |x fx| <= 0.65 W z        (z > 0),
// likewise in y.  The largest distance of a seen Gaussian is an INTEGER max on the bits of positive floats (order-independent: two runs give the
// same bits), the largest focal length falls out of the same camera walk; both land in two scratch words.  mip_fill, a second short kernel over
// [P], gives unseen Gaussians that maximum and scales by sqrt(0.2) / focal.  No host synchronisation anywhere.
//
// mip_activations / _backward -- the activations upstream evaluates on every iteration,
//     s'_i = sqrt(exp(r_i)^2 + f^2),        o' = sigmoid(r_o) prod_i c_i,   c_i = s_i / s'_i
// as one streaming pass each way (20 bytes in, 16 out per Gaussian forward).  The opacity factor is evaluated PER AXIS: upstream's
// sqrt(prod s^2 / prod (s^2 + f^2)) forms products of six scales, which leave fp32's normal range for scales near 1e-7; no quantity here is
// smaller than s^2.  Gradients (f is a constant): ds'_i/dr_i = s_i c_i, do'/dr_i = o' (f / s'_i)^2, do'/dr_o = prod c_i sigma (1 - sigma) with
// sigma (1 - sigma) = e / (1 + e)^2, e = exp(-|r_o|) (no cancellation at either end).
#include "gsr_internal.h"

namespace {

constexpr int kSweepItems = 4;           // Gaussians per lane of the sweep: one camera record (a 64-byte scalar load) serves 256 pairs of a wave
constexpr int kSweepBlock = 256;
constexpr float kNearZ = 0.2f;           // upstream's depth test
constexpr float kFarDistance = 100000.f; // upstream's initial distance
constexpr float kScreenHalf = 0.65f;     // half a screen enlarged by 15 % on every side
constexpr float kSqrtFifth = 0.4472135955f;      // 0.2 ** 0.5
constexpr float kFltMax = 3.402823466e38f;
constexpr int kActGridCap = 2048;        // blocks of 256: 8 per CU on 256 CUs, the rest is grid-stride (mcmc.hip)

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= kFltMax; }      // false for NaN and +-inf

// words[0]: bits of the largest distance of a seen Gaussian (0: none seen), words[1]: bits of the largest focal_x; both zero at the launch.
// dist[i] = the smallest z over the cameras that see Gaussian i, -1 when none does.
__global__ void __launch_bounds__(kSweepBlock)
mip_sweep_kernel(int P, const float* __restrict__ means, int C, const float* __restrict__ cams, float* __restrict__ dist,
                 uint8_t* __restrict__ seen, uint32_t* __restrict__ words) {
    const int64_t first = (int64_t)blockIdx.x * (kSweepBlock * kSweepItems) + threadIdx.x;
    float mx[kSweepItems], my[kSweepItems], mz[kSweepItems], d[kSweepItems];      // d: the smallest z of a camera that sees it; +inf: none yet
#pragma unroll
    for (int k = 0; k < kSweepItems; ++k) {      // unconditional loads from a clamped address: the four rows are in flight together
        const int64_t i = first + (int64_t)k * kSweepBlock, j = i < P ? i : (int64_t)P - 1;
        mx[k] = means[3 * j]; my[k] = means[3 * j + 1]; mz[k] = means[3 * j + 2];
    }
#pragma unroll
    for (int k = 0; k < kSweepItems; ++k) {
        const int64_t i = first + (int64_t)k * kSweepBlock;
        // a mean that is not finite (and a lane past the end) fails every comparison below
        const bool ok = (i < P) & finite1(mx[k]) & finite1(my[k]) & finite1(mz[k]);
        const float nan = __uint_as_float(0x7FC00000u);
        mx[k] = ok ? mx[k] : nan; my[k] = ok ? my[k] : nan; mz[k] = ok ? mz[k] : nan;
        d[k] = __uint_as_float(0x7F800000u);
    }
    float focal_max = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ r = cams + 16 * (int64_t)c;      // wave-uniform: scalar loads
        const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
        const float t0 = r[9], t1 = r[10], t2 = r[11], fx = r[12], fy = r[13];
        const float lx = kScreenHalf * r[14], ly = kScreenHalf * r[15];
        focal_max = fmaxf(focal_max, fx);
#pragma unroll
        for (int k = 0; k < kSweepItems; ++k) {
            const float z = fmaf(mx[k], r02, fmaf(my[k], r12, fmaf(mz[k], r22, t2)));      // cam = xyz R + T
            const float x = fmaf(mx[k], r00, fmaf(my[k], r10, fmaf(mz[k], r20, t0)));
            const float y = fmaf(mx[k], r01, fmaf(my[k], r11, fmaf(mz[k], r21, t1)));
            // (z <= FLT_MAX: a depth that overflowed is upstream's inf / inf = NaN on the screen, i.e. not seen)
            // (bitwise: four comparisons and three mask operations, no branch in the loop)
            const bool valid = (z > kNearZ) & (z <= kFltMax) & (fabsf(x * fx) <= lx * z) & (fabsf(y * fy) <= ly * z);
            d[k] = valid ? fminf(d[k], z) : d[k];      // (a seeing camera has z <= FLT_MAX: d below +inf IS upstream's valid_points)
        }
    }
    uint32_t top = 0u;      // bits of a positive float order like the float
#pragma unroll
    for (int k = 0; k < kSweepItems; ++k) {
        const int64_t i = first + (int64_t)k * kSweepBlock;
        const bool any = d[k] <= kFltMax;
        const float dd = fminf(d[k], kFarDistance);      // upstream's distance starts at 100000
        if (i < P) {
            dist[i] = any ? dd : -1.f;
            if (seen) seen[i] = any ? 1 : 0;
            if (any) top = max(top, __float_as_uint(dd));
        }
    }
    // every lane of the wave is still here (no early exit above): butterfly max, one integer atomic per wave
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) top = max(top, __shfl_xor(top, m));
    if ((threadIdx.x & 63) == 0 && top != 0u) atomicMax(&words[0], top);
    if (blockIdx.x == 0 && threadIdx.x == 0) words[1] = __float_as_uint(focal_max);
}

__global__ void __launch_bounds__(256)
mip_fill_kernel(int P, float* __restrict__ filter, const uint32_t* __restrict__ words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t top = words[0];
    const float fill = top ? __uint_as_float(top) : kFarDistance;      // nothing seen at all: the initial distance stays
    const float focal = __uint_as_float(words[1]);
    float dd = filter[i];
    if (!(dd >= 0.f)) dd = fill;
    filter[i] = __fmul_rn(__fdiv_rn(dd, focal), kSqrtFifth);
}

// ---- activations -------------------------------------------------------------------------------------------------------------------------
struct ActRow { float sp0, sp1, sp2, c0, c1, c2, s0, s1, s2, e, op; };      // s'_i, c_i, s_i, exp(-|r_o|), o'

__device__ __forceinline__ void act_axis(float r, float f2, float& s, float& sp, float& c) {
    s = (float)exp((double)r);      // (fp64 exp rounded once, as mcmc.hip: hidden behind the memory traffic, and the same float on every libm)
    sp = __fsqrt_rn(__fadd_rn(__fmul_rn(s, s), f2));
    c = __fdiv_rn(s, sp);
}

__device__ __forceinline__ ActRow act_row(float r0, float r1, float r2, float ro, float f) {
    ActRow a;
    const float f2 = __fmul_rn(f, f);
    act_axis(r0, f2, a.s0, a.sp0, a.c0);
    act_axis(r1, f2, a.s1, a.sp1, a.c1);
    act_axis(r2, f2, a.s2, a.sp2, a.c2);
    a.e = (float)exp(-(double)fabsf(ro));
    const float den = 1.f + a.e;
    const float sig = ro >= 0.f ? __fdiv_rn(1.f, den) : (ro < 0.f ? __fdiv_rn(a.e, den) : ro /*NaN*/);
    a.op = sig * (a.c0 * a.c1 * a.c2);
    return a;
}

// gradients of one row; false: the row is contained (a raw value or f not finite, or an output not finite) and its gradients are zero
__device__ __forceinline__ bool act_row_grad(float r0, float r1, float r2, float ro, float f, float g0, float g1, float g2, float go, float& d0,
                                             float& d1, float& d2, float& dopac) {
    const ActRow a = act_row(r0, r1, r2, ro, f);
    const bool ok = finite1(r0) && finite1(r1) && finite1(r2) && finite1(ro) && finite1(f) && finite1(a.sp0) && finite1(a.sp1) &&
                    finite1(a.sp2) && finite1(a.op);
    const float t0 = __fdiv_rn(f, a.sp0), t1 = __fdiv_rn(f, a.sp1), t2 = __fdiv_rn(f, a.sp2);
    const float w = go * a.op;
    const float den = 1.f + a.e;
    d0 = g0 * (a.s0 * a.c0) + w * (t0 * t0);
    d1 = g1 * (a.s1 * a.c1) + w * (t1 * t1);
    d2 = g2 * (a.s2 * a.c2) + w * (t2 * t2);
    dopac = go * ((a.c0 * a.c1 * a.c2) * __fdiv_rn(a.e, den * den));
    if (!ok) d0 = d1 = d2 = dopac = 0.f;
    return ok;
}

// `vec`: every pointer is 16-byte aligned -> a lane takes FOUR consecutive Gaussians (three 16-byte accesses per [P,3] array, one per [P] array,
// as mcmc.hip); the P mod 4 rows left over, and every row when a pointer is not aligned, go through scalar accesses.  The arithmetic is the same.
__global__ void __launch_bounds__(256)
mip_activations_kernel(int P, const float* __restrict__ rs, const float* __restrict__ ro, const float* __restrict__ flt, float* __restrict__ so,
                       float* __restrict__ oo, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    auto row = [&](int64_t i) {
        const ActRow a = act_row(rs[3 * i], rs[3 * i + 1], rs[3 * i + 2], ro[i], flt[i]);
        so[3 * i] = a.sp0; so[3 * i + 1] = a.sp1; so[3 * i + 2] = a.sp2;
        oo[i] = a.op;
    };
    if (!vec) {
        for (int64_t i = tid; i < P; i += stride) row(i);
        return;
    }
    const int64_t groups = (int64_t)P >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(rs);
    const float4* o4 = reinterpret_cast<const float4*>(ro);
    const float4* f4 = reinterpret_cast<const float4*>(flt);
    float4* so4 = reinterpret_cast<float4*>(so);
    float4* oo4 = reinterpret_cast<float4*>(oo);
    for (int64_t g = tid; g < groups; g += stride) {
        const float4 sa = s4[3 * g], sb = s4[3 * g + 1], sc = s4[3 * g + 2], op = o4[g], ff = f4[g];
        const ActRow a = act_row(sa.x, sa.y, sa.z, op.x, ff.x), b = act_row(sa.w, sb.x, sb.y, op.y, ff.y);
        const ActRow c = act_row(sb.z, sb.w, sc.x, op.z, ff.z), d = act_row(sc.y, sc.z, sc.w, op.w, ff.w);
        so4[3 * g] = make_float4(a.sp0, a.sp1, a.sp2, b.sp0);
        so4[3 * g + 1] = make_float4(b.sp1, b.sp2, c.sp0, c.sp1);
        so4[3 * g + 2] = make_float4(c.sp2, d.sp0, d.sp1, d.sp2);
        oo4[g] = make_float4(a.op, b.op, c.op, d.op);
    }
    if (tid < (P & 3)) row((groups << 2) + tid);
}

// gs / go may be NULL: an absent incoming gradient is a zero, through the same arithmetic (the bits of a call that passes zeros)
__global__ void __launch_bounds__(256)
mip_activations_bwd_kernel(int P, const float* __restrict__ rs, const float* __restrict__ ro, const float* __restrict__ flt,
                           const float* __restrict__ gs, const float* __restrict__ go, float* __restrict__ ds, float* __restrict__ dop, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    auto row = [&](int64_t i) {
        float d0, d1, d2, dd;
        act_row_grad(rs[3 * i], rs[3 * i + 1], rs[3 * i + 2], ro[i], flt[i], gs ? gs[3 * i] : 0.f, gs ? gs[3 * i + 1] : 0.f,
                     gs ? gs[3 * i + 2] : 0.f, go ? go[i] : 0.f, d0, d1, d2, dd);
        ds[3 * i] = d0; ds[3 * i + 1] = d1; ds[3 * i + 2] = d2;
        dop[i] = dd;
    };
    if (!vec) {
        for (int64_t i = tid; i < P; i += stride) row(i);
        return;
    }
    const int64_t groups = (int64_t)P >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(rs);
    const float4* o4 = reinterpret_cast<const float4*>(ro);
    const float4* f4 = reinterpret_cast<const float4*>(flt);
    const float4* gs4 = reinterpret_cast<const float4*>(gs);
    const float4* go4 = reinterpret_cast<const float4*>(go);
    float4* ds4 = reinterpret_cast<float4*>(ds);
    float4* dop4 = reinterpret_cast<float4*>(dop);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t g = tid; g < groups; g += stride) {
        const float4 sa = s4[3 * g], sb = s4[3 * g + 1], sc = s4[3 * g + 2], op = o4[g], ff = f4[g];
        const float4 ga = gs ? gs4[3 * g] : zero, gb = gs ? gs4[3 * g + 1] : zero, gc = gs ? gs4[3 * g + 2] : zero, gq = go ? go4[g] : zero;
        float4 da, db, dc, dq;
        act_row_grad(sa.x, sa.y, sa.z, op.x, ff.x, ga.x, ga.y, ga.z, gq.x, da.x, da.y, da.z, dq.x);
        act_row_grad(sa.w, sb.x, sb.y, op.y, ff.y, ga.w, gb.x, gb.y, gq.y, da.w, db.x, db.y, dq.y);
        act_row_grad(sb.z, sb.w, sc.x, op.z, ff.z, gb.z, gb.w, gc.x, gq.z, db.z, db.w, dc.x, dq.z);
        act_row_grad(sc.y, sc.z, sc.w, op.w, ff.w, gc.y, gc.z, gc.w, gq.w, dc.y, dc.z, dc.w, dq.w);
        ds4[3 * g] = da; ds4[3 * g + 1] = db; ds4[3 * g + 2] = dc;
        dop4[g] = dq;
    }
    if (tid < (P & 3)) row((groups << 2) + tid);
}

inline int act_grid(int P, int vec) {
    const int64_t items = vec ? (((int64_t)P + 3) >> 2) : (int64_t)P;      // (ceil: the block that owns the tail rows exists when P < 4)
    int64_t nb = (items + 255) / 256;
    if (nb > kActGridCap) nb = kActGridCap;
    return nb < 1 ? 1 : (int)nb;
}

}  // namespace

void gsr_launch_mip_filter(int P, const float* means, int C, const float* cameras, float* filter, uint8_t* seen, uint32_t* words, hipStream_t st) {
    (void)hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), st);
    const int64_t per_block = (int64_t)kSweepBlock * kSweepItems;
    hipLaunchKernelGGL(mip_sweep_kernel, dim3((unsigned)(((int64_t)P + per_block - 1) / per_block)), dim3(kSweepBlock), 0, st, P, means, C, cameras,
                       filter, seen, words);
    hipLaunchKernelGGL(mip_fill_kernel, dim3((unsigned)(((int64_t)P + 255) / 256)), dim3(256), 0, st, P, filter, (const uint32_t*)words);
}

void gsr_launch_mip_activations(int P, const float* raw_scales, const float* raw_opacity, const float* filter, float* scales_out,
                                float* opacity_out, hipStream_t st) {
    const int vec = (((uintptr_t)raw_scales | (uintptr_t)raw_opacity | (uintptr_t)filter | (uintptr_t)scales_out | (uintptr_t)opacity_out) & 15) == 0;
    hipLaunchKernelGGL(mip_activations_kernel, dim3(act_grid(P, vec)), dim3(256), 0, st, P, raw_scales, raw_opacity, filter, scales_out, opacity_out,
                       vec);
}

void gsr_launch_mip_activations_backward(int P, const float* raw_scales, const float* raw_opacity, const float* filter, const float* dL_dscales,
                                         const float* dL_dopacity, float* dL_draw_scales, float* dL_draw_opacity, hipStream_t st) {
    const int vec = (((uintptr_t)raw_scales | (uintptr_t)raw_opacity | (uintptr_t)filter | (uintptr_t)dL_dscales | (uintptr_t)dL_dopacity |
                      (uintptr_t)dL_draw_scales | (uintptr_t)dL_draw_opacity) & 15) == 0;      // (a NULL gradient counts as aligned)
    hipLaunchKernelGGL(mip_activations_bwd_kernel, dim3(act_grid(P, vec)), dim3(256), 0, st, P, raw_scales, raw_opacity, filter, dL_dscales,
                       dL_dopacity, dL_draw_scales, dL_draw_opacity, vec);
}
