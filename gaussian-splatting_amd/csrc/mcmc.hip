// 3DGS-MCMC density control (Kheradmand et al. 2024; gsplat's MCMCStrategy): the two native pieces, DESIGN.md 5.9.
//
// mcmc_noise -- the per-iteration part, every Gaussian after every optimizer step:
//     xyz[i] += R diag(s^2) R^T xi[i] * g * noise_scale,      g = 1 / (1 + exp(-k ((1 - o) - x0)))
// Upstream this is ~20 small torch kernels with [P,3,3] temporaries (L = R diag(s), Sigma = L L^T, bmm with the noise); here ONE streaming
// pass, 56 bytes in and 12 out per Gaussian, Sigma never formed.  The gate multiplies every error of its argument by k (100): it is evaluated
// in fp64 (two exp per Gaussian, hidden behind the memory traffic), the 3x3 work in fp32 without contraction.  A row whose displacement is not
// finite in all three components (NaN / inf scale, zero quaternion, NaN opacity, inf noise) keeps its mean bit for bit.
//
// mcmc_relocation -- every 100 iterations on a few per cent of the Gaussians, fp64 throughout: the opacity / scale of a Gaussian that is
// replaced by N copies of itself so that the rendered image does not change,
//     o' = 1 - (1 - o)^(1/N) = -expm1(log1p(-o) / N),    D = sum_{k=0}^{N-1} (-1)^k C(N, k+1) o'^(k+1) / sqrt(k+1),    s' = s o / D
// D is upstream's double sum  sum_{i=1}^{N} sum_{k<i} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)  with the inner binomials summed over i by the
// hockey-stick identity  sum_{i=k+1}^{N} C(i-1, k) = C(N, k+1).
#include "gsr_internal.h"

namespace {

constexpr int kNoiseGridCap = 2048;      // blocks of 256: 8 per CU on 256 CUs, the rest is grid-stride
constexpr int kRelocMaxRatio = 51;       // upstream's binomial table has 51 rows

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= 3.402823466e38f; }      // false for NaN and +-inf

// One Gaussian: the displacement d and whether all of it is finite.  (sx, sy, sz) and op are raw (log scale, logit) unless `activated`.
__device__ __forceinline__ bool noise_delta(float sx, float sy, float sz, float qw, float qx, float qy, float qz, float op, float e0, float e1,
                                            float e2, int activated, float noise_scale, float gate_k, float gate_x0, float& dx, float& dy,
                                            float& dz) {
    if (!activated) { sx = expf(sx); sy = expf(sy); sz = expf(sz); }
    const double o = activated ? (double)op : 1.0 / (1.0 + exp(-(double)op));
    const double gs = (double)noise_scale / (1.0 + exp(-(double)gate_k * ((1.0 - o) - (double)gate_x0)));
    const float n = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    const float r = qw / n, x = qx / n, y = qy / n, z = qz / n;
    const float r00 = 1.f - 2.f * (y * y + z * z), r01 = 2.f * (x * y - r * z), r02 = 2.f * (x * z + r * y);
    const float r10 = 2.f * (x * y + r * z), r11 = 1.f - 2.f * (x * x + z * z), r12 = 2.f * (y * z - r * x);
    const float r20 = 2.f * (x * z - r * y), r21 = 2.f * (y * z + r * x), r22 = 1.f - 2.f * (x * x + y * y);
    const float w0 = sx * sx * (r00 * e0 + r10 * e1 + r20 * e2);      // s^2 (.) R^T xi
    const float w1 = sy * sy * (r01 * e0 + r11 * e1 + r21 * e2);
    const float w2 = sz * sz * (r02 * e0 + r12 * e1 + r22 * e2);
    // the product with g noise_scale in fp64, rounded once: g goes down to e^-99 and the result may be an fp32 denormal
    dx = (float)((double)(r00 * w0 + r01 * w1 + r02 * w2) * gs);
    dy = (float)((double)(r10 * w0 + r11 * w1 + r12 * w2) * gs);
    dz = (float)((double)(r20 * w0 + r21 * w1 + r22 * w2) * gs);
    return finite1(dx) && finite1(dy) && finite1(dz);
}

__device__ __forceinline__ void noise_row(int64_t i, float* __restrict__ xyz, const float* __restrict__ scales, const float* __restrict__ rot,
                                          const float* __restrict__ opac, const float* __restrict__ xi, int activated, float noise_scale,
                                          float gate_k, float gate_x0) {
    float dx, dy, dz;
    if (!noise_delta(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2], rot[4 * i], rot[4 * i + 1], rot[4 * i + 2], rot[4 * i + 3], opac[i],
                     xi[3 * i], xi[3 * i + 1], xi[3 * i + 2], activated, noise_scale, gate_k, gate_x0, dx, dy, dz))
        return;
    xyz[3 * i] += dx; xyz[3 * i + 1] += dy; xyz[3 * i + 2] += dz;
}

// `vec`: every pointer is 16-byte aligned -> a lane takes FOUR consecutive Gaussians: the 48 bytes of their xyz / scale / noise rows are three
// aligned 16-byte accesses each, the quaternions four, the opacities one (1 KB per wave instruction); the P mod 4 rows left over, and every row
// when a pointer is not aligned, go through scalar accesses.
__global__ void __launch_bounds__(256)
mcmc_noise_kernel(int P, float* __restrict__ xyz, const float* __restrict__ scales, const float* __restrict__ rot, const float* __restrict__ opac,
                  const float* __restrict__ xi, int activated, float noise_scale, float gate_k, float gate_x0, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (!vec) {
        for (int64_t i = tid; i < P; i += stride) noise_row(i, xyz, scales, rot, opac, xi, activated, noise_scale, gate_k, gate_x0);
        return;
    }
    const int64_t groups = (int64_t)P >> 2;
    float4* x4 = reinterpret_cast<float4*>(xyz);
    const float4* s4 = reinterpret_cast<const float4*>(scales);
    const float4* q4 = reinterpret_cast<const float4*>(rot);
    const float4* o4 = reinterpret_cast<const float4*>(opac);
    const float4* e4 = reinterpret_cast<const float4*>(xi);
    for (int64_t g = tid; g < groups; g += stride) {
        float4 xa = x4[3 * g], xb = x4[3 * g + 1], xc = x4[3 * g + 2];
        const float4 sa = s4[3 * g], sb = s4[3 * g + 1], sc = s4[3 * g + 2];
        const float4 ea = e4[3 * g], eb = e4[3 * g + 1], ec = e4[3 * g + 2];
        const float4 qa = q4[4 * g], qb = q4[4 * g + 1], qc = q4[4 * g + 2], qd = q4[4 * g + 3];
        const float4 oo = o4[g];
        float dx, dy, dz;
        if (noise_delta(sa.x, sa.y, sa.z, qa.x, qa.y, qa.z, qa.w, oo.x, ea.x, ea.y, ea.z, activated, noise_scale, gate_k, gate_x0, dx, dy, dz)) {
            xa.x += dx; xa.y += dy; xa.z += dz;
        }
        if (noise_delta(sa.w, sb.x, sb.y, qb.x, qb.y, qb.z, qb.w, oo.y, ea.w, eb.x, eb.y, activated, noise_scale, gate_k, gate_x0, dx, dy, dz)) {
            xa.w += dx; xb.x += dy; xb.y += dz;
        }
        if (noise_delta(sb.z, sb.w, sc.x, qc.x, qc.y, qc.z, qc.w, oo.z, eb.z, eb.w, ec.x, activated, noise_scale, gate_k, gate_x0, dx, dy, dz)) {
            xb.z += dx; xb.w += dy; xc.x += dz;
        }
        if (noise_delta(sc.y, sc.z, sc.w, qd.x, qd.y, qd.z, qd.w, oo.w, ec.y, ec.z, ec.w, activated, noise_scale, gate_k, gate_x0, dx, dy, dz)) {
            xc.y += dx; xc.z += dy; xc.w += dz;
        }
        x4[3 * g] = xa; x4[3 * g + 1] = xb; x4[3 * g + 2] = xc;      // (a row that was skipped is written back with the bits that were read)
    }
    if (tid < (P & 3)) noise_row((groups << 2) + tid, xyz, scales, rot, opac, xi, activated, noise_scale, gate_k, gate_x0);
}

__global__ void __launch_bounds__(256)
mcmc_relocation_kernel(int n, const float* __restrict__ opac, const float* __restrict__ scales /*[n,3]*/, const int32_t* __restrict__ ratios,
                       float* __restrict__ new_opac, float* __restrict__ new_scales) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float of = opac[i];
    const float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    float no = of;
    double f = 1.0;
    if (of > 0.f && of < 1.f) {      // (false for NaN; o == 0 is the limit: opacity 0, scale unchanged; anything else is handed back as it came)
        const int N = min(max(ratios[i], 1), kRelocMaxRatio);
        const double o = (double)of, o1 = -expm1(log1p(-o) / (double)N);
        double D = 0.0, c = 1.0, p = 1.0, sign = 1.0;
        for (int k = 0; k < N; ++k) {
            c = c * (double)(N - k) / (double)(k + 1);      // C(N, k+1): an integer below 2^53 at every step, so the recurrence is exact
            p *= o1;
            D += sign * c * p / sqrt((double)(k + 1));
            sign = -sign;
        }
        no = (float)o1;
        f = o / D;
    }
    new_opac[i] = no;
    new_scales[3 * i] = (float)((double)s0 * f); new_scales[3 * i + 1] = (float)((double)s1 * f); new_scales[3 * i + 2] = (float)((double)s2 * f);
}

}  // namespace

void gsr_launch_mcmc_noise(int P, float* xyz, const float* scales, const float* rot, const float* opac, const float* noise, int activated,
                           float noise_scale, float gate_k, float gate_x0, hipStream_t st) {
    const int vec = (((uintptr_t)xyz | (uintptr_t)scales | (uintptr_t)rot | (uintptr_t)opac | (uintptr_t)noise) & 15) == 0;
    const int64_t items = vec ? (((int64_t)P + 3) >> 2) : (int64_t)P;      // (ceil: the block that owns the tail rows exists when P < 4)
    int64_t nb = (items + 255) / 256;
    if (nb > kNoiseGridCap) nb = kNoiseGridCap;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3((int)nb), dim3(256), 0, st, P, xyz, scales, rot, opac, noise, activated, noise_scale, gate_k,
                       gate_x0, vec);
}

void gsr_launch_mcmc_relocation(int n, const float* opac, const float* scales, const int32_t* ratios, float* new_opac, float* new_scales,
                                hipStream_t st) {
    hipLaunchKernelGGL(mcmc_relocation_kernel, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, st, n, opac, scales, ratios, new_opac,
                       new_scales);
}
