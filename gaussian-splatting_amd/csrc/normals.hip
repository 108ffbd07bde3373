// Normal-consistency regulariser (2DGS / GOF / RaDe-GS / PGSR): per-Gaussian normals, normals of a depth map, and the fused loss
//     loss = (1 / (H W)) sum_p [1 - w(p) <normals(p), Nd(p)>],                                                          DESIGN.md 5.11.
//
// Per-Gaussian normals -- one streaming pass, a row per thread: the column of R(q) (gsr_math.h's matrix, q as given) that belongs to the smallest
// scale (lowest index on ties), rotated into the camera by the 3x3 part of the view matrix, normalised, and flipped to face the camera.  The
// backward recomputes the column index and the sign from its inputs and differentiates the column and the normalisation only.
//
// Depth normals -- the DIFFERENCE form of include/gsr.h: with dz = z(x+1) - z(x-1), sz their sum (dz', sz' along y), the ray r = (nx tanfovx,
// ny tanfovy, 1), alpha = tanfovy 2 / H and beta = tanfovx 2 / W the cross product dv x du of the contract collapses to
//     c = (alpha P,  beta Q,  -(r_x alpha P + r_y beta Q + alpha beta S)),      P = sz' dz,  Q = sz dz',  S = sz sz'
// (the products n dz dz' of the two tangents cancel identically; they are never formed).  The only subtractions of nearly equal numbers are the
// depth differences themselves, which are exact to half an ulp of the depth.  Nd = c / |c|.
//
// A workgroup takes a 64 x 16 tile and stages the depths it needs in LDS once (halo 1 for the forward kernels, halo 2 for the depth backward); a
// depth outside the image is staged as 0, i.e. as an invalid depth.  The depth backward is a gather without atomics: phase 1 computes, for every
// pixel q of the tile and a halo of 1, what q hands to its left / right / upper / lower neighbour (four floats in LDS); phase 2 adds, per pixel,
// the four values addressed to it in a fixed order.  Two runs give the same bits.  The loss is summed in fp64: one partial per workgroup, a
// one-workgroup kernel adds them in index order.
#include <cfloat>

#include "gsr_internal.h"
#include "gsr_reduce.h"

namespace {

constexpr int kTW = 64, kTH = 16;      // tile: one lane per column, 4 rows per wave

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= FLT_MAX; }      // false for NaN and +-inf
__device__ __forceinline__ bool pos_finite(float z) { return z > 0.f && z <= FLT_MAX; }

// ---- per-Gaussian normals -----------------------------------------------------------------------------------------------------------------------
struct GnRow {
    float n[3];        // the output normal (0 when !ok)
    float u[3];        // v / |v| before the flip
    float inv, sgn;    // 1 / |v|, +-1
    int k;
    bool ok;
};

__device__ __forceinline__ GnRow gn_row(int64_t g, const float* __restrict__ scales, const float* __restrict__ rot, const float* __restrict__ means,
                                        const float* __restrict__ vm, float (&q)[4]) {
    GnRow o;
    const float s0 = scales[3 * g], s1 = scales[3 * g + 1], s2 = scales[3 * g + 2];
    const float r = rot[4 * g], x = rot[4 * g + 1], y = rot[4 * g + 2], z = rot[4 * g + 3];
    const float m0 = means[3 * g], m1 = means[3 * g + 1], m2 = means[3 * g + 2];
    q[0] = r; q[1] = x; q[2] = y; q[3] = z;
    int k = 0;
    float smin = s0;
    if (s1 < smin) { k = 1; smin = s1; }
    if (s2 < smin) k = 2;
    o.k = k;
    float a0, a1, a2;      // column k of R(q)
    if (k == 0) { a0 = 1.f - 2.f * (y * y + z * z); a1 = 2.f * (x * y + r * z); a2 = 2.f * (x * z - r * y); }
    else if (k == 1) { a0 = 2.f * (x * y - r * z); a1 = 1.f - 2.f * (x * x + z * z); a2 = 2.f * (y * z + r * x); }
    else { a0 = 2.f * (x * z + r * y); a1 = 2.f * (y * z - r * x); a2 = 1.f - 2.f * (x * x + y * y); }
    float v[3], p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = vm[i] * a0 + vm[4 + i] * a1 + vm[8 + i] * a2;
        p[i] = vm[i] * m0 + vm[4 + i] * m1 + vm[8 + i] * m2 + vm[12 + i];
    }
    const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    o.ok = finite1(s0) && finite1(s1) && finite1(s2) && finite1(r) && finite1(x) && finite1(y) && finite1(z) && finite1(m0) && finite1(m1) &&
           finite1(m2) && finite1(p[0]) && finite1(p[1]) && finite1(p[2]) && len > 0.f && len <= FLT_MAX;
    o.inv = o.ok ? 1.f / len : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.u[i] = o.ok ? v[i] * o.inv : 0.f;
    o.sgn = (o.u[0] * p[0] + o.u[1] * p[1] + o.u[2] * p[2] > 0.f) ? -1.f : 1.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.n[i] = o.ok ? o.sgn * o.u[i] : 0.f;
    return o;
}

__global__ void __launch_bounds__(256)
gaussian_normals_kernel(int P, const float* __restrict__ scales, const float* __restrict__ rot, const float* __restrict__ means,
                        const float* __restrict__ vm, float* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    float q[4];
    const GnRow o = gn_row(g, scales, rot, means, vm, q);
    out[3 * g] = o.n[0]; out[3 * g + 1] = o.n[1]; out[3 * g + 2] = o.n[2];
}

__global__ void __launch_bounds__(256)
gaussian_normals_bwd_kernel(int P, const float* __restrict__ scales, const float* __restrict__ rot, const float* __restrict__ means,
                            const float* __restrict__ vm, const float* __restrict__ dn, float* __restrict__ drot) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    float q[4];
    const GnRow o = gn_row(g, scales, rot, means, vm, q);
    const float g0 = dn[3 * g], g1 = dn[3 * g + 1], g2 = dn[3 * g + 2];
    const bool ok = o.ok && finite1(g0) && finite1(g1) && finite1(g2);
    // n = sgn u, u = v / |v|:  dL/dv = sgn (g - u <u, g>) / |v|
    const float dot = o.u[0] * g0 + o.u[1] * g1 + o.u[2] * g2;
    const float sc = o.sgn * o.inv;
    const float dv0 = (g0 - o.u[0] * dot) * sc, dv1 = (g1 - o.u[1] * dot) * sc, dv2 = (g2 - o.u[2] * dot) * sc;
    // v_i = sum_j vm[4 j + i] a_j
    const float d0 = vm[0] * dv0 + vm[1] * dv1 + vm[2] * dv2;
    const float d1 = vm[4] * dv0 + vm[5] * dv1 + vm[6] * dv2;
    const float d2 = vm[8] * dv0 + vm[9] * dv1 + vm[10] * dv2;
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    float dr, dx, dy, dz;
    if (o.k == 0) {          // a = (1 - 2 (yy + zz), 2 (xy + rz), 2 (xz - ry))
        dr = 2.f * (z * d1 - y * d2);
        dx = 2.f * (y * d1 + z * d2);
        dy = 2.f * (x * d1 - r * d2) - 4.f * y * d0;
        dz = 2.f * (r * d1 + x * d2) - 4.f * z * d0;
    } else if (o.k == 1) {   // a = (2 (xy - rz), 1 - 2 (xx + zz), 2 (yz + rx))
        dr = 2.f * (x * d2 - z * d0);
        dx = 2.f * (y * d0 + r * d2) - 4.f * x * d1;
        dy = 2.f * (x * d0 + z * d2);
        dz = 2.f * (y * d2 - r * d0) - 4.f * z * d1;
    } else {                 // a = (2 (xz + ry), 2 (yz - rx), 1 - 2 (xx + yy))
        dr = 2.f * (y * d0 - x * d1);
        dx = 2.f * (z * d0 - r * d1) - 4.f * x * d2;
        dy = 2.f * (r * d0 + z * d1) - 4.f * y * d2;
        dz = 2.f * (x * d0 + y * d1);
    }
    drot[4 * g] = ok ? dr : 0.f; drot[4 * g + 1] = ok ? dx : 0.f; drot[4 * g + 2] = ok ? dy : 0.f; drot[4 * g + 3] = ok ? dz : 0.f;
}

// ---- depth normals: one pixel ---------------------------------------------------------------------------------------------------------------------
struct NdPix {
    float n[3];                  // Nd (0 when !ok)
    float inv;                   // 1 / |c| (0 when !ok)
    float dz, sz, dzy, szy;      // the differences and sums of the stencil
    float rx, ry;                // the ray (rx, ry, 1)
    bool ok;
};

__device__ __forceinline__ NdPix nd_pixel(const GsrNormalsFrame& f, int x, int y, float zc, float zl, float zr, float zu, float zd) {
    NdPix q;
    q.dz = zr - zl; q.sz = zr + zl; q.dzy = zd - zu; q.szy = zd + zu;
    // nx = (2 x + 1) / W - 1 as (2 x + 1 - W) / W: the numerator is an exact integer, nothing cancels near the principal point
    q.rx = (float)(2 * x + 1 - f.W) * f.inv_w * f.tx;
    q.ry = (float)(2 * y + 1 - f.H) * f.inv_h * f.ty;
    const float cx = f.alpha * (q.szy * q.dz), cy = f.beta * (q.sz * q.dzy);
    const float cz = -(q.rx * cx + q.ry * cy + f.ab * (q.sz * q.szy));
    const float len = sqrtf(cx * cx + cy * cy + cz * cz);
    q.ok = x >= 1 && x <= f.W - 2 && y >= 1 && y <= f.H - 2 && pos_finite(zc) && pos_finite(zl) && pos_finite(zr) && pos_finite(zu) &&
           pos_finite(zd) && len > 0.f && len <= FLT_MAX;
    q.inv = q.ok ? 1.f / len : 0.f;
    q.n[0] = q.ok ? cx * q.inv : 0.f; q.n[1] = q.ok ? cy * q.inv : 0.f; q.n[2] = q.ok ? cz * q.inv : 0.f;
    return q;
}

// g = dL/dNd of a valid pixel -> what the pixel hands to its left (x - 1), right, upper (y - 1) and lower neighbour's depth gradient
__device__ __forceinline__ float4 nd_backward(const GsrNormalsFrame& f, const NdPix& q, float g0, float g1, float g2) {
    const float dot = q.n[0] * g0 + q.n[1] * g1 + q.n[2] * g2;
    const float G0 = (g0 - q.n[0] * dot) * q.inv, G1 = (g1 - q.n[1] * dot) * q.inv, G2 = (g2 - q.n[2] * dot) * q.inv;      // dL/dc
    const float dP = f.alpha * (G0 - q.rx * G2), dQ = f.beta * (G1 - q.ry * G2), dS = -f.ab * G2;
    const float g_dz = q.szy * dP, g_szy = q.dz * dP + q.sz * dS, g_dzy = q.sz * dQ, g_sz = q.dzy * dQ + q.szy * dS;
    return make_float4(g_sz - g_dz, g_sz + g_dz, g_szy - g_dzy, g_szy + g_dzy);
}

__device__ __forceinline__ void tile_origin(const GsrNormalsFrame& f, int& x0, int& y0) {
    const int ty = (int)blockIdx.x / f.tiles_x, tx = (int)blockIdx.x - ty * f.tiles_x;
    x0 = tx * kTW;
    y0 = ty * kTH;
}

// the depths of the tile at (x0, y0) and HALO pixels around it -> s[(kTH + 2 HALO)][(kTW + 2 HALO)]; outside the image: 0
template <int HALO>
__device__ __forceinline__ void stage_depth(const GsrNormalsFrame& f, const float* __restrict__ depth, int x0, int y0, float* s) {
    constexpr int SW = kTW + 2 * HALO, SH = kTH + 2 * HALO;
    for (int t = (int)threadIdx.x; t < SW * SH; t += 256) {
        const int ly = t / SW, lx = t - ly * SW, gx = x0 - HALO + lx, gy = y0 - HALO + ly;
        const bool in = gx >= 0 && gx < f.W && gy >= 0 && gy < f.H;
        const float v = depth[in ? (size_t)gy * f.W + gx : 0];      // (an unconditional load from a clamped address, the select afterwards)
        s[t] = in ? v : 0.f;
    }
}

// the pixel at column lx, row ly of a staged tile (coordinates of the halo-less tile; -HALO .. allowed up to the halo minus 1)
template <int HALO>
__device__ __forceinline__ NdPix nd_staged(const GsrNormalsFrame& f, const float* s, int x0, int y0, int lx, int ly) {
    constexpr int SW = kTW + 2 * HALO;
    const float* c = s + (ly + HALO) * SW + lx + HALO;
    return nd_pixel(f, x0 + lx, y0 + ly, c[0], c[-1], c[1], c[-SW], c[SW]);
}

// ---- depth -> normals ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
depth_normals_kernel(GsrNormalsFrame f, const float* __restrict__ depth, float* __restrict__ out) {
    __shared__ float sZ[(kTW + 2) * (kTH + 2)];
    int x0, y0;
    tile_origin(f, x0, y0);
    stage_depth<1>(f, depth, x0, y0, sZ);
    __syncthreads();
    const int lx = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, x = x0 + lx;
    const size_t plane = (size_t)f.H * f.W;
#pragma unroll
    for (int k = 0; k < kTH / 4; ++k) {
        const int ly = 4 * k + wave, y = y0 + ly;
        if (x >= f.W || y >= f.H) continue;
        const NdPix q = nd_staged<1>(f, sZ, x0, y0, lx, ly);
        const size_t idx = (size_t)y * f.W + x;
        out[idx] = q.n[0]; out[plane + idx] = q.n[1]; out[2 * plane + idx] = q.n[2];
    }
}

// ---- the fused loss -------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
normal_loss_kernel(GsrNormalsFrame f, const float* __restrict__ depth, const float* __restrict__ normals, const float* __restrict__ weight,
                   double* __restrict__ partials) {
    __shared__ float sZ[(kTW + 2) * (kTH + 2)];
    __shared__ double sSum[256];
    int x0, y0;
    tile_origin(f, x0, y0);
    stage_depth<1>(f, depth, x0, y0, sZ);
    __syncthreads();
    const int lx = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, x = x0 + lx;
    const size_t plane = (size_t)f.H * f.W;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kTH / 4; ++k) {
        const int ly = 4 * k + wave, y = y0 + ly;
        if (x >= f.W || y >= f.H) continue;
        const NdPix q = nd_staged<1>(f, sZ, x0, y0, lx, ly);
        const size_t idx = (size_t)y * f.W + x;
        const float n0 = normals[idx], n1 = normals[plane + idx], n2 = normals[2 * plane + idx];
        const float w = weight ? weight[idx] : 1.f;
        // (a select, not a product with zero: whatever `normals` holds where Nd = 0 or w = 0, the pixel contributes exactly 1)
        const float t = (q.ok && w != 0.f) ? w * (q.n[0] * n0 + q.n[1] * n1 + q.n[2] * n2) : 0.f;
        acc += 1.0 - (double)t;
    }
    const double sum = gsrw::block_sum_f64(acc, sSum);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256)
normal_loss_sum_kernel(int n, double pixels, const double* __restrict__ partials, float* __restrict__ loss_out) {
    __shared__ double s[256];
    gsrw::block_sum_partials_f64(n, partials, pixels, loss_out, s);
}

// dL/dnormals of the loss alone: -w Nd dL / (H W)
__global__ void __launch_bounds__(256)
normal_loss_bwd_normals_kernel(GsrNormalsFrame f, const float* __restrict__ depth, const float* __restrict__ weight,
                               const float* __restrict__ dL_dloss, float* __restrict__ dnormals) {
    __shared__ float sZ[(kTW + 2) * (kTH + 2)];
    int x0, y0;
    tile_origin(f, x0, y0);
    stage_depth<1>(f, depth, x0, y0, sZ);
    __syncthreads();
    const int lx = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, x = x0 + lx;
    const size_t plane = (size_t)f.H * f.W;
    const float s = dL_dloss[0] * f.inv_hw;
#pragma unroll
    for (int k = 0; k < kTH / 4; ++k) {
        const int ly = 4 * k + wave, y = y0 + ly;
        if (x >= f.W || y >= f.H) continue;
        const NdPix q = nd_staged<1>(f, sZ, x0, y0, lx, ly);
        const size_t idx = (size_t)y * f.W + x;
        const float w = weight ? weight[idx] : 1.f;
        const bool on = q.ok && w != 0.f;
        const float ws = -(w * s);
        dnormals[idx] = on ? ws * q.n[0] : 0.f; dnormals[plane + idx] = on ? ws * q.n[1] : 0.f; dnormals[2 * plane + idx] = on ? ws * q.n[2] : 0.f;
    }
}

// dL/ddepth (and, for the loss, dL/dnormals in the same pass).  LOSS = false: the incoming gradient is the tensor `gin` [3,H,W];
// LOSS = true: it is -w normals dL / (H W) formed on the fly from `gin` = normals, and `dnormals` (may be NULL) receives -w Nd dL / (H W).
template <bool LOSS>
__global__ void __launch_bounds__(256)
depth_normals_bwd_kernel(GsrNormalsFrame f, const float* __restrict__ depth, const float* __restrict__ gin, const float* __restrict__ weight,
                         const float* __restrict__ dL_dloss, float* __restrict__ dnormals, float* __restrict__ ddepth) {
    constexpr int GW = kTW + 2, GH = kTH + 2;
    __shared__ float sZ[(kTW + 4) * (kTH + 4)];
    __shared__ float4 sG[GW * GH];      // per pixel of the tile and a halo of 1: (to the left, to the right, to the upper, to the lower neighbour)
    int x0, y0;
    tile_origin(f, x0, y0);
    stage_depth<2>(f, depth, x0, y0, sZ);
    __syncthreads();
    const size_t plane = (size_t)f.H * f.W;
    const float s = LOSS ? dL_dloss[0] * f.inv_hw : 0.f;
    for (int t = (int)threadIdx.x; t < GW * GH; t += 256) {
        const int gy = t / GW, gx = t - gy * GW, lx = gx - 1, ly = gy - 1, x = x0 + lx, y = y0 + ly;
        const bool in = x >= 0 && x < f.W && y >= 0 && y < f.H;
        const size_t idx = in ? (size_t)y * f.W + x : 0;
        const NdPix q = nd_staged<2>(f, sZ, x0, y0, lx, ly);      // (!ok outside the image: the border test)
        float g0 = gin[idx], g1 = gin[plane + idx], g2 = gin[2 * plane + idx];
        bool on = q.ok;
        if (LOSS) {
            const float w = weight ? weight[idx] : 1.f;
            on = on && w != 0.f;
            const float ws = -(w * s);
            g0 *= ws; g1 *= ws; g2 *= ws;
            if (dnormals && in && lx >= 0 && lx < kTW && ly >= 0 && ly < kTH) {
                dnormals[idx] = on ? ws * q.n[0] : 0.f; dnormals[plane + idx] = on ? ws * q.n[1] : 0.f;
                dnormals[2 * plane + idx] = on ? ws * q.n[2] : 0.f;
            }
        }
        const float4 h = nd_backward(f, q, g0, g1, g2);
        sG[t] = on ? h : make_float4(0.f, 0.f, 0.f, 0.f);      // (selects: an invalid pixel hands on exact zeros, whatever it holds)
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, x = x0 + lx;
#pragma unroll
    for (int k = 0; k < kTH / 4; ++k) {
        const int ly = 4 * k + wave, y = y0 + ly;
        if (x >= f.W || y >= f.H) continue;
        const float4* c = sG + (ly + 1) * GW + lx + 1;
        // z(x, y) is the LEFT depth of (x + 1, y), the right depth of (x - 1, y), the upper depth of (x, y + 1), the lower depth of (x, y - 1)
        ddepth[(size_t)y * f.W + x] = (c[1].x + c[-1].y) + (c[GW].z + c[-GW].w);
    }
}

}  // namespace

void gsr_normals_frame(int H, int W, float tanfovx, float tanfovy, GsrNormalsFrame* out) {
    GsrNormalsFrame f;
    f.H = H; f.W = W;
    f.tiles_x = (W + kTW - 1) / kTW;
    f.tiles_y = (H + kTH - 1) / kTH;
    f.tx = tanfovx; f.ty = tanfovy;
    f.inv_w = (float)(1.0 / (double)W);
    f.inv_h = (float)(1.0 / (double)H);
    f.alpha = (float)(2.0 * (double)tanfovy / (double)H);
    f.beta = (float)(2.0 * (double)tanfovx / (double)W);
    f.ab = (float)((2.0 * (double)tanfovy / (double)H) * (2.0 * (double)tanfovx / (double)W));
    f.inv_hw = (float)(1.0 / ((double)H * (double)W));
    *out = f;
}

void gsr_launch_gaussian_normals(int P, const float* scales, const float* rot, const float* means, const float* vm, float* out, hipStream_t st) {
    hipLaunchKernelGGL(gaussian_normals_kernel, dim3((unsigned)(((int64_t)P + 255) / 256)), dim3(256), 0, st, P, scales, rot, means, vm, out);
}

void gsr_launch_gaussian_normals_backward(int P, const float* scales, const float* rot, const float* means, const float* vm, const float* dn,
                                          float* drot, hipStream_t st) {
    hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3((unsigned)(((int64_t)P + 255) / 256)), dim3(256), 0, st, P, scales, rot, means, vm, dn,
                       drot);
}

void gsr_launch_depth_normals(const GsrNormalsFrame& f, const float* depth, float* out, hipStream_t st) {
    hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)gsr_normals_tiles(f)), dim3(256), 0, st, f, depth, out);
}

void gsr_launch_depth_normals_backward(const GsrNormalsFrame& f, const float* depth, const float* dL_dnormals, float* dL_ddepth, hipStream_t st) {
    hipLaunchKernelGGL((depth_normals_bwd_kernel<false>), dim3((unsigned)gsr_normals_tiles(f)), dim3(256), 0, st, f, depth, dL_dnormals,
                       (const float*)nullptr, (const float*)nullptr, (float*)nullptr, dL_ddepth);
}

void gsr_launch_normal_loss(const GsrNormalsFrame& f, const float* depth, const float* normals, const float* weight, double* partials,
                            float* loss_out, hipStream_t st) {
    const int nb = gsr_normals_tiles(f);
    hipLaunchKernelGGL(normal_loss_kernel, dim3((unsigned)nb), dim3(256), 0, st, f, depth, normals, weight, partials);
    hipLaunchKernelGGL(normal_loss_sum_kernel, dim3(1), dim3(256), 0, st, nb, (double)f.H * (double)f.W, (const double*)partials, loss_out);
}

void gsr_launch_normal_loss_backward(const GsrNormalsFrame& f, const float* depth, const float* normals, const float* weight,
                                     const float* dL_dloss, float* dL_dnormals, float* dL_ddepth, hipStream_t st) {
    const dim3 g((unsigned)gsr_normals_tiles(f)), b(256);
    if (dL_ddepth) hipLaunchKernelGGL((depth_normals_bwd_kernel<true>), g, b, 0, st, f, depth, normals, weight, dL_dloss, dL_dnormals, dL_ddepth);
    else if (dL_dnormals) hipLaunchKernelGGL(normal_loss_bwd_normals_kernel, g, b, 0, st, f, depth, weight, dL_dloss, dL_dnormals);
}
