// Fused SSIM map forward / backward -- "next row" N1 of SURVEY.md 8(f): the loss on the far side of the rasterizer in
// every training iteration (train.py:119-126).  The reference either calls the un-vendored `fused_ssim` CUDA extension
// (train.py:31-35,122) or falls back to utils/loss_utils.py:56-87: five grouped 11x11 conv2d over the 1080p frame plus
// their autograd backward, which measured 10.7 ms per step on MI355X (MIOpen) against 2 ms for everything else in the
// step.  Here: one kernel per direction, the separable 11-tap Gaussian window (sigma 1.5) applied inside LDS.
//
//   forward : per 64x16 output tile, the 74x26 halo of img1 / img2 is staged in LDS (zero outside the image = conv2d's
//             zero padding 5); a horizontal pass produces the 5 windowed moments (x, y, x^2, y^2, xy) for the 26 halo
//             rows -- one thread per 8 adjacent outputs, every input read once and spread over the outputs it feeds from
//             registers -- a vertical pass finishes them, four vertically adjacent pixels per thread; the SSIM value and
//             the three partial derivatives dm/dmu1, dm/dE[x^2], dm/dE[xy] (statistics held, as in the published
//             fused-ssim scheme) are written with row-contiguous 256-byte stores.
//   backward: dL/dimg1 = G * (dL/dm dm/dmu1) + 2 img1 (G * (dL/dm dm/dE[x^2])) + img2 (G * (dL/dm dm/dE[xy])), the same
//             separable window applied to three maps.
// Measured (3 x 1080 x 1920, MI355X): 82 us forward + 62 us backward -- THE SAME as round 1's 16x16-tile, one-output-per-thread
// version (2.6x halo, 91 LDS reads per pixel) although this form reads LDS 14 (horizontal) + 17.5 (vertical) times per pixel
// and stages a 1.9x halo: the kernel is not LDS- or HBM-bound (0.125 GB per direction = 1.5 TB/s) but sits on the FMA floor
// of the separable window -- 5 moments x 11 taps x 2 passes x 1.6 (halo rows) = 144 FMA per pixel = ~41 us of VALU issue
// even with v_pk_fma_f32 -- plus the load -> barrier -> horizontal -> barrier -> vertical phases of only three resident
// workgroups per CU (50 KB of LDS each).  A barrier-free "marching" form (one wave per column strip, 11-row ring of the
// horizontal moments in registers) was costed and dropped: at 1080p it has either < 3 waves per SIMD or > 30 % halo rows.
#include "gsr_internal.h"
#include <algorithm>
#include <type_traits>

namespace {

constexpr int TXO = 64, TYO = 16;      // output tile (x, y)
constexpr int HALO = 5;
constexpr int HX = TXO + 2 * HALO;     // 74 staged columns
constexpr int HY = TYO + 2 * HALO;     // 26 staged rows
// LDS row strides (floats), both ODD: in the horizontal pass a wave is 8 rows x 8 tasks whose addresses are
// r * stride + 8 t + j -- with an odd stride the eight rows start in eight different residues mod 8, so the 64 lanes hit 64
// different banks; the vertical pass reads 64 consecutive columns of one row.
constexpr int SW = 77;                 // staged halo rows
constexpr int SHW = 65;                // horizontally filtered rows
constexpr int HTASKS = HY * (TXO / 8); // 208 horizontal tasks of 8 outputs
// Halo staging: thread t stages elements t, t + 256, ... of the HY x HX halo.  Written as the obvious loop
// "s[r][c] = inside ? p[..] : 0" the compiler emits load -> s_waitcnt vmcnt(0) -> LDS write per element: 15 serial memory
// round trips per workgroup in the forward kernel.  So: NSTAGE unrolled, unconditional loads (address 0 when outside the
// image) into registers first, then unconditional LDS writes -- the last iteration's surplus threads write into
// STAGE_PAD spare rows nobody reads (a conditional write makes the compiler sink the load back into the branch).
constexpr int NSTAGE = (HY * HX + 255) / 256;                       // 8
constexpr int STAGE_PAD = (NSTAGE * 256 + HX - 1) / HX - HY;        // 2 spare rows
constexpr float C1 = 0.01f * 0.01f;
constexpr float C2 = 0.03f * 0.03f;

// normalised 11-tap Gaussian, sigma = 1.5 (utils/loss_utils.py:43-46), each tap the fp32 nearest to its fp64 value: the eleven sum to
// 1 - 1.4e-9.  (Until the loss tests on smooth content, taps 4 / 6 were one ulp low -- 2.1300552785e-01 -- and the window summed to 1 - 3.1e-8:
// sigma^2 = E[x^2] - mu^2 of a flat patch of level c came out as +6.2e-8 c^2 instead of 0, which next to C2 = 9e-4 biased the mean SSIM of
// smooth images by 3e-6 .. 6e-6, ten times the fp32 formula's own error.)
#define GSR_WIN(k)                                                                                                        \
    ((k) == 0 || (k) == 10 ? 1.0283801239e-03f : (k) == 1 || (k) == 9 ? 7.5987582095e-03f                                \
     : (k) == 2 || (k) == 8 ? 3.6000773311e-02f : (k) == 3 || (k) == 7 ? 1.0936068743e-01f                                \
     : (k) == 4 || (k) == 6 ? 2.1300554276e-01f : 2.6601171494e-01f)

// MEAN: instead of the SSIM map the workgroup writes the SUM of its tile's SSIM values (partials[plane][tile]); a second
// one-workgroup kernel adds the partials in fixed order -> mean (deterministic, no 25 MB map round trip, no torch reduce)
// XCD-aware tile order (round 3, VERDICT r02 weak #7: the 5-pixel halo of a 64x16 tile is 1.88x its pixels, and with the default
// x-fastest workgroup order the neighbours of a tile run on OTHER XCDs -- workgroup b goes to XCD b % 8 -- so every halo was
// fetched from HBM / Infinity Cache again: FETCH+WRITE 1.6-1.8x the algorithmic bytes).  The launch is 1-D; XCD k gets the k-th
// contiguous eighth of the (plane, tile row, tile column) order, so a tile's left / right neighbours and the rows above / below
// share its L2.  Results do not depend on the order (per-tile partial sums are indexed by tile and added in index order).
__device__ __forceinline__ bool ssim_tile_of_block(int ntx, int nty, int planes, int& tx, int& ty, int& plane, int64_t& tlin) {
    const int64_t ntiles = (int64_t)ntx * nty * planes;
    const int64_t per = (ntiles + 7) / 8;
    const int64_t b = blockIdx.x;
    tlin = (b & 7) * per + (b >> 3);
    if ((b >> 3) >= per || tlin >= ntiles) return false;
    tx = (int)(tlin % ntx);
    const int64_t r = tlin / ntx;
    ty = (int)(r % nty);
    plane = (int)(r / nty);
    return true;
}

// MODE 0: SSIM map.  MODE 1 (MEAN): per-tile partial sums instead of the map.  MODE 2 (round 3, the training loss of
// train.py:119-126 in one pass): as MODE 1, and the tile's sum of |img1 - img2| (the L1 term, utils/loss_utils.py:40-41) goes to
// partials[n_tiles + tile] -- the pixels are already in LDS, so the L1 half of the loss costs no extra read of either image.
template <int MODE>
__global__ void __launch_bounds__(256)
ssim_fwd_kernel(int H, int W, int planes, const float* __restrict__ img1, const float* __restrict__ img2, float* __restrict__ ssim_map,
                float* __restrict__ dm_dmu1, float* __restrict__ dm_dex2, float* __restrict__ dm_dexy) {
    constexpr bool MEAN = MODE != 0;
    __shared__ float s_part[8];
    __shared__ float s_x[HY + STAGE_PAD][SW];
    __shared__ float s_y[HY + STAGE_PAD][SW];
    __shared__ float s_h[5][HY][SHW];
    const int tid = threadIdx.x;
    const int ntx = (W + TXO - 1) / TXO, nty = (H + TYO - 1) / TYO;
    int txi, tyi, plane;                                // plane = b * C + c
    int64_t tlin;
    if (!ssim_tile_of_block(ntx, nty, planes, txi, tyi, plane, tlin)) return;
    const int x0 = txi * TXO, y0 = tyi * TYO;
    const float* p1 = img1 + (int64_t)plane * H * W;
    const float* p2 = img2 + (int64_t)plane * H * W;
    {   // halo staging: ALL loads are issued before the first LDS write, branch-free (see NSTAGE)
        float vx[NSTAGE], vy[NSTAGE];
#pragma unroll
        for (int k = 0; k < NSTAGE; ++k) {
            const int i = tid + k * 256;
            const int r = i / HX, c = i - r * HX;
            const int gy = y0 + r - HALO, gx = x0 + c - HALO;
            const bool in = i < HY * HX && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int64_t o = in ? (int64_t)gy * W + gx : 0;
            const float a = p1[o], b = p2[o];
            vx[k] = in ? a : 0.f;
            vy[k] = in ? b : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NSTAGE; ++k) {
            const int i = tid + k * 256;
            const int r = i / HX, c = i - r * HX;
            s_x[r][c] = vx[k];
            s_y[r][c] = vy[k];
        }
    }
    __syncthreads();
    if (tid < HTASKS) {                                 // horizontal pass: row r, outputs c0 .. c0+7
        const int r = tid >> 3, c0 = (tid & 7) * 8;
        float acc[8][5];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[i][m] = 0.f;
#pragma unroll
        for (int j = 0; j < 18; ++j) {                  // input column c0 + j feeds output i with tap j - i
            const float x = s_x[r][c0 + j], y = s_y[r][c0 + j];
            const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = j - i;
                if (k >= 0 && k <= 10) {
                    const float w = GSR_WIN(k);
                    acc[i][0] = fmaf(w, x, acc[i][0]); acc[i][1] = fmaf(w, y, acc[i][1]); acc[i][2] = fmaf(w, xx, acc[i][2]);
                    acc[i][3] = fmaf(w, yy, acc[i][3]); acc[i][4] = fmaf(w, xy, acc[i][4]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int m = 0; m < 5; ++m) s_h[m][r][c0 + i] = acc[i][m];
    }
    __syncthreads();
    const int cx = tid & 63, rg = tid >> 6;             // vertical pass: column cx, rows 4 rg .. 4 rg + 3
    float acc[4][5];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] = 0.f;
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        float v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) v[m] = s_h[m][4 * rg + j][cx];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;
            if (k >= 0 && k <= 10) {
                const float w = GSR_WIN(k);
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[o][m] = fmaf(w, v[m], acc[o][m]);
            }
        }
    }
    const int gx = x0 + cx;
    float m_own = 0.f, l1_own = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + 4 * rg + o;
        if (gy < H && gx < W) {
            if (MODE == 2) l1_own += fabsf(s_x[4 * rg + o + HALO][cx + HALO] - s_y[4 * rg + o + HALO][cx + HALO]);
            const float mu1 = acc[o][0], mu2 = acc[o][1], ex2 = acc[o][2], ey2 = acc[o][3], exy = acc[o][4];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float sigma1_sq = fmaf(-mu1, mu1, ex2), sigma2_sq = fmaf(-mu2, mu2, ey2), sigma12 = fmaf(-mu2, mu1, exy);
            const float A = mu1_sq + mu2_sq + C1, B = sigma1_sq + sigma2_sq + C2;
            const float Cc = 2.f * mu12 + C1, D = 2.f * sigma12 + C2;
            const float inv_AB = 1.f / (A * B);
            const float m = Cc * D * inv_AB;
            const int64_t oo = (int64_t)plane * H * W + (int64_t)gy * W + gx;
            m_own += m;
            if (!MEAN) ssim_map[oo] = m;
            if (dm_dmu1) {
                dm_dmu1[oo] = 2.f * mu2 * (D - Cc) * inv_AB - 2.f * mu1 * m / A + 2.f * mu1 * m / B;
                dm_dex2[oo] = -m / B;
                dm_dexy[oo] = 2.f * Cc * inv_AB;
            }
        }
    }
    if (MEAN) {
        float v = m_own, u = l1_own;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v += __shfl_xor(v, off, 64);
            if (MODE == 2) u += __shfl_xor(u, off, 64);
        }
        if ((tid & 63) == 0) { s_part[tid >> 6] = v; s_part[4 + (tid >> 6)] = u; }
        __syncthreads();
        if (tid == 0) {
            ssim_map[tlin] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
            if (MODE == 2) ssim_map[(int64_t)planes * nty * ntx + tlin] = (s_part[4] + s_part[5]) + (s_part[6] + s_part[7]);
        }
    }
}

// one workgroup: out = [loss, L1, SSIM] with loss = (1 - lambda) L1 + lambda (1 - SSIM) (train.py:123), sums in fixed order
__global__ void __launch_bounds__(256)
loss_mean_kernel(const float* __restrict__ partials, int n, float inv_count, float lambda, float* __restrict__ out) {
    __shared__ float s_part[8];
    const int tid = threadIdx.x;
    float v = 0.f, u = 0.f;
    int i = tid;
    for (; i + 3 * 256 < n; i += 4 * 256) {          // coalesced, eight independent loads in flight per trip (see ssim_mean_kernel)
        float a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = partials[i + k * 256]; b[k] = partials[n + i + k * 256]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { v += a[k]; u += b[k]; }
    }
    for (; i < n; i += 256) { v += partials[i]; u += partials[n + i]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { v += __shfl_xor(v, off, 64); u += __shfl_xor(u, off, 64); }
    if ((tid & 63) == 0) { s_part[tid >> 6] = v; s_part[4 + (tid >> 6)] = u; }
    __syncthreads();
    if (tid == 0) {
        const float ssim = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) * inv_count;
        const float l1 = ((s_part[4] + s_part[5]) + (s_part[6] + s_part[7])) * inv_count;
        out[0] = (1.0f - lambda) * l1 + lambda * (1.0f - ssim);
        out[1] = l1;
        out[2] = ssim;
    }
}

// one workgroup: mean = (sum of the per-tile partial sums, fixed order) / count
__global__ void __launch_bounds__(256)
ssim_mean_kernel(const float* __restrict__ partials, int n, float inv_count, float* __restrict__ mean_out) {
    __shared__ float s_part[4];
    const int tid = threadIdx.x;
    // thread t adds elements t, t + 256, ... (coalesced; eight independent loads in flight per trip: the chunk-per-thread form
    // was a chain of dependent trips, 6-9 us for 6 000 partials); any FIXED order is deterministic
    float v = 0.f;
    int i = tid;
    for (; i + 7 * 256 < n; i += 8 * 256) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = partials[i + k * 256];
#pragma unroll
        for (int k = 0; k < 8; ++k) v += t[k];
    }
    for (; i < n; i += 256) v += partials[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) mean_out[0] = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) * inv_count;
}

// MEAN: dL/dmap is the same for every pixel, dL/dmean / count, read from one device scalar
// MODE 2: dL/dmap[0] is dL/dloss of the fused training loss: the SSIM maps are weighted with -lambda dL/dloss / count and
// (1 - lambda) dL/dloss / count * sign(img1 - img2) -- the L1 term's gradient -- is added in the same store.
template <int MODE>
__global__ void __launch_bounds__(256)
ssim_bwd_kernel(int H, int W, int planes, const float* __restrict__ img1, const float* __restrict__ img2,
                const float* __restrict__ dL_dmap, float inv_count, float lambda, const float* __restrict__ dm_dmu1,
                const float* __restrict__ dm_dex2, const float* __restrict__ dm_dexy, float* __restrict__ dL_dimg1) {
    constexpr bool MEAN = MODE != 0;
    __shared__ float s_in[3][HY + STAGE_PAD][SW];
    __shared__ float s_h[3][HY][SHW];
    const int tid = threadIdx.x;
    const int ntx = (W + TXO - 1) / TXO, nty = (H + TYO - 1) / TYO;
    int txi, tyi, plane;
    int64_t tlin;
    if (!ssim_tile_of_block(ntx, nty, planes, txi, tyi, plane, tlin)) return;
    const int x0 = txi * TXO, y0 = tyi * TYO;
    const int64_t pbase = (int64_t)plane * H * W;
    const float gmean = MODE == 2 ? -lambda * dL_dmap[0] * inv_count : (MEAN ? dL_dmap[0] * inv_count : 0.f);
    const float gl1 = MODE == 2 ? (1.0f - lambda) * dL_dmap[0] * inv_count : 0.f;
    // the two images are only needed by the last expression: requested first, they arrive during the two passes
    const int cx = tid & 63, rg = tid >> 6;
    const int gx_out = x0 + cx;
    float im1[4], im2[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + 4 * rg + o;
        const int64_t oo = (gy < H && gx_out < W) ? pbase + (int64_t)gy * W + gx_out : pbase;
        im1[o] = img1[oo];
        im2[o] = img2[oo];
    }
    {   // halo staging, all loads before the first LDS write (see NSTAGE)
        float v0[NSTAGE], v1[NSTAGE], v2[NSTAGE];
#pragma unroll
        for (int k = 0; k < NSTAGE; ++k) {
            const int i = tid + k * 256;
            const int r = i / HX, c = i - r * HX;
            const int gy = y0 + r - HALO, gx = x0 + c - HALO;
            const bool in = i < HY * HX && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int64_t o = in ? pbase + (int64_t)gy * W + gx : pbase;
            const float g = MEAN ? gmean : dL_dmap[o];
            const float a = dm_dmu1[o], b = dm_dex2[o], c2 = dm_dexy[o];
            v0[k] = in ? g * a : 0.f;
            v1[k] = in ? g * b : 0.f;
            v2[k] = in ? g * c2 : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NSTAGE; ++k) {
            const int i = tid + k * 256;
            const int r = i / HX, c = i - r * HX;
            s_in[0][r][c] = v0[k];
            s_in[1][r][c] = v1[k];
            s_in[2][r][c] = v2[k];
        }
    }
    __syncthreads();
    if (tid < HTASKS) {
        const int r = tid >> 3, c0 = (tid & 7) * 8;
        float acc[8][3];
#pragma unroll
        for (int i = 0; i < 8; ++i) { acc[i][0] = 0.f; acc[i][1] = 0.f; acc[i][2] = 0.f; }
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            const float a = s_in[0][r][c0 + j], b = s_in[1][r][c0 + j], c = s_in[2][r][c0 + j];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = j - i;
                if (k >= 0 && k <= 10) {
                    const float w = GSR_WIN(k);
                    acc[i][0] = fmaf(w, a, acc[i][0]); acc[i][1] = fmaf(w, b, acc[i][1]); acc[i][2] = fmaf(w, c, acc[i][2]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) { s_h[0][r][c0 + i] = acc[i][0]; s_h[1][r][c0 + i] = acc[i][1]; s_h[2][r][c0 + i] = acc[i][2]; }
    }
    __syncthreads();
    float acc[4][3];
#pragma unroll
    for (int o = 0; o < 4; ++o) { acc[o][0] = 0.f; acc[o][1] = 0.f; acc[o][2] = 0.f; }
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        const float a = s_h[0][4 * rg + j][cx], b = s_h[1][4 * rg + j][cx], c = s_h[2][4 * rg + j][cx];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;
            if (k >= 0 && k <= 10) {
                const float w = GSR_WIN(k);
                acc[o][0] = fmaf(w, a, acc[o][0]); acc[o][1] = fmaf(w, b, acc[o][1]); acc[o][2] = fmaf(w, c, acc[o][2]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + 4 * rg + o;
        if (gy < H && gx_out < W) {
            const int64_t oo = pbase + (int64_t)gy * W + gx_out;
            float v = acc[o][0] + 2.f * im1[o] * acc[o][1] + im2[o] * acc[o][2];
            if (MODE == 2) { const float d = im1[o] - im2[o]; v += d > 0.f ? gl1 : (d < 0.f ? -gl1 : 0.f); }      // torch's sign(0) = 0
            dL_dimg1[oo] = v;
        }
    }
}

// ================================================================================================
// Round 3, second form: MARCHING waves (the default).  The tiled kernels above stay as A/B variant 1 (`ssim_variant`).
//
// The tiled form is neither HBM- nor FMA-bound: it is a sequence of phases (global -> LDS, barrier, horizontal, barrier, vertical)
// with three resident workgroups per CU (50 KB of LDS each) and nothing to overlap them with: 78 us forward + 58 us backward for
// 25 MB planes, against ~15 us of FMA issue.  Here a wave owns a strip of 64 image columns and walks DOWN it, one image row per
// step, with no LDS and no barrier:
//   * lane = column.  The horizontal 11-tap window needs the five neighbours on either side: x and y (not the five moments)
//     travel across the lanes with `v_mov_b32_dpp wave_shr:1 / wave_shl:1` chains -- plain VALU moves, gfx9's whole-wave DPP
//     shifts -- and the three products are formed per tap; symmetric taps are paired (w (a + b), w (a a + b b)).  The outer five
//     lanes on either side only feed their neighbours: 54 outputs per 64 lanes.
//   * the vertical window is a SYSTOLIC register pipeline: eleven partial outputs per moment, and a new horizontally filtered
//     row h updates them as A[j] = fma(w[j], h, A[j + 1]) -- the shift of the pipeline is the choice of the destination
//     register, no moves, no unrolling by eleven; A[0] is complete five rows behind the row just read.
//   * rows are requested MPF steps ahead into a register ring; the zero padding is applied when a row is CONSUMED (a select next
//     to the load would pin the wait there).
// A strip is cut into segments of `seg` rows (ten extra rows per segment) so that ~3-4 waves sit on every SIMD.
// ================================================================================================
constexpr int MW = 54;            // output columns per wave
constexpr int MPF = 5;            // rows in flight
constexpr int MWARM = 10;         // warm-up rows (= 2 * HALO, a multiple of MPF): the pipeline fills, nothing is written
constexpr uint32_t OOB = 0x80000000u;      // a buffer offset beyond every plane: loads return 0, stores are dropped

__device__ __forceinline__ float wave_shr1(float v) {       // lane i <- lane i - 1 (lane 0 <- 0)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_shl1(float v) {       // lane i <- lane i + 1 (lane 63 <- 0)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}
// Raw buffer access (stride 0, range-checked by the hardware): every plane is its own buffer of H * W * 4 bytes, so the
// conv2d zero padding is an out-of-range LOAD and a lane / row without an output is an out-of-range STORE.  No select next to
// a load, no exec-masked store block, no branch in the row loop: the loop body is straight-line code, which is what lets the
// compiler count the memory operations in flight.  (With `if (valid) store` the waitcnt pass had to assume the worst at every
// join and drained the queue -- s_waitcnt vmcnt(0) -- once per four rows: the prefetch ring was one row deep in effect.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_buffer(const float* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float buf_load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}
__device__ __forceinline__ void buf_store(__amdgpu_buffer_rsrc_t r, uint32_t off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(v), r, (int)off, 0, 0);
}

template <int MODE, bool DERIV>
__global__ void __launch_bounds__(64)
ssim_fwd_march(int H, int W, int planes, int nsx, int nsy, int seg, const float* __restrict__ img1, const float* __restrict__ img2,
               float* __restrict__ ssim_map, float* __restrict__ dm_dmu1, float* __restrict__ dm_dex2, float* __restrict__ dm_dexy) {
    constexpr bool MEAN = MODE != 0;
    const int lane = threadIdx.x;
    int sx, sy, plane;
    int64_t tlin;
    if (!ssim_tile_of_block(nsx, nsy, planes, sx, sy, plane, tlin)) return;
    const int col = sx * MW - HALO + lane;              // this lane's image column (input AND output)
    const bool col_ok = col >= 0 && col < W;
    const bool col_out = lane >= HALO && lane < HALO + MW && col < W;
    const int y0 = sy * seg, y1 = min(y0 + seg, H);      // output rows [y0, y1)
    const int r_last = min(y1 + HALO, H);                // input rows beyond it are never needed
    const int64_t pbase = (int64_t)plane * H * W;
    const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
    const __amdgpu_buffer_rsrc_t b1 = plane_buffer(img1 + pbase, pbytes), b2 = plane_buffer(img2 + pbase, pbytes);
    const __amdgpu_buffer_rsrc_t bm = plane_buffer(MEAN ? img1 : ssim_map + pbase, MEAN ? 0u : pbytes);
    const __amdgpu_buffer_rsrc_t d1 = plane_buffer(DERIV ? dm_dmu1 + pbase : img1, DERIV ? pbytes : 0u);
    const __amdgpu_buffer_rsrc_t d2 = plane_buffer(DERIV ? dm_dex2 + pbase : img1, DERIV ? pbytes : 0u);
    const __amdgpu_buffer_rsrc_t d3 = plane_buffer(DERIV ? dm_dexy + pbase : img1, DERIV ? pbytes : 0u);
    const uint32_t col4 = (uint32_t)col * 4u, row4 = (uint32_t)W * 4u;
    float rx[MPF], ry[MPF];
    float A[5][11];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int j = 0; j < 11; ++j) A[m][j] = 0.f;
    float m_own = 0.f, l1_own = 0.f;
    auto request = [&](int rr, int k) {
        const uint32_t off = (col_ok && rr >= 0 && rr < r_last) ? (uint32_t)rr * row4 + col4 : OOB;
        rx[k] = buf_load(b1, off);
        ry[k] = buf_load(b2, off);
    };
    // one image row; ONE loop with one body, the MWARM rows that only fill the pipeline included (their output offset is out
    // of range) -- see the backward kernel for what a separate warm-up loop did to the waits
    auto step = [&](int r, int k) {
        const float x = rx[k], y = ry[k];
        if (MODE == 2) l1_own += (col_out && r >= y0 && r < y1) ? fabsf(x - y) : 0.f;
        // ---- horizontal: x, y of the five lanes on either side ----
        float xm[6], xp[6], ym[6], yp[6];
        xm[0] = x; xp[0] = x; ym[0] = y; yp[0] = y;
#pragma unroll
        for (int d = 1; d <= 5; ++d) {
            xm[d] = wave_shr1(xm[d - 1]); xp[d] = wave_shl1(xp[d - 1]);
            ym[d] = wave_shr1(ym[d - 1]); yp[d] = wave_shl1(yp[d - 1]);
        }
        float h[5];
        {   const float w = GSR_WIN(5);
            h[0] = w * x; h[1] = w * y; h[2] = w * (x * x); h[3] = w * (y * y); h[4] = w * (x * y);
        }
#pragma unroll
        for (int d = 1; d <= 5; ++d) {
            const float w = GSR_WIN(5 - d);
            const float a = xm[d], b = xp[d], c = ym[d], e = yp[d];
            h[0] = fmaf(w, a + b, h[0]);
            h[1] = fmaf(w, c + e, h[1]);
            h[2] = fmaf(w, fmaf(b, b, a * a), h[2]);
            h[3] = fmaf(w, fmaf(e, e, c * c), h[3]);
            h[4] = fmaf(w, fmaf(b, e, a * c), h[4]);
        }
        // the slot's registers are free now: request the row MPF steps ahead INTO THEM.  The fences keep the scheduler from
        // hoisting the loads above the last use of the old values -- it then needs a fifth set of registers and rotates the
        // ring with v_mov at the loop latch, and moves of loaded registers are waits (s_waitcnt vmcnt(1..5) every trip)
        __builtin_amdgcn_sched_barrier(0);
        request(r + MPF, k);
        __builtin_amdgcn_sched_barrier(0);
        // ---- vertical: the systolic pipeline; A[.][0] is now complete for output row r - 5 ----
#pragma unroll
        for (int m = 0; m < 5; ++m) {
#pragma unroll
            for (int j = 0; j < 10; ++j) A[m][j] = fmaf(GSR_WIN(j), h[m], A[m][j + 1]);
            A[m][10] = GSR_WIN(10) * h[m];
        }
        {
            const int o = r - HALO;
            const bool valid = col_out && o >= y0 && o < y1;
            const uint32_t off = valid ? (uint32_t)o * row4 + col4 : OOB;
            const float mu1 = A[0][0], mu2 = A[1][0], ex2 = A[2][0], ey2 = A[3][0], exy = A[4][0];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float sigma1_sq = fmaf(-mu1, mu1, ex2), sigma2_sq = fmaf(-mu2, mu2, ey2), sigma12 = fmaf(-mu2, mu1, exy);
            // (the three fmaf: the cancellation with ONE rounding.  hipcc contracts `ex2 - mu1 * mu1` to this v_fma_f32 anyway -- the gfx950 code is
            //  unchanged -- but a build without contraction, as the host build of the tests, rounded mu^2 first: 1.6x the error of the mean SSIM on edges)
            const float Aa = mu1_sq + mu2_sq + C1, B = sigma1_sq + sigma2_sq + C2;
            const float Cc = 2.f * mu12 + C1, D = 2.f * sigma12 + C2;
            const float inv_A = __builtin_amdgcn_rcpf(Aa), inv_B = __builtin_amdgcn_rcpf(B);
            const float inv_AB = inv_A * inv_B;
            const float mv = Cc * D * inv_AB;
            m_own += valid ? mv : 0.f;
            if (!MEAN) buf_store(bm, off, mv);
            if (DERIV) {
                buf_store(d1, off, 2.f * mu2 * (D - Cc) * inv_AB + 2.f * mu1 * mv * (inv_B - inv_A));
                buf_store(d2, off, -mv * inv_B);
                buf_store(d3, off, 2.f * Cc * inv_AB);
            }
        }
        __builtin_amdgcn_sched_barrier(0);          // (keeps the four unrolled steps apart: without stores the scheduler
                                                    //  batches their formulas and holds all four rows' moments in registers)
    };
    int r = y0 + HALO - MWARM;
#pragma unroll
    for (int k = 0; k < MPF; ++k) request(r + k, k);
    const int r_end = y1 + HALO;                         // (rows past it are padding of the last group: no output, no load)
#pragma unroll 1
    for (; r < r_end; r += MPF) {
#pragma unroll
        for (int k = 0; k < MPF; ++k) step(r + k, k);
    }
    if (MEAN) {
        float v = m_own, u = l1_own;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v += __shfl_xor(v, off, 64);
            if (MODE == 2) u += __shfl_xor(u, off, 64);
        }
        if (lane == 0) {
            ssim_map[tlin] = v;
            if (MODE == 2) ssim_map[(int64_t)planes * nsy * nsx + tlin] = u;
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(64)
ssim_bwd_march(int H, int W, int planes, int nsx, int nsy, int seg, const float* __restrict__ img1, const float* __restrict__ img2,
               const float* __restrict__ dL_dmap, float inv_count, float lambda, const float* __restrict__ dm_dmu1,
               const float* __restrict__ dm_dex2, const float* __restrict__ dm_dexy, float* __restrict__ dL_dimg1) {
    constexpr bool MEAN = MODE != 0;
    const int lane = threadIdx.x;
    int sx, sy, plane;
    int64_t tlin;
    if (!ssim_tile_of_block(nsx, nsy, planes, sx, sy, plane, tlin)) return;
    const int col = sx * MW - HALO + lane;
    const bool col_ok = col >= 0 && col < W;
    const bool col_out = lane >= HALO && lane < HALO + MW && col < W;
    const int y0 = sy * seg, y1 = min(y0 + seg, H);
    const int r_last = min(y1 + HALO, H);
    const int64_t pbase = (int64_t)plane * H * W;
    const uint32_t pbytes = (uint32_t)H * (uint32_t)W * 4u;
    const __amdgpu_buffer_rsrc_t ba = plane_buffer(dm_dmu1 + pbase, pbytes), bb = plane_buffer(dm_dex2 + pbase, pbytes);
    const __amdgpu_buffer_rsrc_t bc = plane_buffer(dm_dexy + pbase, pbytes);
    const __amdgpu_buffer_rsrc_t bg = plane_buffer(MEAN ? img1 : dL_dmap + pbase, MEAN ? 0u : pbytes);
    const __amdgpu_buffer_rsrc_t b1 = plane_buffer(img1 + pbase, pbytes), b2 = plane_buffer(img2 + pbase, pbytes);
    const __amdgpu_buffer_rsrc_t bo = plane_buffer(dL_dimg1 + pbase, pbytes);
    const uint32_t col4 = (uint32_t)col * 4u, row4 = (uint32_t)W * 4u;
    const float gmean = MODE == 2 ? -lambda * dL_dmap[0] * inv_count : (MEAN ? dL_dmap[0] * inv_count : 0.f);
    const float gl1 = MODE == 2 ? (1.0f - lambda) * dL_dmap[0] * inv_count : 0.f;
    // ring slot k: the three maps (and dL/dmap) of input row r, and the two images at the OUTPUT row r - 5 of the same step
    float ra[MPF], rb[MPF], rc[MPF], rg[MPF], ri1[MPF], ri2[MPF];
    auto request_maps = [&](int rr, int k) {
        const uint32_t off = (col_ok && rr >= 0 && rr < r_last) ? (uint32_t)rr * row4 + col4 : OOB;
        ra[k] = buf_load(ba, off);
        rb[k] = buf_load(bb, off);
        rc[k] = buf_load(bc, off);
        if (!MEAN) rg[k] = buf_load(bg, off);
    };
    auto request_images = [&](int rr, int k) {
        const int ro = rr - HALO;
        const uint32_t oo = (col_out && ro >= y0 && ro < y1) ? (uint32_t)ro * row4 + col4 : OOB;
        ri1[k] = buf_load(b1, oo);
        ri2[k] = buf_load(b2, oo);
    };
    float A[3][11];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int j = 0; j < 11; ++j) A[m][j] = 0.f;
    // ONE loop with one body, warm-up rows included (their output offset is out of range): with a separate warm-up loop the
    // compiler dropped the image loads there, re-issued them in a batch in front of the main loop, and the wait for them --
    // the youngest loads on the first trip -- became s_waitcnt vmcnt(5) on EVERY trip
    auto step = [&](int r, int k) {
        const float g = MEAN ? gmean : rg[k];
        const float v0 = g * ra[k], v1 = g * rb[k], v2 = g * rc[k];       // an out-of-range row / column loaded 0
        float am[6], ap[6], bmm[6], bp[6], cm[6], cp[6];
        am[0] = v0; ap[0] = v0; bmm[0] = v1; bp[0] = v1; cm[0] = v2; cp[0] = v2;
#pragma unroll
        for (int d = 1; d <= 5; ++d) {
            am[d] = wave_shr1(am[d - 1]); ap[d] = wave_shl1(ap[d - 1]);
            bmm[d] = wave_shr1(bmm[d - 1]); bp[d] = wave_shl1(bp[d - 1]);
            cm[d] = wave_shr1(cm[d - 1]); cp[d] = wave_shl1(cp[d - 1]);
        }
        float h[3];
        h[0] = GSR_WIN(5) * v0; h[1] = GSR_WIN(5) * v1; h[2] = GSR_WIN(5) * v2;
#pragma unroll
        for (int d = 1; d <= 5; ++d) {
            const float w = GSR_WIN(5 - d);
            h[0] = fmaf(w, am[d] + ap[d], h[0]);
            h[1] = fmaf(w, bmm[d] + bp[d], h[1]);
            h[2] = fmaf(w, cm[d] + cp[d], h[2]);
        }
        __builtin_amdgcn_sched_barrier(0);          // (see the forward kernel: loads go into registers that are dead by now)
        request_maps(r + MPF, k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
#pragma unroll
            for (int j = 0; j < 10; ++j) A[m][j] = fmaf(GSR_WIN(j), h[m], A[m][j + 1]);
            A[m][10] = GSR_WIN(10) * h[m];
        }
        {
            const float im1 = ri1[k], im2 = ri2[k];
            const int o = r - HALO;
            const uint32_t off = (col_out && o >= y0 && o < y1) ? (uint32_t)o * row4 + col4 : OOB;
            float v = A[0][0] + 2.f * im1 * A[1][0] + im2 * A[2][0];
            if (MODE == 2) { const float d = im1 - im2; v += d > 0.f ? gl1 : (d < 0.f ? -gl1 : 0.f); }      // torch's sign(0) = 0
            buf_store(bo, off, v);
        }
        __builtin_amdgcn_sched_barrier(0);
        request_images(r + MPF, k);
        __builtin_amdgcn_sched_barrier(0);
    };
    int r = y0 + HALO - MWARM;
#pragma unroll
    for (int k = 0; k < MPF; ++k) { request_maps(r + k, k); request_images(r + k, k); }
    const int r_end = y1 + HALO;
#pragma unroll 1
    for (; r < r_end; r += MPF) {
#pragma unroll
        for (int k = 0; k < MPF; ++k) step(r + k, k);
    }
}

int g_ssim_variant = 0;           // 0 = marching waves, 1 = LDS tiles (A/B)
// waves a launch of the marching form aims for (1024 SIMDs x waves per SIMD): [0] forward kernels, [1] backward kernels
constexpr int SSIM_TARGET_WAVES_FWD = 4096, SSIM_TARGET_WAVES_BWD = 2048;
int g_ssim_target_waves[2] = {SSIM_TARGET_WAVES_FWD, SSIM_TARGET_WAVES_BWD};

struct MarchPlan { int nsx, nsy, seg; unsigned lds; };
// Launch shape.  A launch has FEWER waves than the chip has slots for, and the dispatcher fills a CU to its limit before it
// moves on: 3 672 one-wave workgroups went to 184 CUs, five per SIMD, 72 CUs idle (SQ_BUSY_CYCLES 42 %, mean wave life 43 us of
// a 78 us kernel).  So every workgroup also asks for 160 KB / (workgroups per CU) of LDS it never touches: that caps a CU at
// the even share and the launch spreads over all 256.  Measured at 1080p (forward / backward, us) against the waves per CU,
// MPF = 4: 8 -> 52 / 35, 12 -> 71 / 45, 16 -> 55 / 38, 20 -> 57 / 40 -- the waves of one-wave workgroups reach the four SIMDs
// in pairs, so 12 per CU run as 4 + 4 + 2 + 2; workgroups of four waves were worse still (72 / 56).  With MPF = 5 (ten
// warm-up rows instead of twelve): 8 per CU 48.8 / 33.8, 16 per CU 50.5 / 34.6.  Two waves per SIMD do not saturate the VALU
// (a wave issues one instruction per ~5 cycles) but carry 10 halo rows per 57 instead of per 30.  Inside the training step,
// on the slower kind of box, two waves per SIMD leave the forward kernel waiting on memory: 77 us against 62 us with four (the
// backward 49 against 51), reproducibly on one box; on the faster kind the two shapes are within 2 us.  Forward 4096, backward 2048.
// 16 <= seg <= 128 rows.
MarchPlan march_plan(int planes, int H, int W, int bwd) {
    MarchPlan p;
    p.nsx = (W + MW - 1) / MW;
    const int64_t strips = (int64_t)planes * p.nsx;
    const int want = (int)std::max<int64_t>(1, g_ssim_target_waves[bwd ? 1 : 0] / strips);       // segments per strip
    int seg = (H + want - 1) / want;
    seg = std::min(std::max(seg, 16), 128);
    p.seg = seg;
    p.nsy = (H + seg - 1) / seg;
    const int64_t waves = strips * p.nsy;
    const int64_t per_cu = (waves + 255) / 256;
    p.lds = per_cu >= 20 ? 0u : (unsigned)(((160 * 1024) / per_cu) & ~(int64_t)511);
    if (p.lds > 64 * 1024) p.lds = 64 * 1024;                        // (the default dynamic-LDS limit; small images need no cap)
    return p;
}
dim3 march_grid(const MarchPlan& p, int planes) {
    const int64_t n = (int64_t)planes * p.nsx * p.nsy;
    return dim3((unsigned)(8 * ((n + 7) / 8)));
}

// tiled form, 1-D launch: 8 x ceil(tiles / 8) workgroups, see ssim_tile_of_block
dim3 ssim_grid(int planes, int H, int W) {
    const int64_t ntiles = (int64_t)planes * ((W + TXO - 1) / TXO) * ((H + TYO - 1) / TYO);
    return dim3((unsigned)(8 * ((ntiles + 7) / 8)));
}

}  // namespace

// the LDS-tiled form: on request (A/B), for planes beyond a 2 GB buffer descriptor, and for the mean forms without maps
static bool ssim_use_tiles(int H, int W, bool mean_without_maps) {
    return g_ssim_variant == 1 || (int64_t)H * W * 4 >= 0x7FFFFFFFll || mean_without_maps;
}

void gsr_set_ssim_variant(int v) { g_ssim_variant = v; }
// 0 restores the defaults (forward and backward differ, so no single value can); any other value goes into both slots
void gsr_set_ssim_target_waves(int v) {
    if (v == 0) { g_ssim_target_waves[0] = SSIM_TARGET_WAVES_FWD; g_ssim_target_waves[1] = SSIM_TARGET_WAVES_BWD; return; }
    g_ssim_target_waves[0] = g_ssim_target_waves[1] = std::max(v, 256);
}

/* the tiled form also serves the mean forms WITHOUT derivative maps (no-grad evaluation): with nothing to store per row the  \
   marching loop compiles to 170+ registers */                                                                                    \
#define GSR_SSIM_FWD(MODE_, OUT_)                                                                                                  \
    do {                                                                                                                           \
        if (ssim_use_tiles(H, W, MODE_ != 0 && !dm_dmu1)) {                                                                        \
            hipLaunchKernelGGL(ssim_fwd_kernel<MODE_>, ssim_grid(planes, H, W), dim3(256), 0, st, H, W, planes, img1, img2, OUT_,  \
                               dm_dmu1, dm_dex2, dm_dexy);                                                                         \
        } else {                                                                                                                   \
            const MarchPlan mp = march_plan(planes, H, W, 0);                                                                         \
            if (dm_dmu1)                                                                                                           \
                hipLaunchKernelGGL((ssim_fwd_march<MODE_, true>), march_grid(mp, planes), dim3(64), mp.lds, st, H, W, planes,      \
                                   mp.nsx, mp.nsy, mp.seg, img1, img2, OUT_, dm_dmu1, dm_dex2, dm_dexy);                           \
            else                                                                                                                   \
                hipLaunchKernelGGL((ssim_fwd_march<0, false>), march_grid(mp, planes), dim3(64), mp.lds, st, H, W, planes,         \
                                   mp.nsx, mp.nsy, mp.seg, img1, img2, OUT_, dm_dmu1, dm_dex2, dm_dexy);                           \
        }                                                                                                                          \
    } while (0)
#define GSR_SSIM_BWD(MODE_, G_, INV_, LAMBDA_)                                                                                     \
    do {                                                                                                                           \
        if (ssim_use_tiles(H, W, false)) {                                                                                         \
            hipLaunchKernelGGL(ssim_bwd_kernel<MODE_>, ssim_grid(planes, H, W), dim3(256), 0, st, H, W, planes, img1, img2, G_,    \
                               INV_, LAMBDA_, dm_dmu1, dm_dex2, dm_dexy, dL_dimg1);                                                \
        } else {                                                                                                                   \
            const MarchPlan mp = march_plan(planes, H, W, 1);                                                                         \
            hipLaunchKernelGGL(ssim_bwd_march<MODE_>, march_grid(mp, planes), dim3(64), mp.lds, st, H, W, planes, mp.nsx, mp.nsy,       \
                               mp.seg, img1, img2, G_, INV_, LAMBDA_, dm_dmu1, dm_dex2, dm_dexy, dL_dimg1);                        \
        }                                                                                                                          \
    } while (0)

// partial sums the forward that WILL run writes (per tile / per wave)
static int64_t ssim_partials_now(int planes, int H, int W, bool no_maps) {
    if (ssim_use_tiles(H, W, no_maps)) return (int64_t)planes * ((W + TXO - 1) / TXO) * ((H + TYO - 1) / TYO);
    const MarchPlan mp = march_plan(planes, H, W, 0);
    return (int64_t)planes * mp.nsx * mp.nsy;
}

void gsr_launch_ssim_forward(int planes, int H, int W, const float* img1, const float* img2, float* ssim_map, float* dm_dmu1,
                             float* dm_dex2, float* dm_dexy, hipStream_t st) {
    GSR_SSIM_FWD(0, ssim_map);
}

// callers size `partials` with this: enough for either variant
int64_t gsr_ssim_partial_count_impl(int planes, int H, int W) {
    const MarchPlan mp = march_plan(planes, H, W, 0);
    return std::max((int64_t)planes * ((W + TXO - 1) / TXO) * ((H + TYO - 1) / TYO), (int64_t)planes * mp.nsx * mp.nsy);
}

void gsr_launch_ssim_mean_forward(int planes, int H, int W, const float* img1, const float* img2, float* partials,
                                  float* mean_out, float* dm_dmu1, float* dm_dex2, float* dm_dexy, hipStream_t st) {
    GSR_SSIM_FWD(1, partials);
    const double count = (double)planes * H * W;
    hipLaunchKernelGGL(ssim_mean_kernel, dim3(1), dim3(256), 0, st, partials, (int)ssim_partials_now(planes, H, W, dm_dmu1 == nullptr),
                       (float)(1.0 / count), mean_out);
}

void gsr_launch_ssim_mean_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmean,
                                   const float* dm_dmu1, const float* dm_dex2, const float* dm_dexy, float* dL_dimg1,
                                   hipStream_t st) {
    const double count = (double)planes * H * W;
    GSR_SSIM_BWD(1, dL_dmean, (float)(1.0 / count), 0.f);
}

void gsr_launch_ssim_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmap,
                              const float* dm_dmu1, const float* dm_dex2, const float* dm_dexy, float* dL_dimg1, hipStream_t st) {
    GSR_SSIM_BWD(0, dL_dmap, 0.f, 0.f);
}

// fused training loss (train.py:119-126): loss = (1 - lambda) L1 + lambda (1 - SSIM); partials holds 2 x gsr_ssim_partial_count floats
void gsr_launch_train_loss_forward(int planes, int H, int W, const float* img1, const float* img2, float lambda, float* partials,
                                   float* loss_out /*[3]: loss, L1, SSIM*/, float* dm_dmu1, float* dm_dex2, float* dm_dexy, hipStream_t st) {
    GSR_SSIM_FWD(2, partials);
    const double count = (double)planes * H * W;
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(256), 0, st, partials, (int)ssim_partials_now(planes, H, W, dm_dmu1 == nullptr),
                       (float)(1.0 / count), lambda, loss_out);
}

void gsr_launch_train_loss_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dloss, float lambda,
                                    const float* dm_dmu1, const float* dm_dex2, const float* dm_dexy, float* dL_dimg1, hipStream_t st) {
    const double count = (double)planes * H * W;
    GSR_SSIM_BWD(2, dL_dloss, (float)(1.0 / count), lambda);
}
