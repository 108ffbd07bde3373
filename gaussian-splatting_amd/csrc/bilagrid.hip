// Bilateral-grid appearance model ("Bilateral Guided Radiance Field Processing"; gsplat's lib_bilagrid / fused_bilagrid), DESIGN.md 5.10.
//
// One grid A[12, L, Gh, Gw]: channel 4 i + j is entry (i, j) of a 3x4 affine colour map.  A pixel (x, y) of a planar [3, H, W] image samples it
// trilinearly at  fx = (x + 0.5) / W (Gw - 1),  fy = (y + 0.5) / H (Gh - 1),  fz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)  and is mapped
// through the sampled matrix (include/gsr.h has the full statement).
//
// fx and fy depend on the pixel's position only, so every xy cell of the grid owns a pixel RECTANGLE.  A workgroup takes a tile of one cell's
// rectangle: the 2 x 2 x L x 12 corner values it needs (a strided gather from the channel-major grid) are staged into LDS once, then the pixels
// stream.  The cell of a pixel column / row is bg_cell() below -- ONE fp32 expression, evaluated by the host (plan), by the kernels that find
// their rectangle (bg_start) and per pixel for the fraction -- so a pixel is never attributed to two cells or to none.
//
// Backward, grid gradient: no floating-point atomics anywhere.  Per wave step and per z level that a lane of the wave touches (ballot) the 4 xy
// weights x the tent weight x the 12 products dL/dout_i [r, g, b, 1]_j are summed over the wave (gsr_wave.h reduce4) and added by one lane per
// address into the wave's OWN LDS accumulator, in program order; the four accumulators are added in a fixed order into one partial block per
// workgroup in scratch; bilagrid_reduce_kernel then sums, one thread per grid element, the partial blocks of the at most 4 cells x tiles that
// reach that vertex, cells and tiles in index order.  Two runs give the same bits.
//
// Total variation: fp64 inside (every squared difference of two fp32 values is exact in fp64), per-workgroup partial sums in a fixed order, a
// one-workgroup kernel adds them in index order.
#include "gsr_internal.h"
#include "gsr_wave.h"
#include "gsr_reduce.h"

namespace {

constexpr int kMaxSteps = 8;             // wave steps per tile: a thread handles at most 8 pixels
constexpr int kTvGridCap = 1024;         // workgroups (= partial sums) of the TV forward
constexpr int kTvBwdGridCap = 1 << 16;
constexpr float kWr = 0.299f, kWg = 0.587f, kWb = 0.114f;

// ---- the pixel -> cell map of one axis -------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ float bg_coord(int x, const GsrBilagridAxis& a) { return ((float)x + 0.5f) * a.gm1 * a.inv; }
// (the coordinate is never negative; the last cell is closed on both sides)
__host__ __device__ __forceinline__ int bg_cell(int x, const GsrBilagridAxis& a) {
    const int c = (int)bg_coord(x, a);
    return c < a.n - 2 ? c : a.n - 2;
}
// first pixel of cell c (c = n - 1: one past the last pixel).  bg_cell is monotonic in x (every step of it is a correctly rounded, monotonic
// operation), so the two loops end at THE boundary whatever the guess was.
__host__ __device__ inline int bg_start(int c, const GsrBilagridAxis& a) {
    if (c <= 0) return 0;
    if (c >= a.n - 1) return a.size;
    int x = (int)((float)c * (float)a.size / a.gm1);
    x = x < 0 ? 0 : (x > a.size ? a.size : x);
    while (x > 0 && bg_cell(x - 1, a) >= c) --x;
    while (x < a.size && bg_cell(x, a) < c) ++x;
    return x;
}

__host__ __device__ __forceinline__ int bg_tiles(int x0, int x1, int y0, int y1, const GsrBilagridPlan& p) {
    return ((x1 - x0 + p.tw - 1) >> p.twl) * ((y1 - y0 + p.th - 1) / p.th);
}

// The tile of this workgroup: cell (cx, cy), the cell's pixel columns end at x1 and rows at y1, the tile starts at (xt, yt).  false: the cell's
// rectangle has fewer tiles than the plan's maximum and this workgroup has none.
__device__ __forceinline__ bool bg_tile(const GsrBilagridPlan& p, int& cx, int& cy, int& xt, int& x1, int& yt, int& y1) {
    const int cell = (int)blockIdx.x / p.maxchunks, chunk = (int)blockIdx.x - cell * p.maxchunks;
    cy = cell / (p.ax.n - 1);
    cx = cell - cy * (p.ax.n - 1);
    const int x0 = bg_start(cx, p.ax), y0 = bg_start(cy, p.ay);
    x1 = bg_start(cx + 1, p.ax);
    y1 = bg_start(cy + 1, p.ay);
    const int tiles_x = (x1 - x0 + p.tw - 1) >> p.twl;
    if (chunk >= bg_tiles(x0, x1, y0, y1, p)) return false;
    const int ty = chunk / tiles_x, tx = chunk - ty * tiles_x;
    xt = x0 + (tx << p.twl);
    yt = y0 + ty * p.th;
    return true;
}

// the 2 x 2 x L x 12 corner values of cell (cx, cy) -> s[corner = 2 dy + dx][z][12]
__device__ __forceinline__ void bg_stage(const GsrBilagridPlan& p, const float* __restrict__ grid, int cx, int cy, float* s) {
    const int L = p.L, Gw = p.ax.n, Gh = p.ay.n;
    for (int t = (int)threadIdx.x; t < 48 * L; t += (int)blockDim.x) {
        const int ch = t % 12, z = (t / 12) % L, c = t / (12 * L);
        s[t] = grid[(((size_t)ch * L + z) * Gh + cy + (c >> 1)) * Gw + cx + (c & 1)];
    }
}

struct BgPix {
    float w00, w01, w10, w11, tz;      // xy corner weights (corner = 2 dy + dx) and the fraction along z
    int z0;
    bool inside;                       // the unclamped fz lies in [0, L - 1]: the guidance has a slope
};
// Indices come from the clamped value: fmaxf(NaN, 0) = 0, so a NaN guidance lands in cell 0 with fraction 0, +-inf at the ends.
__device__ __forceinline__ BgPix bg_pixel(const GsrBilagridPlan& p, int x, int y, int cx, int cy, float r, float g, float b) {
    BgPix q;
    const float tx = bg_coord(x, p.ax) - (float)cx, ty = bg_coord(y, p.ay) - (float)cy;
    q.w00 = (1.f - ty) * (1.f - tx); q.w01 = (1.f - ty) * tx; q.w10 = ty * (1.f - tx); q.w11 = ty * tx;
    const float zmax = (float)(p.L - 1);
    const float fz = (kWr * r + kWg * g + kWb * b) * zmax;
    q.inside = fz >= 0.f && fz <= zmax;
    const float fzc = fminf(fmaxf(fz, 0.f), zmax);
    const int zi = (int)fzc;
    q.z0 = zi < p.L - 2 ? zi : p.L - 2;
    q.tz = fzc - (float)q.z0;
    return q;
}
// the xy blend of the four corners at level z
__device__ __forceinline__ void bg_blend_xy(const float* s, int L, int z, const BgPix& q, float (&A)[12]) {
    const float* c0 = s + z * 12;
    const float* c1 = c0 + 12 * L;
    const float* c2 = c1 + 12 * L;
    const float* c3 = c2 + 12 * L;
#pragma unroll
    for (int j = 0; j < 12; ++j) A[j] = q.w00 * c0[j] + q.w01 * c1[j] + q.w10 * c2[j] + q.w11 * c3[j];
}

// ---- slice forward --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
bilagrid_slice_kernel(GsrBilagridPlan p, const float* __restrict__ grid, const float* __restrict__ image, float* __restrict__ out) {
    __shared__ float sA[48 * GSR_BILAGRID_MAX] __attribute__((aligned(16)));
    int cx, cy, xt, x1, yt, y1;
    if (!bg_tile(p, cx, cy, xt, x1, yt, y1)) return;      // (the whole workgroup)
    bg_stage(p, grid, cx, cy, sA);
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, rsl = 6 - p.twl;
    const int x = xt + (lane & (p.tw - 1));
    const size_t plane = (size_t)p.ax.size * p.ay.size;
    for (int k = 0; k < p.steps; ++k) {
        const int y = yt + (((k << 2) + wave) << rsl) + (lane >> p.twl);
        if (x >= x1 || y >= y1) continue;
        const size_t idx = (size_t)y * p.ax.size + x;
        const float r = image[idx], g = image[plane + idx], b = image[2 * plane + idx];
        const BgPix q = bg_pixel(p, x, y, cx, cy, r, g, b);
        float lo[12], hi[12];
        bg_blend_xy(sA, p.L, q.z0, q, lo);
        bg_blend_xy(sA, p.L, q.z0 + 1, q, hi);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float A[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) A[j] = lo[4 * i + j] + q.tz * (hi[4 * i + j] - lo[4 * i + j]);
            out[i * plane + idx] = A[0] * r + A[1] * g + A[2] * b + A[3];
        }
    }
}

// ---- slice backward -------------------------------------------------------------------------------------------------------------------------
// scratch: one block of [corner][z][12] floats per (cell, tile slot); tile slots beyond a cell's own tile count are never written and never read.
template <int LMAX, bool IMG>
__global__ void __launch_bounds__(256)
bilagrid_slice_bwd_kernel(GsrBilagridPlan p, const float* __restrict__ grid, const float* __restrict__ image, const float* __restrict__ dout,
                          float* __restrict__ dimage, float* __restrict__ scratch) {
    __shared__ float sA[IMG ? 48 * LMAX : 4] __attribute__((aligned(16)));
    __shared__ float sAcc[gsrw::WG_WAVES][48 * LMAX];      // one accumulator per wave: a single writer per address, in program order
    int cx, cy, xt, x1, yt, y1;
    if (!bg_tile(p, cx, cy, xt, x1, yt, y1)) return;      // (the whole workgroup)
    const int L = p.L, n = 48 * L;
    for (int t = (int)threadIdx.x; t < n; t += 256) {
#pragma unroll
        for (int w = 0; w < gsrw::WG_WAVES; ++w) sAcc[w][t] = 0.f;
    }
    if (IMG) bg_stage(p, grid, cx, cy, sA);
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, rsl = 6 - p.twl;
    const int x = xt + (lane & (p.tw - 1));
    const size_t plane = (size_t)p.ax.size * p.ay.size;
    const float zmax = (float)(L - 1);
    // reduce4 leaves its four sums in the last lane of the rows 0..3 in the order (a, c, b, d): the corner this lane adds
    const int row = lane >> 4, corner = ((row & 1) << 1) | (row >> 1);
    float* acc = sAcc[wave] + corner * 12 * L;
    for (int k = 0; k < p.steps; ++k) {
        const int y = yt + (((k << 2) + wave) << rsl) + (lane >> p.twl);
        const bool valid = x < x1 && y < y1;
        if (__ballot(valid) == 0) continue;      // (wave-uniform: every lane of the wave takes part in the reductions below)
        const size_t idx = valid ? (size_t)y * p.ax.size + x : 0;
        float r = image[idx], g = image[plane + idx], b = image[2 * plane + idx];
        float d0 = dout[idx], d1 = dout[plane + idx], d2 = dout[2 * plane + idx];
        if (!valid) { r = g = b = 0.f; d0 = d1 = d2 = 0.f; }
        const BgPix q = bg_pixel(p, x, y, cx, cy, r, g, b);
        if (IMG) {
            float lo[12], hi[12];
            bg_blend_xy(sA, L, q.z0, q, lo);
            bg_blend_xy(sA, L, q.z0 + 1, q, hi);
            const float d[3] = {d0, d1, d2};
            float gr = 0.f, gg = 0.f, gb = 0.f, s = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float e0 = hi[4 * i] - lo[4 * i], e1 = hi[4 * i + 1] - lo[4 * i + 1], e2 = hi[4 * i + 2] - lo[4 * i + 2],
                            e3 = hi[4 * i + 3] - lo[4 * i + 3];
                gr += d[i] * (lo[4 * i] + q.tz * e0);
                gg += d[i] * (lo[4 * i + 1] + q.tz * e1);
                gb += d[i] * (lo[4 * i + 2] + q.tz * e2);
                s += d[i] * (e0 * r + e1 * g + e2 * b + e3);
            }
            s = q.inside ? s * zmax : 0.f;
            if (valid) {
                dimage[idx] = gr + kWr * s;
                dimage[plane + idx] = gg + kWg * s;
                dimage[2 * plane + idx] = gb + kWb * s;
            }
        }
        const float P[12] = {d0 * r, d0 * g, d0 * b, d0, d1 * r, d1 * g, d1 * b, d1, d2 * r, d2 * g, d2 * b, d2};
        for (int z = 0; z < L; ++z) {
            const bool touch = valid && (z == q.z0 || z == q.z0 + 1);
            if (__ballot(touch) == 0) continue;
            // (selects, not products with a zero weight: a non-finite pixel reaches the two levels it touches and no other)
            const float wz = touch ? (z == q.z0 ? 1.f - q.tz : q.tz) : 0.f;
            const float t0 = wz * q.w00, t1 = wz * q.w01, t2 = wz * q.w10, t3 = wz * q.w11;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const float pj = touch ? P[j] : 0.f;
                const float v = gsrw::reduce4(t0 * pj, t1 * pj, t2 * pj, t3 * pj);
                if ((lane & 15) == 15) acc[z * 12 + j] += v;
            }
        }
    }
    __syncthreads();
    float* dst = scratch + (size_t)blockIdx.x * n;
    for (int t = (int)threadIdx.x; t < n; t += 256) dst[t] = (sAcc[0][t] + sAcc[1][t]) + (sAcc[2][t] + sAcc[3][t]);
}

// one thread per grid element, (vertex, z, channel) with the channel fastest: the threads of a vertex read runs of 12 L floats of a partial block
__global__ void __launch_bounds__(256)
bilagrid_reduce_kernel(GsrBilagridPlan p, const float* __restrict__ scratch, float* __restrict__ dgrid) {
    const int L = p.L, Gw = p.ax.n, Gh = p.ay.n;
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= 12 * L * Gh * Gw) return;
    const int ch = t % 12, z = (t / 12) % L, v = t / (12 * L), gx = v % Gw, gy = v / Gw;
    const size_t block = (size_t)48 * L;
    float sum = 0.f;
    for (int cy = gy - 1; cy <= gy; ++cy) {
        if (cy < 0 || cy > Gh - 2) continue;
        for (int cx = gx - 1; cx <= gx; ++cx) {
            if (cx < 0 || cx > Gw - 2) continue;
            const int tiles = bg_tiles(bg_start(cx, p.ax), bg_start(cx + 1, p.ax), bg_start(cy, p.ay), bg_start(cy + 1, p.ay), p);
            const int corner = ((gy - cy) << 1) | (gx - cx);
            const float* s = scratch + (size_t)(cy * (Gw - 1) + cx) * p.maxchunks * block + ((size_t)corner * L + z) * 12 + ch;
            int c = 0;
            for (; c + 4 <= tiles; c += 4) {      // (four loads in flight; the adds keep the index order)
                const float a0 = s[c * block], a1 = s[(c + 1) * block], a2 = s[(c + 2) * block], a3 = s[(c + 3) * block];
                sum += a0; sum += a1; sum += a2; sum += a3;
            }
            for (; c < tiles; ++c) sum += s[c * block];
        }
    }
    dgrid[(((size_t)ch * L + z) * Gh + gy) * Gw + gx] = sum;
}

// ---- total variation --------------------------------------------------------------------------------------------------------------------------
struct BgTv { int L, Gh, Gw; double cL, cH, cW; };      // c = 1 / (N * elements of the axis' difference tensor per grid)

__global__ void __launch_bounds__(256)
bilagrid_tv_kernel(int64_t total, BgTv a, const float* __restrict__ X, double* __restrict__ partials) {
    __shared__ double s[256];
    const int64_t sH = a.Gw, sL = (int64_t)a.Gw * a.Gh;
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int gx = (int)(e % a.Gw), gy = (int)((e / sH) % a.Gh), z = (int)((e / sL) % a.L);
        // (unconditional loads from a clamped address, the selects afterwards: a load inside a branch is waited for on its own)
        const bool hx = gx + 1 < a.Gw, hy = gy + 1 < a.Gh, hz = z + 1 < a.L;
        const float v = X[e], vx = X[hx ? e + 1 : e], vy = X[hy ? e + sH : e], vz = X[hz ? e + sL : e];
        const double dx = hx ? (double)vx - (double)v : 0.0, dy = hy ? (double)vy - (double)v : 0.0, dz = hz ? (double)vz - (double)v : 0.0;
        acc += dx * dx * a.cW;
        acc += dy * dy * a.cH;
        acc += dz * dz * a.cL;
    }
    const double sum = gsrw::block_sum_f64(acc, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256)
bilagrid_tv_sum_kernel(int n, const double* __restrict__ partials, float* __restrict__ tv_out) {
    __shared__ double s[256];
    gsrw::block_sum_partials_f64(n, partials, 1.0, tv_out, s);
}

__global__ void __launch_bounds__(256)
bilagrid_tv_bwd_kernel(int64_t total, BgTv a, const float* __restrict__ X, const float* __restrict__ dL_dtv, float* __restrict__ dX) {
    const int64_t sH = a.Gw, sL = (int64_t)a.Gw * a.Gh;
    const double scale = 2.0 * (double)dL_dtv[0];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int gx = (int)(e % a.Gw), gy = (int)((e / sH) % a.Gh), z = (int)((e / sL) % a.L);
        const bool lx = gx > 0, hx = gx + 1 < a.Gw, ly = gy > 0, hy = gy + 1 < a.Gh, lz = z > 0, hz = z + 1 < a.L;
        const float vf = X[e], x0 = X[lx ? e - 1 : e], x1 = X[hx ? e + 1 : e], y0 = X[ly ? e - sH : e], y1 = X[hy ? e + sH : e],
                    z0 = X[lz ? e - sL : e], z1 = X[hz ? e + sL : e];
        const double v = (double)vf;
        double g = 0.0;
        g += (lx ? v - (double)x0 : 0.0) * a.cW;
        g -= (hx ? (double)x1 - v : 0.0) * a.cW;
        g += (ly ? v - (double)y0 : 0.0) * a.cH;
        g -= (hy ? (double)y1 - v : 0.0) * a.cH;
        g += (lz ? v - (double)z0 : 0.0) * a.cL;
        g -= (hz ? (double)z1 - v : 0.0) * a.cL;
        dX[e] = (float)(g * scale);
    }
}

BgTv tv_args(int N, int L, int Gh, int Gw) {
    BgTv a;
    a.L = L; a.Gh = Gh; a.Gw = Gw;
    a.cL = 1.0 / ((double)N * 12.0 * (L - 1) * Gh * Gw);
    a.cH = 1.0 / ((double)N * 12.0 * L * (Gh - 1) * Gw);
    a.cW = 1.0 / ((double)N * 12.0 * L * Gh * (Gw - 1));
    return a;
}

}  // namespace

// The launch plan of an image / grid pair: tile shape (tw = 2^twl columns, 8..64, one lane per column and 64 / tw rows per wave step; th rows =
// `steps` wave steps of the 4 waves) from the LARGEST cell rectangle, and the tile slots per cell.  Sizes were checked by the caller.
void gsr_bilagrid_plan(int H, int W, int L, int Gh, int Gw, GsrBilagridPlan* out) {
    GsrBilagridPlan p;
    p.ax.n = Gw; p.ax.size = W; p.ax.gm1 = (float)(Gw - 1); p.ax.inv = (float)(1.0 / (double)W);
    p.ay.n = Gh; p.ay.size = H; p.ay.gm1 = (float)(Gh - 1); p.ay.inv = (float)(1.0 / (double)H);
    p.L = L;
    int maxw = 1, maxh = 1;
    for (int c = 0; c < Gw - 1; ++c) { const int w = bg_start(c + 1, p.ax) - bg_start(c, p.ax); if (w > maxw) maxw = w; }
    for (int c = 0; c < Gh - 1; ++c) { const int h = bg_start(c + 1, p.ay) - bg_start(c, p.ay); if (h > maxh) maxh = h; }
    p.twl = 3;
    while ((1 << p.twl) < maxw && p.twl < 6) ++p.twl;
    p.tw = 1 << p.twl;
    const int rows = 4 * (64 >> p.twl);                                              // rows of one wave step of the workgroup
    const int tiles_y = (maxh + kMaxSteps * rows - 1) / (kMaxSteps * rows);          // as few tiles as 8 steps allow, then as even as possible
    p.steps = ((maxh + tiles_y - 1) / tiles_y + rows - 1) / rows;
    p.th = p.steps * rows;
    p.maxchunks = ((maxw + p.tw - 1) >> p.twl) * ((maxh + p.th - 1) / p.th);
    p.ncells = (Gw - 1) * (Gh - 1);
    *out = p;
}

void gsr_launch_bilagrid_slice(const GsrBilagridPlan& p, const float* grid, const float* image, float* out, hipStream_t st) {
    hipLaunchKernelGGL(bilagrid_slice_kernel, dim3((unsigned)((int64_t)p.ncells * p.maxchunks)), dim3(256), 0, st, p, grid, image, out);
}

void gsr_launch_bilagrid_slice_backward(const GsrBilagridPlan& p, const float* grid, const float* image, const float* dL_dout, float* dL_dgrid,
                                        float* dL_dimage, float* scratch, hipStream_t st) {
    const dim3 g((unsigned)((int64_t)p.ncells * p.maxchunks)), b(256);
    if (p.L <= 16) {
        if (dL_dimage) hipLaunchKernelGGL((bilagrid_slice_bwd_kernel<16, true>), g, b, 0, st, p, grid, image, dL_dout, dL_dimage, scratch);
        else hipLaunchKernelGGL((bilagrid_slice_bwd_kernel<16, false>), g, b, 0, st, p, grid, image, dL_dout, dL_dimage, scratch);
    } else {
        if (dL_dimage) hipLaunchKernelGGL((bilagrid_slice_bwd_kernel<GSR_BILAGRID_MAX, true>), g, b, 0, st, p, grid, image, dL_dout, dL_dimage, scratch);
        else hipLaunchKernelGGL((bilagrid_slice_bwd_kernel<GSR_BILAGRID_MAX, false>), g, b, 0, st, p, grid, image, dL_dout, dL_dimage, scratch);
    }
    const int total = 12 * p.L * p.ay.n * p.ax.n;
    hipLaunchKernelGGL(bilagrid_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p, scratch, dL_dgrid);
}

int64_t gsr_bilagrid_tv_partial_count_impl(int N, int L, int Gh, int Gw) {
    const int64_t total = (int64_t)N * 12 * L * Gh * Gw, nb = (total + 1023) / 1024;
    return nb < 1 ? 1 : (nb > kTvGridCap ? kTvGridCap : nb);
}

void gsr_launch_bilagrid_tv(int N, int L, int Gh, int Gw, const float* grids, double* partials, float* tv_out, hipStream_t st) {
    const int64_t total = (int64_t)N * 12 * L * Gh * Gw;
    const int nb = (int)gsr_bilagrid_tv_partial_count_impl(N, L, Gh, Gw);
    hipLaunchKernelGGL(bilagrid_tv_kernel, dim3(nb), dim3(256), 0, st, total, tv_args(N, L, Gh, Gw), grids, partials);
    hipLaunchKernelGGL(bilagrid_tv_sum_kernel, dim3(1), dim3(256), 0, st, nb, (const double*)partials, tv_out);
}

void gsr_launch_bilagrid_tv_backward(int N, int L, int Gh, int Gw, const float* grids, const float* dL_dtv, float* dL_dgrids, hipStream_t st) {
    const int64_t total = (int64_t)N * 12 * L * Gh * Gw;
    int64_t nb = (total + 255) / 256;
    if (nb > kTvBwdGridCap) nb = kTvBwdGridCap;
    hipLaunchKernelGGL(bilagrid_tv_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, st, total, tv_args(N, L, Gh, Gw), grids, dL_dtv, dL_dgrids);
}
