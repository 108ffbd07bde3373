// Vector quantisation of per-Gaussian parameters (k-means over codebooks of up to 65536 entries; "Compressed 3D Gaussian Splatting", Compact3D,
// LightGaussian, gsplat's PngCompression): the two steps of a Lloyd iteration as native pieces, DESIGN.md 5.13.  gsr_scene/compress.py is the
// package side.
//
// vq_norms   -- per centroid: cnorm[k] = sum_i c_ki^2 as an ascending fmaf chain, +inf for a centroid that is not finite (or past K: the padding of
//               the last tile), and the codebook rewritten as the LDS image of the assignment: tiles of 32 centroids, [tile][d][32], d padded to
//               an even count with zeros, a centroid that is not finite all zeros.  score = +inf never wins a strict `<`.
// vq_assign  -- argmin_k (cnorm[k] - 2 x_p . c_k) for every row, never writing a P x K block.  A workgroup of four waves owns 256 rows; a wave keeps
//               its 64 rows (two tiles of 32) as the A operands of v_mfma_f32_32x32x2_f32 in registers, premultiplied by -2 (exact), for the
//               whole sweep over K.  Centroid images stream through LDS, 64 centroids per stage, double-buffered: the next stage's global loads
//               are issued before the current stage's matrix work and held in registers across it, one barrier per stage.  The accumulators START at cnorm[column], so the
//               instruction's own fmaf chain ends at the score and the epilogue is compare + two selects per element: lane l holds column
//               l & 31 of 16 rows per tile and keeps a running (score, tile) per row with strict `<` over ascending tiles.  One butterfly over
//               the 32 lanes of a half wave at the end takes the minimum by (score, then index): the lowest index wins an exact fp32 tie.
//               dist2 is recomputed from the winner directly, the ascending fmaf chain of (x_i - c_i)^2, not from the cancelling score form.
//               A row with a non-finite component gives idx -1, dist2 0 (its scores are NaN / inf in its own accumulator rows only).
// vq_update  -- keys (idx, -1 -> K) with values p through the stable pair sort of sort.hip (rows of a cluster stay in ascending p), segment
//               bounds by binary search, then sums of w_p x_p and w_p per cluster in fp64 in a fixed order: segments are cut into chunks of 256
//               rows, one wave per chunk (lane = dimension, rows in sorted order), and a second kernel adds a cluster's chunks in chunk order.
//               No floating-point atomics: two runs give the same bits.
#include "gsr_internal.h"
#include "gsr_mfma.h"

namespace {

constexpr int kChunk = 64;               // centroids per LDS stage: two MFMA tiles of 32
constexpr int kRowTiles = 2;             // tiles of 32 rows per wave
constexpr int kBlockRows = 256;          // rows per workgroup: 4 waves x 2 tiles x 32
constexpr int kSumRows = 256;            // rows per chunk of the update's segment sums
constexpr float kFltMax = 3.402823466e38f;
#ifdef GSR_SIMT_SHIM
constexpr bool kSkipIdleTiles = true;    // host build: a row tile past P is skipped (34 fiber round trips per instruction); its results are never stored
#else
constexpr bool kSkipIdleTiles = false;
#endif

typedef float vq_f4 __attribute__((vector_size(16)));      // a native 16-byte vector: an array of these is promoted to registers where HIP's float4 class is not
__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= kFltMax; }      // false for NaN and +-inf
__device__ __forceinline__ float pos_inf() { return __uint_as_float(0x7F800000u); }

// one thread per centroid of the padded range [0, Kpad)
__global__ void __launch_bounds__(256)
vq_norms_kernel(int D, int K, int DP, int Kpad, const float* __restrict__ cb, float* __restrict__ cnorm, float* __restrict__ image) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= Kpad) return;
    bool ok = k < K;
    const float* c = cb + (int64_t)(ok ? k : 0) * D;
    float n = 0.f;
    for (int d = 0; d < D; ++d) {
        const float v = c[d];
        ok = ok && finite1(v);
        n = fmaf(v, v, n);
    }
    ok = ok && finite1(n);
    cnorm[k] = ok ? n : pos_inf();
    float* img = image + (int64_t)(k >> 5) * DP * 32 + (k & 31);
    for (int d = 0; d < DP; ++d) img[d * 32] = (ok && d < D) ? c[d] : 0.f;
}

// NP: k-pairs of the padded dimension (DP = 2 NP >= D).  `cnorm` and `image` are deliberately NOT __restrict__: loads the compiler knows to be
// invariant are free to be scheduled at their use, behind the matrix work they are meant to overlap (the sched_barrier below does not hold them).
// (two waves per SIMD: 256 registers at most, so that a second workgroup on the CU covers this one's epilogues and barriers)
template <int NP>
__global__ void __launch_bounds__(256, 2)
vq_assign_kernel(int P, int D, int nchunks, const float* __restrict__ rows, const float* __restrict__ cb, const float* cnorm,
                 const vq_f4* image, int32_t* __restrict__ idx, float* __restrict__ dist2) {
    constexpr int DP = 2 * NP;
    constexpr int kVecs = kChunk * DP / 4;                 // float4 per stage
    constexpr int NV = (kVecs + 255) / 256;                // ... per thread
    __shared__ vq_f4 s_b[2][kVecs];
    __shared__ float s_cn[2][kChunk];
    __shared__ int32_t s_idx[kBlockRows];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int64_t wrow0 = (int64_t)blockIdx.x * kBlockRows + wave * 64;
    bool act[kRowTiles];
    float a[kRowTiles][NP];
#pragma unroll
    for (int rt = 0; rt < kRowTiles; ++rt) {
        const int64_t row = wrow0 + rt * 32 + j;
        act[rt] = wrow0 + rt * 32 < P;
        const float* x = rows + (row < P ? row : (int64_t)P - 1) * D;      // (lanes past the end read the last row: never stored)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int d = 2 * p + h;
            const float v = x[d < D ? d : D - 1];
            a[rt][p] = d < D ? -2.f * v : 0.f;
        }
    }
    float best_s[kRowTiles][16];
    int best_t[kRowTiles][16];
#pragma unroll
    for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { best_s[rt][r] = pos_inf(); best_t[rt][r] = -1; }

    // the stage in flight: NV float4 and one norm per thread, in registers from the load to the LDS write (no lambda, no conditional load: the last
    // trip re-reads its own stage into the buffer nobody reads any more)
    vq_f4 pre[NV];
    float pre_cn;
#define VQ_FETCH(c_)                                                                        \
    {                                                                                       \
        const vq_f4* src_ = image + (int64_t)(c_) * kVecs;                                 \
        _Pragma("unroll") for (int v = 0; v < NV; ++v) {                                    \
            const int e = v * 256 + tid;                                                    \
            pre[v] = src_[e < kVecs ? e : kVecs - 1];                                       \
        }                                                                                   \
        pre_cn = cnorm[(int64_t)(c_) * kChunk + lane];                                      \
    }
#define VQ_STASH(buf_)                                                                      \
    {                                                                                       \
        _Pragma("unroll") for (int v = 0; v < NV; ++v) {                                    \
            const int e = v * 256 + tid;                                                    \
            if (kVecs % 256 == 0 || e < kVecs) s_b[buf_][e] = pre[v];                       \
        }                                                                                   \
        if (tid < kChunk) s_cn[buf_][tid] = pre_cn;                                         \
    }
    VQ_FETCH(0)
    VQ_STASH(0)
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        VQ_FETCH(c + 1 < nchunks ? c + 1 : c)
        __builtin_amdgcn_sched_barrier(0);      // the loads are issued HERE, ahead of the matrix work that hides them
        // (no branch around the matrix work on the device: behind one, the compiler sinks the loads to their use.  A wave whose rows are all past P
        // works on copies of the last row, which are never stored; the host build skips it)
        if (!kSkipIdleTiles || act[0]) {
            const float* sb = reinterpret_cast<const float*>(s_b[buf]);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float cn = s_cn[buf][t * 32 + j];
                float acc[kRowTiles][16];
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[rt][r] = cn;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float b = sb[t * DP * 32 + p * 64 + lane];
#pragma unroll
                    for (int rt = 0; rt < kRowTiles; ++rt)
                        if (!kSkipIdleTiles || act[rt]) gsr_mfma_32x32x2_f32(a[rt][p], b, acc[rt]);
                }
                const int tile = c * 2 + t;
#pragma unroll
                for (int rt = 0; rt < kRowTiles; ++rt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool take = acc[rt][r] < best_s[rt][r];      // (NaN never takes)
                        best_s[rt][r] = take ? acc[rt][r] : best_s[rt][r];
                        best_t[rt][r] = take ? tile : best_t[rt][r];
                    }
            }
        }
        VQ_STASH(buf ^ 1)
        __syncthreads();
    }
    if (act[0]) {
#pragma unroll
        for (int rt = 0; rt < kRowTiles; ++rt) {
            if (kSkipIdleTiles && !act[rt]) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float s = best_s[rt][r];
                uint32_t i = best_t[rt][r] < 0 ? 0xFFFFFFFFu : (uint32_t)(best_t[rt][r] * 32 + j);
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) {      // (inside a half wave: the two halves hold different rows)
                    const float os = __shfl_xor(s, m);
                    const uint32_t oi = __shfl_xor(i, m);
                    const bool take = os < s || (os == s && oi < i);
                    s = take ? os : s;
                    i = take ? oi : i;
                }
                if (j == 0) s_idx[wave * 64 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = (int32_t)i;
            }
        }
    }
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * kBlockRows + tid;
    if (row < P) {
        int32_t k = s_idx[tid];
        const float* x = rows + row * D;
        const float* c = cb + (int64_t)(k < 0 ? 0 : k) * D;
        bool ok = k >= 0;
        float d2 = 0.f;
        for (int d = 0; d < D; ++d) {
            const float xv = x[d];
            const float diff = xv - c[d];
            ok = ok && finite1(xv);
            d2 = fmaf(diff, diff, d2);
        }
        idx[row] = ok ? k : -1;
        dist2[row] = ok ? d2 : 0.f;
    }
}

// ---- update ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vq_keys_kernel(int P, int K, const int32_t* __restrict__ idx, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t k = idx[i];
        keys[i] = (k >= 0 && k < K) ? (uint32_t)k : (uint32_t)K;      // -1 (and anything out of range) sorts last and is summed by nobody
        vals[i] = (uint32_t)i;
    }
}

// start[k] = the first sorted position whose key is >= k, k = 0 .. K
__global__ void __launch_bounds__(256)
vq_bounds_kernel(int P, int K, const uint32_t* __restrict__ keys, uint32_t* __restrict__ start) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    uint32_t lo = 0u, hi = (uint32_t)P;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < (uint32_t)k) lo = mid + 1u; else hi = mid;
    }
    start[k] = lo;
}

__device__ __forceinline__ uint32_t seg_chunks(const uint32_t* start, int k) { return (start[k + 1] - start[k] + (kSumRows - 1)) / kSumRows; }

// one workgroup: first[k] = chunks of the clusters before k, first[K] = all chunks
__global__ void __launch_bounds__(256)
vq_scan_kernel(int K, const uint32_t* __restrict__ start, uint32_t* __restrict__ first) {
    __shared__ uint32_t s_sum[256];
    const int tid = (int)threadIdx.x, per = (K + 255) / 256;
    const int k0 = min(tid * per, K), k1 = min(k0 + per, K);
    uint32_t local = 0u;
    for (int k = k0; k < k1; ++k) local += seg_chunks(start, k);
    s_sum[tid] = local;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0u;
        for (int i = 0; i < 256; ++i) { const uint32_t t = s_sum[i]; s_sum[i] = run; run += t; }
        first[K] = run;
    }
    __syncthreads();
    uint32_t run = s_sum[tid];
    for (int k = k0; k < k1; ++k) { first[k] = run; run += seg_chunks(start, k); }
}

// one wave per chunk: lane d adds w_p x_p[d] over the chunk's rows in sorted order, in fp64 (the products are exact)
__global__ void __launch_bounds__(64)
vq_chunk_kernel(int D, int K, const float* __restrict__ rows, const float* __restrict__ weights, const uint32_t* __restrict__ order,
                const uint32_t* __restrict__ start, const uint32_t* __restrict__ first, double* __restrict__ partial) {
    const uint32_t g = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (g >= first[K]) return;
    int lo = 0, hi = K;      // the first index whose count of earlier chunks exceeds g; its predecessor owns chunk g (empty clusters repeat a value)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] > g) hi = mid; else lo = mid + 1;
    }
    const int k = lo - 1;
    const uint32_t b = start[k] + (g - first[k]) * (uint32_t)kSumRows, e = min(b + (uint32_t)kSumRows, start[k + 1]);
    const int dl = lane < D ? lane : D - 1;
    double acc = 0.0, wacc = 0.0;
    for (uint32_t pos = b; pos < e; pos += 64u) {
        const uint32_t q = pos + (uint32_t)lane;
        const uint32_t pv = order[q < e ? q : e - 1u];
        float wv = weights ? weights[pv] : 1.f;
        wv = (wv > 0.f && wv <= kFltMax) ? wv : 0.f;      // negative, NaN, inf: 0
        const int n = (int)min(64u, e - pos);
        for (int i0 = 0; i0 < n; i0 += 8) {      // eight rows in flight: unconditional loads (slots past n repeat row n - 1 with weight 0), then the adds in order
            float x[8], w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u < n ? i0 + u : n - 1;
                const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pv, i);
                w[u] = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(wv), i));
                w[u] = i0 + u < n ? w[u] : 0.f;
                x[u] = rows[(int64_t)p * D + dl];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc += w[u] > 0.f ? (double)w[u] * (double)x[u] : 0.0;      // (a row of weight 0 adds nothing, whatever it holds)
                wacc += (double)w[u];
            }
        }
    }
    double* out = partial + (int64_t)g * (D + 1);
    if (lane < D) out[lane] = acc;
    if (lane == 0) out[D] = wacc;
}

// one wave per cluster: its chunks in chunk order; an empty cluster (no weight) keeps its centroid
__global__ void __launch_bounds__(64)
vq_finish_kernel(int D, const uint32_t* __restrict__ first, const double* __restrict__ partial, float* __restrict__ cb, float* __restrict__ mass) {
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int dl = lane < D ? lane : D - 1;
    double tot = 0.0, wt = 0.0;
    for (uint32_t c = first[k]; c < first[k + 1]; ++c) {
        const double* in = partial + (int64_t)c * (D + 1);
        tot += in[dl];
        wt += in[D];
    }
    if (wt > 0.0 && lane < D) cb[(int64_t)k * D + lane] = (float)(tot / wt);
    if (lane == 0) mass[k] = (float)wt;
}

inline int vq_pairs(int D) { return D <= 8 ? 4 : D <= 16 ? 8 : D <= 32 ? 16 : D <= 48 ? 24 : 32; }
inline int vq_kpad(int K) { return (K + kChunk - 1) / kChunk * kChunk; }
inline int64_t vq_max_chunks(int P, int K) { return (int64_t)(K < P ? K : P) + (int64_t)P / kSumRows; }

struct VqScratch {
    float* cnorm;             // [Kpad]
    float* image;             // [Kpad * DP]
    uint32_t* keys[2];        // [P] x2
    uint32_t* vals[2];        // [P] x2
    uint32_t* sort_hist;
    uint32_t* digit_total;    // [2048]
    uint32_t* start;          // [K + 2]
    uint32_t* first;          // [K + 2]
    double* partial;          // [max chunks][D + 1]
    size_t bytes;
};

VqScratch vq_carve(char* base, int P, int D, int K) {
    VqScratch s;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += gsr_align128(bytes);
        return p;
    };
    const int Kpad = vq_kpad(K), DP = 2 * vq_pairs(D);
    s.cnorm = (float*)take((size_t)Kpad * 4);
    s.image = (float*)take((size_t)Kpad * DP * 4);
    for (int i = 0; i < 2; ++i) s.keys[i] = (uint32_t*)take((size_t)P * 4);
    for (int i = 0; i < 2; ++i) s.vals[i] = (uint32_t*)take((size_t)P * 4);
    s.sort_hist = (uint32_t*)take((size_t)256 * (size_t)gsr_sort_blocks(P, true) * 4);
    s.digit_total = (uint32_t*)take(2048 * 4);
    s.start = (uint32_t*)take((size_t)(K + 2) * 4);
    s.first = (uint32_t*)take((size_t)(K + 2) * 4);
    s.partial = (double*)take((size_t)vq_max_chunks(P, K) * (size_t)(D + 1) * 8);
    s.bytes = off;
    return s;
}

inline int grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b > 2048) b = 2048;
    return b < 1 ? 1 : (int)b;
}

}  // namespace

size_t gsr_vq_scratch_bytes_impl(int P, int D, int K) { return vq_carve(nullptr, P, D, K).bytes; }

void gsr_launch_vq_assign(int P, int D, int K, const float* rows, const float* codebook, int32_t* idx, float* dist2, void* scratch, hipStream_t st) {
    const VqScratch s = vq_carve((char*)scratch, P, D, K);
    const int Kpad = vq_kpad(K), NP = vq_pairs(D), nchunks = Kpad / kChunk;
    hipLaunchKernelGGL(vq_norms_kernel, dim3((unsigned)((Kpad + 255) / 256)), dim3(256), 0, st, D, K, 2 * NP, Kpad, codebook, s.cnorm, s.image);
    const dim3 grid((unsigned)(((int64_t)P + kBlockRows - 1) / kBlockRows));
    const vq_f4* image = reinterpret_cast<const vq_f4*>(s.image);
    switch (NP) {
        case 4: hipLaunchKernelGGL(vq_assign_kernel<4>, grid, dim3(256), 0, st, P, D, nchunks, rows, codebook, (const float*)s.cnorm, image, idx, dist2); break;
        case 8: hipLaunchKernelGGL(vq_assign_kernel<8>, grid, dim3(256), 0, st, P, D, nchunks, rows, codebook, (const float*)s.cnorm, image, idx, dist2); break;
        case 16: hipLaunchKernelGGL(vq_assign_kernel<16>, grid, dim3(256), 0, st, P, D, nchunks, rows, codebook, (const float*)s.cnorm, image, idx, dist2); break;
        case 24: hipLaunchKernelGGL(vq_assign_kernel<24>, grid, dim3(256), 0, st, P, D, nchunks, rows, codebook, (const float*)s.cnorm, image, idx, dist2); break;
        default: hipLaunchKernelGGL(vq_assign_kernel<32>, grid, dim3(256), 0, st, P, D, nchunks, rows, codebook, (const float*)s.cnorm, image, idx, dist2); break;
    }
}

void gsr_launch_vq_update(int P, int D, int K, const float* rows, const float* weights, const int32_t* idx, float* codebook, float* mass,
                          void* scratch, hipStream_t st) {
    VqScratch s = vq_carve((char*)scratch, P, D, K);
    hipLaunchKernelGGL(vq_keys_kernel, dim3(grid_for(P)), dim3(256), 0, st, P, K, idx, s.keys[0], s.vals[0]);
    int nbits = 1;
    while ((1 << nbits) <= K) ++nbits;      // keys 0 .. K
    const int cur = gsr_radix_sort_pairs(s.keys, s.vals, P, nbits, 8, s.sort_hist, s.digit_total, P < (1 << 21) ? GSR_SORT_ITEMS_SMALL : GSR_SORT_ITEMS, st);
    hipLaunchKernelGGL(vq_bounds_kernel, dim3((unsigned)((K + 1 + 255) / 256)), dim3(256), 0, st, P, K, (const uint32_t*)s.keys[cur], s.start);
    hipLaunchKernelGGL(vq_scan_kernel, dim3(1), dim3(256), 0, st, K, (const uint32_t*)s.start, s.first);
    hipLaunchKernelGGL(vq_chunk_kernel, dim3((unsigned)vq_max_chunks(P, K)), dim3(64), 0, st, D, K, rows, weights, (const uint32_t*)s.vals[cur],
                       (const uint32_t*)s.start, (const uint32_t*)s.first, s.partial);
    hipLaunchKernelGGL(vq_finish_kernel, dim3((unsigned)K), dim3(64), 0, st, D, (const uint32_t*)s.first, (const double*)s.partial, codebook, mass);
}
