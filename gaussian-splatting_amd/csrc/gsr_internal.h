// Internal declarations shared by the translation units of libgsr_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "gsr.h"
#include "gsr_math.h"
#include "gsr_frame.h"

// ---- per-call camera block handed to kernels by value (matrices are read from device memory) ----
struct GsrCamDev {
    int W, H, gx, gy;
    float focal_x, focal_y, limx, limy, scale_modifier;
    int sh_degree, M, antialiasing, tile_y0, tile_y1;
    int snug;                // gsr_math.h GsrCam::snug
    const float* view;
    const float* proj;
    const float* campos;
    const float* bg;
    const float* sh_dc;      // split SH form (GsrRasterSettings.sh_dc), else NULL
    float* dL_dsh_dc;
};

// ---- scratch layouts (GeometryState / BinningState / ImageState), 128-byte aligned carve ----
static inline size_t gsr_align128(size_t x) { return (x + 127) & ~(size_t)127; }

#define GSR_SORT_ITEMS 4096      // items per workgroup in a radix pass (256 threads x 16)
#define GSR_SORT_ITEMS_SMALL 1024
#define GSR_SCAN_ITEMS 1024      // items per workgroup in the tiles_touched scan
#ifndef GSR_TS_ITEMS
#define GSR_TS_ITEMS 4096        // instances per workgroup of the fused emission / tile sort (tilesort.hip).  (Round 3 tuned it with -DGSR_TS_ITEMS=2048 builds; the
                                 // block tables of depthsort.hip / gsr_api.cpp have since been sized for 4096 and a 2048 build aborts: not a supported switch any more.)
#endif
// capacity of the per-block "first Gaussian" table the scan kernel fills: enough for 64 tiles per Gaussian on average;
// frames beyond that get the table from a fallback kernel once R is known (gsr_launch_fill_block_first)
static inline size_t gsr_block_first_cap(int P) { return (size_t)(P > 0 ? P : 1) / 64 + 66; }

// ---- bucket depth sort (depthsort.hip): one bucket pass over the keys + an LDS sort per segment of buckets ----
#define GSR_DS_ITEMS 4096        // keys per workgroup of the bucket histogram / scatter
#define GSR_DS_BITS 11
#define GSR_DS_BUCKETS 2048      // bucket 2047: Gaussians without a tile (they sort last)
#define GSR_DS_SEG 2048          // a segment = the buckets that start inside one window of this many elements
#define GSR_DS_CAP 4096          // largest segment sorted in LDS; beyond: the same passes through global memory (slow, reported)
#define GSR_DS_MAX_P (3 << 20)   // above: the LSD radix sort (the [workgroup][bucket] tables grow with P)
// Histogram-equalised bucket mapping (round 6, depthsort.hip ds_hist).  The 27-bit key space is cut into GSR_EQ_BINS coarse bins of 2^GSR_EQ_SHIFT keys
// (64 per octave of depth); every ds_hist workgroup reads the same GSR_EQ_SAMPLE keys -- GSR_EQ_SAMPLE / 16 windows of 16 consecutive keys spread
// evenly over the array -- and builds the same tables from them: (first bucket, buckets) per coarse bin, and for ONE "hot" coarse bin (an eighth of
// the sample or more) the same per sub-bin of 2^GSR_EQ_SHIFT2 keys.
#define GSR_EQ_SHIFT 17
#define GSR_EQ_BINS 1024         // 2^(GSR_DEPTH_KEY_BITS - GSR_EQ_SHIFT)
#define GSR_EQ_SHIFT2 7          // GSR_EQ_SHIFT - log2(GSR_EQ_BINS)
#define GSR_EQ_SAMPLE 4096
#define GSR_EQ_NO_HOT 0xFFFFFFFFu
// table buffer (ds_hist -> ds_scatter): GSR_EQ_BINS words level 1, GSR_EQ_BINS words level 2, then the hot bin (GSR_EQ_NO_HOT: no second level)
#define GSR_EQ_TAB_WORDS (2 * GSR_EQ_BINS + 16)
#define GSR_DS_PLAN_WORDS 12           // words per window of the segment plan (depthsort.hip ds_scatter)
#define GSR_DS_NO_HELP 0xFFFFFFFFu     // plan word 8: the window's workgroup has no helper job
#define GSR_DS_TIE_HELPED 0x80000000u  // plan word 3, bit 31: the segment's last bucket is more than a capacity of one key value; helpers write its chunks behind the first
struct GsrDepthSortBufs {
    uint2* pairs[2];             // [P] (key, id) in bucket order / scratch of an oversized segment
    uint32_t* cnt_tab;           // [workgroups][2048] keys per bucket, then their exclusive prefix over the workgroups
    uint32_t* tile_tab;          // [workgroups][2048] tile instances per bucket
    uint32_t* cnt_total;         // [2048]
    uint32_t* tile_total;        // [2048]
    uint32_t* plan;              // [segments][GSR_DS_PLAN_WORDS]
    uint16_t* bucket_of;         // [P] the depth bucket of every key (written by ds_hist, read by ds_scatter: the table lookup is done once)
    uint32_t* eq_tab;            // [GSR_EQ_TAB_WORDS] first bucket | buckets << 16 per coarse bin, the same per sub-bin of the hot coarse bin, the hot bin (ds_hist's workgroup 0)
};
size_t gsr_depth_bucket_blocks(int P);
size_t gsr_depth_bucket_segments(int P);

struct GsrGeom {                 // P-sized
    float4* splats;              // [4P]  (x,y,conA,conB) (conC,opacity,r,g) (b,depth,tau,1/depth) (rect.x,rect.y,goffset,tiles as bits)
    uint2* rect;                 // [P]   x = minx | maxx<<16 ; y = miny | maxy<<16 (band-clamped)
    uint32_t* tiles;             // [P]   tiles_touched
    uint32_t* clamped;           // [P]   colour clamp bits
    uint32_t* keys[2];           // [P]x2 depth-sort keys (ping-pong)
    uint32_t* vals[2];           // [P]x2 Gaussian ids   (ping-pong); vals[0] = depth order (4 passes: even)
    uint2* rect_sorted;          // [P]   tile rectangles in depth order (written by the scan)
    uint32_t* offsets;           // [P]   inclusive scan of tiles_touched in depth order
    uint64_t* block_sums;        // [ceil(P/GSR_SCAN_ITEMS)]
    uint2* block_first;          // [gsr_block_first_cap(P)] per 4096-instance block: (depth-order index of its first Gaussian, instances before it)
    uint32_t* sort_hist;         // [512 * nblocks_small(P)] radix block histograms (LSD depth sort)
    uint32_t* digit_total;       // [512]
    GsrDepthSortBufs ds;         // bucket depth sort (depthsort.hip); carved for P <= GSR_DS_MAX_P
    uint32_t* num_rendered;      // frame words (gsr_frame.h): [0..1] R as 64 bits, [2] smallest, [3] largest depth key of a listed Gaussian
    uint2* wg_range;             // [GSR_FRAME_MAX_GROUPS] per-workgroup depth-key ranges of the key-producing kernel
    size_t bytes;
};
GsrGeom gsr_carve_geom(char* base, int P);

// ---- depth-sort keys (round 3): 27 bits instead of 32 -> 3 radix passes of 9 bits instead of 4 of 8 ----
// Every listed Gaussian passed the near cull view.z > 0.2 (Appendix A.2 step 1), and positive fp32 bit patterns order like the
// floats, so key = bits(depth) - bits(0.2f) >= 1 orders the listed Gaussians exactly like bits(depth).  27 bits cover
// 16 octaves: depths below 0.2 * 2^16 = 13 107.  A deeper Gaussian sets *key_overflow (a mapped host word); the host then
// re-keys with the full 32 bits and repeats the depth sort with 4 passes (gsr_api.cpp) -- bit-identical order either way.
// Gaussians without a tile in the band sort last (key = 2^27 - 1; stable sort: among themselves in index order).
#define GSR_DEPTH_KEY_BITS 27
#define GSR_DEPTH_KEY_BASE 0x3E4CCCCDu
#define GSR_DEPTH_KEY_CULLED ((1u << GSR_DEPTH_KEY_BITS) - 1u)
static_assert((1 << (GSR_DEPTH_KEY_BITS - GSR_EQ_SHIFT)) == GSR_EQ_BINS && (1 << (GSR_EQ_SHIFT - GSR_EQ_SHIFT2)) == GSR_EQ_BINS, "equalised bucket tables");
#ifdef __HIPCC__
// `overflow` is a per-thread flag the caller reports ONCE, after its loop, through gsr_frame_stats_commit: a store through an
// (unrestricted) host-word pointer inside the streaming loop made hipcc serialise the loop's batched loads (ISA audit: the
// split-SH loader of the preprocess became a 14-long load -> wait chain).
__device__ __forceinline__ uint32_t gsr_depth_key(float depth, bool listed, bool& overflow) {
    if (!listed) return GSR_DEPTH_KEY_CULLED;
    uint32_t k = __float_as_uint(depth) - GSR_DEPTH_KEY_BASE;
    if (k >= GSR_DEPTH_KEY_CULLED) {
        overflow = true;
        k = GSR_DEPTH_KEY_CULLED - 1u;
    }
    return k;
}
// the two derived fields of a splat record, written by the preprocess and recomputed bit-identically from (opacity, depth) by the
// receiver of a packed record (route.hip): tau = gsr_tau(opacity) (gsr_math.h) and 1 / depth, an explicit single rounding
__device__ __forceinline__ float gsr_inv_depth(float depth) { return __fdiv_rn(1.0f, depth); }
#endif

struct GsrBinning {              // R-sized
    // > 65536 tiles (LSD sort, sort.hip): keys[2] tile ids / vals[2] Gaussian ids, ping-pong; list = vals[passes & 1]
    // <= 65536 tiles (fused emission + two-level sort, tilesort.hip): words = keys[0] (8R bytes, contiguous with
    //   keys[1]) holds the packed level-1 output, vals[0] the final point_list
    uint32_t* keys[2];
    uint32_t* vals[2];
    uint32_t* sort_hist;         // LSD: [256 * nblocks_small(R)]; fused: level-1 table [nb1 * nblk]
    uint32_t* hist2;             // fused: level-2 table [(nblk + 256) * 256]
    uint32_t* digit_total;       // [256]
    uint32_t* bucket_base;       // [257]
    uint32_t* blk2_start;        // [257]
    uint32_t* tile_base;         // [65536]
    uint2* block_first;          // [ceil(R / GSR_TS_ITEMS) + 2]  (fallback table, see gsr_block_first_cap)
    uint32_t* meta;
    size_t bytes;
};
GsrBinning gsr_carve_binning(char* base, int64_t R);

struct GsrImage {
    float* final_T;              // [H*W]
    uint32_t* n_contrib;         // [H*W]
    uint2* ranges;               // [n_tiles]
    uint32_t* block_steps;       // [n_tiles*4] list entries the forward blended per 8x8 block (tracking build): the backward's work estimate
    uint32_t* tile_order;        // [n_tiles]   band-local tile indices, heaviest first (written by the backward's plan kernel)
    size_t bytes;
};
GsrImage gsr_carve_image(char* base, int W, int H);

// ---- what a finished tracking forward leaves in the three buffers for the calls that read it back (blend backward, contribution statistics, pixel
// probe, feature render, gsr_forward_views): filled in ONE place, saved_frame() of gsr_api.cpp, which alone knows which ping-pong buffers hold the
// sorted list and the depth order.  Host side only: launchers unpack it at the launch, no kernel takes it.
struct GsrSavedFrame {
    const uint2* ranges;            // [n_tiles]
    const uint32_t* point_list;     // [R] Gaussian ids, tile by tile, front to back (NULL without a binning buffer or with R <= 0)
    const float4* splats;           // [4P]
    const float* final_T;           // [H*W]
    const uint32_t* n_contrib;      // [H*W]
    const uint32_t* block_steps;    // [n_tiles*4]
    uint32_t* tile_order;           // [n_tiles*2] scratch of the backward's plan kernel (the one entry a reader writes)
    const uint32_t* order;          // [P] the depth order
    const uint32_t* offsets;        // [P] the tile scan: inclusive scan of tiles_touched in depth order
    const uint32_t* tiles;          // [P] tiles_touched (shown by gsr_forward_views; no kernel reads it back)
};

// the band's pixel rows [row0, row1) are one contiguous range of every [H,W] array: `pixels` pixels from pixel `first` on
struct GsrBandRows { int row0, row1; size_t first, pixels; };
static inline GsrBandRows gsr_band_rows(const GsrCamDev& cam) {
    const int t0 = cam.tile_y0 * GSR_TILE, t1 = cam.tile_y1 * GSR_TILE;
    GsrBandRows b;
    b.row0 = t0 < cam.H ? t0 : cam.H;
    b.row1 = t1 < cam.H ? t1 : cam.H;
    b.first = (size_t)b.row0 * cam.W;
    b.pixels = b.row1 > b.row0 ? (size_t)(b.row1 - b.row0) * cam.W : 0;
    return b;
}

// the band's tiles, and the launch groups that cover n of them (8 tiles per group: a wave per 8x8 block, 32 to a group; 16: a wave per half tile)
static inline int gsr_band_tiles(const GsrCamDev& cam) { return cam.gx * (cam.tile_y1 - cam.tile_y0); }
static inline int gsr_tile_groups(int n_tiles, int tiles_per_group) { return (n_tiles + tiles_per_group - 1) / tiles_per_group; }

// ---- kernel launchers (one per translation unit) ----
// preprocess.hip  (compiled with -ffp-contract=off)
// (the key-producing launchers return their grid size: the number of entries of fs.wg_range they fill)
int gsr_launch_preprocess(const GsrCamDev& cam, int P, const float* means3D, const float* shs,
                          const float* colors_precomp, const float* opacities, const float* scales,
                          const float* rotations, const float* cov3D_precomp, GsrGeom g, int32_t* radii,
                          const GsrFrameStatsDev& fs, hipStream_t st);
void gsr_launch_preprocess_backward(const GsrCamDev& cam, int P, const float* means3D, const float* shs,
                                    const float* colors_precomp, const float* opacities, const float* scales,
                                    const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                    GsrGeom g, const float* splat_grads /*[P,12]*/, float* dL_dmeans2D,
                                    float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D,
                                    float* dL_dsh, float* dL_dscales, float* dL_drotations, hipStream_t st,
                                    const struct GsrCamGradDev* camg = nullptr);
// camera gradients (gsr_backward_preprocess_camera): with `camg` the launcher runs the kernel's CAM instantiation, which also writes
// per-workgroup fp64 partial sums [27][grid] into `partials`, and a one-workgroup kernel that sums them into the three fp32 outputs
struct GsrCamGradDev {
    double* partials;      // gsr_camera_grad_rows(P) * 27 doubles
    float* dview;          // [16]
    float* dproj;          // [16]
    float* dcampos;        // [3]
};
#define GSR_CAM_MAX_ROWS 1024
size_t gsr_camera_grad_rows(int P);      // workgroups of the CAM launch at most: ceil(P / 256) capped at GSR_CAM_MAX_ROWS
// the same kernel, but the SH gradient of the split form is not written: the Adam update of the two SH tensors is applied in
// place from the gradient tile (gsr_backward_preprocess_sh_adam); dense: every row, sparse: rows with radii > 0
struct GsrShAdamDev {
    float* dc;  float* dc_m;  float* dc_v;            // [P,1,3]
    float* rest; float* rest_m; float* rest_v;        // [P,15,3]
    // dense (torch.optim.Adam): om_b1, b2, om_b2, step_size, inv_bc2_sqrt, eps;  sparse: lr, b1, om_b1, b2, om_b2, eps
    float dc_a[6], rest_a[6];
    int sparse;
};
void gsr_launch_preprocess_backward_sh_adam(const GsrCamDev& cam, int P, const float* means3D, const float* opacities,
                                            const float* scales, const float* rotations, const float* cov3D_precomp,
                                            const int32_t* radii, GsrGeom g, const float* splat_grads, float* dL_dmeans2D,
                                            float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dscales,
                                            float* dL_drotations, const GsrShAdamDev& adam, hipStream_t st);
void gsr_set_preprocess_grid_cap(int cap);      // tuning knob (option preprocess_grid_cap)
void gsr_set_preprocess_generic(int on);        // A/B switch (option preprocess_generic): 1 = the forward always runs its generic instantiation
void gsr_set_preprocess_hot_grid(int groups);   // tuning knob (option preprocess_hot_grid): workgroups of the hot forward instantiations, 0 = from the occupancy
int gsr_preprocess_last_path(void);             // the most recent gsr_launch_preprocess: 1 = generic instantiation, 2 = hot (0: none yet)
void gsr_launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t st);

// sort.hip: LSD radix sort of (u32 key, u32 value) pairs on bits [0, nbits); returns the index (0/1) of the
// ping-pong buffer that holds the result.  n is known on the host.  items = keys per workgroup: 1024, 2048 or 4096
// (hist must hold 2^digit_bits * ceil(n / items) counters).
// rect / rect_sorted (optional): the last pass also writes rect_sorted[pos] = rect[value] (depth sort: the tile rectangles
// in depth order, which the scan and the emission stream afterwards)
int gsr_radix_sort_pairs(uint32_t* keys[2], uint32_t* vals[2], int64_t n, int nbits, int max_digit_bits, uint32_t* hist,
                         uint32_t* digit_total, int items, hipStream_t st, const uint2* rect = nullptr, uint2* rect_sorted = nullptr);
int gsr_radix_sort_pairs_k16(uint16_t* keys[2], uint32_t* vals[2], int64_t n, int nbits, int max_digit_bits, uint32_t* hist,
                             uint32_t* digit_total, int items, hipStream_t st);
// depthsort.hip: depth order + rectangles in depth order + inclusive scan of the tile counts + the emission's block table
void gsr_launch_depth_bucket_sort(int P, const uint32_t* keys, const uint32_t* tiles, const uint2* rect, uint32_t* frame,
                                  const uint2* wg_range, int n_range, const GsrDepthSortBufs& b, uint32_t* order, uint2* rect_sorted,
                                  uint32_t* offsets, uint2* block_first, uint32_t block_first_cap, uint32_t* slow_word, hipStream_t st);
// pass plan shared by the sorter and by code that must know which ping-pong buffer holds the result
int gsr_sort_plan(int nbits, int max_digit_bits, int* pass_bits /*[8]*/);
#define GSR_DEPTH_DIGIT_BITS 9      // 27-bit depth keys: 3 passes of 9 bits (round 2: 4 x 8 on 32 bits; 3 x 11 measured slower: 113 vs 91 us)
#define GSR_SORT_MAX_DIGITS 512     // table rows (digit values) the geometry buffer provides for the depth sort
#define GSR_TILE_DIGIT_BITS 8       // tile ids: ceil(bits/8) passes of equal width
static inline int64_t gsr_sort_blocks(int64_t n, bool small_blocks) {
    const int64_t items = small_blocks ? GSR_SORT_ITEMS_SMALL : GSR_SORT_ITEMS;
    return (n + items - 1) / items;
}

// binning.hip: scan of tiles_touched in depth order, instance emission, tile ranges
// host_word (mapped pinned, may be NULL): [0] = R low word, [2] = R high word, [1] = seq (stored last)
void gsr_launch_scan_tiles(int P, const uint32_t* order, const uint2* rect, uint2* rect_sorted /*[P]*/, uint32_t* offsets,
                           uint64_t* block_sums, uint2* block_first, uint32_t block_first_cap, uint32_t* num_rendered,
                           uint32_t* host_word, uint32_t seq, bool rect_already_sorted, hipStream_t st);
// legacy emission (frames with more than 65536 tiles): 32-bit tile ids
void gsr_launch_emit(int P, int gx, const uint32_t* order, const uint32_t* offsets, const uint2* rect_sorted,
                     void* inst_keys, bool key16, uint32_t* inst_vals, float4* splats /*NULL: skip the goffset write*/,
                     hipStream_t st);

// tilesort.hip: fused emission + two-level stable tile sort + ranges (frames with <= 65536 tiles)
struct GsrTileSortPlan { bool fused; int lb, hb; bool word64; };
void gsr_tile_sort_plan(int n_tiles, int P, GsrTileSortPlan* plan);
void gsr_launch_fill_block_first(int P, const uint32_t* offsets, uint2* block_first, uint32_t cap, hipStream_t st);
void gsr_launch_tile_sort_level1(const GsrTileSortPlan& plan, int64_t R, int gx, const uint2* block_first,
                                 const uint32_t* offsets, const uint2* rect_sorted, const uint32_t* order, void* words,
                                 uint32_t* hist1, uint32_t* digit_total, uint32_t* bucket_base, uint32_t* blk2_start,
                                 float4* splats /*NULL: inference*/, hipStream_t st);
void gsr_launch_tile_sort_level2(const GsrTileSortPlan& plan, int64_t R, int n_tiles, const void* words, uint32_t* point_list,
                                 const uint32_t* bucket_base, const uint32_t* blk2_start, uint32_t* hist2, uint32_t* tile_base,
                                 uint2* ranges, hipStream_t st, int h0 = 0, int h1 = 0 /*level-1 buckets [h0, h1) of a band; (0, 0) = all*/);
void gsr_set_level2_scan_mode(int v);      // tilesort.hip (option level2_scan_mode)
// option ranking_generic: 1 = the ranking kernels of tilesort.hip and depthsort.hip in their run-time-digit-width forms only (A/B, tests; ds_scatter has one form).  Defined here
// (C++17 inline variable): either file is also compiled on its own (tests/simt).
inline int g_ranking_generic = 0;
inline void gsr_set_ranking_generic(int v) { g_ranking_generic = v; }
// option ranking_pad_last: 1 (default) = emit_scatter / bucket_scatter rank the slots a partial block does not have as padding items of the highest digit,
// 0 = they carry a validity predicate per item (the earlier form; A/B, tests).  tilesort.hip local_stable_sort
inline int g_ranking_pad_last = 1;
inline void gsr_set_ranking_pad_last(int v) { g_ranking_pad_last = v; }
// TEST HOOK (option debug_last_ranking_widths): the digit widths the most recent emit_scatter / bucket_scatter launches were instantiated for (0: generic, -1: none yet)
inline int g_ranking_last_hb = -1, g_ranking_last_lb = -1;
// sort.hip: in-place exclusive scan of every digit row of a [ndigits][nblocks] block-histogram table + row totals
void gsr_launch_rs_scan(uint32_t* block_hist, int nblocks, int ndigits, uint32_t* digit_total, hipStream_t st);
void gsr_launch_ranges(int64_t R, int n_tiles, const void* sorted_keys, bool key16, uint2* ranges, bool already_zeroed,
                       hipStream_t st);

// render_fwd.hip / render_bwd.hip
// ---- measurement block of the blend kernels (device memory, allocated by gsr_profile_enable only) -------------------------------------
// [0..5] work counters (include/gsr.h), [6] mode: 0 = counters (atomics at the end of every wave), 1 = per-wave trace, [8 + 4 w ..] trace
// entry of wave w: start, end (s_memrealtime), placement | kernel << 40, steps.
#define GSR_TRACE_MODE_WORD 6
#define GSR_TRACE_BASE 8
#define GSR_MEASURE_WORDS (GSR_TRACE_BASE + 4 * (size_t)GSR_TRACE_WAVES)
#ifdef __HIPCC__
__device__ __forceinline__ bool gsr_trace_mode(const unsigned long long* counters) {
    return __builtin_nontemporal_load(counters + GSR_TRACE_MODE_WORD) != 0ull;
}
// steps: bits 0-15 blend steps; in trace mode the kernels also pack the time (10 ns ticks, saturating at 65535) they spent walking survivors
// (bits 16-31), getting batches ready -- waiting for the gathered records, box tests, staging -- (bits 32-47) and storing (bits 48-63)
__device__ __forceinline__ unsigned long long gsr_trace_pack(uint32_t steps, unsigned long long walk, unsigned long long prep, unsigned long long store) {
    auto sat = [](unsigned long long v) { return v > 65535ull ? 65535ull : v; };
    return (unsigned long long)(steps > 65535u ? 65535u : steps) | (sat(walk) << 16) | (sat(prep) << 32) | (sat(store) << 48);
}
__device__ __forceinline__ void gsr_trace_wave(unsigned long long* counters, unsigned long long t0, uint32_t wave, uint32_t kernel, unsigned long long steps) {
    if (wave >= (uint32_t)GSR_TRACE_WAVES) return;
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);         // HW_REG_HW_ID: wave [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]
    const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);        // HW_REG_XCC_ID [3:0]
    unsigned long long* e = counters + GSR_TRACE_BASE + (size_t)wave * 4;
    e[0] = t0;
    e[1] = wall_clock64();
    e[2] = (unsigned long long)hw | ((unsigned long long)(xcc & 15u) << 32) | ((unsigned long long)kernel << 40);
    e[3] = steps;
}
#endif

// optional inputs / outputs of the two blend kernels beyond the reference's contract (gsr_rasterize_forward_composite /
// gsr_backward_blend_composite): every pointer may be NULL, and all NULL is the plain call
struct GsrCompositeDev {
    float* out_alpha;            // forward: [H*W] 1 - final_T
    const float* bg_image;       // both: [3,H*W] per-pixel background instead of cam.bg
    const float* dL_dalpha;      // backward: [H*W] gradient of the alpha image
};
void gsr_launch_render_forward(const GsrCamDev& cam, const uint2* ranges, const uint32_t* point_list,
                               const float4* splats, float* final_T, uint32_t* n_contrib, uint32_t* block_steps /*NULL unless tracking*/,
                               float* out_color, float* out_invdepth, int variant,
                               unsigned long long* counters /*NULL or [4] work counters*/, hipStream_t st,
                               int tile_off = 0, int tile_cnt = -1 /*the launch blends tiles [tile_off, tile_off + tile_cnt) of the band (multiple of 8; -1 = all)*/,
                               const GsrCompositeDev* comp = nullptr);
void gsr_set_render_fwd_lds_pad(int bytes);      // render_fwd.hip (tuning option render_fwd_lds_pad)
// variant: 0 = default (independent quadrant waves); 1 (global atomics) and 4 (round 1's workgroup-per-tile kernel) exist
// only in builds with -DGSR_AB_VARIANTS
int gsr_render_backward_variant_available(int variant);
int gsr_render_forward_variant_available(int variant);
// Two launchers keep their pointer lists, this one and gsr_launch_reduce_instances: tests/simt/forward_harness.cpp drives both with vectors of its own
// (no carved buffers) and, as the frozen harness of the kernel-source tests, is compiled unchanged against this header.  backward_blend unpacks its
// GsrSavedFrame at these two calls; every other reader takes the view.
void gsr_launch_render_backward(const GsrCamDev& cam, const uint2* ranges, const uint32_t* point_list,
                                const float4* splats, const float* final_T, const uint32_t* n_contrib,
                                const uint32_t* block_steps, uint32_t* tile_order /*NULL: tiles in index order*/,
                                const float* dL_dpix, const float* dL_dinvdepth, float* splat_grads /*[P,12] variant 1*/,
                                float* inst_grads /*[4][R,12]*/, uint32_t* inst_flag /*[R]*/, int64_t R, int variant,
                                int order_mode /*plan kernel: 1 tiles by the sum of their blocks, 2 tiles by their heaviest half, 3 half tiles (waves)*/,
                                unsigned long long* counters, hipStream_t st);
// the same with the optional per-pixel background / alpha-image gradient of gsr_backward_blend_composite (comp may be NULL: the plain call)
void gsr_launch_render_backward_composite(const GsrCamDev& cam, const GsrSavedFrame& f /*tile_order NULL: tiles in index order*/,
                                          const float* dL_dpix, const float* dL_dinvdepth, float* splat_grads, float* inst_grads,
                                          uint32_t* inst_flag, int64_t R, int variant, int order_mode, unsigned long long* counters,
                                          hipStream_t st, const GsrCompositeDev* comp);
// the walk's ABS instantiations (gsr_backward_blend_abs): the same launch (plan kernel, flags, order) with words 10, 11 of every instance record
// carrying the two absolute sums of absgrad.hip; default kernel only (no measurement-build variant)
void gsr_launch_render_backward_abs(const GsrCamDev& cam, const GsrSavedFrame& f, const float* dL_dpix, const float* dL_dinvdepth,
                                    float* inst_grads, uint32_t* inst_flag, int64_t R, int order_mode,
                                    unsigned long long* counters, hipStream_t st, const GsrCompositeDev* comp);
// absgrad.hip: words 10, 11 of splat_grads[g] <- the sum of words 10, 11 of g's flagged instance records (after gsr_launch_reduce_instances, same
// stream); means2D_abs[P,3] = (0.5 W word 10, 0.5 H word 11, 0)
void gsr_launch_absgrad_reduce(int P, int64_t R, const GsrSavedFrame& f, const float* inst_grads, const uint32_t* inst_flag, float* splat_grads,
                               hipStream_t st);
void gsr_launch_absgrad_from_records(int P, int W, int H, const float* splat_grads, float* means2D_abs, hipStream_t st);
// background gradient (render_bwd.hip): dL_dbg_image[c][p] = T(p) * dL_dpix[c][p] and / or dL_dbg[c] = sum over p, with T = final_T inside the
// band's pixel rows [row0, row1) (1 where final_T is NULL: no Gaussian at all) and 0 outside.  partials: gsr_bg_grad_blocks(W * H) * 3 doubles.
#define GSR_BG_GRAD_PIXELS 2048      // pixels per workgroup (256 threads x 8)
static inline size_t gsr_bg_grad_blocks(int64_t npix) { return (size_t)((npix + GSR_BG_GRAD_PIXELS - 1) / GSR_BG_GRAD_PIXELS); }
void gsr_launch_bg_grad(int64_t npix, int W, int row0, int row1, const float* final_T, const float* dL_dpix, float* dL_dbg_image,
                        float* dL_dbg, double* partials, hipStream_t st);
// Clears the flag words of the R instances and, given block_steps and tile_order (both non-NULL), sorts the band's tiles (order_mode 1, 2) or half
// tiles (3) by the forward's step counts, heaviest first, into tile_order in the same launch.  Returns whether tile_order was written.
bool gsr_launch_bwd_plan(const GsrCamDev& cam, const uint32_t* block_steps, uint32_t* tile_order, uint32_t* inst_flag, int64_t R, int order_mode,
                         hipStream_t st);
size_t gsr_reduce_units(int64_t R);      // units of 1024 instance records the reduce works in
void gsr_launch_reduce_instances(int P, int64_t R, const uint32_t* order, const uint32_t* offsets, const float4* splats,
                                 const float* inst_grads, const uint32_t* inst_flag, float* splat_grads, uint2* unit_first,
                                 float* unit_piece, hipStream_t st);

// backward scratch (caller-owned, gsr_backward_scratch_bytes): per-Gaussian record, per-instance records, maps
// record slots per instance: one per 16x8 half tile (the measurement build's per-quadrant kernel needs four)
#ifdef GSR_AB_VARIANTS
#define GSR_BWD_SLOTS 4
#else
#define GSR_BWD_SLOTS 2
#endif
struct GsrBwdScratch {
    float* splat_grads;     // [P,12]
    float* inst_grads;      // [GSR_BWD_SLOTS][R,12]  one record slot per (half tile, instance), slot-major
    uint32_t* inst_flag;    // [R]  byte q != 0: slot q of the instance has a record
    uint2* unit_first;      // [units]  reduce: (owner of the unit's first record, that owner's first record)
    float* unit_piece;      // [units][2][12]  reduce: head / tail partial rows of every unit
    size_t bytes;
};
GsrBwdScratch gsr_carve_bwd(char* base, int P, int64_t R);

// contrib.hip: per-Gaussian blend-weight statistics (gsr_contribution_stats).  Scratch (caller-owned, gsr_contribution_scratch_bytes): one
// 16-byte record slot per (8x8 block of the tile, instance), slot-major, and a flag word per instance -- 68 R bytes, so every offset is 64-bit
struct GsrContribScratch {
    float4* slots;          // [4][R]  (sum, max, count bits, -) of the block's pixels
    uint32_t* flags;        // [R]     byte q != 0: slot q of the instance has a record
    size_t bytes;
};
GsrContribScratch gsr_carve_slots(char* base, int64_t R, int nb /*float4 per slot record*/);      // contrib.hip; the one carve of this shape
static inline GsrContribScratch gsr_carve_contrib(char* base, int64_t R) { return gsr_carve_slots(base, R, 1); }
void gsr_launch_contribution_stats(const GsrCamDev& cam, int P, int64_t R, const GsrSavedFrame& f, const float* pixel_weight /*[H*W] or NULL*/,
                                   const GsrContribScratch& w, float* weight_sum, float* weight_max, int32_t* pixel_count /*each [P] or NULL*/,
                                   int accumulate, hipStream_t st);

// probe.hip: per-pixel probe (gsr_pixel_probe).  No scratch.  The kernel writes every in-band, in-image pixel of the non-NULL arrays, the defaults
// included; _defaults fills the band's rows without reading any state (the call with P == 0 or num_rendered == 0).
void gsr_launch_pixel_probe(const GsrCamDev& cam, const GsrSavedFrame& f, const GsrPixelProbeOut& out, hipStream_t st);
void gsr_launch_pixel_probe_defaults(const GsrCamDev& cam, const GsrPixelProbeOut& out, hipStream_t st);

// features.hip: N-channel per-Gaussian features blended with a finished forward's weights (gsr_render_features / _backward).  The forward writes every
// in-band, in-image pixel of out[C,H,W], zeros included; _defaults fills the band's rows of every plane without reading any state (the call with P == 0
// or num_rendered == 0).  The backward's scratch has contrib.hip's shape (GsrContribScratch, gsr_carve_feature_grad: one slot record per (8x8 block of the
// tile, instance) holding the channel sums of one group, slot-major, and a flag word per instance; 64-bit offsets), reused by every channel group of a
// call; rows of dL_dfeatures[P,C] of Gaussians without instances are not touched (the caller zeroes the array).
GsrContribScratch gsr_carve_feature_grad(char* base, int64_t R, int C);
void gsr_launch_render_features(const GsrCamDev& cam, const GsrSavedFrame& f, const float* features, int C, float* out, hipStream_t st);
void gsr_launch_render_features_defaults(const GsrCamDev& cam, int C, float* out, hipStream_t st);
void gsr_launch_render_features_backward(const GsrCamDev& cam, int P, int64_t R, const GsrSavedFrame& f, const float* dL_dout, int C,
                                         const GsrContribScratch& w, float* dL_dfeatures, hipStream_t st);
// feature_geom.hip: the walks of gsr_render_features_backward_geometry, one per channel group on the stream.  They clear the flag words of the R
// instances and leave the blend backward's instance records (words 0..5: the five moments and the zeroth moment; 6..11 zero) in inst_grads / inst_flag
// of a GsrBwdScratch; gsr_launch_reduce_instances on the same stream turns them into the [P,12] rows.  R > 0.
void gsr_launch_feature_geometry_walks(const GsrCamDev& cam, int64_t R, const GsrSavedFrame& f, int order_mode /*the blend backward's: 0 = index order*/,
                                       const float* features, const float* dL_dout, int C, float* inst_grads, uint32_t* inst_flag, hipStream_t st);
// distortion.hip: the distortion loss on a saved frame (gsr_distortion / gsr_distortion_backward).  The forward writes every in-band, in-image pixel of
// distortion[H,W] and, unless NULL, of the two planes of saved[2,H,W], zeros included; _defaults fills the band's rows without reading any state (the
// call with P == 0 or num_rendered == 0).  The walk clears the flag words of the R instances and leaves the blend backward's instance records (words 0..5
// and 9; 6, 7, 8, 10, 11 zero) in inst_grads / inst_flag of a GsrBwdScratch for gsr_launch_reduce_instances on the same stream.  R > 0.
void gsr_launch_distortion(const GsrCamDev& cam, const GsrSavedFrame& f, float* distortion, float* saved /*NULL: not wanted*/, int depth_mode,
                           hipStream_t st);
void gsr_launch_distortion_defaults(const GsrCamDev& cam, float* distortion, float* saved, hipStream_t st);
void gsr_launch_distortion_walk(const GsrCamDev& cam, int64_t R, const GsrSavedFrame& f, int order_mode /*the blend backward's: 0 = index order*/,
                                const float* dL_ddistortion, const float* saved, int depth_mode, float* inst_grads, uint32_t* inst_flag, hipStream_t st);

// adam.hip
void gsr_launch_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                     int step, hipStream_t st);

// ssim.hip
void gsr_launch_ssim_forward(int planes, int H, int W, const float* img1, const float* img2, float* ssim_map, float* dm_dmu1,
                             float* dm_dex2, float* dm_dexy, hipStream_t st);
void gsr_launch_ssim_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmap,
                              const float* dm_dmu1, const float* dm_dex2, const float* dm_dexy, float* dL_dimg1, hipStream_t st);

// adam.hip: sparse step (rows of M elements, skipped entirely when visible[row] == 0)
void gsr_launch_adam_multi(const GsrAdamTensor* tensors, int count /*<= GSR_ADAM_MAX_TENSORS*/, hipStream_t st);
void gsr_launch_sparse_adam_multi(const GsrSparseAdamTensor* tensors, int count, const uint8_t* visible, int64_t N, double beta1, double beta2,
                                  hipStream_t st);
void gsr_launch_sparse_adam(float* p, const float* g, float* m, float* v, const uint8_t* visible, int64_t N, int64_t M,
                            double lr, double beta1, double beta2, double eps, hipStream_t st);
// density.hip: per-iteration density-control statistics
void gsr_launch_density_stats(int P, const float* grad, const uint8_t* visible, const int32_t* radii, float* accum, float* denom,
                              float* max_radii, hipStream_t st);
// mcmc.hip: 3DGS-MCMC density control -- the per-iteration noise on the means (in place; rows whose displacement is not finite are left alone)
// and the opacity / scale correction of relocated Gaussians (fp64 inside)
void gsr_launch_mcmc_noise(int P, float* xyz, const float* scales, const float* rot, const float* opac, const float* noise, int activated,
                           float noise_scale, float gate_k, float gate_x0, hipStream_t st);
void gsr_launch_mcmc_relocation(int n, const float* opac, const float* scales, const int32_t* ratios, float* new_opac, float* new_scales,
                                hipStream_t st);
// bilagrid.hip: bilateral-grid appearance model.  The plan is the one place that maps pixels to xy cells and cells to workgroups:
// the host sizes the scratch with it and the kernels take it by value.
#define GSR_BILAGRID_MAX 64             // largest grid size per axis (the kernels' LDS is sized for it)
#define GSR_BILAGRID_MAX_IMAGE (1 << 23)
struct GsrBilagridAxis { float gm1, inv; int n, size; };      // grid points - 1, 1 / pixels (both as the fp32 factors of the coordinate), grid points, pixels
struct GsrBilagridPlan {
    GsrBilagridAxis ax, ay;
    int L;
    int twl, tw, steps, th;             // tile: tw = 2^twl columns, th = steps * 4 * (64 / tw) rows
    int maxchunks, ncells;              // tile slots per cell (the largest cell's tiles), (Gw - 1) (Gh - 1)
};
void gsr_bilagrid_plan(int H, int W, int L, int Gh, int Gw, GsrBilagridPlan* out);
static inline size_t gsr_bilagrid_scratch_floats(const GsrBilagridPlan& p) { return (size_t)p.ncells * p.maxchunks * 48 * p.L; }
void gsr_launch_bilagrid_slice(const GsrBilagridPlan& p, const float* grid, const float* image, float* out, hipStream_t st);
// dL_dimage may be NULL; scratch: gsr_bilagrid_scratch_floats(p) floats; every element of dL_dgrid is written
void gsr_launch_bilagrid_slice_backward(const GsrBilagridPlan& p, const float* grid, const float* image, const float* dL_dout, float* dL_dgrid,
                                        float* dL_dimage, float* scratch, hipStream_t st);
int64_t gsr_bilagrid_tv_partial_count_impl(int N, int L, int Gh, int Gw);
void gsr_launch_bilagrid_tv(int N, int L, int Gh, int Gw, const float* grids, double* partials, float* tv_out, hipStream_t st);
void gsr_launch_bilagrid_tv_backward(int N, int L, int Gh, int Gw, const float* grids, const float* dL_dtv, float* dL_dgrids, hipStream_t st);
// normals.hip: per-Gaussian normals, normals of a depth map and the fused normal-consistency loss.  The frame record holds the
// fp32 constants of the pixel -> ray map, rounded once on the host from fp64, and the tile grid (64 x 16 pixels per workgroup): the host sizes
// the loss partials with it and the kernels take it by value.
struct GsrNormalsFrame {
    int H, W, tiles_x, tiles_y;
    float tx, ty;                 // tanfovx, tanfovy
    float inv_w, inv_h;           // 1 / W, 1 / H
    float alpha, beta, ab;        // tanfovy 2 / H, tanfovx 2 / W, their product
    float inv_hw;                 // 1 / (H W)
};
void gsr_normals_frame(int H, int W, float tanfovx, float tanfovy, GsrNormalsFrame* out);
static inline int gsr_normals_tiles(const GsrNormalsFrame& f) { return f.tiles_x * f.tiles_y; }
void gsr_launch_gaussian_normals(int P, const float* scales, const float* rot, const float* means, const float* vm, float* out, hipStream_t st);
void gsr_launch_gaussian_normals_backward(int P, const float* scales, const float* rot, const float* means, const float* vm, const float* dn,
                                          float* drot, hipStream_t st);
void gsr_launch_depth_normals(const GsrNormalsFrame& f, const float* depth, float* out, hipStream_t st);
void gsr_launch_depth_normals_backward(const GsrNormalsFrame& f, const float* depth, const float* dL_dnormals, float* dL_ddepth, hipStream_t st);
// weight may be NULL; partials: gsr_normals_tiles(f) doubles
void gsr_launch_normal_loss(const GsrNormalsFrame& f, const float* depth, const float* normals, const float* weight, double* partials,
                            float* loss_out, hipStream_t st);
// dL_dnormals or dL_ddepth may be NULL (both: no launch); each is the same bits whether or not the other is asked for
void gsr_launch_normal_loss_backward(const GsrNormalsFrame& f, const float* depth, const float* normals, const float* weight,
                                     const float* dL_dloss, float* dL_dnormals, float* dL_ddepth, hipStream_t st);
// mip.hip: the 3D smoothing filter of Mip-Splatting.  The sweep leaves the largest seen distance and the largest focal length in
// the two scratch words (cleared on the stream first), the fill kernel behind it turns distances into filter sizes; the activations are one
// streaming pass each way.  dL_dscales / dL_dopacity may be NULL (a zero gradient, same arithmetic).
#define GSR_MIP_SCRATCH_BYTES 64
void gsr_launch_mip_filter(int P, const float* means, int C, const float* cameras /*[C,16]*/, float* filter, uint8_t* seen /*or NULL*/,
                           uint32_t* words /*[2]*/, hipStream_t st);
void gsr_launch_mip_activations(int P, const float* raw_scales, const float* raw_opacity, const float* filter, float* scales_out,
                                float* opacity_out, hipStream_t st);
void gsr_launch_mip_activations_backward(int P, const float* raw_scales, const float* raw_opacity, const float* filter, const float* dL_dscales,
                                         const float* dL_dopacity, float* dL_draw_scales, float* dL_draw_opacity, hipStream_t st);
// vq.hip: vector quantisation.  One scratch layout serves both steps: the assignment's centroid norms and LDS images, the
// update's sort buffers, segment tables and per-chunk fp64 partial sums.  weights may be NULL (1).
#define GSR_VQ_MAX_D 64
#define GSR_VQ_MAX_K 65536
size_t gsr_vq_scratch_bytes_impl(int P, int D, int K);
void gsr_launch_vq_assign(int P, int D, int K, const float* rows, const float* codebook, int32_t* idx, float* dist2, void* scratch, hipStream_t st);
void gsr_launch_vq_update(int P, int D, int K, const float* rows, const float* weights, const int32_t* idx, float* codebook, float* mass,
                          void* scratch, hipStream_t st);
// tsdf.hip: TSDF fusion and marching tetrahedra.  The integrate is one kernel over all views; the extraction leaves per-voxel
// class, vertex mask and in-workgroup prefixes in the scratch at the count and reads them back at the emit (rs_scan of sort.hip in between).
#define GSR_MESH_MAX_VOXELS 178956970      // 12 faces per cell stay below 2^31
size_t gsr_mesh_scratch_bytes_impl(int nx, int ny, int nz);
void gsr_launch_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float sdf_trunc, float near_z, int V,
                               const float* cameras /*[V,16]*/, int H, int W, const float* depth, const float* color /*or NULL*/, float* tsdf,
                               float* weight, float* rgb /*or NULL*/, hipStream_t st);
void gsr_launch_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float min_weight, void* scratch, int32_t* counts_out,
                           hipStream_t st);
void gsr_launch_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf, const float* rgb /*or NULL*/,
                          void* scratch, int nv, int nf, float* vertices, float* colors /*or NULL*/, int32_t* faces, hipStream_t st);
// meshops.hip: clean-up of an indexed mesh.  One scratch layout serves the five operations.  The components launcher runs its rounds
// of hook + compress, reads one device word per round and synchronises the stream: 0 = done, 1 = the round cap was reached, -1 = a HIP call failed.
size_t gsr_meshops_scratch_bytes_impl(int nv, int nf);
int gsr_meshops_round_cap(int nv);      // 2 ceil(log2(nv + 1)) + 8
int gsr_launch_mesh_components(int nv, int nf, const int32_t* faces, int32_t* vertex_label, int32_t* face_count, void* scratch, hipStream_t st,
                               int* rounds_out);
void gsr_launch_mesh_compact_count(int nv, int nf, const int32_t* faces, const uint8_t* keep /*or NULL*/, void* scratch, int32_t* counts_out,
                                   hipStream_t st);
void gsr_launch_mesh_compact_emit(int nv, int nf, const float* vertices, const float* colors /*or NULL*/, const int32_t* faces,
                                  const uint8_t* keep /*or NULL*/, void* scratch, int nv_out, int nf_out, float* vertices_out,
                                  float* colors_out /*or NULL*/, int32_t* faces_out, hipStream_t st);
void gsr_launch_mesh_vertex_normals(int nv, int nf, const float* vertices, const int32_t* faces, float* normals, void* scratch, hipStream_t st);
void gsr_launch_mesh_smooth(int nv, int nf, const float* vertices, const int32_t* faces, int iterations, float lambda, float mu,
                            float* vertices_out, void* scratch, hipStream_t st);
// knn.hip
size_t gsr_knn_scratch_bytes_impl(int N);
void gsr_launch_knn(int N, const float* points, float* out, void* scratch, hipStream_t st);
// ssim.hip: mean-SSIM form (no map round trip)
void gsr_set_ssim_variant(int v);      // 0 = marching waves (default), 1 = LDS tiles (A/B)
void gsr_set_ssim_target_waves(int v); // tuning: waves per launch the marching form aims for (both directions; 0 = the defaults again)
int64_t gsr_ssim_partial_count_impl(int planes, int H, int W);
void gsr_launch_ssim_mean_forward(int planes, int H, int W, const float* img1, const float* img2, float* partials,
                                  float* mean_out, float* dm_dmu1, float* dm_dex2, float* dm_dexy, hipStream_t st);
void gsr_launch_ssim_mean_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmean,
                                   const float* dm_dmu1, const float* dm_dex2, const float* dm_dexy, float* dL_dimg1,
                                   hipStream_t st);
// ssim.hip: the fused training loss (1 - lambda) L1 + lambda (1 - SSIM) in the SSIM kernels' single pass
void gsr_launch_train_loss_forward(int planes, int H, int W, const float* img1, const float* img2, float lambda, float* partials,
                                   float* loss_out, float* dm_dmu1, float* dm_dex2, float* dm_dexy, hipStream_t st);
void gsr_launch_train_loss_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dloss, float lambda,
                                    const float* dm_dmu1, const float* dm_dex2, const float* dm_dexy, float* dL_dimg1, hipStream_t st);
// binning.hip: gathered splat records -> geometry state of this rank's band (two-axis sharding)
int gsr_launch_splat_ingest(int P, const float* records, int y0, int y1, float4* splats, uint2* rect, uint32_t* tiles,
                            uint32_t* keys, uint32_t* vals, const GsrFrameStatsDev& fs, hipStream_t st);
// binning.hip: full 32-bit depth keys from the splat records (fallback of the 27-bit depth sort)
void gsr_launch_rekey_full(int P, const float4* splats, const uint32_t* tiles, uint32_t* keys, uint32_t* vals, hipStream_t st);

// route.hip: Gaussian-sharded rendering -- destination-targeted exchange of packed splat records
#define GSR_MAX_BANDS 64
size_t gsr_route_scratch_bytes_impl(int P, int n_bands);
void gsr_launch_route_count(int P, const float* records, int n_bands, const int32_t* bounds, uint32_t* block_counts,
                            uint32_t* band_counts, hipStream_t st);
void gsr_launch_route_pack(int P, const float* records, int n_bands, const int32_t* bounds, const int64_t* band_offsets,
                           const uint32_t* block_offsets, float* packed, int32_t* send_ids, uint32_t cap /*0xFFFFFFFF: no limit*/,
                           const uint32_t* band_counts /*fixed-capacity form: header rows; else NULL*/, hipStream_t st);
int gsr_launch_ingest_packed(int P, const float* packed, int y0, int y1, float4* splats, uint2* rect, uint32_t* tiles,
                             uint32_t* keys, uint32_t* vals, const GsrFrameStatsDev& fs, int seg_rows /*0 or capacity + 1*/, hipStream_t st);
void gsr_launch_route_add_rows(int64_t n, const int32_t* ids, const float* rows, float* out, hipStream_t st);
