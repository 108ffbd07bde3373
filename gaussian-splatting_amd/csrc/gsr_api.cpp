// C ABI of libgsr_hip.so (include/gsr.h): argument checking, scratch carving, kernel orchestration.
// Host-side counterpart of the reference's rasterize_points.cu / CudaRasterizer::Rasterizer glue
// (un-vendored; call sites gaussian_renderer/__init__.py:91-110, train.py:142) -- re-designed around a
// depth-sort + stable tile-sort binning pipeline instead of one 64-bit key sort.
#include <hip/hip_runtime.h>

#include <sched.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "gsr_internal.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(GSR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

// ---- options / profiling ----
int g_render_fwd_variant = 0;
int g_render_bwd_variant = 0;
int g_depth_sort_mode = 0;      // 0 = automatic (bucket sort, depthsort.hip, up to GSR_DS_MAX_P Gaussians; LSD radix sort beyond, and
                                // for a while after a frame whose depths crowded one bucket), 1 = always LSD, 2 = always bucket sort
int g_snug_tiles = 1;           // 1 = bin every Gaussian into its snug tile rectangle (gsr_math.h); 0 = the reference's square (A/B)
int g_bwd_heavy_first = 2;      // launch order of the blend backward (plan kernel, render_bwd.hip): 0 = tiles in index order, 1 = heaviest tiles first (sum of
                                // the four blocks: round 3), 2 = tiles by their heaviest half (default: blend backward 0.343 -> 0.324 ms on the bench frame),
                                // 3 = every half tile (= wave) on its own, heaviest first (0.325; slower than 2 on the clustered scene: the two halves of
                                // a tile no longer share their gathered records in one XCD's L2)
int g_tile_sort_mode = 0;       // 0 = fused emission + two-level sort (tilesort.hip), 1 = legacy emit + LSD passes (A/B)

struct PendingEvent { int stage; hipEvent_t a, b; };
std::mutex g_prof_mu;
bool g_prof_on = false;
bool g_count_on = false;      // work counters of the blend kernels (bit 1 of gsr_profile_enable): they serialise on two global words
                              // and slow the kernels several times over, so they are never on while stages are being timed
std::vector<PendingEvent> g_pending;
std::vector<hipEvent_t> g_pool;
double g_stage_ms[GSR_STAGE_COUNT] = {0};
int g_stage_n[GSR_STAGE_COUNT] = {0};
constexpr int GSR_MAX_DEVICES = 64;
unsigned long long* g_counters_dev[GSR_MAX_DEVICES] = {nullptr};     // per device: work counters of the blend kernels (measurement only)

hipEvent_t get_event() {
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
struct StageTimer {
    int stage; hipStream_t st; bool on; hipEvent_t a, b;
    StageTimer(int stage_, hipStream_t st_) : stage(stage_), st(st_), on(g_prof_on) {
        if (on) { std::lock_guard<std::mutex> l(g_prof_mu); a = get_event(); b = get_event(); (void)hipEventRecord(a, st); }
    }
    ~StageTimer() {
        if (on) { (void)hipEventRecord(b, st); std::lock_guard<std::mutex> l(g_prof_mu); g_pending.push_back({stage, a, b}); }
    }
};

int check_stage(const GsrRasterSettings* s, hipStream_t st, const char* what) {
    if (s->debug) {
        hipError_t e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return fail(GSR_ERR_HIP, std::string("after ") + what + ": " + hipGetErrorString(e));
    }
    return GSR_OK;
}
#define STAGE_CHECK(what) do { int rc_ = check_stage(settings, st, what); if (rc_ != GSR_OK) return rc_; } while (0)

int bits_for(uint32_t n_values) {   // number of bits needed to represent 0 .. n_values-1
    int b = 0;
    while (b < 32 && (1ull << b) < (unsigned long long)n_values) ++b;
    return b < 1 ? 1 : b;
}

int make_cam(const GsrRasterSettings* s, int M, GsrCamDev& c) {
    if (!s) return fail(GSR_ERR_INVALID_ARG, "settings is NULL");
    if (s->image_width <= 0 || s->image_height <= 0) return fail(GSR_ERR_INVALID_ARG, "image size must be positive");
    if (!s->bg || !s->viewmatrix || !s->projmatrix || !s->campos)
        return fail(GSR_ERR_INVALID_ARG, "bg / viewmatrix / projmatrix / campos must be device pointers");
    if (s->sh_degree < 0 || s->sh_degree > 3) return fail(GSR_ERR_UNSUPPORTED, "sh_degree must be 0..3");
    c.W = s->image_width;
    c.H = s->image_height;
    c.gx = (c.W + GSR_TILE - 1) / GSR_TILE;
    c.gy = (c.H + GSR_TILE - 1) / GSR_TILE;
    if (c.gx > 65535 || c.gy > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 tiles per axis");
    // a Gaussian's tile count (rectangle area) and the tile ids must stay well inside 32 bits
    if ((int64_t)c.gx * c.gy > (1ll << 24)) return fail(GSR_ERR_UNSUPPORTED, "more than 2^24 tiles");
    // fp32 host arithmetic, same expression as oracle/torch_oracle.py:preprocess
    c.focal_x = (float)c.W / (2.0f * s->tanfovx);
    c.focal_y = (float)c.H / (2.0f * s->tanfovy);
    c.limx = 1.3f * s->tanfovx;
    c.limy = 1.3f * s->tanfovy;
    c.scale_modifier = s->scale_modifier;
    c.sh_degree = s->sh_degree;
    c.M = M;
    c.antialiasing = s->antialiasing ? 1 : 0;
    c.snug = g_snug_tiles;
    int y0 = s->tile_y0, y1 = s->tile_y1;
    if (y1 <= 0) { y0 = 0; y1 = c.gy; }
    if (y0 < 0) y0 = 0;
    if (y1 > c.gy) y1 = c.gy;
    if (y0 > y1) y0 = y1;
    c.tile_y0 = y0;
    c.tile_y1 = y1;
    c.view = s->viewmatrix;
    c.proj = s->projmatrix;
    c.campos = s->campos;
    c.bg = s->bg;
    c.sh_dc = s->sh_dc;
    c.dL_dsh_dc = s->dL_dsh_dc;
    return GSR_OK;
}

int check_inputs(int P, int M, const float* means3D, const float* shs, const float* colors_precomp,
                 const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
                 int sh_degree) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !opacities) return fail(GSR_ERR_INVALID_ARG, "means3D / opacities are NULL");
    if ((shs == nullptr) == (colors_precomp == nullptr))
        return fail(GSR_ERR_INVALID_ARG, "provide exactly one of shs / colors_precomp");
    const bool sr = scales != nullptr && rotations != nullptr;
    if ((scales == nullptr) != (rotations == nullptr) || sr == (cov3D_precomp != nullptr))
        return fail(GSR_ERR_INVALID_ARG, "provide exactly one of (scales, rotations) / cov3D_precomp");
    if (shs) {
        if (M <= 0 || M > 16) return fail(GSR_ERR_UNSUPPORTED, "SH coefficient count M must be 1..16");
        if ((sh_degree + 1) * (sh_degree + 1) > M) return fail(GSR_ERR_INVALID_ARG, "sh_degree needs more coefficients than M");
    }
    return GSR_OK;
}

// split SH form (settings->sh_dc): coefficient 0 in sh_dc[P,1,3], coefficients 1..M-1 in shs[P,M-1,3]
int check_split_sh(const GsrRasterSettings* s, int P, int M, const float* shs, bool backward) {
    if (!s->sh_dc || P == 0) return GSR_OK;
    if (!shs) return fail(GSR_ERR_INVALID_ARG, "sh_dc given without shs (the coefficients 1..M-1)");
    if (M != 16) return fail(GSR_ERR_UNSUPPORTED, "split SH form needs M == 16 (degree-3 storage); concatenate smaller records");
    if ((((uintptr_t)s->sh_dc) | ((uintptr_t)shs)) & 15) return fail(GSR_ERR_UNSUPPORTED, "split SH form needs 16-byte aligned sh_dc / shs");
    if (backward && !s->dL_dsh_dc) return fail(GSR_ERR_INVALID_ARG, "sh_dc given but dL_dsh_dc is NULL");
    return GSR_OK;
}

// R read-back word: mapped + portable + coherent pinned host memory: [0] = R low word, [1] = sequence number, [2] = R high word,
// [3] = "a depth key needed more than 27 bits".  ("The bucket depth sort met an oversized segment" is NOT part of the leased slot
// (the segment sort may still be running when the slot goes back to the pool): it is a per-device mapped word, g_slow_word.)
// Written by the last workgroup of the key-producing kernel (gsr_frame.h), which folds the frame's statistics in `state`, a
// 64-byte block of device memory that is zero between frames.  Words are LEASED per call from a per-device pool (ADVICE r02:
// keyed by device, not by thread -- a host thread that comes and goes leaks nothing, concurrent callers never share a word);
// never freed (the runtime releases them with the context).
struct HostWord {
    uint32_t* host = nullptr; uint32_t* dev = nullptr; uint32_t* state = nullptr; uint32_t seq = 0;
};
std::mutex g_hw_mu;
std::vector<HostWord> g_hw_pool[GSR_MAX_DEVICES];
std::atomic<int64_t> g_last_R[GSR_MAX_DEVICES];      // per device: sizes the speculative binning buffer of the next frame
std::atomic<int> g_lsd_frames[GSR_MAX_DEVICES];      // per device: frames for which the automatic depth sort stays with the LSD passes
std::atomic<int> g_lsd_backoff[GSR_MAX_DEVICES];     // per device: length of the next such stay (doubles per failed retry; heuristic only)
std::atomic<int> g_lsd_probation[GSR_MAX_DEVICES];   // per device: clean bucket-sort frames still needed after a stay before the back-off is forgotten
uint32_t* g_slow_word_dev[GSR_MAX_DEVICES] = {nullptr};      // its device-side address
std::atomic<int> g_debug_dirty_tickets{0};           // TEST HOOK (gsr_set_option debug_dirty_control_block): tickets preloaded into the next frame's counter, once
uint32_t* g_slow_word[GSR_MAX_DEVICES] = {nullptr};  // per device, mapped host memory: set (1) by ds_segsort when a segment overflowed the LDS capacity;
                                                     // read and cleared by the next lease on that device.  A heuristic flag: a store that races the
                                                     // clear is at worst seen one frame later or lost once, never attributed to another device
struct HostWordLease {
    int dev = -1;
    HostWord hw;
    hipStream_t st = nullptr;
    bool settled = true;      // false while a kernel that will still write the word may be pending
    ~HostWordLease() {
        if (dev < 0) return;
        if (!settled) {      // error paths only: never hand a word with a pending writer (or a half-filled state block) to the next call
            (void)hipMemsetAsync(hw.state, 0, 64, st);      // the ticket counter of gsr_frame.h (behind whatever kernel may still add to it)
            (void)hipStreamSynchronize(st);
        }
        std::lock_guard<std::mutex> l(g_hw_mu);
        g_hw_pool[dev].push_back(hw);
    }
};
int lease_host_word(HostWordLease& lease, hipStream_t st) {
    int dev_id = 0;
    HIP_OK(hipGetDevice(&dev_id));
    if (dev_id < 0 || dev_id >= GSR_MAX_DEVICES) return fail(GSR_ERR_UNSUPPORTED, "device ordinal out of range");
    {
        std::lock_guard<std::mutex> l(g_hw_mu);
        if (!g_hw_pool[dev_id].empty()) { lease.hw = g_hw_pool[dev_id].back(); g_hw_pool[dev_id].pop_back(); }
    }
    if (!lease.hw.host) {      // a new slot (first call on this device, or one more concurrent caller): 64 B mapped host + 64 B device, kept for good
        HostWord nw;
        hipError_t e = hipHostMalloc((void**)&nw.host, 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&nw.dev, nw.host, 0);
        if (e == hipSuccess) e = hipMalloc((void**)&nw.state, 64);
        // cleared ON THE CALLER'S STREAM, in front of the kernel that will count in it: hipMemset() of device memory is queued on the null stream and
        // returns before it has run, and a non-blocking stream (every torch side stream) is not ordered behind the null stream -- the clear could land
        // in the middle of the first frame, lose its tickets, and leave a counter that is never zero again (round 6: a GPU suite run lost
        // the second caller's first frame of tests/test_gpu_parity.py::test_concurrent_forward_calls_from_two_host_threads and every frame after it)
        if (e == hipSuccess) e = hipMemsetAsync(nw.state, 0, 64, st);
        if (e != hipSuccess) {      // (nothing half-made is leaked or pooled)
            if (nw.state) (void)hipFree(nw.state);
            if (nw.host) (void)hipHostFree(nw.host);
            return fail(GSR_ERR_HIP, std::string("control block allocation: ") + hipGetErrorString(e));
        }
        for (int i = 0; i < 16; ++i) nw.host[i] = 0;
        lease.hw = nw;
    }
    {
        std::lock_guard<std::mutex> l(g_hw_mu);
        if (!g_slow_word[dev_id]) {
            uint32_t* w = nullptr;
            uint32_t* wd = nullptr;
            hipError_t e = hipHostMalloc((void**)&w, 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
            if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&wd, w, 0);
            if (e != hipSuccess) {      // (the slot leased above goes back to the pool -- lease.dev is set first -- nothing leaks)
                if (w) (void)hipHostFree(w);
                lease.dev = dev_id;
                lease.st = st;
                return fail(GSR_ERR_HIP, std::string("slow-word allocation: ") + hipGetErrorString(e));
            }
            for (int i = 0; i < 16; ++i) w[i] = 0;
            g_slow_word_dev[dev_id] = wd;
            g_slow_word[dev_id] = w;
        }
    }
    lease.hw.host[3] = 0;
    uint32_t* slow = g_slow_word[dev_id];
    // (read and cleared in ONE step: two concurrent callers never both see the same report and double the stay twice -- ADVICE r05)
    if (__atomic_load_n(slow, __ATOMIC_RELAXED) && __atomic_exchange_n(slow, 0u, __ATOMIC_RELAXED)) {
                                 // a recent frame on this device: thousands of Gaussians in one depth bucket -- its segment went
                                 // through global memory.  Stay with the LSD passes for a while, then try again: 64 frames the first
        int back = g_lsd_backoff[dev_id].load();      // time, twice as long after every retry that met an oversized segment again
        if (back < 64) back = 64;                     // (a scene that always crowds a bucket pays one slow frame in 65, 129, ... 8193)
        g_lsd_frames[dev_id].store(back);
        g_lsd_backoff[dev_id].store(back >= 8192 ? 8192 : back * 2);
        g_lsd_probation[dev_id].store(0);
    } else if (g_lsd_probation[dev_id].load() > 0 && g_lsd_frames[dev_id].load() == 0) {
        //  the stay is over and bucket-sort frames come back clean: after three of them (the flag is written by a kernel that
        // may still be running when the next lease looks) the doubling is forgotten -- isolated crowded frames of a long run no longer add up
        if (g_lsd_probation[dev_id].fetch_sub(1) == 1) g_lsd_backoff[dev_id].store(64);
    }
    lease.dev = dev_id;
    lease.st = st;
    return GSR_OK;
}
uint32_t* slow_word_dev(int dev_id) {      // device-side address of the device's "oversized segment" flag (mapped host memory; cached with it)
    return g_slow_word[dev_id] ? g_slow_word_dev[dev_id] : nullptr;
}
unsigned long long* counters_for_current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= GSR_MAX_DEVICES) return nullptr;
    return g_counters_dev[d];
}

#if defined(__x86_64__) || defined(__i386__)
#define GSR_CPU_RELAX() __builtin_ia32_pause()
#elif defined(__aarch64__)
#define GSR_CPU_RELAX() asm volatile("yield" ::: "memory")
#else
#define GSR_CPU_RELAX() do { } while (0)
#endif

// keys per workgroup of a radix pass: 1024 below 512 K keys, 2048 below 3 M, 4096 above.  Measured on the depth sort of
// 1 M keys with the round-2 kernels (one box, interleaved): 1024 -> 0.0892 ms, 2048 -> 0.0855 ms, 4096 -> 0.0919 ms.
int64_t g_small_block_threshold = (int64_t)512 * 1024;
int64_t g_mid_block_threshold = (int64_t)3 * 1024 * 1024;
int g_sort_items_large = GSR_SORT_ITEMS;                      // keys per workgroup above the thresholds (1024 / 2048 / 4096 / 8192)
int sort_items(int64_t n) {
    if (n < g_small_block_threshold) return GSR_SORT_ITEMS_SMALL;
    if (n < g_mid_block_threshold) return 2048 < g_sort_items_large ? 2048 : g_sort_items_large;
    return g_sort_items_large;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
GsrGeom gsr_carve_geom(char* base, int P) {
    GsrGeom g;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = gsr_align128(off + bytes); return p; };
    const size_t n = (size_t)(P > 0 ? P : 1);
    g.splats = (float4*)take(n * 64);
    g.rect = (uint2*)take(n * 8);
    g.tiles = (uint32_t*)take(n * 4);
    g.clamped = (uint32_t*)take(n * 4);
    g.keys[0] = (uint32_t*)take(n * 4);
    g.keys[1] = (uint32_t*)take(n * 4);
    g.vals[0] = (uint32_t*)take(n * 4);
    g.vals[1] = (uint32_t*)take(n * 4);
    g.rect_sorted = (uint2*)take(n * 8);
    g.offsets = (uint32_t*)take(n * 4);
    g.block_sums = (uint64_t*)take(((n + GSR_SCAN_ITEMS - 1) / GSR_SCAN_ITEMS) * 8);
    g.block_first = (uint2*)take(gsr_block_first_cap(P) * 8);
    g.sort_hist = (uint32_t*)take((size_t)GSR_SORT_MAX_DIGITS * (size_t)gsr_sort_blocks((int64_t)n, true) * 4);   // small workgroups: worst case
    g.digit_total = (uint32_t*)take(GSR_SORT_MAX_DIGITS * 4);
    {
        const bool ds = P <= GSR_DS_MAX_P;
        const size_t np = ds ? n : 1, nblk = ds ? gsr_depth_bucket_blocks(P) : 1, nseg = ds ? gsr_depth_bucket_segments(P) : 1;
        g.ds.pairs[0] = (uint2*)take(np * 8);
        g.ds.pairs[1] = (uint2*)take(np * 8);
        g.ds.cnt_tab = (uint32_t*)take(nblk * GSR_DS_BUCKETS * 4);
        g.ds.tile_tab = (uint32_t*)take(nblk * GSR_DS_BUCKETS * 4);
        g.ds.cnt_total = (uint32_t*)take(GSR_DS_BUCKETS * 4);
        g.ds.tile_total = (uint32_t*)take(GSR_DS_BUCKETS * 4);
        g.ds.plan = (uint32_t*)take(nseg * GSR_DS_PLAN_WORDS * 4);
        g.ds.eq_tab = (uint32_t*)take((size_t)GSR_EQ_TAB_WORDS * 4);
        g.ds.bucket_of = (uint16_t*)take((np + 64) * 2);
    }
    g.num_rendered = (uint32_t*)take(128);
    g.wg_range = (uint2*)take((size_t)GSR_FRAME_MAX_GROUPS * 8);
    g.bytes = off;
    return g;
}

GsrBinning gsr_carve_binning(char* base, int64_t R) {
    GsrBinning b;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = gsr_align128(off + bytes); return p; };
    const size_t n = (size_t)(R > 0 ? R : 1);
    {   // one contiguous 8n-byte region: the two key buffers of the LSD sort, or the packed words of the fused sort
        char* wk = take(gsr_align128(n * 4) * 2);
        b.keys[0] = (uint32_t*)wk;
        b.keys[1] = (uint32_t*)(wk ? wk + gsr_align128(n * 4) : nullptr);
    }
    b.vals[0] = (uint32_t*)take(n * 4);
    b.vals[1] = (uint32_t*)take(n * 4);
    b.sort_hist = (uint32_t*)take((size_t)256 * (size_t)gsr_sort_blocks((int64_t)n, true) * 4);   // worst case
    const size_t nblk = (n + GSR_TS_ITEMS - 1) / GSR_TS_ITEMS;
    b.hist2 = (uint32_t*)take((nblk + 256) * 256 * 4);
    b.digit_total = (uint32_t*)take(256 * 4);
    b.bucket_base = (uint32_t*)take(257 * 4);
    b.blk2_start = (uint32_t*)take(257 * 4);
    b.tile_base = (uint32_t*)take(65536 * 4);
    b.block_first = (uint2*)take((nblk + 2) * 8);
    b.meta = (uint32_t*)take(128);
    b.bytes = off;
    return b;
}

GsrBwdScratch gsr_carve_bwd(char* base, int P, int64_t R) {
    GsrBwdScratch b;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = gsr_align128(off + bytes); return p; };
    const size_t np = (size_t)(P > 0 ? P : 1), nr = (size_t)(R > 0 ? R : 1);
    b.splat_grads = (float*)take(np * 48);
    b.inst_grads = (float*)take(nr * 48 * GSR_BWD_SLOTS);
    b.inst_flag = (uint32_t*)take(nr * 4);
    const size_t nu = gsr_reduce_units((int64_t)nr);
    b.unit_first = (uint2*)take(nu * 8);
    b.unit_piece = (float*)take(nu * 96);
    b.bytes = off;
    return b;
}

GsrImage gsr_carve_image(char* base, int W, int H) {
    GsrImage im;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = gsr_align128(off + bytes); return p; };
    const size_t npix = (size_t)W * (size_t)H;
    const size_t nt = (size_t)((W + GSR_TILE - 1) / GSR_TILE) * (size_t)((H + GSR_TILE - 1) / GSR_TILE);
    im.final_T = (float*)take(npix * 4);
    im.n_contrib = (uint32_t*)take(npix * 4);
    im.ranges = (uint2*)take(nt * 8);
    im.block_steps = (uint32_t*)take(nt * 16);
    im.tile_order = (uint32_t*)take(nt * 8);      // one entry per half tile (the backward's launch order)
    im.bytes = off;
    return im;
}

extern "C" {

int gsr_abi_version(void) { return GSR_ABI_VERSION; }
const char* gsr_last_error(void) { return g_err.c_str(); }

size_t gsr_geometry_bytes(int P) { return gsr_carve_geom(nullptr, P).bytes; }
size_t gsr_binning_bytes(int64_t R, int n_tiles) { (void)n_tiles; return gsr_carve_binning(nullptr, R).bytes; }
size_t gsr_image_bytes(int width, int height) { return gsr_carve_image(nullptr, width, height).bytes; }
size_t gsr_backward_scratch_bytes(int P, int64_t R) { return gsr_carve_bwd(nullptr, P, R).bytes; }

int gsr_set_option(const char* name, int value) {
    if (!name) return fail(GSR_ERR_INVALID_ARG, "option name is NULL");
    if (!strcmp(name, "render_fwd_variant")) {
        if (!gsr_render_forward_variant_available(value)) return fail(GSR_ERR_UNSUPPORTED, "render_fwd_variant not in this build (A/B variants need -DGSR_AB_VARIANTS)");
        g_render_fwd_variant = value;
        return GSR_OK;
    }
    if (!strcmp(name, "render_bwd_variant")) {
        if (!gsr_render_backward_variant_available(value)) return fail(GSR_ERR_UNSUPPORTED, "render_bwd_variant not in this build (A/B variants need -DGSR_AB_VARIANTS)");
        g_render_bwd_variant = value;
        return GSR_OK;
    }
    if (!strcmp(name, "sort_small_block_threshold")) { g_small_block_threshold = value; return GSR_OK; }
    if (!strcmp(name, "sort_mid_block_threshold")) { g_mid_block_threshold = value; return GSR_OK; }
    if (!strcmp(name, "sort_items_large")) {
        if (value != 1024 && value != 2048 && value != 4096 && value != 8192)
            return fail(GSR_ERR_INVALID_ARG, "sort_items_large must be 1024, 2048, 4096 or 8192");
        g_sort_items_large = value;
        return GSR_OK;
    }
    if (!strcmp(name, "depth_sort_mode")) {
        if (value < 0 || value > 2) return fail(GSR_ERR_INVALID_ARG, "depth_sort_mode must be 0 (automatic), 1 (LSD radix passes) or 2 (bucket sort)");
        g_depth_sort_mode = value;
        return GSR_OK;
    }
    if (!strcmp(name, "preprocess_grid_cap")) { gsr_set_preprocess_grid_cap(value); return GSR_OK; }
    if (!strcmp(name, "preprocess_generic")) {
        if (value != 0 && value != 1) return fail(GSR_ERR_INVALID_ARG, "preprocess_generic must be 0 (the call form picks the forward instantiation) or 1 (always the generic one)");
        gsr_set_preprocess_generic(value);
        return GSR_OK;
    }
    if (!strcmp(name, "preprocess_hot_grid")) {
        if (value < 0 || value > GSR_FRAME_MAX_GROUPS) return fail(GSR_ERR_INVALID_ARG, "preprocess_hot_grid must be 0 (from the occupancy) or 1..2047 workgroups");
        gsr_set_preprocess_hot_grid(value);
        return GSR_OK;
    }
    if (!strcmp(name, "debug_last_preprocess_path")) {      // test hook, changes nothing: succeeds iff the most recent forward took this path
        if (value != 1 && value != 2) return fail(GSR_ERR_INVALID_ARG, "debug_last_preprocess_path: 1 (generic) or 2 (hot)");
        if (gsr_preprocess_last_path() != value)
            return fail(GSR_ERR_INVALID_ARG, gsr_preprocess_last_path() == 2 ? "the last forward preprocess ran a hot instantiation" : gsr_preprocess_last_path() == 1 ? "the last forward preprocess ran the generic instantiation" : "no forward preprocess has run yet");
        return GSR_OK;
    }
    if (!strcmp(name, "ssim_variant")) {
        if (value != 0 && value != 1) return fail(GSR_ERR_INVALID_ARG, "ssim_variant must be 0 (marching waves) or 1 (LDS tiles)");
        gsr_set_ssim_variant(value);
        return GSR_OK;
    }
    if (!strcmp(name, "ssim_target_waves")) { gsr_set_ssim_target_waves(value); return GSR_OK; }      // (0 = the defaults, forward 4096 / backward 2048)
    if (!strcmp(name, "snug_tiles")) {
        if (value != 0 && value != 1) return fail(GSR_ERR_INVALID_ARG, "snug_tiles must be 1 (snug tile rectangles) or 0 (the reference's tile square)");
        g_snug_tiles = value;
        return GSR_OK;
    }
    if (!strcmp(name, "bwd_heavy_first")) {
        if (value < 0 || value > 3) return fail(GSR_ERR_INVALID_ARG, "bwd_heavy_first must be 0 (tiles in index order), 1 (heaviest tiles first), 2 (tiles by their heaviest half) or 3 (half tiles, heaviest first)");
        g_bwd_heavy_first = value;
        return GSR_OK;
    }
    if (!strcmp(name, "ranking_generic")) {
        if (value != 0 && value != 1) return fail(GSR_ERR_INVALID_ARG, "ranking_generic must be 0 (ranking kernels compiled for the frame's digit widths) or 1 (always the run-time-width ones)");
        gsr_set_ranking_generic(value);
        return GSR_OK;
    }
    if (!strcmp(name, "ranking_pad_last")) {
        if (value != 0 && value != 1) return fail(GSR_ERR_INVALID_ARG, "ranking_pad_last must be 1 (partial blocks of the tile sort rank their missing slots as padding of the highest digit) or 0 (per-item validity)");
        gsr_set_ranking_pad_last(value);
        return GSR_OK;
    }
    if (!strcmp(name, "debug_last_ranking_widths")) {      // test hook, changes nothing: succeeds iff the most recent emit_scatter / bucket_scatter launches were
        // instantiated for the bucket digit value >> 4 and the low digit value & 15 (0: the run-time-width kernel)
        if (value < 0 || value > 0x88) return fail(GSR_ERR_INVALID_ARG, "debug_last_ranking_widths: hb << 4 | lb, each 0 (generic) or 5..8");
        if (g_ranking_last_hb != (value >> 4) || g_ranking_last_lb != (value & 15))
            return fail(GSR_ERR_INVALID_ARG, "the last tile sort ran emit_scatter<" + std::to_string(g_ranking_last_hb) + "> and bucket_scatter<" + std::to_string(g_ranking_last_lb) + ">");
        return GSR_OK;
    }
    if (!strcmp(name, "level2_scan_mode")) {
        if (value < 0 || value > 2) return fail(GSR_ERR_INVALID_ARG, "level2_scan_mode must be 0 (automatic), 1 (separate scan launch) or 2 (scan folded into the scatter)");
        gsr_set_level2_scan_mode(value);
        return GSR_OK;
    }
#ifdef GSR_AB_VARIANTS
    if (!strcmp(name, "render_fwd_lds_pad")) {
        if (value < 0 || value > 60000) return fail(GSR_ERR_INVALID_ARG, "render_fwd_lds_pad must be 0..60000 bytes");
        gsr_set_render_fwd_lds_pad(value);
        return GSR_OK;
    }
#endif
    if (!strcmp(name, "debug_dirty_control_block")) {      // test hook, one shot: see frame_stats_for
        if (value < 0 || value > 2047) return fail(GSR_ERR_INVALID_ARG, "debug_dirty_control_block: 0..2047 tickets");
        g_debug_dirty_tickets.store(value);
        return GSR_OK;
    }
    if (!strcmp(name, "tile_sort_mode")) {
        if (value != 0 && value != 1) return fail(GSR_ERR_INVALID_ARG, "tile_sort_mode must be 0 (fused) or 1 (legacy LSD)");
        g_tile_sort_mode = value;
        return GSR_OK;
    }
    return fail(GSR_ERR_INVALID_ARG, std::string("unknown option ") + name);
}

int gsr_profile_enable(int on) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    const bool trace = (on & 4) != 0;
    g_count_on = (on & 2) != 0 || trace;
    int d = 0;
    if (g_count_on && hipGetDevice(&d) == hipSuccess && d >= 0 && d < GSR_MAX_DEVICES) {
        if (!g_counters_dev[d]) {
            // measurement only (the product path never allocates): one block per device ordinal, on the CURRENT device -- the six work
            // counters, the mode word and the per-wave trace area (gsr_internal.h)
            if (hipMalloc((void**)&g_counters_dev[d], GSR_MEASURE_WORDS * sizeof(unsigned long long)) != hipSuccess) g_counters_dev[d] = nullptr;
            else (void)hipMemset(g_counters_dev[d], 0, GSR_MEASURE_WORDS * sizeof(unsigned long long));
        }
        if (g_counters_dev[d]) {
            const unsigned long long mode = trace ? 1ull : 0ull;
            (void)hipMemcpy(g_counters_dev[d] + GSR_TRACE_MODE_WORD, &mode, sizeof(mode), hipMemcpyHostToDevice);
            (void)hipStreamSynchronize(nullptr);      // (null-stream work: finished before a kernel of a non-blocking stream reads the word)
        }
    }
    g_prof_on = (on & 1) != 0;
    return GSR_OK;
}
int gsr_profile_trace(uint64_t* out, int max_waves) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    if (!out || max_waves <= 0) return 0;
    unsigned long long* ctr = counters_for_current_device();
    if (!ctr) return 0;
    const int n = max_waves < GSR_TRACE_WAVES ? max_waves : GSR_TRACE_WAVES;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(out, ctr + GSR_TRACE_BASE, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    (void)hipMemset(ctr + GSR_TRACE_BASE, 0, (size_t)GSR_TRACE_WAVES * 4 * sizeof(unsigned long long));
    (void)hipStreamSynchronize(nullptr);      // (the clear is queued on the null stream: done before a kernel of a non-blocking stream traces again)
    return n;
}
int gsr_profile_counters(uint64_t* out, int n, int reset) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    unsigned long long host[GSR_COUNTER_COUNT] = {0};
    unsigned long long* ctr = counters_for_current_device();
    if (ctr) {
        if (hipDeviceSynchronize() != hipSuccess) return fail(GSR_ERR_HIP, "counter read-back failed");      // (kernels of every stream have counted)
        if (hipMemcpy(host, ctr, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) return fail(GSR_ERR_HIP, "counter read-back failed");
        if (reset) { (void)hipMemset(ctr, 0, sizeof(host)); (void)hipStreamSynchronize(nullptr); }
    }
    for (int i = 0; i < n && i < GSR_COUNTER_COUNT; ++i) out[i] = host[i];
    return GSR_OK;
}
int gsr_profile_reset(void) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    for (auto& p : g_pending) { (void)hipEventSynchronize(p.b); g_pool.push_back(p.a); g_pool.push_back(p.b); }
    g_pending.clear();
    for (int i = 0; i < GSR_STAGE_COUNT; ++i) { g_stage_ms[i] = 0; g_stage_n[i] = 0; }
    return GSR_OK;
}
int gsr_profile_read(float* ms_out, int32_t* count_out, int n) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    for (auto& p : g_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            g_stage_ms[p.stage] += ms;
            g_stage_n[p.stage] += 1;
        }
        g_pool.push_back(p.a);
        g_pool.push_back(p.b);
    }
    g_pending.clear();
    for (int i = 0; i < n && i < GSR_STAGE_COUNT; ++i) {
        if (ms_out) ms_out[i] = (float)g_stage_ms[i];
        if (count_out) count_out[i] = g_stage_n[i];
    }
    return GSR_OK;
}

// (profiling only) an event pair that goes back to the pool unless it was handed to g_pending -- ADVICE r02: the early
// returns of bin_and_render leaked two events per failed frame
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    bool armed = false;
    void arm(hipStream_t st) {
        if (!g_prof_on) return;
        std::lock_guard<std::mutex> l(g_prof_mu);
        a = get_event(); b = get_event(); armed = true;
        (void)hipEventRecord(a, st);
    }
    void commit(int stage, hipStream_t st) {
        if (!armed) return;
        (void)hipEventRecord(b, st);
        std::lock_guard<std::mutex> l(g_prof_mu);
        g_pending.push_back({stage, a, b});
        armed = false;
    }
    ~EventPair() {
        if (!armed) return;
        std::lock_guard<std::mutex> l(g_prof_mu);
        g_pool.push_back(a); g_pool.push_back(b);
    }
};

// THE invariant between a forward and every call that reads its buffers back: which ping-pong buffer holds the depth order and which the sorted
// list is a pure function of the build and of the frame geometry (never of a run-time option or of the frame's content), so a reader finds the
// forward's results without any state passed between the two calls.
//   depth order: 3 passes of 9 bits -> vals[1]; the 32-bit fallback sort (4 passes -> vals[0]) copies its result there.
//   sorted list: <= 65536 tiles: vals[0] (the fused sort writes it; the legacy LSD sort takes 2 passes); more: 3 LSD passes -> vals[1].
// bin_and_render puts the depth order where depth_order_buffer_index says; its tile sort ends in the buffer list_buffer_index derives from the
// same pass plan.  saved_frame is the only other caller of either function.
static int depth_order_buffer_index() {
    int pb[8];
    return gsr_sort_plan(GSR_DEPTH_KEY_BITS, GSR_DEPTH_DIGIT_BITS, pb) & 1;
}
static int list_buffer_index(int n_tiles) {
    if (n_tiles <= 65536) return 0;
    int pb[8];
    return gsr_sort_plan(bits_for((uint32_t)n_tiles), GSR_TILE_DIGIT_BITS, pb) & 1;
}

// The view of a finished forward's three buffers (cam: W, H, gx, gy are read).  Any buffer may be NULL: its pointers are NULL then, and the entry
// points' own checks decide what they need.  point_list is also NULL for R <= 0 (nothing was binned: the binning buffer may not even exist).
static GsrSavedFrame saved_frame(const GsrCamDev& cam, int P, int64_t R, const void* geom_buffer, const void* binning_buffer, const void* image_buffer) {
    const GsrGeom g = gsr_carve_geom((char*)geom_buffer, P);
    const GsrImage im = gsr_carve_image((char*)image_buffer, cam.W, cam.H);
    GsrSavedFrame f;
    f.ranges = im.ranges;
    f.point_list = (binning_buffer && R > 0) ? gsr_carve_binning((char*)binning_buffer, R).vals[list_buffer_index(cam.gx * cam.gy)] : nullptr;
    f.splats = g.splats;
    f.final_T = im.final_T;
    f.n_contrib = im.n_contrib;
    f.block_steps = im.block_steps;
    f.tile_order = im.tile_order;
    f.order = g.vals[depth_order_buffer_index()];
    f.offsets = g.offsets;
    f.tiles = g.tiles;
    return f;
}

// Host side of the R read-back: spin on the mapped word.  ADVICE r02: in training the host runs far ahead of the GPU, so the
// wait can be the whole rest of the previous iteration -- a hard spin would pin a core per rank.  200 us of PAUSE spinning
// (covers the forward-only case, where the wait is the scan bubble), then polls separated by sched_yield(), after 2 s the
// blocking path (which also surfaces kernel faults).
static int wait_for_R(HostWord& hw, uint32_t seq, hipStream_t st, const uint32_t* num_rendered_dev) {
    volatile uint32_t* w = hw.host;
    bool got = false;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 0;; ++spin) {
        if (w[1] == seq) { got = true; break; }
        if ((spin & 63) == 63) {
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (us > 2.0e6) break;
            if (us > 200.0) sched_yield();
        } else {
            GSR_CPU_RELAX();
        }
    }
    if (!got) {
        HIP_OK(hipStreamSynchronize(st));
        if (w[1] != seq) {
            uint32_t r[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // frame words: [0..1] R, [8] "a depth key overflowed", [9] sequence number (gsr_frame.h)
            HIP_OK(hipMemcpy(r, num_rendered_dev, sizeof(r), hipMemcpyDeviceToHost));
            if (r[9] != seq) {
                // the stream is idle and NO workgroup drew the last ticket: the slot's counter was not zero when the frame began (or lost
                // tickets on the way).  It is never handed on in that state, and the frame is refused instead of rendered with a made-up R
                HIP_OK(hipMemsetAsync(hw.state, 0, 64, st));
                HIP_OK(hipStreamSynchronize(st));
                return fail(GSR_ERR_HIP, "the frame statistics of this call were never published (control block reset; the call can be repeated)");
            }
            hw.host[0] = r[0];
            hw.host[2] = r[1];
            hw.host[3] = r[8] ? 1u : 0u;      // (the fallback recovers the key-overflow flag too, not only R)
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return GSR_OK;
}

// The statistics block / frame words / host word a key-producing kernel needs (gsr_frame.h)
static GsrFrameStatsDev frame_stats_for(HostWordLease& lease, GsrGeom& g, uint32_t& seq_out) {
    seq_out = ++lease.hw.seq;
    lease.settled = false;
    GsrFrameStatsDev fs;
    fs.state = lease.hw.state + 2u * (seq_out & 1u);               // two 64-bit counters per slot, used alternately (gsr_frame.h)
    fs.state_other = lease.hw.state + 2u * ((seq_out & 1u) ^ 1u);
    if (const int t = g_debug_dirty_tickets.exchange(0)) {       // test hook: this frame meets a counter that is not zero (tests/test_simt_abi_cpu.py)
        const unsigned long long dirt = ((unsigned long long)t << 53) | 5ull;
        (void)hipMemcpyAsync(fs.state, &dirt, sizeof(dirt), hipMemcpyHostToDevice, lease.st);
        (void)hipStreamSynchronize(lease.st);
    }
    fs.frame = g.num_rendered;
    fs.wg_range = g.wg_range;
    fs.host_word = lease.hw.dev;
    fs.seq = seq_out;
    return fs;
}

static bool use_bucket_sort(int P, int dev_id) {
    if (P > GSR_DS_MAX_P || g_depth_sort_mode == 1) return false;
    if (g_depth_sort_mode == 2) return true;
    if (g_lsd_frames[dev_id].load() > 0) {
        const int left = g_lsd_frames[dev_id].fetch_sub(1);
        if (left > 0) {                                               // (concurrent callers: one decrement each, never a lost update)
            if (left == 1) g_lsd_probation[dev_id].store(3);          // the stay ends with this frame: the next ones are on probation
            return false;
        }
        g_lsd_frames[dev_id].store(0);
    }
    return true;
}

// Everything after the key-producing kernel (per-Gaussian preprocess or splat ingest): depth sort + scan, emission, tile sort,
// ranges, blend.  `g` holds the splat records, band-clamped rectangles / tile counts and the depth keys of all P Gaussians;
// `seq` is the sequence number that kernel's last workgroup publishes with R.
static int bin_and_render(const GsrRasterSettings* settings, const GsrCamDev& cam, int P, GsrGeom& g, HostWordLease& lease, uint32_t seq,
                          int n_range /*workgroups of the key-producing kernel*/, GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize, void* image_user,
                          float* out_color, float* out_invdepth, int32_t* num_rendered, hipStream_t st, const GsrCompositeDev* comp = nullptr) {
    const int dev_id = lease.dev;
    HostWord& hw_slot = lease.hw;
    const int order_buf = depth_order_buffer_index();
    const uint32_t bf_cap = (uint32_t)gsr_block_first_cap(P);
    const bool bucket = use_bucket_sort(P, dev_id);
    // R = number of (Gaussian, tile) instances sizes the binning buffer and the emission grids, so the host must learn it
    // mid-pipeline (the reference has the same read-back).  It does not depend on the depth order: the key-producing kernel
    // has already summed it, and its last workgroup stores it with a sequence number straight into mapped pinned host memory
    // (gsr_frame.h).  The host queues the whole depth sort FIRST and only then looks at the word, so the read-back, the
    // callbacks and the emission launches all happen while the GPU sorts -- no idle bubble (rounds 1-3: R came from the
    // scan, after the sort, and the GPU idled 5-7 us per frame).
    {   StageTimer t(GSR_STAGE_DEPTH_SORT, st);
        if (bucket) {
            gsr_launch_depth_bucket_sort(P, g.keys[0], g.tiles, g.rect, g.num_rendered, g.wg_range, n_range, g.ds, g.vals[order_buf], g.rect_sorted, g.offsets,
                                         g.block_first, bf_cap, slow_word_dev(dev_id), st);
        } else {
            const int ob = gsr_radix_sort_pairs(g.keys, g.vals, P, GSR_DEPTH_KEY_BITS, GSR_DEPTH_DIGIT_BITS, g.sort_hist, g.digit_total,
                                                sort_items(P), st, g.rect, g.rect_sorted);
            if (ob != order_buf) return fail(GSR_ERR_HIP, "depth sort: unexpected result buffer");
        }
    }
    STAGE_CHECK("depth sort");
    if (!bucket) {
        StageTimer t(GSR_STAGE_SCAN, st);
        gsr_launch_scan_tiles(P, g.vals[order_buf], g.rect, g.rect_sorted, g.offsets, g.block_sums, g.block_first, bf_cap,
                              g.num_rendered + 4, nullptr, 0u, /*rect_already_sorted=*/true, st);
    }
    // (profiling only) what is left of the read-back on the GPU's time line: from the end of the depth sort / scan to the
    // first launch after the host has R
    EventPair wait_ev;
    wait_ev.arm(st);
    const int n_tiles = cam.gx * cam.gy;
    GsrTileSortPlan plan;
    gsr_tile_sort_plan(n_tiles, P, &plan);
    if (g_tile_sort_mode == 1) plan.fused = false;
    char* ibase = (char*)image_resize(image_user, gsr_image_bytes(cam.W, cam.H));
    // legacy path: the tile-range table is cleared here; the fused path writes every entry of the table itself
    if (ibase && !plan.fused)
        HIP_OK(hipMemsetAsync(gsr_carve_image(ibase, cam.W, cam.H).ranges, 0, sizeof(uint2) * (size_t)n_tiles, st));
    char* bbase = nullptr;
    size_t spec_bytes = 0;
    const int64_t last_R = g_last_R[dev_id].load();
    if (last_R > 0) {
        spec_bytes = gsr_binning_bytes(last_R + last_R / 4 + 4096, n_tiles);
        bbase = (char*)binning_resize(binning_user, spec_bytes);
    }
    int rc = wait_for_R(hw_slot, seq, st, g.num_rendered);
    if (rc != GSR_OK) return rc;
    lease.settled = true;
    if (hw_slot.host[3] != 0u) {
        // a listed Gaussian lies deeper than 0.2 * 2^16: its 27-bit key was clamped and the depth order above is not
        // trustworthy.  Rare path: full 32-bit keys from the splat records, 4 passes of 8 bits (round 2's sort), result
        // copied into the buffer the backward reads, scan again (R itself does not depend on the order).
        gsr_launch_rekey_full(P, g.splats, g.tiles, g.keys[0], g.vals[0], st);
        const int ob = gsr_radix_sort_pairs(g.keys, g.vals, P, 32, 8, g.sort_hist, g.digit_total, sort_items(P), st, g.rect, g.rect_sorted);
        if (ob != order_buf) HIP_OK(hipMemcpyAsync(g.vals[order_buf], g.vals[ob], (size_t)P * 4, hipMemcpyDeviceToDevice, st));
        gsr_launch_scan_tiles(P, g.vals[order_buf], g.rect, g.rect_sorted, g.offsets, g.block_sums, g.block_first, bf_cap,
                              g.num_rendered + 4, nullptr, 0u, true, st);
    }
    const uint64_t R64 = ((uint64_t)hw_slot.host[2] << 32) | (uint64_t)hw_slot.host[0];
    if (R64 > 0x7FFFFFFFull) return fail(GSR_ERR_UNSUPPORTED, "more than 2^31-1 tile instances");
    const int64_t R = (int64_t)R64;
    *num_rendered = (int32_t)R;
    g_last_R[dev_id].store(R);
    const size_t need_bytes = gsr_binning_bytes(R, n_tiles);
    if (!bbase || need_bytes > spec_bytes) bbase = (char*)binning_resize(binning_user, need_bytes);
    if (!bbase || !ibase) return fail(GSR_ERR_ALLOC, "binning / image buffer resize returned NULL");
    GsrBinning b = gsr_carve_binning(bbase, R);
    GsrImage im = gsr_carve_image(ibase, cam.W, cam.H);
    wait_ev.commit(GSR_STAGE_R_WAIT, st);
    float4* goffset_splats = settings->no_backward ? nullptr : g.splats;

    int list_buf = 0;
    if (R > 0 && plan.fused) {
        const uint2* block_first = g.block_first;
        const int64_t nblk = (R + GSR_TS_ITEMS - 1) / GSR_TS_ITEMS;
        {   StageTimer t(GSR_STAGE_EMIT, st);
            if ((uint64_t)nblk + 1 > (uint64_t)bf_cap) {      // more than ~64 tiles per Gaussian: table sized by R instead
                gsr_launch_fill_block_first(P, g.offsets, b.block_first, (uint32_t)(nblk + 2), st);
                block_first = b.block_first;
            }
            gsr_launch_tile_sort_level1(plan, R, cam.gx, block_first, g.offsets, g.rect_sorted, g.vals[order_buf], b.keys[0],
                                        b.sort_hist, b.digit_total, b.bucket_base, b.blk2_start, goffset_splats, st);
        }
        STAGE_CHECK("emit + level-1 sort");
        {   StageTimer t(GSR_STAGE_TILE_SORT, st);
            gsr_launch_tile_sort_level2(plan, R, n_tiles, b.keys[0], b.vals[0], b.bucket_base, b.blk2_start, b.hist2, b.tile_base,
                                        im.ranges, st);
        }
        STAGE_CHECK("level-2 sort + ranges");
    } else if (R > 0) {
        const bool key16 = n_tiles <= 65536;     // (only reachable through the A/B option: <= 65536 tiles normally take the fused path)
        {   StageTimer t(GSR_STAGE_EMIT, st);
            gsr_launch_emit(P, cam.gx, g.vals[order_buf], g.offsets, g.rect_sorted, b.keys[0], key16, b.vals[0], goffset_splats, st);
        }
        STAGE_CHECK("emit");
        {   StageTimer t(GSR_STAGE_TILE_SORT, st);
            if (key16) {
                uint16_t* k16[2] = {(uint16_t*)b.keys[0], (uint16_t*)b.keys[1]};
                // always two passes (zero high bits sort harmlessly), so that the list lands in vals[0] like the fused path's
                const int kb = bits_for((uint32_t)n_tiles) < 9 ? 9 : bits_for((uint32_t)n_tiles);
                list_buf = gsr_radix_sort_pairs_k16(k16, b.vals, R, kb, GSR_TILE_DIGIT_BITS, b.sort_hist,
                                                    b.digit_total, sort_items(R), st);
            } else {
                list_buf = gsr_radix_sort_pairs(b.keys, b.vals, R, bits_for((uint32_t)n_tiles), GSR_TILE_DIGIT_BITS, b.sort_hist,
                                                b.digit_total, sort_items(R), st);
            }
        }
        STAGE_CHECK("tile sort");
        {   StageTimer t(GSR_STAGE_RANGES, st);
            gsr_launch_ranges(R, n_tiles, b.keys[list_buf], key16, im.ranges, /*already_zeroed=*/true, st);
        }
        STAGE_CHECK("ranges");
    } else if (plan.fused) {
        HIP_OK(hipMemsetAsync(im.ranges, 0, sizeof(uint2) * (size_t)n_tiles, st));
    }
    {   StageTimer t(GSR_STAGE_RENDER, st);
        gsr_launch_render_forward(cam, im.ranges, b.vals[list_buf], g.splats, settings->no_backward ? nullptr : im.final_T,
                                  settings->no_backward ? nullptr : im.n_contrib, settings->no_backward ? nullptr : im.block_steps,
                                  out_color, out_invdepth, g_render_fwd_variant, g_count_on ? counters_for_current_device() : nullptr, st, 0, -1, comp);
    }
    STAGE_CHECK("render");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}


// gsr_rasterize_forward and, with `extra`, gsr_rasterize_forward_composite
static int rasterize_forward(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                             const float* colors_precomp, const float* opacities, const float* scales,
                             const float* rotations, const float* cov3D_precomp, GsrResizeFn geom_resize, void* geom_user,
                             GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize, void* image_user,
                             float* out_color, float* out_invdepth, int32_t* radii, int32_t* num_rendered, const GsrCompositeOut* extra,
                             void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCompositeDev comp{nullptr, nullptr, nullptr};
    if (extra) { comp.out_alpha = extra->out_alpha; comp.bg_image = extra->bg_image; }
    const bool composite = extra != nullptr;      // (P == 0: the composite call blends the background, see below)
    GsrCamDev cam;
    int rc = make_cam(settings, M, cam);
    if (rc != GSR_OK) return rc;
    rc = check_inputs(P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, cam.sh_degree);
    if (rc != GSR_OK) return rc;
    rc = check_split_sh(settings, P, M, shs, false);
    if (rc != GSR_OK) return rc;
    if (!out_color || !num_rendered) return fail(GSR_ERR_INVALID_ARG, "out_color / num_rendered are NULL");
    const size_t npix = (size_t)cam.W * cam.H;
    *num_rendered = 0;
    if (P == 0 && composite) {
        // the composite contract: alpha = 0 and color = B in the band (zeros outside it) -- the blend over empty tile ranges, inference
        // build: no state is kept, the composite backward needs none for P == 0
        if (!image_resize) return fail(GSR_ERR_INVALID_ARG, "resize callbacks are NULL");
        char* ibase = (char*)image_resize(image_user, gsr_image_bytes(cam.W, cam.H));
        if (!ibase) return fail(GSR_ERR_ALLOC, "image buffer resize returned NULL");
        GsrImage im = gsr_carve_image(ibase, cam.W, cam.H);
        HIP_OK(hipMemsetAsync(im.ranges, 0, sizeof(uint2) * (size_t)cam.gx * cam.gy, st));
        HIP_OK(hipMemsetAsync(out_color, 0, npix * 3 * sizeof(float), st));
        if (out_invdepth) HIP_OK(hipMemsetAsync(out_invdepth, 0, npix * sizeof(float), st));
        if (comp.out_alpha) HIP_OK(hipMemsetAsync(comp.out_alpha, 0, npix * sizeof(float), st));
        gsr_launch_render_forward(cam, im.ranges, nullptr, nullptr, nullptr, nullptr, nullptr, out_color, out_invdepth, 0, nullptr, st, 0, -1, &comp);
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    if (P == 0) {   // reference behaviour: zero image (not background), nothing else touched
        HIP_OK(hipMemsetAsync(out_color, 0, npix * 3 * sizeof(float), st));
        if (out_invdepth) HIP_OK(hipMemsetAsync(out_invdepth, 0, npix * sizeof(float), st));
        return GSR_OK;
    }
    if (!radii) return fail(GSR_ERR_INVALID_ARG, "radii is NULL");
    if (!geom_resize || !binning_resize || !image_resize) return fail(GSR_ERR_INVALID_ARG, "resize callbacks are NULL");

    char* gbase = (char*)geom_resize(geom_user, gsr_geometry_bytes(P));
    if (!gbase) return fail(GSR_ERR_ALLOC, "geometry buffer resize returned NULL");
    GsrGeom g = gsr_carve_geom(gbase, P);
    HostWordLease lease;
    rc = lease_host_word(lease, st);
    if (rc != GSR_OK) return rc;
    uint32_t seq;
    const GsrFrameStatsDev fs = frame_stats_for(lease, g, seq);
    int n_range;
    {   StageTimer t(GSR_STAGE_PREPROCESS, st);
        n_range = gsr_launch_preprocess(cam, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, g, radii, fs, st);
    }
    STAGE_CHECK("preprocess");
    return bin_and_render(settings, cam, P, g, lease, seq, n_range, binning_resize, binning_user, image_resize, image_user, out_color, out_invdepth,
                          num_rendered, st, (comp.out_alpha || comp.bg_image) ? &comp : nullptr);
}

int gsr_rasterize_forward(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                          const float* colors_precomp, const float* opacities, const float* scales,
                          const float* rotations, const float* cov3D_precomp, GsrResizeFn geom_resize, void* geom_user,
                          GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize, void* image_user,
                          float* out_color, float* out_invdepth, int32_t* radii, int32_t* num_rendered, void* stream) {
    return rasterize_forward(settings, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, geom_resize, geom_user,
                             binning_resize, binning_user, image_resize, image_user, out_color, out_invdepth, radii, num_rendered, nullptr, stream);
}

int gsr_rasterize_forward_composite(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                                    const float* colors_precomp, const float* opacities, const float* scales,
                                    const float* rotations, const float* cov3D_precomp, GsrResizeFn geom_resize, void* geom_user,
                                    GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize, void* image_user,
                                    float* out_color, float* out_invdepth, int32_t* radii, int32_t* num_rendered,
                                    const GsrCompositeOut* extra, void* stream) {
    if (!extra) return fail(GSR_ERR_INVALID_ARG, "extra (GsrCompositeOut) is NULL");
    return rasterize_forward(settings, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, geom_resize, geom_user,
                             binning_resize, binning_user, image_resize, image_user, out_color, out_invdepth, radii, num_rendered, extra, stream);
}

int gsr_preprocess_forward(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                           const float* colors_precomp, const float* opacities, const float* scales, const float* rotations,
                           const float* cov3D_precomp, void* geom_scratch, int32_t* radii, float* splat_records,
                           void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    int rc = make_cam(settings, M, cam);
    if (rc != GSR_OK) return rc;
    rc = check_inputs(P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, cam.sh_degree);
    if (rc != GSR_OK) return rc;
    rc = check_split_sh(settings, P, M, shs, false);
    if (rc != GSR_OK) return rc;
    if (P == 0) return GSR_OK;
    if (!geom_scratch || !radii || !splat_records) return fail(GSR_ERR_INVALID_ARG, "geom_scratch / radii / splat_records are NULL");
    if ((uintptr_t)splat_records & 15) return fail(GSR_ERR_INVALID_ARG, "splat_records must be 16-byte aligned");
    // the records leave this rank: rectangles and tile counts are those of the FULL frame, whatever band the settings name
    cam.tile_y0 = 0;
    cam.tile_y1 = cam.gy;
    GsrGeom g = gsr_carve_geom((char*)geom_scratch, P);
    g.splats = reinterpret_cast<float4*>(splat_records);
    {   StageTimer t(GSR_STAGE_PREPROCESS, st);
        GsrFrameStatsDev none;      // nothing is binned here: no frame statistics
        none.state = nullptr; none.frame = nullptr; none.wg_range = nullptr; none.host_word = nullptr; none.seq = 0;
        gsr_launch_preprocess(cam, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, g, radii, none, st);
    }
    STAGE_CHECK("preprocess (shard)");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// shared body of gsr_rasterize_from_splats (64-byte records) / gsr_rasterize_from_packed (48-byte records)
static int rasterize_from_records(const GsrRasterSettings* settings, int P, const float* records, bool packed, int seg_rows, GsrResizeFn geom_resize,
                                  void* geom_user, GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize,
                                  void* image_user, float* out_color, float* out_invdepth, int32_t* num_rendered, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    int rc = make_cam(settings, 0, cam);
    if (rc != GSR_OK) return rc;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (!out_color || !num_rendered) return fail(GSR_ERR_INVALID_ARG, "out_color / num_rendered are NULL");
    const size_t npix = (size_t)cam.W * cam.H;
    *num_rendered = 0;
    if (P == 0) {
        // No record reached this rank's band while the scene itself is not empty (the caller renders a band of a sharded frame):
        // the band's pixels are what the blend leaves where no splat lands -- the BACKGROUND (T = 1), not the zero image of the
        // reference's P == 0 early-out (with a white or random background the gathered frame, and the loss, differed
        // from one GPU's).  The blend runs over empty tile ranges.
        HIP_OK(hipMemsetAsync(out_color, 0, npix * 3 * sizeof(float), st));
        if (out_invdepth) HIP_OK(hipMemsetAsync(out_invdepth, 0, npix * sizeof(float), st));
        if (!image_resize) return fail(GSR_ERR_INVALID_ARG, "resize callbacks are NULL");
        char* ibase = (char*)image_resize(image_user, gsr_image_bytes(cam.W, cam.H));
        if (!ibase) return fail(GSR_ERR_ALLOC, "image buffer resize returned NULL");
        GsrImage im = gsr_carve_image(ibase, cam.W, cam.H);
        HIP_OK(hipMemsetAsync(im.ranges, 0, sizeof(uint2) * (size_t)cam.gx * cam.gy, st));
        const bool nb = settings->no_backward != 0;
        gsr_launch_render_forward(cam, im.ranges, nullptr, nullptr, nb ? nullptr : im.final_T, nb ? nullptr : im.n_contrib,
                                  nb ? nullptr : im.block_steps, out_color, out_invdepth, 0, nullptr, st);
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    if (!records) return fail(GSR_ERR_INVALID_ARG, "records pointer is NULL");
    if ((uintptr_t)records & 15) return fail(GSR_ERR_INVALID_ARG, "records must be 16-byte aligned");
    if (!geom_resize || !binning_resize || !image_resize) return fail(GSR_ERR_INVALID_ARG, "resize callbacks are NULL");
    char* gbase = (char*)geom_resize(geom_user, gsr_geometry_bytes(P));
    if (!gbase) return fail(GSR_ERR_ALLOC, "geometry buffer resize returned NULL");
    GsrGeom g = gsr_carve_geom(gbase, P);
    HostWordLease lease;
    rc = lease_host_word(lease, st);
    if (rc != GSR_OK) return rc;
    uint32_t seq;
    const GsrFrameStatsDev fs = frame_stats_for(lease, g, seq);
    int n_range;
    {   StageTimer t(GSR_STAGE_PREPROCESS, st);
        if (packed) n_range = gsr_launch_ingest_packed(P, records, cam.tile_y0, cam.tile_y1, g.splats, g.rect, g.tiles, g.keys[0], g.vals[0], fs, seg_rows, st);
        else n_range = gsr_launch_splat_ingest(P, records, cam.tile_y0, cam.tile_y1, g.splats, g.rect, g.tiles, g.keys[0], g.vals[0], fs, st);
    }
    STAGE_CHECK("splat ingest");
    return bin_and_render(settings, cam, P, g, lease, seq, n_range, binning_resize, binning_user, image_resize, image_user, out_color, out_invdepth,
                          num_rendered, st);
}

int gsr_rasterize_from_splats(const GsrRasterSettings* settings, int P, const float* splat_records, GsrResizeFn geom_resize,
                              void* geom_user, GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize,
                              void* image_user, float* out_color, float* out_invdepth, int32_t* num_rendered, void* stream) {
    return rasterize_from_records(settings, P, splat_records, false, 0, geom_resize, geom_user, binning_resize, binning_user, image_resize,
                                  image_user, out_color, out_invdepth, num_rendered, stream);
}

int gsr_rasterize_from_packed(const GsrRasterSettings* settings, int P, const float* packed_records, GsrResizeFn geom_resize,
                              void* geom_user, GsrResizeFn binning_resize, void* binning_user, GsrResizeFn image_resize,
                              void* image_user, float* out_color, float* out_invdepth, int32_t* num_rendered, void* stream) {
    return rasterize_from_records(settings, P, packed_records, true, 0, geom_resize, geom_user, binning_resize, binning_user, image_resize,
                                  image_user, out_color, out_invdepth, num_rendered, stream);
}

int gsr_rasterize_from_segments(const GsrRasterSettings* settings, int n_segments, int capacity, const float* segments,
                                GsrResizeFn geom_resize, void* geom_user, GsrResizeFn binning_resize, void* binning_user,
                                GsrResizeFn image_resize, void* image_user, float* out_color, float* out_invdepth,
                                int32_t* num_rendered, void* stream) {
    if (n_segments < 1 || n_segments > GSR_MAX_BANDS) return fail(GSR_ERR_INVALID_ARG, "n_segments must be 1..64");
    if (capacity < 1) return fail(GSR_ERR_INVALID_ARG, "capacity < 1");
    const int64_t rows = (int64_t)n_segments * ((int64_t)capacity + 1);
    if (rows > 0x7FFFFFFFll) return fail(GSR_ERR_UNSUPPORTED, "n_segments * (capacity + 1) exceeds 2^31-1 rows");
    return rasterize_from_records(settings, (int)rows, segments, true, capacity + 1, geom_resize, geom_user, binning_resize, binning_user,
                                  image_resize, image_user, out_color, out_invdepth, num_rendered, stream);
}

// ---- Gaussian-sharded exchange (route.hip) ----
static int check_bands(int n_bands, const int32_t* band_bounds) {
    if (n_bands < 1 || n_bands > GSR_MAX_BANDS) return fail(GSR_ERR_UNSUPPORTED, "n_bands must be 1..64");
    if (!band_bounds) return fail(GSR_ERR_INVALID_ARG, "band_bounds is NULL");
    for (int b = 0; b < n_bands; ++b)
        if (band_bounds[b] > band_bounds[b + 1] || band_bounds[b] < 0) return fail(GSR_ERR_INVALID_ARG, "band_bounds must be non-negative and non-decreasing");
    return GSR_OK;
}

size_t gsr_route_scratch_bytes(int P, int n_bands) { return gsr_route_scratch_bytes_impl(P, n_bands < 1 ? 1 : n_bands); }

int gsr_route_count(int P, const float* splat_records, int n_bands, const int32_t* band_bounds, void* scratch, uint32_t* band_counts,
                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_bands(n_bands, band_bounds);
    if (rc != GSR_OK) return rc;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (!band_counts) return fail(GSR_ERR_INVALID_ARG, "band_counts is NULL");
    if (P == 0) { HIP_OK(hipMemsetAsync(band_counts, 0, sizeof(uint32_t) * (size_t)n_bands, st)); return GSR_OK; }
    if (!splat_records || !scratch) return fail(GSR_ERR_INVALID_ARG, "splat_records / scratch are NULL");
    if ((uintptr_t)splat_records & 15) return fail(GSR_ERR_INVALID_ARG, "splat_records must be 16-byte aligned");
    gsr_launch_route_count(P, splat_records, n_bands, band_bounds, (uint32_t*)scratch, band_counts, st);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_route_pack(int P, const float* splat_records, int n_bands, const int32_t* band_bounds, const int64_t* band_offsets,
                   const void* scratch, float* packed, int32_t* send_ids, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_bands(n_bands, band_bounds);
    if (rc != GSR_OK) return rc;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!band_offsets) return fail(GSR_ERR_INVALID_ARG, "band_offsets is NULL");
    if (band_offsets[n_bands] == band_offsets[0]) return GSR_OK;      // nothing to send
    if (!splat_records || !scratch || !packed || !send_ids) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (((uintptr_t)splat_records | (uintptr_t)packed) & 15) return fail(GSR_ERR_INVALID_ARG, "splat_records / packed must be 16-byte aligned");
    gsr_launch_route_pack(P, splat_records, n_bands, band_bounds, band_offsets, (const uint32_t*)scratch, packed, send_ids, 0xFFFFFFFFu,
                          nullptr, st);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_route_pack_fixed(int P, const float* splat_records, int n_bands, const int32_t* band_bounds, int capacity, const void* scratch,
                         const uint32_t* band_counts, float* packed, int32_t* send_ids, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_bands(n_bands, band_bounds);
    if (rc != GSR_OK) return rc;
    if (P < 0 || capacity < 1) return fail(GSR_ERR_INVALID_ARG, "P < 0 or capacity < 1");
    if (!packed || !send_ids) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)packed & 15) return fail(GSR_ERR_INVALID_ARG, "packed must be 16-byte aligned");
    const size_t seg_rows = (size_t)capacity + 1;
    // unused rows and header rows carry the id -1 (gsr_route_return skips them)
    HIP_OK(hipMemsetAsync(send_ids, 0xFF, sizeof(int32_t) * seg_rows * (size_t)n_bands, st));
    if (P == 0) {      // an empty shard still sends its (zero) headers
        for (int b = 0; b < n_bands; ++b) HIP_OK(hipMemsetAsync(packed + (size_t)b * seg_rows * 12, 0, 48, st));
        return GSR_OK;
    }
    if (!splat_records || !scratch || !band_counts) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)splat_records & 15) return fail(GSR_ERR_INVALID_ARG, "splat_records must be 16-byte aligned");
    int64_t off[GSR_MAX_BANDS + 1];
    for (int b = 0; b <= n_bands; ++b) off[b] = (int64_t)b * (int64_t)seg_rows + 1;      // first record row of segment b
    gsr_launch_route_pack(P, splat_records, n_bands, band_bounds, off, (const uint32_t*)scratch, packed, send_ids, (uint32_t)capacity,
                          band_counts, st);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_route_return(int P, int n_bands, const int64_t* band_offsets, const int32_t* send_ids, const float* returned,
                     float* splat_grads, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (P < 0 || n_bands < 1 || n_bands > GSR_MAX_BANDS) return fail(GSR_ERR_INVALID_ARG, "bad P / n_bands");
    if (P == 0) return GSR_OK;
    if (!band_offsets || !splat_grads) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    HIP_OK(hipMemsetAsync(splat_grads, 0, (size_t)P * 48, st));
    for (int b = 0; b < n_bands; ++b) {      // band order: fixed association order of the <= n_bands terms per Gaussian
        const int64_t n = band_offsets[b + 1] - band_offsets[b];
        if (n < 0) return fail(GSR_ERR_INVALID_ARG, "band_offsets must be non-decreasing");
        if (n == 0) continue;
        if (!send_ids || !returned) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
        gsr_launch_route_add_rows(n, send_ids + band_offsets[b], returned + band_offsets[b] * 12, splat_grads, st);
    }
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

size_t gsr_composite_grad_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return gsr_bg_grad_blocks((int64_t)width * height) * 3 * sizeof(double);
}

// gsr_backward_blend and, with `extra`, gsr_backward_blend_composite
static int backward_blend(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                          const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                          const float* dL_dout_invdepth, void* bwd_scratch, float** splat_grads_out, const GsrCompositeGrads* extra,
                          void* stream, bool absgrad = false) {
    hipStream_t st = (hipStream_t)stream;
#ifdef GSR_AB_VARIANTS
    if (absgrad) return fail(GSR_ERR_UNSUPPORTED, "gsr_backward_blend_abs is not part of the measurement build (-DGSR_AB_VARIANTS)");
#endif
    if (absgrad && g_render_bwd_variant != 0) return fail(GSR_ERR_UNSUPPORTED, "gsr_backward_blend_abs needs the default blend backward (render_bwd_variant 0)");
    GsrCamDev cam;
    int rc = make_cam(settings, 0, cam);
    if (rc != GSR_OK) return rc;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    GsrCompositeDev comp{nullptr, nullptr, nullptr};
    const bool bg_grad = extra && (extra->dL_dbg_image || extra->dL_dbg);
    if (extra) {
        comp.bg_image = extra->bg_image;
        comp.dL_dalpha = extra->dL_dout_alpha;
        if (extra->dL_dbg && !extra->scratch) return fail(GSR_ERR_INVALID_ARG, "dL_dbg needs scratch (gsr_composite_grad_scratch_bytes)");
        if (((uintptr_t)extra->scratch) & 7) return fail(GSR_ERR_INVALID_ARG, "composite gradient scratch must be 8-byte aligned");
        if (bg_grad && (!dL_dout_color || (P > 0 && !image_buffer)))
            return fail(GSR_ERR_INVALID_ARG, "dL_dbg_image / dL_dbg need dL_dout_color and the image buffer");
    }
    if (bg_grad) {
        // every pixel of the band, also those no Gaussian reaches; P == 0: the forward kept no state and T_final = 1 everywhere.  (Only the image
        // buffer has been checked so far: the view's other pointers may be NULL here and are not looked at.)
        const float* final_T = P > 0 ? saved_frame(cam, P, num_rendered, geom_buffer, binning_buffer, image_buffer).final_T : nullptr;
        const GsrBandRows band = gsr_band_rows(cam);
        StageTimer t(GSR_STAGE_RENDER_BWD, st);
        gsr_launch_bg_grad((int64_t)cam.W * cam.H, cam.W, band.row0, band.row1, final_T, dL_dout_color, extra->dL_dbg_image, extra->dL_dbg,
                           (double*)extra->scratch, st);
    }
    if (P == 0) { HIP_OK(hipGetLastError()); return GSR_OK; }
    if (!geom_buffer || !binning_buffer || !image_buffer || !dL_dout_color || !bwd_scratch)
        return fail(GSR_ERR_INVALID_ARG, "state buffers / dL_dout_color / bwd_scratch are NULL");
    const GsrCompositeDev* compp = (comp.bg_image || comp.dL_dalpha) ? &comp : nullptr;
    GsrSavedFrame f = saved_frame(cam, P, num_rendered, geom_buffer, binning_buffer, image_buffer);
    if (!g_bwd_heavy_first) f.tile_order = nullptr;      // tiles in index order
    GsrBwdScratch w = gsr_carve_bwd((char*)bwd_scratch, P, num_rendered);
    float* sg = w.splat_grads;
    if (splat_grads_out) *splat_grads_out = sg;
    {   StageTimer t(GSR_STAGE_RENDER_BWD, st);
        if (g_render_bwd_variant == 1 || num_rendered <= 0) {
            HIP_OK(hipMemsetAsync(sg, 0, (size_t)P * 12 * sizeof(float), st));
            if (num_rendered > 0)
                gsr_launch_render_backward(cam, f.ranges, f.point_list, f.splats, f.final_T, f.n_contrib, f.block_steps, nullptr,
                                           dL_dout_color, dL_dout_invdepth, sg, nullptr, nullptr, num_rendered, 1, 0, nullptr, st);
        } else if (absgrad) {
            gsr_launch_render_backward_abs(cam, f, dL_dout_color, dL_dout_invdepth, w.inst_grads, w.inst_flag, num_rendered, g_bwd_heavy_first,
                                           g_count_on ? counters_for_current_device() : nullptr, st, compp);
        } else {
            // (the flag words of the instances are cleared by the launcher: in the plan kernel's launch, or with a fill)
            gsr_launch_render_backward_composite(cam, f, dL_dout_color, dL_dout_invdepth, nullptr, w.inst_grads, w.inst_flag, num_rendered,
                                                 g_render_bwd_variant, g_bwd_heavy_first, g_count_on ? counters_for_current_device() : nullptr, st, compp);
        }
    }
    STAGE_CHECK("render backward blend");
    if (g_render_bwd_variant != 1 && num_rendered > 0) {
        StageTimer t(GSR_STAGE_GATHER_BWD, st);
        gsr_launch_reduce_instances(P, num_rendered, f.order, f.offsets, f.splats, w.inst_grads, w.inst_flag, sg, w.unit_first, w.unit_piece, st);
        if (absgrad) gsr_launch_absgrad_reduce(P, num_rendered, f, w.inst_grads, w.inst_flag, sg, st);
    }
    STAGE_CHECK("render backward reduce");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_backward_blend(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                       const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                       const float* dL_dout_invdepth, void* bwd_scratch, float** splat_grads_out, void* stream) {
    return backward_blend(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, dL_dout_color, dL_dout_invdepth, bwd_scratch,
                          splat_grads_out, nullptr, stream);
}

int gsr_backward_blend_composite(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                                 const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                                 const float* dL_dout_invdepth, void* bwd_scratch, float** splat_grads_out,
                                 const GsrCompositeGrads* extra, void* stream) {
    if (!extra) return fail(GSR_ERR_INVALID_ARG, "extra (GsrCompositeGrads) is NULL");
    return backward_blend(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, dL_dout_color, dL_dout_invdepth, bwd_scratch,
                          splat_grads_out, extra, stream);
}

int gsr_backward_blend_abs(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                           const void* binning_buffer, const void* image_buffer, const float* dL_dout_color,
                           const float* dL_dout_invdepth, void* bwd_scratch, float** splat_grads_out,
                           const GsrCompositeGrads* extra, void* stream) {
    return backward_blend(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, dL_dout_color, dL_dout_invdepth, bwd_scratch,
                          splat_grads_out, extra, stream, true);
}

int gsr_absgrad_from_records(const GsrRasterSettings* settings, int P, const float* splat_grads, float* means2D_abs, void* stream) {
    GsrCamDev cam;
    int rc = make_cam(settings, 0, cam);
    if (rc != GSR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!splat_grads || !means2D_abs) return fail(GSR_ERR_INVALID_ARG, "splat_grads / means2D_abs are NULL");
    if (((uintptr_t)splat_grads) & 7) return fail(GSR_ERR_INVALID_ARG, "splat_grads must be 8-byte aligned");
    gsr_launch_absgrad_from_records(P, cam.W, cam.H, splat_grads, means2D_abs, st);
    STAGE_CHECK("absgrad from records");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// The checks the read-only calls on a saved frame share (gsr_contribution_stats, gsr_pixel_probe, gsr_render_features, gsr_render_features_backward), in
// the order their errors are reported: the settings, the counts, `own_error` -- what the call found wrong with its own arguments (NULL: nothing), which
// needs none of the state -- and the state buffers.
static int reader_args(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer, const void* binning_buffer,
                       const void* image_buffer, const char* own_error, GsrCamDev& cam) {
    int rc = make_cam(settings, 0, cam);
    if (rc != GSR_OK) return rc;
    if (P < 0 || num_rendered < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0 or num_rendered < 0");
    if (own_error) return fail(GSR_ERR_INVALID_ARG, own_error);
    if (P > 0 && num_rendered > 0 && (!geom_buffer || !binning_buffer || !image_buffer))
        return fail(GSR_ERR_INVALID_ARG, "state buffers are NULL (run the forward with no_backward == 0)");
    return GSR_OK;
}

size_t gsr_contribution_scratch_bytes(int P, int64_t R) { (void)P; return gsr_carve_contrib(nullptr, R).bytes; }

int gsr_contribution_stats(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                           const void* binning_buffer, const void* image_buffer, const float* pixel_weight, void* scratch,
                           const GsrContribOut* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t R = num_rendered;
    const char* own = !out                                             ? "out (GsrContribOut) is NULL"
                      : (out->accumulate != 0 && out->accumulate != 1) ? "GsrContribOut.accumulate must be 0 or 1"
                      : (R > 0 && !scratch)                            ? "scratch is NULL (gsr_contribution_scratch_bytes)"
                      : (((uintptr_t)scratch) & 15)                    ? "contribution scratch must be 16-byte aligned"
                                                                       : nullptr;
    GsrCamDev cam;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    if (!out->accumulate && P > 0) {      // every row is written: Gaussians without instances keep these zeros
        if (out->weight_sum) HIP_OK(hipMemsetAsync(out->weight_sum, 0, (size_t)P * sizeof(float), st));
        if (out->weight_max) HIP_OK(hipMemsetAsync(out->weight_max, 0, (size_t)P * sizeof(float), st));
        if (out->pixel_count) HIP_OK(hipMemsetAsync(out->pixel_count, 0, (size_t)P * sizeof(int32_t), st));
    }
    if (P == 0 || R == 0) { HIP_OK(hipGetLastError()); return GSR_OK; }
    gsr_launch_contribution_stats(cam, P, R, saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer), pixel_weight,
                                  gsr_carve_contrib((char*)scratch, R), out->weight_sum, out->weight_max, out->pixel_count, out->accumulate, st);
    STAGE_CHECK("contribution statistics");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_pixel_probe(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer, const void* binning_buffer,
                    const void* image_buffer, const GsrPixelProbeOut* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* own = !out                                                 ? "out (GsrPixelProbeOut) is NULL"
                      : !(out->threshold > 0.0f && out->threshold < 1.0f) ? "GsrPixelProbeOut.threshold must be inside (0, 1)"      // (a NaN fails both comparisons)
                                                                           : nullptr;
    GsrCamDev cam;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    const int64_t R = num_rendered;
    if (P == 0 || R == 0) {      // no state to read: the defaults over the band
        gsr_launch_pixel_probe_defaults(cam, *out, st);
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    gsr_launch_pixel_probe(cam, saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer), *out, st);
    STAGE_CHECK("pixel probe");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_render_features(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer, const void* binning_buffer,
                        const void* image_buffer, const float* features, int C, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    const char* own = (C < 1 || C > GSR_MAX_FEATURE_CHANNELS) ? "C (feature channels) must be inside [1, 1024]" : nullptr;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    if (P > 0 && (!features || !out)) return fail(GSR_ERR_INVALID_ARG, "features / out are NULL");
    const int64_t R = num_rendered;
    if (P == 0 || R == 0) {      // no state to read: zeros over the band
        if (out) gsr_launch_render_features_defaults(cam, C, out, st);
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    gsr_launch_render_features(cam, saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer), features, C, out, st);
    STAGE_CHECK("render features");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

size_t gsr_feature_grad_scratch_bytes(int P, int64_t R, int C) { (void)P; return gsr_carve_feature_grad(nullptr, R, C < 1 ? 1 : C).bytes; }

int gsr_render_features_backward(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                                 const void* binning_buffer, const void* image_buffer, const float* dL_dout, int C, void* scratch,
                                 float* dL_dfeatures, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    const char* own = (C < 1 || C > GSR_MAX_FEATURE_CHANNELS) ? "C (feature channels) must be inside [1, 1024]" : nullptr;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    if (P > 0 && (!dL_dout || !dL_dfeatures)) return fail(GSR_ERR_INVALID_ARG, "dL_dout / dL_dfeatures are NULL");
    const int64_t R = num_rendered;
    if (R > 0 && !scratch) return fail(GSR_ERR_INVALID_ARG, "scratch is NULL (gsr_feature_grad_scratch_bytes)");
    if (((uintptr_t)scratch) & 15) return fail(GSR_ERR_INVALID_ARG, "feature gradient scratch must be 16-byte aligned");
    // every row is written: Gaussians without instances keep these zeros
    if (P > 0) HIP_OK(hipMemsetAsync(dL_dfeatures, 0, (size_t)P * (size_t)C * sizeof(float), st));
    if (P == 0 || R == 0) { HIP_OK(hipGetLastError()); return GSR_OK; }
    gsr_launch_render_features_backward(cam, P, R, saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer), dL_dout, C,
                                        gsr_carve_feature_grad((char*)scratch, R, C), dL_dfeatures, st);
    STAGE_CHECK("render features backward");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_render_features_backward_geometry(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer,
                                          const void* binning_buffer, const void* image_buffer, const float* features, const float* dL_dout,
                                          int C, void* bwd_scratch, float** splat_grads_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    const char* own = (C < 1 || C > GSR_MAX_FEATURE_CHANNELS) ? "C (feature channels) must be inside [1, 1024]"
                      : !splat_grads_out                      ? "splat_grads_out is NULL"
                                                              : nullptr;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    *splat_grads_out = nullptr;
    if (P > 0 && (!features || !dL_dout)) return fail(GSR_ERR_INVALID_ARG, "features / dL_dout are NULL");
    if (P > 0 && !bwd_scratch) return fail(GSR_ERR_INVALID_ARG, "bwd_scratch is NULL (gsr_backward_scratch_bytes)");
    if (((uintptr_t)bwd_scratch) & 15) return fail(GSR_ERR_INVALID_ARG, "backward scratch must be 16-byte aligned");
    if (P == 0) { HIP_OK(hipGetLastError()); return GSR_OK; }
    const int64_t R = num_rendered;
    GsrBwdScratch w = gsr_carve_bwd((char*)bwd_scratch, P, R);
    *splat_grads_out = w.splat_grads;
    if (R == 0) {      // no state to read: zero rows
        HIP_OK(hipMemsetAsync(w.splat_grads, 0, (size_t)P * 12 * sizeof(float), st));
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    const GsrSavedFrame f = saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer);
    {   StageTimer t(GSR_STAGE_RENDER_BWD, st);
        gsr_launch_feature_geometry_walks(cam, R, f, g_bwd_heavy_first, features, dL_dout, C, w.inst_grads, w.inst_flag, st);
    }
    STAGE_CHECK("render features backward geometry walk");
    {   StageTimer t(GSR_STAGE_GATHER_BWD, st);
        gsr_launch_reduce_instances(P, R, f.order, f.offsets, f.splats, w.inst_grads, w.inst_flag, w.splat_grads, w.unit_first, w.unit_piece, st);
    }
    STAGE_CHECK("render features backward geometry reduce");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_distortion(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer, const void* binning_buffer,
                   const void* image_buffer, const GsrDistortionOut* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* own = !out                                             ? "out (GsrDistortionOut) is NULL"
                      : !out->distortion                               ? "GsrDistortionOut.distortion is NULL"
                      : (out->depth_mode != 0 && out->depth_mode != 1) ? "GsrDistortionOut.depth_mode must be 0 (z) or 1 (1/z)"
                                                                       : nullptr;
    GsrCamDev cam;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    const int64_t R = num_rendered;
    if (P == 0 || R == 0) {      // no state to read: zeros over the band
        gsr_launch_distortion_defaults(cam, out->distortion, out->saved, st);
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    gsr_launch_distortion(cam, saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer), out->distortion, out->saved, out->depth_mode, st);
    STAGE_CHECK("distortion");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_distortion_backward(const GsrRasterSettings* settings, int P, int32_t num_rendered, const void* geom_buffer, const void* binning_buffer,
                            const void* image_buffer, const float* dL_ddistortion, const float* saved, int depth_mode, void* bwd_scratch,
                            float** splat_grads_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    const char* own = (depth_mode != 0 && depth_mode != 1) ? "depth_mode must be 0 (z) or 1 (1/z)"
                      : !splat_grads_out                   ? "splat_grads_out is NULL"
                                                           : nullptr;
    int rc = reader_args(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, own, cam);
    if (rc != GSR_OK) return rc;
    *splat_grads_out = nullptr;
    if (P > 0 && !bwd_scratch) return fail(GSR_ERR_INVALID_ARG, "bwd_scratch is NULL (gsr_backward_scratch_bytes)");
    if (((uintptr_t)bwd_scratch) & 15) return fail(GSR_ERR_INVALID_ARG, "backward scratch must be 16-byte aligned");
    const int64_t R = num_rendered;
    if (P > 0 && R > 0 && (!dL_ddistortion || !saved)) return fail(GSR_ERR_INVALID_ARG, "dL_ddistortion / saved are NULL");
    if (P == 0) { HIP_OK(hipGetLastError()); return GSR_OK; }
    GsrBwdScratch w = gsr_carve_bwd((char*)bwd_scratch, P, R);
    *splat_grads_out = w.splat_grads;
    if (R == 0) {      // no state to read: zero rows
        HIP_OK(hipMemsetAsync(w.splat_grads, 0, (size_t)P * 12 * sizeof(float), st));
        HIP_OK(hipGetLastError());
        return GSR_OK;
    }
    const GsrSavedFrame f = saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer);
    {   StageTimer t(GSR_STAGE_RENDER_BWD, st);
        gsr_launch_distortion_walk(cam, R, f, g_bwd_heavy_first, dL_ddistortion, saved, depth_mode, w.inst_grads, w.inst_flag, st);
    }
    STAGE_CHECK("distortion backward walk");
    {   StageTimer t(GSR_STAGE_GATHER_BWD, st);
        gsr_launch_reduce_instances(P, R, f.order, f.offsets, f.splats, w.inst_grads, w.inst_flag, w.splat_grads, w.unit_first, w.unit_piece, st);
    }
    STAGE_CHECK("distortion backward reduce");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// gsr_backward_preprocess and, with `camera`, gsr_backward_preprocess_camera
static int backward_preprocess(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                               const float* colors_precomp, const float* opacities, const float* scales,
                               const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                               const void* geom_buffer, const float* splat_grads, float* dL_dmeans2D, float* dL_dcolors,
                               float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                               float* dL_drotations, const GsrCameraGrads* camera, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GsrCamDev cam;
    int rc = make_cam(settings, M, cam);
    if (rc != GSR_OK) return rc;
    rc = check_inputs(P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, cam.sh_degree);
    if (rc != GSR_OK) return rc;
    rc = check_split_sh(settings, P, M, shs, true);
    if (rc != GSR_OK) return rc;
    if (camera) {
        if (!camera->dL_dviewmatrix || !camera->dL_dprojmatrix || !camera->dL_dcampos)
            return fail(GSR_ERR_INVALID_ARG, "camera gradient outputs are NULL");
        if (P > 0 && !camera->scratch) return fail(GSR_ERR_INVALID_ARG, "camera gradient scratch is NULL");
        if (((uintptr_t)camera->scratch) & 7) return fail(GSR_ERR_INVALID_ARG, "camera gradient scratch must be 8-byte aligned");
    }
    if (P == 0) {
        if (camera) {      // no Gaussian, no gradient
            HIP_OK(hipMemsetAsync(camera->dL_dviewmatrix, 0, 16 * sizeof(float), st));
            HIP_OK(hipMemsetAsync(camera->dL_dprojmatrix, 0, 16 * sizeof(float), st));
            HIP_OK(hipMemsetAsync(camera->dL_dcampos, 0, 3 * sizeof(float), st));
        }
        return GSR_OK;
    }
    (void)geom_buffer;      // the colour clamp bits are recomputed; a NULL geometry buffer is accepted (Gaussian-sharded backward)
    if (!radii || !splat_grads) return fail(GSR_ERR_INVALID_ARG, "radii / splat_grads are NULL");
    if (!dL_dmeans2D || !dL_dopacity || !dL_dmeans3D) return fail(GSR_ERR_INVALID_ARG, "gradient outputs are NULL");
    if (colors_precomp && !dL_dcolors) return fail(GSR_ERR_INVALID_ARG, "dL_dcolors is NULL");
    if (cov3D_precomp && !dL_dcov3D) return fail(GSR_ERR_INVALID_ARG, "dL_dcov3D is NULL");
    if (shs && !dL_dsh) return fail(GSR_ERR_INVALID_ARG, "dL_dsh is NULL");
    if (settings->sh_dc && ((((uintptr_t)dL_dsh) | ((uintptr_t)settings->dL_dsh_dc)) & 15))
        return fail(GSR_ERR_UNSUPPORTED, "split SH form needs 16-byte aligned dL_dsh / dL_dsh_dc");
    if (scales && (!dL_dscales || !dL_drotations)) return fail(GSR_ERR_INVALID_ARG, "dL_dscales / dL_drotations are NULL");
    GsrGeom g = gsr_carve_geom(geom_buffer ? (char*)geom_buffer : nullptr, P);
    GsrCamGradDev camg{};
    if (camera) {
        camg.partials = (double*)camera->scratch;
        camg.dview = camera->dL_dviewmatrix;
        camg.dproj = camera->dL_dprojmatrix;
        camg.dcampos = camera->dL_dcampos;
    }
    {   StageTimer t(GSR_STAGE_PREPROCESS_BWD, st);
        gsr_launch_preprocess_backward(cam, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                       radii, g, splat_grads, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D,
                                       dL_dsh, scales ? dL_dscales : nullptr, scales ? dL_drotations : nullptr, st,
                                       camera ? &camg : nullptr);
    }
    STAGE_CHECK("preprocess backward");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_backward_preprocess(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                            const float* colors_precomp, const float* opacities, const float* scales,
                            const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                            const void* geom_buffer, const float* splat_grads, float* dL_dmeans2D, float* dL_dcolors,
                            float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                            float* dL_drotations, void* stream) {
    return backward_preprocess(settings, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii,
                               geom_buffer, splat_grads, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
                               dL_dscales, dL_drotations, nullptr, stream);
}

size_t gsr_camera_grad_scratch_bytes(int P) { return gsr_camera_grad_rows(P) * 27 * sizeof(double); }

int gsr_backward_preprocess_camera(const GsrRasterSettings* settings, int P, int M, const float* means3D, const float* shs,
                                   const float* colors_precomp, const float* opacities, const float* scales,
                                   const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                   const void* geom_buffer, const float* splat_grads, float* dL_dmeans2D, float* dL_dcolors,
                                   float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                                   float* dL_drotations, const GsrCameraGrads* camera, void* stream) {
    if (!camera) return fail(GSR_ERR_INVALID_ARG, "camera is NULL");
    return backward_preprocess(settings, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii,
                               geom_buffer, splat_grads, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
                               dL_dscales, dL_drotations, camera, stream);
}

int gsr_backward_preprocess_sh_adam(const GsrRasterSettings* settings, int P, int M, const float* means3D, float* shs_rest,
                                    const float* opacities, const float* scales, const float* rotations,
                                    const float* cov3D_precomp, const int32_t* radii, const void* geom_buffer,
                                    const float* splat_grads, float* dL_dmeans2D, float* dL_dopacity, float* dL_dmeans3D,
                                    float* dL_dcov3D, float* dL_dscales, float* dL_drotations, const GsrShAdam* adam,
                                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!settings || !adam) return fail(GSR_ERR_INVALID_ARG, "settings / adam are NULL");
    GsrCamDev cam;
    int rc = make_cam(settings, M, cam);
    if (rc != GSR_OK) return rc;
    rc = check_inputs(P, M, means3D, shs_rest, nullptr, opacities, scales, rotations, cov3D_precomp, cam.sh_degree);
    if (rc != GSR_OK) return rc;
    rc = check_split_sh(settings, P, M, shs_rest, false);
    if (rc != GSR_OK) return rc;
    if (M != 16 || !settings->sh_dc) return fail(GSR_ERR_UNSUPPORTED, "the fused SH Adam step needs the split SH form with M = 16 (sh_dc + 15 coefficients)");
    if (P == 0) return GSR_OK;
    if (!radii || !splat_grads) return fail(GSR_ERR_INVALID_ARG, "radii / splat_grads are NULL");
    if (!dL_dmeans2D || !dL_dopacity || !dL_dmeans3D) return fail(GSR_ERR_INVALID_ARG, "gradient outputs are NULL");
    if (cov3D_precomp && !dL_dcov3D) return fail(GSR_ERR_INVALID_ARG, "dL_dcov3D is NULL");
    if (scales && (!dL_dscales || !dL_drotations)) return fail(GSR_ERR_INVALID_ARG, "dL_dscales / dL_drotations are NULL");
    if (!adam->dc_exp_avg || !adam->dc_exp_avg_sq || !adam->rest_exp_avg || !adam->rest_exp_avg_sq)
        return fail(GSR_ERR_INVALID_ARG, "Adam moments are NULL");
    if (((uintptr_t)settings->sh_dc | (uintptr_t)shs_rest | (uintptr_t)adam->dc_exp_avg | (uintptr_t)adam->dc_exp_avg_sq |
         (uintptr_t)adam->rest_exp_avg | (uintptr_t)adam->rest_exp_avg_sq) & 15)
        return fail(GSR_ERR_UNSUPPORTED, "the fused SH Adam step needs 16-byte aligned SH tensors and moments");
    if (!adam->sparse && (adam->step_dc < 1 || adam->step_rest < 1)) return fail(GSR_ERR_INVALID_ARG, "step < 1");
    GsrShAdamDev d;
    d.dc = const_cast<float*>(settings->sh_dc); d.dc_m = adam->dc_exp_avg; d.dc_v = adam->dc_exp_avg_sq;
    d.rest = shs_rest; d.rest_m = adam->rest_exp_avg; d.rest_v = adam->rest_exp_avg_sq;
    d.sparse = adam->sparse ? 1 : 0;
    auto fill = [&](float (&a)[6], double lr, int step) {
        if (d.sparse) {      // lr, b1, 1 - b1, b2, 1 - b2, eps  (gsr_launch_sparse_adam)
            a[0] = (float)lr; a[1] = (float)adam->beta1; a[2] = (float)(1.0 - adam->beta1); a[3] = (float)adam->beta2;
            a[4] = (float)(1.0 - adam->beta2); a[5] = (float)adam->eps;
        } else {             // 1 - b1, b2, 1 - b2, step size, 1 / sqrt(1 - b2^t), eps  (gsr_launch_adam: doubles until the last moment)
            const double bc1 = 1.0 - pow(adam->beta1, (double)step), bc2 = 1.0 - pow(adam->beta2, (double)step);
            a[0] = (float)(1.0 - adam->beta1); a[1] = (float)adam->beta2; a[2] = (float)(1.0 - adam->beta2);
            a[3] = (float)(lr / bc1); a[4] = (float)(1.0 / sqrt(bc2)); a[5] = (float)adam->eps;
        }
    };
    fill(d.dc_a, adam->lr_dc, adam->step_dc);
    fill(d.rest_a, adam->lr_rest, adam->step_rest);
    GsrGeom g = gsr_carve_geom(geom_buffer ? (char*)geom_buffer : nullptr, P);
    {   StageTimer t(GSR_STAGE_PREPROCESS_BWD, st);
        gsr_launch_preprocess_backward_sh_adam(cam, P, means3D, opacities, scales, rotations, cov3D_precomp, radii, g, splat_grads,
                                               dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dcov3D, scales ? dL_dscales : nullptr,
                                               scales ? dL_drotations : nullptr, d, st);
    }
    STAGE_CHECK("preprocess backward (fused SH Adam)");
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_rasterize_backward(const GsrRasterSettings* settings, int P, int M, int32_t num_rendered, const float* means3D,
                           const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                           const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                           const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                           const float* dL_dout_color, const float* dL_dout_invdepth, float* dL_dmeans2D,
                           float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                           float* dL_dscales, float* dL_drotations, void* bwd_scratch, float** splat_grads_out, void* stream) {
    if (P == 0) return GSR_OK;
    float* sg = nullptr;
    int rc = gsr_backward_blend(settings, P, num_rendered, geom_buffer, binning_buffer, image_buffer, dL_dout_color,
                                dL_dout_invdepth, bwd_scratch, &sg, stream);
    if (rc != GSR_OK) return rc;
    if (splat_grads_out) *splat_grads_out = sg;
    return gsr_backward_preprocess(settings, P, M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   radii, geom_buffer, sg, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D,
                                   dL_dsh, dL_dscales, dL_drotations, stream);
}

int gsr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                  double beta2, double eps, int32_t step, void* stream) {
    if (n < 0 || step < 1) return fail(GSR_ERR_INVALID_ARG, "n < 0 or step < 1");
    if (n == 0) return GSR_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_adam_step_multi(const GsrAdamTensor* tensors, int32_t count, void* stream) {
    if (count < 0) return fail(GSR_ERR_INVALID_ARG, "count < 0");
    if (count == 0) return GSR_OK;
    if (!tensors) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    for (int i = 0; i < count; ++i) {
        const GsrAdamTensor& a = tensors[i];
        if (a.n < 0 || a.step < 1) return fail(GSR_ERR_INVALID_ARG, "n < 0 or step < 1");
        if (a.n > 0 && (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq)) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    }
    for (int i = 0; i < count; i += GSR_ADAM_MAX_TENSORS)
        gsr_launch_adam_multi(tensors + i, count - i < GSR_ADAM_MAX_TENSORS ? count - i : GSR_ADAM_MAX_TENSORS, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_sparse_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* visible,
                         int64_t N, int64_t M, double lr, double beta1, double beta2, double eps, void* stream) {
    if (N < 0 || M < 0) return fail(GSR_ERR_INVALID_ARG, "N < 0 or M < 0");
    if (N == 0 || M == 0) return GSR_OK;
    if (M >= (1ll << 31) || N >= (1ll << 31)) return fail(GSR_ERR_UNSUPPORTED, "sparse Adam: N and M must be below 2^31 (the kernel indexes rows and columns with 32 bits)");
    if (!param || !grad || !exp_avg || !exp_avg_sq || !visible) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_sparse_adam(param, grad, exp_avg, exp_avg_sq, visible, N, M, lr, beta1, beta2, eps, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_sparse_adam_step_multi(const GsrSparseAdamTensor* tensors, int32_t count, const uint8_t* visible, int64_t N, double beta1, double beta2,
                               void* stream) {
    if (count < 0 || N < 0) return fail(GSR_ERR_INVALID_ARG, "count < 0 or N < 0");
    if (count == 0 || N == 0) return GSR_OK;
    if (!tensors || !visible) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (N >= (1ll << 31)) return fail(GSR_ERR_UNSUPPORTED, "sparse Adam: N and M must be below 2^31 (the kernel indexes rows and columns with 32 bits)");
    for (int i = 0; i < count; ++i) {
        const GsrSparseAdamTensor& a = tensors[i];
        if (a.M < 0) return fail(GSR_ERR_INVALID_ARG, "M < 0");
        if (a.M >= (1ll << 31)) return fail(GSR_ERR_UNSUPPORTED, "sparse Adam: N and M must be below 2^31 (the kernel indexes rows and columns with 32 bits)");
        if (a.M > 0 && (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq)) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    }
    for (int i = 0; i < count; i += GSR_ADAM_MAX_TENSORS)
        gsr_launch_sparse_adam_multi(tensors + i, count - i < GSR_ADAM_MAX_TENSORS ? count - i : GSR_ADAM_MAX_TENSORS, visible, N, beta1, beta2,
                                     (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_density_stats(int P, const float* viewspace_grad, const uint8_t* visible, const int32_t* radii, float* grad_accum, float* denom,
                      float* max_radii2D, void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!viewspace_grad || !grad_accum || !denom) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (!visible && !radii) return fail(GSR_ERR_INVALID_ARG, "give the visibility mask or the radii (visible = radii > 0)");
    if (radii && !max_radii2D) return fail(GSR_ERR_INVALID_ARG, "radii given but max_radii2D is NULL");
    gsr_launch_density_stats(P, viewspace_grad, visible, radii, grad_accum, denom, max_radii2D, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_inject_noise(int P, float* xyz, const float* scales, const float* rotations, const float* opacities, const float* noise,
                          int activated, float noise_scale, float gate_k, float gate_x0, void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!xyz || !scales || !rotations || !opacities || !noise) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_mcmc_noise(P, xyz, scales, rotations, opacities, noise, activated != 0, noise_scale, gate_k, gate_x0, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mcmc_relocation(int n, const float* opacities, const float* scales, const int32_t* ratios, float* new_opacities, float* new_scales,
                        void* stream) {
    if (n < 0) return fail(GSR_ERR_INVALID_ARG, "n < 0");
    if (n == 0) return GSR_OK;
    if (!opacities || !scales || !ratios || !new_opacities || !new_scales) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_mcmc_relocation(n, opacities, scales, ratios, new_opacities, new_scales, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// ---- bilateral grid (bilagrid.hip) ----
static int bilagrid_grid_ok(int L, int Gh, int Gw) {
    if (L < 2 || Gh < 2 || Gw < 2 || L > GSR_BILAGRID_MAX || Gh > GSR_BILAGRID_MAX || Gw > GSR_BILAGRID_MAX)
        return fail(GSR_ERR_UNSUPPORTED, "bilateral grid: L, Gh, Gw must be 2..64, got " + std::to_string(L) + " x " + std::to_string(Gh) + " x " +
                                             std::to_string(Gw));
    return GSR_OK;
}

static int bilagrid_plan_checked(int H, int W, int L, int Gh, int Gw, GsrBilagridPlan* p) {
    if (H < 1 || W < 1) return fail(GSR_ERR_INVALID_ARG, "bilateral grid: image size must be positive, got " + std::to_string(H) + " x " + std::to_string(W));
    if (H > GSR_BILAGRID_MAX_IMAGE || W > GSR_BILAGRID_MAX_IMAGE) return fail(GSR_ERR_UNSUPPORTED, "bilateral grid: image side above 2^23 pixels");
    if (int rc = bilagrid_grid_ok(L, Gh, Gw)) return rc;
    gsr_bilagrid_plan(H, W, L, Gh, Gw, p);
    if ((int64_t)p->ncells * p->maxchunks > 0x7FFFFFFFll) return fail(GSR_ERR_UNSUPPORTED, "bilateral grid: more than 2^31-1 workgroups");
    return GSR_OK;
}

size_t gsr_bilagrid_scratch_bytes(int H, int W, int L, int Gh, int Gw) {
    GsrBilagridPlan p;
    if (bilagrid_plan_checked(H, W, L, Gh, Gw, &p) != GSR_OK) return 0;
    return gsr_bilagrid_scratch_floats(p) * sizeof(float);
}

int gsr_bilagrid_slice(int H, int W, int L, int Gh, int Gw, const float* grid, const float* image, float* out, void* stream) {
    GsrBilagridPlan p;
    if (int rc = bilagrid_plan_checked(H, W, L, Gh, Gw, &p)) return rc;
    if (!grid || !image || !out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_bilagrid_slice(p, grid, image, out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_bilagrid_slice_backward(int H, int W, int L, int Gh, int Gw, const float* grid, const float* image, const float* dL_dout,
                                float* dL_dgrid, float* dL_dimage, void* scratch, size_t scratch_bytes, void* stream) {
    GsrBilagridPlan p;
    if (int rc = bilagrid_plan_checked(H, W, L, Gh, Gw, &p)) return rc;
    if (!grid || !image || !dL_dout || !dL_dgrid || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only dL_dimage may be NULL)");
    const size_t need = gsr_bilagrid_scratch_floats(p) * sizeof(float);
    if (scratch_bytes < need)
        return fail(GSR_ERR_INVALID_ARG, "bilateral grid: scratch of " + std::to_string(scratch_bytes) + " bytes, gsr_bilagrid_scratch_bytes asks for " +
                                             std::to_string(need));
    if ((uintptr_t)scratch & 3) return fail(GSR_ERR_INVALID_ARG, "bilateral grid: scratch must be 4-byte aligned");
    gsr_launch_bilagrid_slice_backward(p, grid, image, dL_dout, dL_dgrid, dL_dimage, (float*)scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

static int bilagrid_tv_ok(int N, int L, int Gh, int Gw) {
    if (N < 1) return fail(GSR_ERR_INVALID_ARG, "bilateral grid: N must be positive, got " + std::to_string(N));
    return bilagrid_grid_ok(L, Gh, Gw);
}

int64_t gsr_bilagrid_tv_partial_count(int N, int L, int Gh, int Gw) {
    if (bilagrid_tv_ok(N, L, Gh, Gw) != GSR_OK) return 0;
    return gsr_bilagrid_tv_partial_count_impl(N, L, Gh, Gw);
}

int gsr_bilagrid_tv(int N, int L, int Gh, int Gw, const float* grids, double* partials, float* tv_out, void* stream) {
    if (int rc = bilagrid_tv_ok(N, L, Gh, Gw)) return rc;
    if (!grids || !partials || !tv_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)partials & 7) return fail(GSR_ERR_INVALID_ARG, "bilateral grid: partials must be 8-byte aligned");
    gsr_launch_bilagrid_tv(N, L, Gh, Gw, grids, partials, tv_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_bilagrid_tv_backward(int N, int L, int Gh, int Gw, const float* grids, const float* dL_dtv, float* dL_dgrids, void* stream) {
    if (int rc = bilagrid_tv_ok(N, L, Gh, Gw)) return rc;
    if (!grids || !dL_dtv || !dL_dgrids) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_bilagrid_tv_backward(N, L, Gh, Gw, grids, dL_dtv, dL_dgrids, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// ---- normals (normals.hip) ----
int gsr_gaussian_normals(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix, float* normals_out,
                         void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!scales || !rotations || !means3D || !viewmatrix || !normals_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_gaussian_normals(P, scales, rotations, means3D, viewmatrix, normals_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_gaussian_normals_backward(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                  const float* dL_dnormals, float* dL_drotations, void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!scales || !rotations || !means3D || !viewmatrix || !dL_dnormals || !dL_drotations) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_gaussian_normals_backward(P, scales, rotations, means3D, viewmatrix, dL_dnormals, dL_drotations, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

static int normals_frame_checked(int H, int W, float tanfovx, float tanfovy, GsrNormalsFrame* f) {
    if (H < 1 || W < 1) return fail(GSR_ERR_INVALID_ARG, "normals: image size must be positive, got " + std::to_string(H) + " x " + std::to_string(W));
    if ((int64_t)H * W > 0x7FFFFFFFll) return fail(GSR_ERR_UNSUPPORTED, "normals: more than 2^31-1 pixels");
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f) || !std::isfinite(tanfovx) || !std::isfinite(tanfovy))
        return fail(GSR_ERR_INVALID_ARG, "normals: tanfovx and tanfovy must be positive and finite, got " + std::to_string(tanfovx) + ", " +
                                             std::to_string(tanfovy));
    gsr_normals_frame(H, W, tanfovx, tanfovy, f);
    return GSR_OK;
}

int gsr_depth_normals(int H, int W, float tanfovx, float tanfovy, const float* depth, float* normals_out, void* stream) {
    GsrNormalsFrame f;
    if (int rc = normals_frame_checked(H, W, tanfovx, tanfovy, &f)) return rc;
    if (!depth || !normals_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_depth_normals(f, depth, normals_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_depth_normals_backward(int H, int W, float tanfovx, float tanfovy, const float* depth, const float* dL_dnormals, float* dL_ddepth,
                               void* stream) {
    GsrNormalsFrame f;
    if (int rc = normals_frame_checked(H, W, tanfovx, tanfovy, &f)) return rc;
    if (!depth || !dL_dnormals || !dL_ddepth) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_depth_normals_backward(f, depth, dL_dnormals, dL_ddepth, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int64_t gsr_normal_loss_partial_count(int H, int W) {
    GsrNormalsFrame f;
    if (normals_frame_checked(H, W, 1.f, 1.f, &f) != GSR_OK) return 0;
    return gsr_normals_tiles(f);
}

int gsr_normal_loss(int H, int W, float tanfovx, float tanfovy, const float* depth, const float* normals, const float* weight, double* partials,
                    float* loss_out, void* stream) {
    GsrNormalsFrame f;
    if (int rc = normals_frame_checked(H, W, tanfovx, tanfovy, &f)) return rc;
    if (!depth || !normals || !partials || !loss_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only weight may be NULL)");
    if ((uintptr_t)partials & 7) return fail(GSR_ERR_INVALID_ARG, "normals: partials must be 8-byte aligned");
    gsr_launch_normal_loss(f, depth, normals, weight, partials, loss_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_normal_loss_backward(int H, int W, float tanfovx, float tanfovy, const float* depth, const float* normals, const float* weight,
                             const float* dL_dloss, float* dL_dnormals, float* dL_ddepth, void* stream) {
    GsrNormalsFrame f;
    if (int rc = normals_frame_checked(H, W, tanfovx, tanfovy, &f)) return rc;
    if (!depth || !normals || !dL_dloss) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only weight, dL_dnormals and dL_ddepth may be NULL)");
    if (!dL_dnormals && !dL_ddepth) return GSR_OK;
    gsr_launch_normal_loss_backward(f, depth, normals, weight, dL_dloss, dL_dnormals, dL_ddepth, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// ---- 3D smoothing filter of Mip-Splatting (mip.hip) ----
size_t gsr_mip_filter_scratch_bytes(int P) { return P < 0 ? 0 : GSR_MIP_SCRATCH_BYTES; }

int gsr_mip_filter_3d(int P, const float* means3D, int C, const float* cameras, float* filter_3D, uint8_t* seen, void* scratch, void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (C < 1) return fail(GSR_ERR_INVALID_ARG, "3D filter: at least one camera is needed, got C = " + std::to_string(C));
    if (P == 0) return GSR_OK;
    if (!means3D || !cameras || !filter_3D || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only seen may be NULL)");
    if ((uintptr_t)scratch & 3) return fail(GSR_ERR_INVALID_ARG, "3D filter: scratch must be 4-byte aligned");
    gsr_launch_mip_filter(P, means3D, C, cameras, filter_3D, seen, (uint32_t*)scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mip_activations(int P, const float* raw_scales, const float* raw_opacity, const float* filter_3D, float* scales_out, float* opacity_out,
                        void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!raw_scales || !raw_opacity || !filter_3D || !scales_out || !opacity_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_mip_activations(P, raw_scales, raw_opacity, filter_3D, scales_out, opacity_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mip_activations_backward(int P, const float* raw_scales, const float* raw_opacity, const float* filter_3D, const float* dL_dscales,
                                 const float* dL_dopacity, float* dL_draw_scales, float* dL_draw_opacity, void* stream) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!raw_scales || !raw_opacity || !filter_3D || !dL_draw_scales || !dL_draw_opacity)
        return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only dL_dscales and dL_dopacity may be NULL)");
    gsr_launch_mip_activations_backward(P, raw_scales, raw_opacity, filter_3D, dL_dscales, dL_dopacity, dL_draw_scales, dL_draw_opacity,
                                        (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// ---- vector quantisation: the two steps of a Lloyd iteration (vq.hip) ----
static bool vq_sizes_ok(int P, int D, int K) { return P >= 0 && D >= 1 && D <= GSR_VQ_MAX_D && K >= 1 && K <= GSR_VQ_MAX_K; }

size_t gsr_vq_scratch_bytes(int P, int D, int K) { return vq_sizes_ok(P, D, K) ? gsr_vq_scratch_bytes_impl(P, D, K) : 0; }

int gsr_vq_assign(int P, int D, int K, const float* rows, const float* codebook, int32_t* idx, float* dist2, void* scratch, void* stream) {
    if (!vq_sizes_ok(P, D, K))
        return fail(GSR_ERR_INVALID_ARG, "vq: need 0 <= P, 1 <= D <= 64, 1 <= K <= 65536, got P = " + std::to_string(P) + ", D = " + std::to_string(D) +
                                             ", K = " + std::to_string(K));
    if (P == 0) return GSR_OK;
    if (!rows || !codebook || !idx || !dist2 || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)scratch & 15) return fail(GSR_ERR_INVALID_ARG, "vq: scratch must be 16-byte aligned");
    gsr_launch_vq_assign(P, D, K, rows, codebook, idx, dist2, scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_vq_update(int P, int D, int K, const float* rows, const float* weights, const int32_t* idx, float* codebook, float* mass, void* scratch,
                  void* stream) {
    if (!vq_sizes_ok(P, D, K))
        return fail(GSR_ERR_INVALID_ARG, "vq: need 0 <= P, 1 <= D <= 64, 1 <= K <= 65536, got P = " + std::to_string(P) + ", D = " + std::to_string(D) +
                                             ", K = " + std::to_string(K));
    if (!codebook || !mass) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (P == 0) {      // every cluster is empty: the centroids stay, the masses are zero
        HIP_OK(hipMemsetAsync(mass, 0, (size_t)K * sizeof(float), (hipStream_t)stream));
        return GSR_OK;
    }
    if (!rows || !idx || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only weights may be NULL)");
    if ((uintptr_t)scratch & 15) return fail(GSR_ERR_INVALID_ARG, "vq: scratch must be 16-byte aligned");
    gsr_launch_vq_update(P, D, K, rows, weights, idx, codebook, mass, scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// ---- TSDF fusion and marching tetrahedra (tsdf.hip) ----
static int tsdf_dims_checked(int nx, int ny, int nz, int64_t* cells) {
    if (nx < 0 || ny < 0 || nz < 0)
        return fail(GSR_ERR_INVALID_ARG, "tsdf: the volume's dimensions must be >= 0, got " + std::to_string(nx) + " x " + std::to_string(ny) + " x " +
                                             std::to_string(nz));
    const bool empty = nx == 0 || ny == 0 || nz == 0;
    if (!empty && ((int64_t)nx * ny >= ((int64_t)1 << 31) || (int64_t)nx * ny * nz >= ((int64_t)1 << 31)))
        return fail(GSR_ERR_INVALID_ARG, "tsdf: a volume of " + std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz) +
                                             " voxels has 2^31 or more");
    *cells = empty ? 0 : (int64_t)nx * ny * nz;
    return GSR_OK;
}

int gsr_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float sdf_trunc, float near_z, int V,
                       const float* cameras, int H, int W, const float* depth, const float* color, float* tsdf, float* weight, float* rgb,
                       void* stream) {
    int64_t cells = 0;
    if (int rc = tsdf_dims_checked(nx, ny, nz, &cells)) return rc;
    if (V < 0) return fail(GSR_ERR_INVALID_ARG, "tsdf: V < 0");
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31))
        return fail(GSR_ERR_INVALID_ARG, "tsdf: the depth maps must be at least 1 x 1 and below 2^31 pixels, got H = " + std::to_string(H) + ", W = " +
                                             std::to_string(W));
    if (!(voxel_size > 0.f) || !(sdf_trunc > 0.f) || !(near_z >= 0.f) || !std::isfinite(voxel_size) || !std::isfinite(sdf_trunc) ||
        !std::isfinite(near_z) || !std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz))
        return fail(GSR_ERR_INVALID_ARG, "tsdf: need voxel_size > 0, sdf_trunc > 0, near >= 0 and a finite origin");
    if (V == 0 || cells == 0) return GSR_OK;
    if (!cameras || !depth || !tsdf || !weight) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only color and rgb may be NULL)");
    if ((color == nullptr) != (rgb == nullptr)) return fail(GSR_ERR_INVALID_ARG, "tsdf: give color and rgb together or neither");
    gsr_launch_tsdf_integrate(nx, ny, nz, ox, oy, oz, voxel_size, sdf_trunc, near_z, V, cameras, H, W, depth, color, tsdf, weight, rgb,
                              (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

static bool mesh_sizes_ok(int nx, int ny, int nz) {
    return nx >= 0 && ny >= 0 && nz >= 0 && (nx == 0 || ny == 0 || nz == 0 || ((int64_t)nx * ny <= GSR_MESH_MAX_VOXELS &&
                                                                             (int64_t)nx * ny * nz <= GSR_MESH_MAX_VOXELS));
}
static bool mesh_has_cell(int nx, int ny, int nz) { return nx >= 2 && ny >= 2 && nz >= 2; }

size_t gsr_mesh_scratch_bytes(int nx, int ny, int nz) { return mesh_sizes_ok(nx, ny, nz) ? gsr_mesh_scratch_bytes_impl(nx, ny, nz) : 0; }

int gsr_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float min_weight, void* scratch, int32_t* counts_out,
                   void* stream) {
    if (!mesh_sizes_ok(nx, ny, nz))
        return fail(GSR_ERR_INVALID_ARG, "mesh: need 0 <= nx, ny, nz and nx ny nz <= " + std::to_string(GSR_MESH_MAX_VOXELS) + ", got " +
                                             std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz));
    if (std::isnan(min_weight)) return fail(GSR_ERR_INVALID_ARG, "mesh: min_weight is NaN");
    if (!counts_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (!mesh_has_cell(nx, ny, nz)) {      // no cell: an empty mesh, no launch
        HIP_OK(hipMemsetAsync(counts_out, 0, 2 * sizeof(int32_t), (hipStream_t)stream));
        return GSR_OK;
    }
    if (!tsdf || !weight || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "mesh: scratch must be 128-byte aligned");
    gsr_launch_mesh_count(nx, ny, nz, tsdf, weight, min_weight, scratch, counts_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf, const float* rgb, void* scratch,
                  int nv, int nf, float* vertices, float* colors, int32_t* faces, void* stream) {
    if (!mesh_sizes_ok(nx, ny, nz))
        return fail(GSR_ERR_INVALID_ARG, "mesh: need 0 <= nx, ny, nz and nx ny nz <= " + std::to_string(GSR_MESH_MAX_VOXELS) + ", got " +
                                             std::to_string(nx) + " x " + std::to_string(ny) + " x " + std::to_string(nz));
    if (nv < 0 || nf < 0) return fail(GSR_ERR_INVALID_ARG, "mesh: nv < 0 or nf < 0");
    if (nv == 0 || !mesh_has_cell(nx, ny, nz)) return GSR_OK;
    if (!tsdf || !scratch || !vertices || (nf > 0 && !faces)) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only rgb and colors may be NULL)");
    if ((rgb == nullptr) != (colors == nullptr)) return fail(GSR_ERR_INVALID_ARG, "mesh: give rgb and colors together or neither");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "mesh: scratch must be 128-byte aligned");
    gsr_launch_mesh_emit(nx, ny, nz, ox, oy, oz, voxel_size, tsdf, rgb, scratch, nv, nf, vertices, colors, faces, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

// ---- mesh clean-up: components, compaction, normals, smoothing (meshops.hip) ----
static bool meshops_sizes_ok(int nv, int nf) { return nv >= 0 && nf >= 0 && 3 * (int64_t)nf < ((int64_t)1 << 31); }
static int meshops_sizes_checked(int nv, int nf) {
    if (!meshops_sizes_ok(nv, nf))
        return fail(GSR_ERR_INVALID_ARG, "meshops: need 0 <= nv and 0 <= 3 nf < 2^31, got nv = " + std::to_string(nv) + ", nf = " + std::to_string(nf));
    return GSR_OK;
}
static int g_mesh_component_rounds = 0;

size_t gsr_meshops_scratch_bytes(int nv, int nf) { return meshops_sizes_ok(nv, nf) ? gsr_meshops_scratch_bytes_impl(nv, nf) : 0; }

int gsr_mesh_components(int nv, int nf, const int32_t* faces, int32_t* vertex_label, int32_t* face_count, void* scratch, void* stream) {
    if (int rc = meshops_sizes_checked(nv, nf)) return rc;
    g_mesh_component_rounds = 0;
    if (nv == 0) {      // nothing to label: the call still synchronises
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        return GSR_OK;
    }
    if ((nf > 0 && !faces) || !vertex_label || !face_count || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "meshops: scratch must be 128-byte aligned");
    const int rc = gsr_launch_mesh_components(nv, nf, faces, vertex_label, face_count, scratch, (hipStream_t)stream, &g_mesh_component_rounds);
    HIP_OK(hipGetLastError());
    if (rc < 0) return fail(GSR_ERR_HIP, "meshops: reading the round word back failed");
    if (rc > 0)
        return fail(GSR_ERR_UNSUPPORTED, "meshops: the components did not settle within " + std::to_string(gsr_meshops_round_cap(nv)) + " rounds (nv = " +
                                          std::to_string(nv) + ", nf = " + std::to_string(nf) + ")");
    return GSR_OK;
}

int gsr_mesh_components_rounds(void) { return g_mesh_component_rounds; }

int gsr_mesh_compact_count(int nv, int nf, const int32_t* faces, const uint8_t* keep_face, void* scratch, int32_t* counts_out, void* stream) {
    if (int rc = meshops_sizes_checked(nv, nf)) return rc;
    if (!counts_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (nv == 0 || nf == 0) {      // no row can be a face: an empty mesh, no launch
        HIP_OK(hipMemsetAsync(counts_out, 0, 2 * sizeof(int32_t), (hipStream_t)stream));
        return GSR_OK;
    }
    if (!faces || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only keep_face may be NULL)");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "meshops: scratch must be 128-byte aligned");
    gsr_launch_mesh_compact_count(nv, nf, faces, keep_face, scratch, counts_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mesh_compact_emit(int nv, int nf, const float* vertices, const float* colors, const int32_t* faces, const uint8_t* keep_face, void* scratch,
                          int nv_out, int nf_out, float* vertices_out, float* colors_out, int32_t* faces_out, void* stream) {
    if (int rc = meshops_sizes_checked(nv, nf)) return rc;
    if (nv_out < 0 || nf_out < 0) return fail(GSR_ERR_INVALID_ARG, "meshops: nv_out < 0 or nf_out < 0");
    if (nv_out == 0 || nv == 0 || nf == 0) return GSR_OK;      // (a kept face keeps three vertices: no vertex, no face)
    if (!vertices || !faces || !scratch || !vertices_out || (nf_out > 0 && !faces_out))
        return fail(GSR_ERR_INVALID_ARG, "NULL pointer (only colors, colors_out and keep_face may be NULL)");
    if ((colors == nullptr) != (colors_out == nullptr)) return fail(GSR_ERR_INVALID_ARG, "meshops: give colors and colors_out together or neither");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "meshops: scratch must be 128-byte aligned");
    gsr_launch_mesh_compact_emit(nv, nf, vertices, colors, faces, keep_face, scratch, nv_out, nf_out, vertices_out, colors_out, faces_out,
                                 (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mesh_vertex_normals(int nv, int nf, const float* vertices, const int32_t* faces, float* normals_out, void* scratch, void* stream) {
    if (int rc = meshops_sizes_checked(nv, nf)) return rc;
    if (nv == 0) return GSR_OK;
    if (!vertices || (nf > 0 && !faces) || !normals_out || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "meshops: scratch must be 128-byte aligned");
    gsr_launch_mesh_vertex_normals(nv, nf, vertices, faces, normals_out, scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mesh_smooth(int nv, int nf, const float* vertices, const int32_t* faces, int iterations, float lambda, float mu, float* vertices_out,
                    void* scratch, void* stream) {
    if (int rc = meshops_sizes_checked(nv, nf)) return rc;
    if (iterations < 0 || iterations > (1 << 20)) return fail(GSR_ERR_INVALID_ARG, "meshops: need 0 <= iterations <= 2^20, got " + std::to_string(iterations));
    if (std::isnan(lambda) || std::isnan(mu)) return fail(GSR_ERR_INVALID_ARG, "meshops: lambda or mu is NaN");
    if (nv == 0) return GSR_OK;
    if (!vertices || (nf > 0 && !faces) || !vertices_out || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if (vertices == vertices_out) return fail(GSR_ERR_INVALID_ARG, "meshops: vertices_out must not be the input (the input is never written)");
    if ((uintptr_t)scratch & 127) return fail(GSR_ERR_INVALID_ARG, "meshops: scratch must be 128-byte aligned");
    if (iterations == 0) {
        HIP_OK(hipMemcpyAsync(vertices_out, vertices, (size_t)nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return GSR_OK;
    }
    gsr_launch_mesh_smooth(nv, nf, vertices, faces, iterations, lambda, mu, vertices_out, scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

size_t gsr_knn_scratch_bytes(int N) { return gsr_knn_scratch_bytes_impl(N); }

int gsr_knn_mean_dist2(int N, const float* points, float* mean_dist2, void* scratch, void* stream) {
    if (N < 0) return fail(GSR_ERR_INVALID_ARG, "N < 0");
    if (N == 0) return GSR_OK;
    if (!points || !mean_dist2 || !scratch) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_knn(N, points, mean_dist2, scratch, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_ssim_forward(int planes, int H, int W, const float* img1, const float* img2, float* ssim_map, float* dm_dmu1,
                     float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    if (planes < 0 || H <= 0 || W <= 0) return fail(GSR_ERR_INVALID_ARG, "bad image size");
    if (planes == 0) return GSR_OK;
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 image planes");
    if (!img1 || !img2 || !ssim_map) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((dm_dmu1 == nullptr) != (dm_dsigma1_sq == nullptr) || (dm_dmu1 == nullptr) != (dm_dsigma12 == nullptr))
        return fail(GSR_ERR_INVALID_ARG, "give all three derivative maps or none");
    gsr_launch_ssim_forward(planes, H, W, img1, img2, ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int64_t gsr_ssim_partial_count(int planes, int H, int W) {
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    return gsr_ssim_partial_count_impl(planes, H, W);
}

int gsr_ssim_mean_forward(int planes, int H, int W, const float* img1, const float* img2, float* partials, float* mean_out,
                          float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    if (planes <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_INVALID_ARG, "bad image size");
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 image planes");
    if (gsr_ssim_partial_count_impl(planes, H, W) > 0x7FFFFFFFll) return fail(GSR_ERR_UNSUPPORTED, "too many tiles");
    if (!img1 || !img2 || !partials || !mean_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((dm_dmu1 == nullptr) != (dm_dsigma1_sq == nullptr) || (dm_dmu1 == nullptr) != (dm_dsigma12 == nullptr))
        return fail(GSR_ERR_INVALID_ARG, "give all three derivative maps or none");
    gsr_launch_ssim_mean_forward(planes, H, W, img1, img2, partials, mean_out, dm_dmu1, dm_dsigma1_sq, dm_dsigma12,
                                 (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_ssim_mean_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmean,
                           const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1,
                           void* stream) {
    if (planes <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_INVALID_ARG, "bad image size");
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 image planes");
    if (!img1 || !img2 || !dL_dmean || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_ssim_mean_backward(planes, H, W, img1, img2, dL_dmean, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1,
                                  (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_train_loss_forward(int planes, int H, int W, const float* img1, const float* img2, float lambda_dssim, float* partials,
                           float* loss_out, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream) {
    if (planes <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_INVALID_ARG, "bad image size");
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 image planes");
    if (gsr_ssim_partial_count_impl(planes, H, W) > 0x3FFFFFFFll) return fail(GSR_ERR_UNSUPPORTED, "too many tiles");
    if (!img1 || !img2 || !partials || !loss_out) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    if ((dm_dmu1 == nullptr) != (dm_dsigma1_sq == nullptr) || (dm_dmu1 == nullptr) != (dm_dsigma12 == nullptr))
        return fail(GSR_ERR_INVALID_ARG, "give all three derivative maps or none");
    gsr_launch_train_loss_forward(planes, H, W, img1, img2, lambda_dssim, partials, loss_out, dm_dmu1, dm_dsigma1_sq, dm_dsigma12,
                                  (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_train_loss_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dloss, float lambda_dssim,
                            const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, void* stream) {
    if (planes <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_INVALID_ARG, "bad image size");
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 image planes");
    if (!img1 || !img2 || !dL_dloss || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_train_loss_backward(planes, H, W, img1, img2, dL_dloss, lambda_dssim, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1,
                                   (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_ssim_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmap,
                      const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1, void* stream) {
    if (planes < 0 || H <= 0 || W <= 0) return fail(GSR_ERR_INVALID_ARG, "bad image size");
    if (planes == 0) return GSR_OK;
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "more than 65535 image planes");
    if (!img1 || !img2 || !dL_dmap || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1)
        return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_ssim_backward(planes, H, W, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream) {
    (void)projmatrix;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P < 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !present) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    gsr_launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return GSR_OK;
}

int gsr_forward_views(int P, int64_t R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                      const void* image_buffer, GsrForwardViews* out) {
    if (!out || !geom_buffer || !image_buffer) return fail(GSR_ERR_INVALID_ARG, "NULL pointer");
    GsrCamDev cam{};      // (the view depends on the frame size alone)
    cam.W = width;
    cam.H = height;
    cam.gx = (width + GSR_TILE - 1) / GSR_TILE;
    cam.gy = (height + GSR_TILE - 1) / GSR_TILE;
    const GsrSavedFrame f = saved_frame(cam, P, R, geom_buffer, binning_buffer, image_buffer);
    out->splats = (const float*)f.splats;
    out->tiles_touched = f.tiles;
    out->depth_order = f.order;
    out->point_list = f.point_list;      // (NULL without a binning buffer or with R <= 0)
    out->ranges = (const uint32_t*)f.ranges;
    out->final_T = f.final_T;
    out->n_contrib = f.n_contrib;
    out->tile_scan = f.offsets;
    return GSR_OK;
}

}  // extern "C"
