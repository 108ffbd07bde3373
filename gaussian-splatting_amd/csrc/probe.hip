// Per-pixel probe of one forward (gsr_pixel_probe, include/gsr.h; no reference counterpart): what the frame meant for every PIXEL beyond colour,
// inverse depth and alpha.  With w = alpha * T (the forward's `alpha * Tl`) and T' = T (1 - alpha) (its testT) of a contributor at view-space
// depth z with Gaussian index g, per pixel, front to back:
//     expected_depth = sum w z (fp32, list order, not normalised),   median_depth / median_id = z / g of the first contributor with T' < threshold,
//     top_id / top_weight = g / w of the contributor with the largest w (strict >, so the nearest wins ties),   count = number of contributors.
// The pixel-side counterpart of contrib.hip, read from the same state (ranges, point_list, the 64-byte splat records, n_contrib).
//
// One kernel, no scratch, no reduce, no atomics:
//
//  probe_walk       contrib_walk's structure (one wave64 per 8x8 pixel block, front to back: ids two batches ahead, the 64-byte record gather one
//                   batch ahead, the forward's exact box test, the survivors parked compacted in the wave's LDS, then the lanes act as pixel lanes with
//                   the forward's p2, alpha and testT from gsr_blend.h) and its rules: a pixel takes a valid entry (power <= 0, alpha >= 1/255)
//                   exactly when its list position is <= n_contrib[p], T < 1e-4 is not re-tested, and the wave walks no further than the largest
//                   n_contrib of its pixels.  The compacted record carries two more values than contrib_walk's -- the entry's depth (q2.y) and its
//                   Gaussian id (the point_list value) -- in a third, 8-byte table (LDS 2.5 KB).  Nothing crosses lanes in the inner loop: every
//                   lane keeps its own pixel's six values in registers, and the entry's list position stays a per-lane LDS broadcast.
//  Stores           each lane stores its own pixel once, with plain vector stores, after the walk.  THE KERNEL WRITES THE DEFAULTS ITSELF: where
//                   contrib_walk returns early (a tile with an empty range, a block whose largest n_contrib is 0) this kernel skips the walk and
//                   still reaches the stores with the initial values (0, 0 / -1, -1 / 0, 0), so every in-band, in-image pixel is written and no pixel
//                   outside the band is touched.  Only the call without state (P == 0 or num_rendered == 0: no ranges to read) is served by the
//                   launcher, which fills the band's rows -- one contiguous range per array -- with memsets on the same stream.
// Every value of a pixel is computed by one lane in a fixed order -> two runs give the same bits.
#include "gsr_internal.h"
#include "gsr_blend.h"

namespace {

__global__ void __launch_bounds__(64)
probe_walk(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
           const float4* __restrict__ splats, const uint32_t* __restrict__ n_contrib, GsrPixelProbeOut out) {
    __shared__ float4 s_rec[64 * 2];      // the batch's survivors, compacted: (x, y, a2, b2) (c2, opacity, lane bits, -)
    __shared__ float2 s_zid[64];          // ... and (depth, Gaussian id bits)
    const gsrb::TileQuad tq = gsrb::block8_of_workgroup(blockIdx.x);      // the forward's mapping: the four blocks of a tile on one XCD
    const int tile_local = tq.tile_local, quad = tq.quad;
    if (tile_local >= n_band_tiles) return;
    const gsrb::Block8 blk(cam, tile_local, quad);
    const int tile = blk.tile;
    const int lane = threadIdx.x;
    const int bx0 = blk.bx0, by0 = blk.by0;
    if (bx0 >= cam.W || by0 >= cam.H) return;      // (a block without a pixel)
    const int px = bx0 + (lane & 7), py = by0 + (lane >> 3);
    const bool inside = px < cam.W && py < cam.H;
    const float pxf = (float)px, pyf = (float)py;
    const float x0 = (float)bx0, x1 = (float)min(bx0 + 7, cam.W - 1);
    const float y0 = (float)by0, y1 = (float)min(by0 + 7, cam.H - 1);
    const uint2 range = ranges[tile];
    const int64_t pix = inside ? (int64_t)py * cam.W + px : 0;
    // (an unconditional load from a clamped address: a load behind a test of another load's value is a serial chain)
    const uint32_t nc = n_contrib[pix];
    const uint32_t last = inside ? nc : 0u;      // list position (from 1) of the pixel's last contributor; 0: the pixel takes no entry
    uint32_t mx = last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    // (the same value in every lane, which the compiler cannot know: as a scalar the loop tests move to the SALU)
    const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)min(range.y - range.x, mx), 0);
    const uint32_t list_end = range.x + end;      // end == 0 (empty range, nobody contributed anywhere): no walk, the defaults are stored
    const float threshold = out.threshold;
    float Tl = 1.0f;      // transmittance in front of the next entry (the forward's live T; read while the pixel still contributes)
    float e_depth = 0.0f, med_z = 0.0f, top_w = 0.0f;
    int32_t med_id = -1, top_id = -1, count = 0;

    auto load_id = [&](uint32_t e) -> uint32_t { return (e + lane < list_end) ? point_list[e + lane] : 0xFFFFFFFFu; };
    uint32_t id_n0 = load_id(range.x);      // the ids of the batch whose records are in n0..n2, then of the batch after it
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 n0 = zero4, n1 = zero4, n2 = zero4;
    if (id_n0 != 0xFFFFFFFFu) { n0 = splats[id_n0 * 4 + 0]; n1 = splats[id_n0 * 4 + 1]; n2 = splats[id_n0 * 4 + 2]; }
    uint32_t id_n1 = load_id(range.x + 64);
    for (uint32_t base = range.x; base < list_end; base += 64) {
        const uint32_t n = min(64u, list_end - base);
        float4 q0 = n0, q1 = n1;
        const float4 q2 = n2;
        const uint32_t id = id_n0;
        // issue the next batch's record gather and the id fetch of the batch after it
        id_n0 = id_n1;
        if (id_n1 != 0xFFFFFFFFu) { n0 = splats[id_n1 * 4 + 0]; n1 = splats[id_n1 * 4 + 1]; n2 = splats[id_n1 * 4 + 2]; }
        id_n1 = load_id(base + 128);
        bool keep = false;
        if ((uint32_t)lane < n) {
            const float qmin = gsrb::min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, x0, x1, y0, y1);
            keep = !(qmin > q2.z);                 // q2.z = 2 ln(255 opacity) + 0.01, written by the preprocess
            q0.z = gsrb::conic_diag_to_log2(q0.z);      // conic -> log2 units, sign folded in
            q0.w = gsrb::conic_cross_to_log2(q0.w);
            q1.x = gsrb::conic_diag_to_log2(q1.x);
        }
        const uint64_t mask = __ballot(keep);
        if (keep) {
            const int s = (int)__popcll(mask & ((1ull << lane) - 1ull));
            s_rec[s * 2 + 0] = q0;
            s_rec[s * 2 + 1] = make_float4(q1.x, q1.y, __uint_as_float((uint32_t)lane), 0.f);
            s_zid[s] = make_float2(q2.y, __uint_as_float(id));      // q2.y = view-space depth
        }
        __builtin_amdgcn_wave_barrier();      // (no instruction: the wave's LDS accesses stay in program order; the lanes read each other's records)
        const uint32_t left = (uint32_t)__popcll(mask);
        const uint32_t pos_base = base - range.x + 1;
        for (uint32_t u = 0; u < left; ++u) {
            const float4 r0 = s_rec[u * 2 + 0];
            const float4 r1 = s_rec[u * 2 + 1];
            const float2 zg = s_zid[u];
            const float z = zg.x;
            const int32_t g = (int32_t)__float_as_uint(zg.y);
            // ---- the forward's p2, alpha and testT (gsr_blend.h; blend_step_bf), so that the hard masks and T are the forward's bits ----
            const float dx = r0.x - pxf, dy = r0.y - pyf;
            const float p2 = gsrb::p2(dx, dy, r0.z, r0.w, r1.x);           // log2(e) * power
            const float alpha = gsrb::alpha(r1.y, p2);
            const bool contrib = (p2 <= 0.0f) & (alpha >= GSR_ALPHA_MIN) & (pos_base + __float_as_uint(r1.z) <= last);
            const float testT = fmaf(-alpha, Tl, Tl);                // T (1 - alpha)
            const float w = alpha * Tl;
            // ---- the pixel's own state: predicated updates, nothing crosses lanes ----
            const bool first_below = contrib & (testT < threshold) & (med_id < 0);
            const bool larger = contrib & (w > top_w);
            e_depth = contrib ? fmaf(w, z, e_depth) : e_depth;
            med_z = first_below ? z : med_z;
            med_id = first_below ? g : med_id;
            top_w = larger ? w : top_w;
            top_id = larger ? g : top_id;
            count += contrib ? 1 : 0;
            Tl = contrib ? testT : Tl;
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites the tables
    }
    if (inside) {
        if (out.expected_depth) out.expected_depth[pix] = e_depth;
        if (out.median_depth) out.median_depth[pix] = med_z;
        if (out.median_id) out.median_id[pix] = med_id;
        if (out.top_id) out.top_id[pix] = top_id;
        if (out.top_weight) out.top_weight[pix] = top_w;
        if (out.count) out.count[pix] = count;
    }
}

}  // namespace

void gsr_launch_pixel_probe_defaults(const GsrCamDev& cam, const GsrPixelProbeOut& out, hipStream_t st) {
    const GsrBandRows band = gsr_band_rows(cam);
    const size_t first = band.first, pixels = band.pixels;
    if (pixels == 0) return;
    if (out.expected_depth) (void)hipMemsetAsync(out.expected_depth + first, 0, pixels * sizeof(float), st);
    if (out.median_depth) (void)hipMemsetAsync(out.median_depth + first, 0, pixels * sizeof(float), st);
    if (out.median_id) (void)hipMemsetAsync(out.median_id + first, 0xFF, pixels * sizeof(int32_t), st);      // -1
    if (out.top_id) (void)hipMemsetAsync(out.top_id + first, 0xFF, pixels * sizeof(int32_t), st);
    if (out.top_weight) (void)hipMemsetAsync(out.top_weight + first, 0, pixels * sizeof(float), st);
    if (out.count) (void)hipMemsetAsync(out.count + first, 0, pixels * sizeof(int32_t), st);
}

void gsr_launch_pixel_probe(const GsrCamDev& cam, const GsrSavedFrame& f, const GsrPixelProbeOut& out, hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    if (n_band_tiles <= 0) return;
    const int groups = gsr_tile_groups(n_band_tiles, 8);
    hipLaunchKernelGGL(probe_walk, dim3(groups * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats, f.n_contrib, out);
}
