// N-channel per-Gaussian features blended with the weights of a forward that has already run (gsr_render_features /
// gsr_render_features_backward, include/gsr.h; no reference counterpart):
//     F[c,p] = sum_g w_gp f[g,c]            dL/df[g,c] = sum_p w_gp dL/dF[c,p]
// with w = alpha * T (the forward's `alpha * Tl`) under the contributor rule of contrib.hip / probe.hip: a pixel takes a valid entry (power <= 0,
// alpha >= 1/255) exactly when its list position is <= n_contrib[p], T < 1e-4 is not re-tested, and a wave walks no further than the largest
// n_contrib of its pixels.  Read from the state those two read (ranges, point_list, the 64-byte splat records, n_contrib); geometry and opacity
// are constants of the frame, so only `features` gets a gradient.  No background term: F is not normalised.
//
// Three kernels, NO atomics, every sum in a fixed order -> two runs give the same bits, and channel c of a C-channel call has the bits of a
// 1-channel call on column c alone (per channel the operations and their order do not depend on which other channels ride along):
//
//  feature_walk          probe_walk's structure (one wave64 per 8x8 pixel block on block8_of_workgroup's mapping, ids two batches ahead, the 64-byte
//                        record gather one batch ahead, the forward's exact box test, survivors compacted in the wave's LDS, then the lanes act as pixel
//                        lanes with the forward's p2, alpha and testT from gsr_blend.h).  Channels go FEAT_G per walk: C > FEAT_G means further walks
//                        over the same lists, a partly filled last group loads clamped channels it never stores.
//                        THE FEATURE ROW of an entry is wave-uniform in the inner loop.  It is gathered by the Gaussian lanes with the records (one
//                        batch ahead, FEAT_G floats per lane, from a clamped and therefore always valid address: no load behind a test) and parked
//                        beside the compacted record in a third LDS table, which the pixel lanes read as a broadcast (ds_read_b128, one address per
//                        wave).  The alternative, a scalar load from features + g * C per survivor, puts a memory round trip that depends on an LDS
//                        read (the id) into every step of the inner loop, where nothing can be issued ahead of it; the table costs 256 * FEAT_G bytes
//                        of LDS and the loads of entries that fail the box test.  Rows are read as float4 when C is a multiple of 4 and the base is
//                        16-byte aligned (feature_walk<true>: a quarter of the gather instructions), else float by float (feature_walk<false>).
//                        Every pixel lane keeps one fp32 accumulator per channel; its only update is acc = contrib ? fmaf(w, f, acc) : acc in list
//                        order (a predicated update, not a zeroed weight: rows of Gaussians that contribute nowhere may hold anything).  Nothing crosses lanes.
//  Stores                planar [C,H,W]: a lane's stores are coalesced per channel.  THE KERNEL WRITES THE ZEROS ITSELF where the walk is skipped (a
//                        tile with an empty range, a block whose largest n_contrib is 0), so every in-band, in-image pixel is written and nothing
//                        outside the band is touched.  Only the call without state (P == 0 or num_rendered == 0) is served by the launcher's memsets.
//  feature_grad_walk     contrib_walk's structure, 4 NB channels per walk (NB = 4, 2, 1: 16 channels while more than 8 remain, then 8, then 4).  Each pixel
//                        lane loads its dL/dF of the group's channels once before the loop; per survivor that somebody took (ballot) the products
//                        w dL/dF_c are summed over the wave four channels at a time (gsr_wave.h reduce4: two permlane swaps, then one DPP chain inside
//                        the 16-lane rows; the totals arrive in lanes 15, 31, 47, 63, which park them -- every channel in the same association
//                        order wherever it sits, so the grouping does not show in the bits).  After the batch the Gaussian lanes store the touched
//                        entries' records (NB float4) to slots[quad][k], k = gsrb::emission_index, plus the flag byte: contrib.hip's scratch shape
//                        with a wider record ((64 NB + 4) R bytes, NB that of the call's first group), reused by every group of a call.
//  feature_grad_reduce   the instance-run reduce of gsr_reduce.h (reduce_instance_runs) over FeatureGradOps: FEAT_NB float4 per instance, slots in slot
//                        order; stores dL_dfeatures[g, c0 .. c0 + 4 NB).  Rows of Gaussians without instances keep the launcher's zeros.
//                        (NB = 2 keeps the frame written out as a specialisation, see there: on the shared frame it compiled to another schedule.)
#include "gsr_internal.h"
#include "gsr_blend.h"
#include "gsr_wave.h"
#include "gsr_reduce.h"

#ifndef GSR_FEAT_G
#define GSR_FEAT_G 16      // channels per forward walk (a multiple of 4); chosen by measurement, DESIGN.md 5.6
#endif
#ifndef GSR_FEAT_GB
#define GSR_FEAT_GB 16     // most channels per backward walk (4, 8 or 16: 16 bytes of a slot record per four); chosen by measurement, DESIGN.md 5.6
#endif

namespace {

constexpr int FEAT_G = GSR_FEAT_G;
constexpr int FEAT_Q = FEAT_G / 4;      // float4 per staged feature row
constexpr int FEAT_GB = GSR_FEAT_GB;    // the widest backward group; a call's last channels go through the narrower instantiations
static_assert(FEAT_G % 4 == 0 && FEAT_G >= 4, "FEAT_G must be a multiple of 4");
static_assert(FEAT_GB == 4 || FEAT_GB == 8 || FEAT_GB == 16, "FEAT_GB must be 4, 8 or 16");

// The FEAT_G features of Gaussian `id` from channel c0 on.  Per lane the loads are unconditional and from clamped addresses (a lane without an entry reads
// row 0, a channel past the last reads the last; what the clamp duplicates is accumulated into registers that are never stored): a load behind a test of
// a loaded value is a serial chain.  A float4 that lies past the last channel altogether is skipped for the whole wave (a scalar test of kernel
// arguments) in the float-by-float instantiation, the one that serves small C: the gather is what this kernel's time goes to.
template <bool VEC4>
__device__ __forceinline__ void load_features(const float* __restrict__ features, uint32_t id, int C, int c0, float4 (&f)[FEAT_Q]) {
    const float* row = features + (int64_t)(id != 0xFFFFFFFFu ? id : 0u) * C;
#pragma unroll
    for (int j = 0; j < FEAT_Q; ++j) {
        if (VEC4) {      // (always loaded: with the skip below this instantiation needs 93 VGPRs instead of 68)
            f[j] = *reinterpret_cast<const float4*>(row + min(c0 + 4 * j, C - 4));
            continue;
        }
        if (j > 0 && c0 + 4 * j >= C) continue;
        f[j] = make_float4(row[min(c0 + 4 * j + 0, C - 1)], row[min(c0 + 4 * j + 1, C - 1)], row[min(c0 + 4 * j + 2, C - 1)],
                               row[min(c0 + 4 * j + 3, C - 1)]);
    }
}

template <bool VEC4>
__global__ void __launch_bounds__(64)
feature_walk(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
             const float4* __restrict__ splats, const uint32_t* __restrict__ n_contrib, const float* __restrict__ features /*[P,C]*/, int C, int c0,
             float* __restrict__ out /*[C,H,W]*/) {
    __shared__ float4 s_rec[64 * 2];           // the batch's survivors, compacted: (x, y, a2, b2) (c2, opacity, lane bits, -)
    __shared__ float4 s_feat[64 * FEAT_Q];     // ... and their feature rows of this channel group
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
    const uint32_t list_end = range.x + end;      // end == 0 (empty range, nobody contributed anywhere): no walk, zeros are stored
    float Tl = 1.0f;      // transmittance in front of the next entry (the forward's live T; read while the pixel still contributes)
    float acc[FEAT_G];
#pragma unroll
    for (int k = 0; k < FEAT_G; ++k) acc[k] = 0.0f;

    auto load_id = [&](uint32_t e) -> uint32_t { return (e + lane < list_end) ? point_list[e + lane] : 0xFFFFFFFFu; };
    uint32_t id_n0 = load_id(range.x);      // the ids of the batch whose records are in n0..n1 / fn, then of the batch after it
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 n0 = zero4, n1 = zero4, n2 = zero4;
    float4 fn[FEAT_Q];
    if (!VEC4) {      // (quads that load_features skips)
#pragma unroll
        for (int j = 0; j < FEAT_Q; ++j) fn[j] = zero4;
    }
    if (id_n0 != 0xFFFFFFFFu) { n0 = splats[id_n0 * 4 + 0]; n1 = splats[id_n0 * 4 + 1]; n2 = splats[id_n0 * 4 + 2]; }
    load_features<VEC4>(features, id_n0, C, c0, fn);
    uint32_t id_n1 = load_id(range.x + 64);
    for (uint32_t base = range.x; base < list_end; base += 64) {
        const uint32_t n = min(64u, list_end - base);
        float4 q0 = n0, q1 = n1;
        const float4 q2 = n2;
        float4 fq[FEAT_Q];
#pragma unroll
        for (int j = 0; j < FEAT_Q; ++j) fq[j] = fn[j];
        // issue the next batch's record and feature gathers and the id fetch of the batch after it
        id_n0 = id_n1;
        if (id_n1 != 0xFFFFFFFFu) { n0 = splats[id_n1 * 4 + 0]; n1 = splats[id_n1 * 4 + 1]; n2 = splats[id_n1 * 4 + 2]; }
        load_features<VEC4>(features, id_n1, C, c0, fn);
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
#pragma unroll
            for (int j = 0; j < FEAT_Q; ++j) s_feat[s * FEAT_Q + j] = fq[j];
        }
        __builtin_amdgcn_wave_barrier();      // (no instruction: the wave's LDS accesses stay in program order; the lanes read each other's records)
        const uint32_t left = (uint32_t)__popcll(mask);
        const uint32_t pos_base = base - range.x + 1;
        for (uint32_t u = 0; u < left; ++u) {
            const float4 r0 = s_rec[u * 2 + 0];
            const float4 r1 = s_rec[u * 2 + 1];
            // ---- the forward's p2, alpha and testT (gsr_blend.h; blend_step_bf), so that the hard masks and T are the forward's bits ----
            const float dx = r0.x - pxf, dy = r0.y - pyf;
            const float p2 = gsrb::p2(dx, dy, r0.z, r0.w, r1.x);           // log2(e) * power
            const float alpha = gsrb::alpha(r1.y, p2);
            const bool contrib = (p2 <= 0.0f) & (alpha >= GSR_ALPHA_MIN) & (pos_base + __float_as_uint(r1.z) <= last);
            const float testT = fmaf(-alpha, Tl, Tl);                // T (1 - alpha)
            const float w = alpha * Tl;
            // ---- the pixel's own accumulators: predicated updates, nothing crosses lanes.  The row is read before the test (one address per wave: a
            // broadcast) and pinned there, or its reads sink, dword by dword, into branches of their own; the updates then share ONE region under
            // the lanes' mask (FEAT_G v_fmac_f32) instead of a select per channel ----
            float4 f[FEAT_Q];
#pragma unroll
            for (int j = 0; j < FEAT_Q; ++j) f[j] = s_feat[u * FEAT_Q + j];
#pragma unroll
            for (int j = 0; j < FEAT_Q; ++j) { gsrw::dpp_pin(f[j].x); gsrw::dpp_pin(f[j].y); gsrw::dpp_pin(f[j].z); gsrw::dpp_pin(f[j].w); }
            if (contrib) {
#pragma unroll
                for (int j = 0; j < FEAT_Q; ++j) {
                    acc[4 * j + 0] = fmaf(w, f[j].x, acc[4 * j + 0]);
                    acc[4 * j + 1] = fmaf(w, f[j].y, acc[4 * j + 1]);
                    acc[4 * j + 2] = fmaf(w, f[j].z, acc[4 * j + 2]);
                    acc[4 * j + 3] = fmaf(w, f[j].w, acc[4 * j + 3]);
                }
                Tl = testT;
            }
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites the tables
    }
    if (inside) {
        const int64_t plane = (int64_t)cam.W * cam.H;
#pragma unroll
        for (int k = 0; k < FEAT_G; ++k)
            if (c0 + k < C) out[(int64_t)(c0 + k) * plane + pix] = acc[k];      // (wave-uniform test)
    }
}

template <int FEAT_NB /*float4 per slot record: 4 FEAT_NB channels per walk*/>
__global__ void __launch_bounds__(64)
feature_grad_walk(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                  const float4* __restrict__ splats, const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dout /*[C,H,W]*/, int C,
                  int c0, float4* __restrict__ slots /*[4][R][FEAT_NB] the channel sums*/, uint8_t* __restrict__ slot_flags /*[R][4]*/, int64_t R) {
    __shared__ float4 s_rec[64 * 2];            // the batch's survivors, compacted: (x, y, a2, b2) (c2, opacity, lane bits, -)
    __shared__ float4 s_out[64 * FEAT_NB];      // per entry of the batch (by lane): the FEAT_GB channel sums
    const gsrb::TileQuad tq = gsrb::block8_of_workgroup(blockIdx.x);      // the forward's mapping: the four blocks of a tile on one XCD
    const int tile_local = tq.tile_local, quad = tq.quad;
    if (tile_local >= n_band_tiles) return;
    const gsrb::Block8 blk(cam, tile_local, quad);
    const int tile = blk.tile, tx = blk.tx, ty = blk.ty;
    const int lane = threadIdx.x;
    const int bx0 = blk.bx0, by0 = blk.by0;
    if (bx0 >= cam.W || by0 >= cam.H) return;
    const int px = bx0 + (lane & 7), py = by0 + (lane >> 3);
    const bool inside = px < cam.W && py < cam.H;
    const float pxf = (float)px, pyf = (float)py;
    const float x0 = (float)bx0, x1 = (float)min(bx0 + 7, cam.W - 1);
    const float y0 = (float)by0, y1 = (float)min(by0 + 7, cam.H - 1);
    const uint2 range = ranges[tile];
    const int64_t pix = inside ? (int64_t)py * cam.W + px : 0;
    const int64_t plane = (int64_t)cam.W * cam.H;
    // (unconditional loads from clamped addresses: a load behind a test of another load's value is a serial chain)
    const uint32_t nc = n_contrib[pix];
    float g[4 * FEAT_NB];      // the pixel's upstream gradient of the group's channels; 0 outside the image and past the last channel
#pragma unroll
    for (int k = 0; k < 4 * FEAT_NB; ++k) g[k] = dL_dout[(int64_t)min(c0 + k, C - 1) * plane + pix];
#pragma unroll
    for (int k = 0; k < 4 * FEAT_NB; ++k) {
        gsrw::dpp_pin(g[k]);      // (no instruction: the four loads are issued together, not sunk one by one into the branches of the selects below)
        g[k] = (inside && c0 + k < C) ? g[k] : 0.0f;
    }
    const uint32_t last = inside ? nc : 0u;      // list position (from 1) of the pixel's last contributor; 0: the pixel takes no entry
    uint32_t mx = last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    // (the same value in every lane, which the compiler cannot know: as a scalar the loop tests move to the SALU)
    const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)min(range.y - range.x, mx), 0);
    if (end == 0) return;
    const uint32_t list_end = range.x + end;
    float Tl = 1.0f;      // transmittance in front of the next entry (the forward's live T; read while the pixel still contributes)

    auto load_id = [&](uint32_t e) -> uint32_t { return (e + lane < list_end) ? point_list[e + lane] : 0xFFFFFFFFu; };
    uint32_t id_n1 = load_id(range.x);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 n0 = zero4, n1 = zero4, n2 = zero4, n3 = zero4;
    if (id_n1 != 0xFFFFFFFFu) { n0 = splats[id_n1 * 4 + 0]; n1 = splats[id_n1 * 4 + 1]; n2 = splats[id_n1 * 4 + 2]; n3 = splats[id_n1 * 4 + 3]; }
    id_n1 = load_id(range.x + 64);
    float4* slot = slots + (int64_t)quad * R * FEAT_NB;
    for (uint32_t base = range.x; base < list_end; base += 64) {
        const uint32_t n = min(64u, list_end - base);
        float4 q0 = n0, q1 = n1;
        const float4 q2 = n2, q3 = n3;
        // issue the next batch's record gather and the id fetch of the batch after it
        if (id_n1 != 0xFFFFFFFFu) { n0 = splats[id_n1 * 4 + 0]; n1 = splats[id_n1 * 4 + 1]; n2 = splats[id_n1 * 4 + 2]; n3 = splats[id_n1 * 4 + 3]; }
        id_n1 = load_id(base + 128);
        bool keep = false;
        uint32_t k_emit = 0;
        if ((uint32_t)lane < n) {
            const float qmin = gsrb::min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, x0, x1, y0, y1);
            keep = !(qmin > q2.z);                 // q2.z = 2 ln(255 opacity) + 0.01, written by the preprocess
            q0.z = gsrb::conic_diag_to_log2(q0.z);      // conic -> log2 units, sign folded in
            q0.w = gsrb::conic_cross_to_log2(q0.w);
            q1.x = gsrb::conic_diag_to_log2(q1.x);
            k_emit = gsrb::emission_index(q3, (uint32_t)tx, (uint32_t)ty);
        }
        const uint64_t mask = __ballot(keep);
        if (keep) {
            const int s = (int)__popcll(mask & ((1ull << lane) - 1ull));
            s_rec[s * 2 + 0] = q0;
            s_rec[s * 2 + 1] = make_float4(q1.x, q1.y, __uint_as_float((uint32_t)lane), 0.f);
        }
        __builtin_amdgcn_wave_barrier();      // (no instruction: the wave's LDS accesses stay in program order; the lanes read each other's records)
        const uint32_t left = (uint32_t)__popcll(mask);
        const uint32_t pos_base = base - range.x + 1;
        uint64_t touched = 0ull;
        for (uint32_t u = 0; u < left; ++u) {
            const float4 r0 = s_rec[u * 2 + 0];
            const float4 r1 = s_rec[u * 2 + 1];
            const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(r1.z), 0);      // (wave-uniform: the entry's lane of the batch, as a scalar)
            // ---- the forward's p2, alpha and testT (gsr_blend.h; blend_step_bf), so that the hard masks and T are the forward's bits ----
            const float dx = r0.x - pxf, dy = r0.y - pyf;
            const float p2 = gsrb::p2(dx, dy, r0.z, r0.w, r1.x);           // log2(e) * power
            const float alpha = gsrb::alpha(r1.y, p2);
            const bool contrib = (p2 <= 0.0f) & (alpha >= GSR_ALPHA_MIN) & (pos_base + j <= last);
            const float testT = fmaf(-alpha, Tl, Tl);                // T (1 - alpha)
            const float w = alpha * Tl;
            Tl = contrib ? testT : Tl;
            const uint64_t hit = __ballot(contrib);
            if (hit == 0ull) continue;
#ifdef GSR_FEAT_BWD_CHAINS
            // one DPP chain per channel, totals in lane 63 (a lane without a DPP source reads 0, the identity of the sum); lane 63 parks them
#pragma unroll
            for (int h = 0; h < FEAT_NB; ++h) {
                const float s0 = gsrw::wave_sum_to_lane63(contrib ? w * g[4 * h + 0] : 0.0f);
                const float s1 = gsrw::wave_sum_to_lane63(contrib ? w * g[4 * h + 1] : 0.0f);
                const float s2 = gsrw::wave_sum_to_lane63(contrib ? w * g[4 * h + 2] : 0.0f);
                const float s3 = gsrw::wave_sum_to_lane63(contrib ? w * g[4 * h + 3] : 0.0f);
                if (lane == 63) s_out[j * FEAT_NB + h] = make_float4(s0, s1, s2, s3);
            }
#else
            // four channels per reduction (gsr_wave.h reduce4: two permlane swaps, then one DPP chain inside the 16-lane rows): the totals of channels
            // 4h .. 4h+3 arrive in lanes 15, 31, 47, 63, which park one float each.  Every channel is summed in the same association order, wherever
            // it sits in its group of four.
#pragma unroll
            for (int h = 0; h < FEAT_NB; ++h) {
                const float r = gsrw::reduce4(contrib ? w * g[4 * h + 0] : 0.0f, contrib ? w * g[4 * h + 2] : 0.0f,
                                              contrib ? w * g[4 * h + 1] : 0.0f, contrib ? w * g[4 * h + 3] : 0.0f);
                if ((lane & 15) == 15) reinterpret_cast<float*>(s_out)[(j * FEAT_NB + h) * 4 + (lane >> 4)] = r;
            }
#endif
            touched |= 1ull << j;
        }
        __builtin_amdgcn_wave_barrier();
        if ((touched >> lane) & 1ull) {
#pragma unroll
            for (int h = 0; h < FEAT_NB; ++h) slot[(int64_t)k_emit * FEAT_NB + h] = s_out[lane * FEAT_NB + h];
            slot_flags[(int64_t)k_emit * 4 + quad] = 1;
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites both tables
    }
}

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// what feature_grad_reduce does with an instance (gsr_reduce.h reduce_instance_runs): the FEAT_NB float4 of channel sums of its up to four blocks
template <int FEAT_NB>
struct FeatureGradOps {
    struct Value { float4 s[FEAT_NB]; };
    const float4* __restrict__ slots;
    int64_t R;
    float4* s_sum;      // LDS, 64 FEAT_NB
    float4 acc[FEAT_NB];
    __device__ __forceinline__ FeatureGradOps(const float4* slots_, int64_t R_, float4* s_sum_) : slots(slots_), R(R_), s_sum(s_sum_) {
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ Value load(uint32_t f, int64_t k) const {
        Value v;
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) {
            float4 rec[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rec[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((f >> (8 * q)) & 0xFFu) rec[q] = slots[((int64_t)q * R + k) * FEAT_NB + h];
            }
            v.s[h] = rec[0];
#pragma unroll
            for (int q = 1; q < 4; ++q) v.s[h] = add4(v.s[h], rec[q]);      // the up to four blocks of the instance's tile, in slot order (a missing slot adds zeros)
        }
        return v;
    }
    __device__ __forceinline__ void fold_take(Value v, bool own_all) {
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                v.s[h].x += __shfl_xor(v.s[h].x, off, 64);
                v.s[h].y += __shfl_xor(v.s[h].y, off, 64);
                v.s[h].z += __shfl_xor(v.s[h].z, off, 64);
                v.s[h].w += __shfl_xor(v.s[h].w, off, 64);
            }
            if (own_all) acc[h] = add4(acc[h], v.s[h]);      // (per float4, between the butterflies, as this kernel always had it: one region after them all compiles to other code)
        }
    }
    __device__ __forceinline__ void take(const Value& v) {
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) acc[h] = add4(acc[h], v.s[h]);
    }
    __device__ __forceinline__ void park(int lane, const Value& v) const {
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) s_sum[lane * FEAT_NB + h] = v.s[h];
    }
    __device__ __forceinline__ Value parked(uint32_t i) const {
        Value v;
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) v.s[h] = s_sum[i * FEAT_NB + h];
        return v;
    }
};

// feature_grad_reduce<2>'s body, written out, not on reduce_instance_runs: there it compiled to another schedule with one more s_waitcnt (523 instructions against 522).
// The frame below is gsr_reduce.h's, line by line: change them together.
template <int FEAT_NB>
__device__ __forceinline__ void feature_grad_reduce_written_out(int P, int64_t R, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets,
                                                                const float4* __restrict__ slots, const uint32_t* __restrict__ flags,
                                                                float* __restrict__ dL_dfeatures /*[P,C]*/, int C, int c0) {
    __shared__ float4 s_sum[64 * FEAT_NB];
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t jc = j < P ? j : (int64_t)P - 1;
    const uint32_t incl = offsets[jc];
    uint32_t excl = jc > 0 ? offsets[jc - 1] : 0u;
    if (j >= P) excl = incl;                      // (lanes past the last Gaussian own nothing)
    const uint32_t g = order[jc];
    const uint32_t c_begin = (uint32_t)__builtin_amdgcn_readlane((int)excl, 0);
    const uint32_t c_end = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    float4 acc[FEAT_NB];
#pragma unroll
    for (int h = 0; h < FEAT_NB; ++h) acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_flags = [&](uint32_t c) -> uint32_t {
        const int64_t k = (int64_t)c + lane;
        return (c < c_end && k < (int64_t)c_end) ? flags[k] : 0u;
    };
    uint32_t f_next = load_flags(c_begin);
    for (uint32_t c = c_begin; c < c_end; c += 64) {
        const uint32_t f = f_next;
        f_next = load_flags(c + 64);
        if (__ballot(f != 0u) == 0ull) continue;      // nobody contributed through these 64 instances (hidden behind nearer ones)
        const int64_t k = (int64_t)c + lane;
        float4 s[FEAT_NB];
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) {
            float4 rec[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rec[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((f >> (8 * q)) & 0xFFu) rec[q] = slots[((int64_t)q * R + k) * FEAT_NB + h];
            }
            s[h] = rec[0];
#pragma unroll
            for (int q = 1; q < 4; ++q) s[h] = add4(s[h], rec[q]);      // the up to four blocks of the instance's tile, in slot order (a missing slot adds zeros)
        }
        // a chunk inside one Gaussian's run: butterfly (the same total in every lane); else the owners add their instances in order
        const uint32_t lo = max(excl, c), hi = min(incl, c + 64u);
        const bool own_all = lo < hi && hi - lo == 64u;
        if (__ballot(own_all) != 0ull) {
#pragma unroll
            for (int h = 0; h < FEAT_NB; ++h) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    s[h].x += __shfl_xor(s[h].x, off, 64);
                    s[h].y += __shfl_xor(s[h].y, off, 64);
                    s[h].z += __shfl_xor(s[h].z, off, 64);
                    s[h].w += __shfl_xor(s[h].w, off, 64);
                }
                if (own_all) acc[h] = add4(acc[h], s[h]);
            }
            continue;
        }
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) s_sum[lane * FEAT_NB + h] = s[h];
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lo; i < hi; ++i) {
#pragma unroll
            for (int h = 0; h < FEAT_NB; ++h) acc[h] = add4(acc[h], s_sum[(i - c) * FEAT_NB + h]);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (j < P && incl > excl) {
        float* row = dL_dfeatures + (int64_t)g * C + c0;
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) {      // (wave-uniform tests)
            if (c0 + 4 * h + 0 < C) row[4 * h + 0] = acc[h].x;
            if (c0 + 4 * h + 1 < C) row[4 * h + 1] = acc[h].y;
            if (c0 + 4 * h + 2 < C) row[4 * h + 2] = acc[h].z;
            if (c0 + 4 * h + 3 < C) row[4 * h + 3] = acc[h].w;
        }
    }
}

template <int FEAT_NB>
__global__ void __launch_bounds__(64)
feature_grad_reduce(int P, int64_t R, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets, const float4* __restrict__ slots,
                    const uint32_t* __restrict__ flags, float* __restrict__ dL_dfeatures /*[P,C]*/, int C, int c0) {
    if constexpr (FEAT_NB == 2) {      // (see feature_grad_reduce_written_out)
        feature_grad_reduce_written_out<2>(P, R, order, offsets, slots, flags, dL_dfeatures, C, c0);
        return;
    }
    __shared__ float4 s_sum[64 * FEAT_NB];
    FeatureGradOps<FEAT_NB> ops(slots, R, s_sum);
    gsrw::reduce_instance_runs(P, order, offsets, flags, ops, [&](uint32_t g) {
        float* row = dL_dfeatures + (int64_t)g * C + c0;
#pragma unroll
        for (int h = 0; h < FEAT_NB; ++h) {      // (wave-uniform tests)
            if (c0 + 4 * h + 0 < C) row[4 * h + 0] = ops.acc[h].x;
            if (c0 + 4 * h + 1 < C) row[4 * h + 1] = ops.acc[h].y;
            if (c0 + 4 * h + 2 < C) row[4 * h + 2] = ops.acc[h].z;
            if (c0 + 4 * h + 3 < C) row[4 * h + 3] = ops.acc[h].w;
        }
    });
}

}  // namespace

// float4 per slot record of the group that starts with `remaining` channels to go: 16 channels per walk while more than 8 remain, then 8, then 4
static int feature_grad_nb(int remaining) {
    const int nb = remaining > 8 ? 4 : remaining > 4 ? 2 : 1;
    return nb < FEAT_GB / 4 ? nb : FEAT_GB / 4;
}

GsrContribScratch gsr_carve_feature_grad(char* base, int64_t R, int C) {
    return gsr_carve_slots(base, R, feature_grad_nb(C));      // (the first group of a call is its widest)
}

void gsr_launch_render_features_defaults(const GsrCamDev& cam, int C, float* out, hipStream_t st) {
    const GsrBandRows band = gsr_band_rows(cam);
    const size_t plane = (size_t)cam.W * cam.H, first = band.first, pixels = band.pixels;
    if (pixels == 0) return;
    if (pixels == plane) {      // the whole frame: the planes are one contiguous range
        (void)hipMemsetAsync(out, 0, plane * (size_t)C * sizeof(float), st);
        return;
    }
    for (int c = 0; c < C; ++c) (void)hipMemsetAsync(out + (size_t)c * plane + first, 0, pixels * sizeof(float), st);
}

void gsr_launch_render_features(const GsrCamDev& cam, const GsrSavedFrame& f, const float* features, int C, float* out, hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    if (n_band_tiles <= 0) return;
    const int groups = gsr_tile_groups(n_band_tiles, 8);
    const bool vec4 = (C % 4 == 0) && (((uintptr_t)features) & 15) == 0;
    for (int c0 = 0; c0 < C; c0 += FEAT_G) {
        if (vec4)
            hipLaunchKernelGGL(feature_walk<true>, dim3(groups * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats, f.n_contrib,
                               features, C, c0, out);
        else
            hipLaunchKernelGGL(feature_walk<false>, dim3(groups * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats, f.n_contrib,
                               features, C, c0, out);
    }
}

void gsr_launch_render_features_backward(const GsrCamDev& cam, int P, int64_t R, const GsrSavedFrame& f, const float* dL_dout, int C,
                                         const GsrContribScratch& w, float* dL_dfeatures, hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    if (n_band_tiles <= 0 || P <= 0 || R <= 0) return;
    const int groups = gsr_tile_groups(n_band_tiles, 8);
    for (int c0 = 0; c0 < C;) {      // one scratch region, reused group after group on the stream
        const int nb = feature_grad_nb(C - c0);
        (void)hipMemsetAsync(w.flags, 0, (size_t)R * 4, st);
#define GSR_FEATURE_GRAD_GROUP(NB)                                                                                                                  \
        hipLaunchKernelGGL(feature_grad_walk<NB>, dim3(groups * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats,          \
                           f.n_contrib, dL_dout, C, c0, w.slots, reinterpret_cast<uint8_t*>(w.flags), R);                                           \
        hipLaunchKernelGGL(feature_grad_reduce<NB>, dim3((P + 63) / 64), dim3(64), 0, st, P, R, f.order, f.offsets, (const float4*)w.slots,         \
                           (const uint32_t*)w.flags, dL_dfeatures, C, c0)
        if (nb == 4) { GSR_FEATURE_GRAD_GROUP(4); }
        else if (nb == 2) { GSR_FEATURE_GRAD_GROUP(2); }
        else { GSR_FEATURE_GRAD_GROUP(1); }
#undef GSR_FEATURE_GRAD_GROUP
        c0 += 4 * nb;
    }
}
