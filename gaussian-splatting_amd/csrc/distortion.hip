// Distortion loss on a rendered frame (gsr_distortion / gsr_distortion_backward, include/gsr.h; no reference counterpart): the Mip-NeRF 360 regulariser
//     D(p) = sum_i sum_j w_i w_j |t_i - t_j|
// over the contributors of pixel p, w = alpha T the forward's blend weight, t the view-space depth z of the Gaussian (depth_mode 0) or 1/z (1): the two
// values the splat record carries.  The lists are sorted by depth, so t is monotone along a list and the pairwise sum is the PREFIX FORM of the contract,
// front to back with A_<i = sum_{j<i} w_j and B_<i = sum_{j<i} w_j t_j:
//     D(p) = 2 sigma sum_i w_i (t_i A_<i - B_<i)                      sigma = +1 for z, -1 for 1/z
// THE PIVOT: D and its derivatives are invariant under t -> t - c.  Both kernels work on t' = t - c with c the t of list position 0 of the pixel's tile
// (wave-uniform, read from the state): t A - B subtracts two numbers of the size of the scene depth to get one of the size of a depth difference, t' A - B'
// does not.  B' below is always the sum of w t'.
//
//  distortion_map    probe_walk's frame (probe.hip): one wave64 per 8x8 pixel block, one lane per pixel, front to back, the survivors of the forward's box
//                    test parked compacted in LDS, p2 / alpha / testT by the forward's operation sequence (gsr_blend.h), a pixel takes a valid entry
//                    exactly when its list position is <= n_contrib[p].  Three running sums per pixel (A, B', D), nothing crosses lanes, no scratch.
//                    The kernel stores every in-band, in-image pixel itself (zeros where nothing contributes): D and, for the backward, the totals
//                    saved[0] = sum w and saved[1] = sum w t'.
//  distortion_walk   feature_geom_walk's frame (feature_geom.hip): one wave64 per 16x8 HALF tile, two pixels per lane, back to front from final_T in batches
//                    of 64, the record gather one batch ahead, the box test per quadrant, `pos < last` per pixel, the blend backward's launch plan.  Beside
//                    (T, acc) every pixel keeps the SUFFIX sums A_>, B'_> of the entries behind the one at hand; the totals turn them into the prefix
//                    sums, A_< = A_tot - A_> - w.  Per entry
//                        u = dD/dw = 2 sigma [t' (A_< - A_>) - B'_< + B'_>]       v = dD/dt = 2 sigma w (A_< - A_>)
//                    The suffix sums are carried in the combinations the step needs, E = A_tot - 2 A_> and F = 2 B'_> - B'_tot (they start at A_tot and
//                    -B'_tot): A_< - A_> = E - w and -B'_< + B'_> = F + w t', so u = 2 sigma (t' E + F) is one fma and v = 2 sigma w (E - w).
//                    s = g u (g = dL/dD(p), a select under the pair's predicate) enters feature_geom_walk's recurrence T <- T rcp(1 - alpha), diff = s - acc,
//                    dL/dalpha = diff T, acc <- fma(alpha, diff, acc), and m = opacity G dL/dalpha gives the six sums of the instance record's words 0..5.
//                    The SEVENTH sum, sum_p g v, is the depth path: word 9, dL/d(1/z) -- times 1 (depth_mode 1) or -z^2 (depth_mode 0: dL/dz = sum g v and
//                    the per-Gaussian backward applies dtz += -word9 / tz^2), a per-entry factor applied once, by the entry's own lane at the store.
//                    SEVEN sums cross the wave in two registers: [px, A, py, B] and [C, depth, opacity, -], one value per 16-lane row through the permlane
//                    folds, then four DPP row shifts, the two chains interleaved stage by stage.  The reduce (gsr_launch_reduce_instances) adds word 9 of the
//                    records like every other word.
// No atomics, every sum in a fixed order -> two runs give the same bits.
#include "gsr_internal.h"
#include "gsr_blend.h"
#include "gsr_wave.h"

namespace {

using gsrw::dpp_add;
using gsrw::dpp_pin;
using gsrw::fold16;
using gsrw::fold32;

__global__ void __launch_bounds__(64)
distortion_map(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
               const float4* __restrict__ splats, const uint32_t* __restrict__ n_contrib, float* __restrict__ distortion /*[H,W]*/,
               float* __restrict__ saved /*[2,H,W] or NULL*/, int inverse /*t = 1/z*/) {
    __shared__ float4 s_rec[64 * 2];      // the batch's survivors, compacted: (x, y, a2, b2) (c2, opacity, lane bits, t - c)
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
    float Tl = 1.0f;                               // transmittance in front of the next entry (the forward's live T)
    float sumA = 0.0f, sumB = 0.0f, sumD = 0.0f;   // A_<, B'_< and sum w (t' A_< - B'_<) of the entries taken so far

    auto load_id = [&](uint32_t e) -> uint32_t { return (e + lane < list_end) ? point_list[e + lane] : 0xFFFFFFFFu; };
    uint32_t id_n0 = load_id(range.x);      // the ids of the batch whose records are in n0..n2, then of the batch after it
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 n0 = zero4, n1 = zero4, n2 = zero4;
    if (id_n0 != 0xFFFFFFFFu) { n0 = splats[id_n0 * 4 + 0]; n1 = splats[id_n0 * 4 + 1]; n2 = splats[id_n0 * 4 + 2]; }
    uint32_t id_n1 = load_id(range.x + 64);
    // the pivot: t of list position 0 of the tile, which lane 0 of the first batch holds (end == 0: unused)
    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inverse ? n2.w : n2.y), 0));
    for (uint32_t base = range.x; base < list_end; base += 64) {
        const uint32_t n = min(64u, list_end - base);
        float4 q0 = n0, q1 = n1;
        const float4 q2 = n2;
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
            s_rec[s * 2 + 1] = make_float4(q1.x, q1.y, __uint_as_float((uint32_t)lane), (inverse ? q2.w : q2.y) - c);      // q2.y = depth, q2.w = 1 / depth
        }
        __builtin_amdgcn_wave_barrier();      // (no instruction: the wave's LDS accesses stay in program order; the lanes read each other's records)
        const uint32_t left = (uint32_t)__popcll(mask);
        const uint32_t pos_base = base - range.x + 1;
        for (uint32_t u = 0; u < left; ++u) {
            const float4 r0 = s_rec[u * 2 + 0];
            const float4 r1 = s_rec[u * 2 + 1];
            const float tp = r1.w;
            // ---- the forward's p2, alpha and testT (gsr_blend.h; blend_step_bf), so that the hard masks and T are the forward's bits ----
            const float dx = r0.x - pxf, dy = r0.y - pyf;
            const float p2 = gsrb::p2(dx, dy, r0.z, r0.w, r1.x);           // log2(e) * power
            const float alpha = gsrb::alpha(r1.y, p2);
            const bool contrib = (p2 <= 0.0f) & (alpha >= GSR_ALPHA_MIN) & (pos_base + __float_as_uint(r1.z) <= last);
            const float testT = fmaf(-alpha, Tl, Tl);                // T (1 - alpha)
            const float w = alpha * Tl;
            // ---- the pixel's own state: predicated updates, nothing crosses lanes.  The first contributor meets A = B' = 0: it adds an exact 0 to D ----
            const float inner = fmaf(tp, sumA, -sumB);
            sumD = contrib ? fmaf(w, inner, sumD) : sumD;
            sumA = contrib ? sumA + w : sumA;
            sumB = contrib ? fmaf(w, tp, sumB) : sumB;
            Tl = contrib ? testT : Tl;
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites the table
    }
    if (inside) {
        distortion[pix] = (inverse ? -2.0f : 2.0f) * sumD + 0.0f;      // (+ 0: a pixel without a pair stores +0 in both modes)
        if (saved) {
            saved[pix] = sumA;
            saved[(int64_t)cam.H * cam.W + pix] = sumB;
        }
    }
}

// one stage of the walk's two reduction chains: between two DPP adds of one chain stands the other chain's add
template <int CTRL>
__device__ __forceinline__ void dpp_stage2(float& a, float& b) {
    a = dpp_add<CTRL, 0xf>(a); dpp_pin(a);
    b = dpp_add<CTRL, 0xf>(b); dpp_pin(b);
}

constexpr int GRAD_WORDS = 8;      // floats per parked entry: the seven sums and a word that is always zero (two float4)

__global__ void __launch_bounds__(64)
distortion_walk(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                const float4* __restrict__ splats, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                const float* __restrict__ dL_dD /*[H,W]*/, const float* __restrict__ saved /*[2,H,W]*/, int inverse /*t = 1/z*/,
                float4* __restrict__ slot_grads /*[slots][R] records of 3 float4*/, uint8_t* __restrict__ slot_flags /*[R][4]*/, int64_t R,
                const uint32_t* __restrict__ tile_order /*NULL: index order*/, int wave_order /*tile_order lists (tile << 1 | half) per WAVE*/) {
    __shared__ float4 s_rec[64 * 2];            // per entry of the batch (by lane): (x, y, a2, b2) (c2, opacity, t - c, -)
    __shared__ float s_grad[64 * GRAD_WORDS];   // ... and its seven sums
    // the two halves of a tile get workgroup ids b and b + 16 -> same XCD -> they share the gathered records in L2; with tile_order (the blend backward's
    // plan, render_bwd.hip bwd_plan_kernel) the heaviest tiles, or half tiles, start first
    const int b = blockIdx.x;
    int tile_local, half;
    if (wave_order) {
        if (b >= 2 * n_band_tiles) return;
        const uint32_t e = tile_order[b];
        tile_local = (int)(e >> 1);
        half = (int)(e & 1u);
    } else {
        const int grp = b >> 5, r32 = b & 31;
        const int turn = grp * 16 + (r32 & 15);
        half = r32 >> 4;
        if (turn >= n_band_tiles) return;
        tile_local = tile_order ? (int)tile_order[turn] : turn;
    }
    const int tile = cam.tile_y0 * cam.gx + tile_local;
    const int tx = tile % cam.gx, ty = tile / cam.gx;
    const int lane = threadIdx.x;
    const int bx0 = tx * GSR_TILE, by0 = ty * GSR_TILE + half * 8;
    if (by0 >= cam.H) return;
    const int pxA = bx0 + (lane & 7), pxB = pxA + 8, py = by0 + (lane >> 3);
    const bool inA = pxA < cam.W && py < cam.H, inB = pxB < cam.W && py < cam.H;
    const float pxfA = (float)pxA, pxfB = (float)pxB;
    const float pyf = (float)py;
    // boxes of the existing pixels of the two quadrants (the right one may be empty at the image border)
    const float y0 = (float)by0, y1 = (float)min(by0 + 7, cam.H - 1);
    const float xa0 = (float)bx0, xa1 = (float)min(bx0 + 7, cam.W - 1);
    const float xb0 = (float)(bx0 + 8), xb1 = (float)min(bx0 + 15, cam.W - 1);
    const bool quadB_alive = bx0 + 8 < cam.W;
    const uint2 range = ranges[tile];
    // (unconditional loads from clamped addresses: a load behind a test of another load's value is a serial chain)
    const int64_t pixA = inA ? (int64_t)py * cam.W + pxA : 0, pixB = inB ? (int64_t)py * cam.W + pxB : 0;
    const int64_t plane = (int64_t)cam.H * cam.W;
    const float TfA = final_T[pixA], TfB = final_T[pixB];
    const uint32_t ncA = n_contrib[pixA], ncB = n_contrib[pixB];
    float gA = dL_dD[pixA], gB = dL_dD[pixB];                        // the two pixels' upstream gradient, times 2 sigma; 0 outside the image
    float EA = saved[pixA], EB = saved[pixB];                        // E = A_tot - 2 A_>: starts at the forward's sum w of the whole pixel
    float FA = -saved[plane + pixA], FB = -saved[plane + pixB];      // F = 2 B'_> - B'_tot: starts at minus its sum w t'
    const float two_sigma = inverse ? -2.0f : 2.0f;
    gA = inA ? two_sigma * gA : 0.0f;
    gB = inB ? two_sigma * gB : 0.0f;
    const uint32_t lastA = inA ? ncA : 0u, lastB = inB ? ncB : 0u;
    uint32_t mxA = lastA, mxB = lastB;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mxA = max(mxA, (uint32_t)__shfl_xor((int)mxA, off, 64));
        mxB = max(mxB, (uint32_t)__shfl_xor((int)mxB, off, 64));
    }
    // (the butterfly leaves the same maximum in every lane, which the compiler cannot know: as a scalar the loop tests move to the SALU)
    const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)min(range.y - range.x, max(mxA, mxB)), 0);
    if (end == 0) return;
    // the pivot: t of list position 0 of the tile (the range is not empty here); the same address in every lane
    const uint32_t id_first = point_list[range.x];
    const float4 first2 = splats[id_first * 4 + 2];
    const float c = inverse ? first2.w : first2.y;

    float TA = inA ? TfA : 0.0f, TB = inB ? TfB : 0.0f;      // transmittance in front of the entry at hand, walked back from final_T
    float accA = 0.0f, accB = 0.0f;                           // (sum over the entries behind it of w s) / T behind it
    float4* s_grad4 = reinterpret_cast<float4*>(s_grad);
    float4* slot = slot_grads + (int64_t)half * R * 3;
    const int nbatch = (int)((end + 63u) >> 6);
    auto load_id = [&](int bi) -> uint32_t {
        const uint32_t e = (uint32_t)bi * 64u + (uint32_t)lane;
        return (bi >= 0 && e < end) ? point_list[range.x + e] : 0xFFFFFFFFu;
    };
    uint32_t id_n = load_id(nbatch - 1);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 n0 = zero4, n1 = zero4, n2 = zero4, n3 = zero4;
    if (id_n != 0xFFFFFFFFu) { n0 = splats[id_n * 4 + 0]; n1 = splats[id_n * 4 + 1]; n2 = splats[id_n * 4 + 2]; n3 = splats[id_n * 4 + 3]; }
    id_n = load_id(nbatch - 2);
    for (int bi = nbatch - 1; bi >= 0; --bi) {
        const uint32_t base = (uint32_t)bi * 64u;
        const uint32_t n = min(64u, end - base);
        const float4 q0 = n0, q1 = n1, q2 = n2, q3 = n3;
        // issue the next batch's record gather and the id fetch of the batch after it
        if (id_n != 0xFFFFFFFFu) { n0 = splats[id_n * 4 + 0]; n1 = splats[id_n * 4 + 1]; n2 = splats[id_n * 4 + 2]; n3 = splats[id_n * 4 + 3]; }
        id_n = load_id(bi - 2);
        bool keepA = false, keepB = false;
        uint32_t k_emit = 0;
        float depth_factor = 0.0f;      // what turns the entry's sum of g v into word 9, dL/d(1/z)
        if ((uint32_t)lane < n) {
            const uint32_t pos = base + (uint32_t)lane;
            // an entry at or behind a quadrant's own last contributor touches none of its pixels
            keepA = pos < mxA && !(gsrb::min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, xa0, xa1, y0, y1) > q2.z);
            keepB = quadB_alive && pos < mxB && !(gsrb::min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, xb0, xb1, y0, y1) > q2.z);
            k_emit = gsrb::emission_index(q3, (uint32_t)tx, (uint32_t)ty);
            depth_factor = inverse ? 1.0f : -(q2.y * q2.y);
            s_rec[lane * 2 + 0] = make_float4(q0.x, q0.y, gsrb::conic_diag_to_log2(q0.z), gsrb::conic_cross_to_log2(q0.w));
            s_rec[lane * 2 + 1] = make_float4(gsrb::conic_diag_to_log2(q1.x), q1.y, (inverse ? q2.w : q2.y) - c, 0.f);
        }
        const uint64_t maskA = __ballot(keepA), maskB = __ballot(keepB);
        uint64_t mask = maskA | maskB;
        uint64_t touched = 0ull;
        __builtin_amdgcn_wave_barrier();      // (no instruction: the wave's LDS accesses stay in program order; the lanes read each other's records)
        while (mask) {
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const uint32_t pos0 = base + (uint32_t)j;
            const bool doA = (maskA >> j) & 1ull, doB = (maskB >> j) & 1ull;      // wave-uniform
            const float4 r0 = s_rec[j * 2 + 0];
            const float4 r1 = s_rec[j * 2 + 1];
            const float a2 = r0.z, b2 = r0.w, c2 = r1.x, op = r1.y, tp = r1.z;
            // ---- geometry: the forward's operation sequence per pixel (gsr_blend.h), so that the hard masks agree with the forward's bit for bit ----
            const float dxA = r0.x - pxfA, dxB = r0.x - pxfB;
            const float dy = r0.y - pyf;
            float p2A, p2B;
            gsrb::p2_pair(dxA, dxB, dy, a2, b2, c2, p2A, p2B);
            const float GA = __builtin_amdgcn_exp2f(p2A), GB = __builtin_amdgcn_exp2f(p2B);
            const float ogA = op * GA, ogB = op * GB;      // (opacity * G is needed beside alpha)
            const float alA = gsrb::alpha_of(ogA), alB = gsrb::alpha_of(ogB);
            const bool actA = doA & (pos0 < lastA) & (p2A <= 0.0f) & (alA >= GSR_ALPHA_MIN);
            const bool actB = doB & (pos0 < lastB) & (p2B <= 0.0f) & (alB >= GSR_ALPHA_MIN);
            if (__builtin_amdgcn_ballot_w64(actA | actB) == 0ull) continue;
            // ---- a skipped pixel takes part with alpha = 0 and opacity * G = 0: T * rcp(1) = T, w = 0, E and F stay, m = 0 ----
            const float alphaA = actA ? alA : 0.0f, alphaB = actB ? alB : 0.0f;
            const float opGA = actA ? ogA : 0.0f, opGB = actB ? ogB : 0.0f;
            TA = TA * __builtin_amdgcn_rcpf(1.0f - alphaA);
            TB = TB * __builtin_amdgcn_rcpf(1.0f - alphaB);
            const float wA = alphaA * TA, wB = alphaB * TB;
            // ---- u = dD/dw and v = dD/dt (without the 2 sigma that g carries) from E and F, which then take the entry in ----
            const float uA = fmaf(tp, EA, FA), uB = fmaf(tp, EB, FB);
            const float gvA = gA * (wA * (EA - wA)), gvB = gB * (wB * (EB - wB));      // (w = 0 for a skipped pixel)
            const float w2A = wA + wA, w2B = wB + wB;
            EA -= w2A; EB -= w2B;
            FA = fmaf(w2A, tp, FA); FB = fmaf(w2B, tp, FB);
            const float sA = actA ? gA * uA : 0.0f, sB = actB ? gB * uB : 0.0f;      // a select under the pair's own predicate, not a zeroed weight
            const float diffA = sA - accA, diffB = sB - accB;
            const float dLdaA = diffA * TA, dLdaB = diffB * TB;
            accA = fmaf(alphaA, diffA, accA);
            accB = fmaf(alphaB, diffB, accB);
            // ---- the per-pair terms (raw moments of m over the pixel offset: render_bwd.hip moments_to_grads), the two pixels added per lane ----
            const float mA = opGA * dLdaA, mB = opGB * dLdaB;
            const float mdxA = mA * dxA, mdxB = mB * dxB;
            const float msum = mA + mB, mdxsum = mdxA + mdxB;
            const float g_px = mdxsum, g_py = msum * dy, g_A = mdxA * dxA + mdxB * dxB, g_B = mdxsum * dy, g_C = (msum * dy) * dy, g_op = msum;
            const float g_d = gvA + gvB;
            float v0 = fold16(fold32(g_px, g_A), fold32(g_py, g_B));     // rows: px, py, A, B     -> words 0, 1, 2, 3 (lanes 15, 31, 47, 63)
            float v1 = fold16(fold32(g_C, g_op), fold32(g_d, 0.0f));     // rows: C, depth, opacity, 0 -> words 4, 5, 6, 7
            dpp_stage2<0x111>(v0, v1);
            dpp_stage2<0x112>(v0, v1);
            dpp_stage2<0x114>(v0, v1);
            dpp_stage2<0x118>(v0, v1);
            if ((lane & 15) == 15) {
                s_grad[j * GRAD_WORDS + (lane >> 4)] = v0;
                s_grad[j * GRAD_WORDS + 4 + (lane >> 4)] = v1;
            }
            touched |= 1ull << j;
        }
        if (touched) {
            __builtin_amdgcn_wave_barrier();
            if ((touched >> lane) & 1ull) {
                float4* dst = slot + (int64_t)k_emit * 3;
                const float4 t1 = s_grad4[lane * 2 + 1];      // (C, depth, opacity, 0)
                dst[0] = s_grad4[lane * 2 + 0];
                dst[1] = make_float4(t1.x, t1.z, 0.f, 0.f);
                dst[2] = make_float4(0.f, depth_factor * t1.y, 0.f, 0.f);      // word 9
                slot_flags[(int64_t)k_emit * 4 + half] = 1;
            }
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites the tables
    }
}

}  // namespace

void gsr_launch_distortion_defaults(const GsrCamDev& cam, float* distortion, float* saved, hipStream_t st) {
    const GsrBandRows band = gsr_band_rows(cam);
    if (band.pixels == 0) return;
    (void)hipMemsetAsync(distortion + band.first, 0, band.pixels * sizeof(float), st);
    if (!saved) return;
    const size_t plane = (size_t)cam.H * cam.W;
    (void)hipMemsetAsync(saved + band.first, 0, band.pixels * sizeof(float), st);
    (void)hipMemsetAsync(saved + plane + band.first, 0, band.pixels * sizeof(float), st);
}

void gsr_launch_distortion(const GsrCamDev& cam, const GsrSavedFrame& f, float* distortion, float* saved, int depth_mode, hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    if (n_band_tiles <= 0) return;
    const int groups = gsr_tile_groups(n_band_tiles, 8);
    hipLaunchKernelGGL(distortion_map, dim3(groups * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats, f.n_contrib, distortion,
                       saved, depth_mode);
}

void gsr_launch_distortion_walk(const GsrCamDev& cam, int64_t R, const GsrSavedFrame& f, int order_mode, const float* dL_ddistortion, const float* saved,
                                int depth_mode, float* inst_grads, uint32_t* inst_flag, hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    // instances that contributed nowhere get no record: only their flag words are cleared -- in the plan kernel's launch, or with a fill
    if (n_band_tiles <= 0) {
        (void)hipMemsetAsync(inst_flag, 0, (size_t)R * 4, st);
        return;
    }
    const uint32_t* tile_order = gsr_launch_bwd_plan(cam, f.block_steps, order_mode ? f.tile_order : nullptr, inst_flag, R, order_mode, st) ? f.tile_order : nullptr;
    const int wave_order = (tile_order && order_mode == 3) ? 1 : 0;
    const int groups16 = gsr_tile_groups(n_band_tiles, 16);
    hipLaunchKernelGGL(distortion_walk, dim3(groups16 * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats, f.final_T, f.n_contrib,
                       dL_ddistortion, saved, depth_mode, reinterpret_cast<float4*>(inst_grads), reinterpret_cast<uint8_t*>(inst_flag), R, tile_order,
                       wave_order);
}
