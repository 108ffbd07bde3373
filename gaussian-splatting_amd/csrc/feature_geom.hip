// Geometry and opacity gradients through the N-channel feature render (gsr_render_features_backward_geometry, include/gsr.h; no reference
// counterpart): with F[c,p] = sum_i w_ip f[id_i,c] of features.hip, g_c = dL/dF[c,p] and s_i = <f[id_i], g>, front to back over the contributors of p
//     dL/dalpha_i = T_i s_i - (sum_{j>i} w_j s_j) / (1 - alpha_i)          (no background / T_final term: F has none)
//     m_i         = opacity_i G_i dL/dalpha_i                              (uncapped opacity * G, straight through the 0.99 cap, as for colour)
// and per Gaussian the five moments of m over the pixel offsets plus the zeroth moment -- words 0..5 of the instance records of the blend backward
// (render_bwd.hip), which its reduce (gsr_launch_reduce_instances) turns into the [P,12] records that the per-Gaussian backward consumes.
//
//  feature_geom_walk   render_bwd_half's frame: one wave64 per 16x8 HALF tile, two pixels per lane, the list walked BACK TO FRONT from final_T in batches
//                      of 64 (ids two batches ahead, the 64-byte record gather one batch ahead, the forward's box test per quadrant, `pos < last` per
//                      pixel, p2 / alpha by the forward's operation sequence of gsr_blend.h), the state (T, acc) with T <- T rcp(1 - alpha),
//                      diff = s - acc, dL/dalpha = diff T, acc <- fma(alpha, diff, acc).  The front-to-back closed form (F . g minus a prefix) cancels
//                      where the suffix is small and then divides by 1 - alpha >= 0.01: not used.
//                      THE FEATURE ROW of an entry is wave-uniform in the step, as in feature_walk: the Gaussian lanes gather it with the record (one batch
//                      ahead, 4 NQ floats per lane, from a clamped and therefore always valid address) and park it in an LDS table beside the record, which
//                      the step reads as a broadcast.  Every lane holds its two pixels' dL/dF of the group's channels in registers (loaded once, from
//                      clamped addresses).  s = act ? sum_k f_k g_k : 0 per pixel -- a select under the pair's own predicate, not a zeroed weight: rows of
//                      Gaussians that contribute nowhere may hold anything.
//                      SIX sums per (half tile, entry) cross the wave: four through the permlane folds (one value per 16-lane row), two through a
//                      permlane32 fold and the row broadcast, both DPP chains interleaved stage by stage.
//  Channel groups      4 NQ channels per walk: 16 (GSR_FEAT_GEOM_G) while more than 8 remain, then 8, then 4.  Which entries a wave touches depends on the geometry alone, so
//                      every group touches the same (half tile, entry) pairs: the first group stores its record and sets the flag byte, a later group
//                      ADDS its six sums to the record its own wave wrote before (launches of one stream: the order is fixed).  The reduce runs once, after
//                      the last group.  No atomics, every sum in a fixed order -> two runs give the same bits.
#include "gsr_internal.h"
#include "gsr_blend.h"
#include "gsr_wave.h"

#ifndef GSR_FEAT_GEOM_G
#define GSR_FEAT_GEOM_G 16      // most channels per walk (8, 16 or 32); chosen by measurement, DESIGN.md 5.7
#endif

namespace {

constexpr int GEOM_G = GSR_FEAT_GEOM_G;
static_assert(GEOM_G == 8 || GEOM_G == 16 || GEOM_G == 32, "GSR_FEAT_GEOM_G must be 8, 16 or 32");

using gsrw::dpp_add;
using gsrw::dpp_pin;
using gsrw::fold16;
using gsrw::fold32;

// The 4 NQ features of Gaussian `id` from channel c0 on: load_features of features.hip (unconditional loads from clamped addresses; what the clamp
// duplicates meets an upstream gradient of 0).  A float4 that lies past the last channel altogether is skipped for the whole wave in the
// float-by-float instantiation (the caller zeroes it once).
template <bool VEC4, int NQ>
__device__ __forceinline__ void load_feature_row(const float* __restrict__ features, uint32_t id, int C, int c0, float4 (&f)[NQ]) {
    const float* row = features + (int64_t)(id != 0xFFFFFFFFu ? id : 0u) * C;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        if (VEC4) {
            f[j] = *reinterpret_cast<const float4*>(row + min(c0 + 4 * j, C - 4));
            continue;
        }
        if (j > 0 && c0 + 4 * j >= C) continue;
        f[j] = make_float4(row[min(c0 + 4 * j + 0, C - 1)], row[min(c0 + 4 * j + 1, C - 1)], row[min(c0 + 4 * j + 2, C - 1)],
                           row[min(c0 + 4 * j + 3, C - 1)]);
    }
}

// one stage of the walk's two reduction chains: between two DPP adds of one chain stands the other chain's add
template <int CTRL>
__device__ __forceinline__ void dpp_stage2(float& a, float& b) {
    a = dpp_add<CTRL, 0xf>(a); dpp_pin(a);
    b = dpp_add<CTRL, 0xf>(b); dpp_pin(b);
}

constexpr int GRAD_WORDS = 8;      // floats per parked entry: the six sums and two words of padding (two float4)

template <bool VEC4, int NQ /*float4 per feature row of the group: 4 NQ channels per walk*/>
__global__ void __launch_bounds__(64)
feature_geom_walk(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                  const float4* __restrict__ splats, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                  const float* __restrict__ features /*[P,C]*/, const float* __restrict__ dL_dout /*[C,H,W]*/, int C, int c0,
                  float4* __restrict__ slot_grads /*[slots][R] records of 3 float4*/, uint8_t* __restrict__ slot_flags /*[R][4]*/, int64_t R,
                  const uint32_t* __restrict__ tile_order /*NULL: index order*/, int wave_order /*tile_order lists (tile << 1 | half) per WAVE*/,
                  int accumulate /*a later channel group: add to the records of the first*/) {
    __shared__ float4 s_rec[64 * 2];            // per entry of the batch (by lane): (x, y, a2, b2) (c2, opacity, -, -)
    __shared__ float4 s_feat[64 * NQ];          // ... and its feature row of this channel group
    __shared__ float s_grad[64 * GRAD_WORDS];   // ... and its six sums
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
    float gA[4 * NQ], gB[4 * NQ];      // the two pixels' upstream gradient of the group's channels; 0 outside the image and past the last channel
#pragma unroll
    for (int k = 0; k < 4 * NQ; ++k) {
        const int64_t ch = (int64_t)min(c0 + k, C - 1) * plane;
        gA[k] = dL_dout[ch + pixA];
        gB[k] = dL_dout[ch + pixB];
    }
#pragma unroll
    for (int k = 0; k < 4 * NQ; ++k) {
        dpp_pin(gA[k]);      // (no instruction: the loads are issued together, not sunk one by one into the branches of the selects below)
        dpp_pin(gB[k]);
        gA[k] = (inA && c0 + k < C) ? gA[k] : 0.0f;
        gB[k] = (inB && c0 + k < C) ? gB[k] : 0.0f;
    }
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
    float4 fn[NQ];
    if (!VEC4) {      // (quads that load_feature_row skips)
#pragma unroll
        for (int j = 0; j < NQ; ++j) fn[j] = zero4;
    }
    if (id_n != 0xFFFFFFFFu) { n0 = splats[id_n * 4 + 0]; n1 = splats[id_n * 4 + 1]; n2 = splats[id_n * 4 + 2]; n3 = splats[id_n * 4 + 3]; }
    load_feature_row<VEC4, NQ>(features, id_n, C, c0, fn);
    id_n = load_id(nbatch - 2);
    for (int bi = nbatch - 1; bi >= 0; --bi) {
        const uint32_t base = (uint32_t)bi * 64u;
        const uint32_t n = min(64u, end - base);
        const float4 q0 = n0, q1 = n1, q2 = n2, q3 = n3;
        float4 fq[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) fq[j] = fn[j];
        // issue the next batch's record and feature gathers and the id fetch of the batch after it
        if (id_n != 0xFFFFFFFFu) { n0 = splats[id_n * 4 + 0]; n1 = splats[id_n * 4 + 1]; n2 = splats[id_n * 4 + 2]; n3 = splats[id_n * 4 + 3]; }
        load_feature_row<VEC4, NQ>(features, id_n, C, c0, fn);
        id_n = load_id(bi - 2);
        bool keepA = false, keepB = false;
        uint32_t k_emit = 0;
        if ((uint32_t)lane < n) {
            const uint32_t pos = base + (uint32_t)lane;
            // an entry at or behind a quadrant's own last contributor touches none of its pixels
            keepA = pos < mxA && !(gsrb::min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, xa0, xa1, y0, y1) > q2.z);
            keepB = quadB_alive && pos < mxB && !(gsrb::min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, xb0, xb1, y0, y1) > q2.z);
            k_emit = gsrb::emission_index(q3, (uint32_t)tx, (uint32_t)ty);
            s_rec[lane * 2 + 0] = make_float4(q0.x, q0.y, gsrb::conic_diag_to_log2(q0.z), gsrb::conic_cross_to_log2(q0.w));
            s_rec[lane * 2 + 1] = make_float4(gsrb::conic_diag_to_log2(q1.x), q1.y, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < NQ; ++j) s_feat[lane * NQ + j] = fq[j];
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
            const float2 r1 = *reinterpret_cast<const float2*>(&s_rec[j * 2 + 1]);
            // the row is read before the test (one address per wave: a broadcast) and pinned there, or its reads sink, dword by dword, into branches
            float4 f[NQ];
#pragma unroll
            for (int h = 0; h < NQ; ++h) f[h] = s_feat[j * NQ + h];
#pragma unroll
            for (int h = 0; h < NQ; ++h) { dpp_pin(f[h].x); dpp_pin(f[h].y); dpp_pin(f[h].z); dpp_pin(f[h].w); }
            const float a2 = r0.z, b2 = r0.w, c2 = r1.x, op = r1.y;
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
            // ---- s = <feature row, dL/dF> under the pair's predicate ----
            float dotA = 0.0f, dotB = 0.0f;
#pragma unroll
            for (int h = 0; h < NQ; ++h) {
                dotA = fmaf(f[h].x, gA[4 * h + 0], dotA); dotB = fmaf(f[h].x, gB[4 * h + 0], dotB);
                dotA = fmaf(f[h].y, gA[4 * h + 1], dotA); dotB = fmaf(f[h].y, gB[4 * h + 1], dotB);
                dotA = fmaf(f[h].z, gA[4 * h + 2], dotA); dotB = fmaf(f[h].z, gB[4 * h + 2], dotB);
                dotA = fmaf(f[h].w, gA[4 * h + 3], dotA); dotB = fmaf(f[h].w, gB[4 * h + 3], dotB);
            }
            const float sA = actA ? dotA : 0.0f, sB = actB ? dotB : 0.0f;
            // ---- a skipped pixel takes part with alpha = 0 and opacity * G = 0: T * rcp(1) = T, fma(0, x, acc) = acc, m = 0 ----
            const float alphaA = actA ? alA : 0.0f, alphaB = actB ? alB : 0.0f;
            const float opGA = actA ? ogA : 0.0f, opGB = actB ? ogB : 0.0f;
            TA = TA * __builtin_amdgcn_rcpf(1.0f - alphaA);
            TB = TB * __builtin_amdgcn_rcpf(1.0f - alphaB);
            const float diffA = sA - accA, diffB = sB - accB;
            const float dLdaA = diffA * TA, dLdaB = diffB * TB;
            accA = fmaf(alphaA, diffA, accA);
            accB = fmaf(alphaB, diffB, accB);
            // ---- the per-pair terms (raw moments of m over the pixel offset: render_bwd.hip moments_to_grads), the two pixels added per lane ----
            const float mA = opGA * dLdaA, mB = opGB * dLdaB;
            const float mdxA = mA * dxA, mdxB = mB * dxB;
            const float msum = mA + mB, mdxsum = mdxA + mdxB;
            const float g_px = mdxsum, g_py = msum * dy, g_A = mdxA * dxA + mdxB * dxB, g_B = mdxsum * dy, g_C = (msum * dy) * dy, g_op = msum;
            float v0 = fold16(fold32(g_px, g_A), fold32(g_py, g_B));     // -> words 0, 1, 2, 3 (lanes 15, 31, 47, 63)
            float v1 = fold32(g_C, g_op);                                // -> words 4 (lane 31), 5 (lane 63)
            dpp_stage2<0x111>(v0, v1);
            dpp_stage2<0x112>(v0, v1);
            dpp_stage2<0x114>(v0, v1);
            dpp_stage2<0x118>(v0, v1);
            v1 = dpp_add<0x142, 0xa>(v1);
            dpp_pin(v1);
            if ((lane & 15) == 15) {
                s_grad[j * GRAD_WORDS + (lane >> 4)] = v0;
                if (lane & 16) s_grad[j * GRAD_WORDS + 4 + (lane >> 5)] = v1;
            }
            touched |= 1ull << j;
        }
        if (touched) {
            __builtin_amdgcn_wave_barrier();
            if ((touched >> lane) & 1ull) {
                float4* dst = slot + (int64_t)k_emit * 3;
                float4 u0 = s_grad4[lane * 2 + 0];
                const float4 t1 = s_grad4[lane * 2 + 1];
                float4 u1 = make_float4(t1.x, t1.y, 0.f, 0.f);
                if (accumulate) {      // (wave-uniform: this wave's own record of the first group)
                    const float4 o0 = dst[0], o1 = dst[1];
                    u0 = make_float4(o0.x + u0.x, o0.y + u0.y, o0.z + u0.z, o0.w + u0.w);
                    u1 = make_float4(o1.x + u1.x, o1.y + u1.y, 0.f, 0.f);
                    dst[0] = u0;
                    dst[1] = u1;
                } else {
                    dst[0] = u0;
                    dst[1] = u1;
                    dst[2] = zero4;
                    slot_flags[(int64_t)k_emit * 4 + half] = 1;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites the tables
    }
}

// float4 per feature row of the group that starts with `remaining` channels to go: GEOM_G channels per walk while more than half of them remain, then
// half as many, down to 4 (GEOM_G = 16: 16 while more than 8 remain, then 8, then 4)
int geom_group_nq(int remaining) {
    int nq = GEOM_G / 4;
    while (nq > 1 && remaining <= 2 * nq) nq >>= 1;
    return nq;
}

}  // namespace

void gsr_launch_feature_geometry_walks(const GsrCamDev& cam, int64_t R, const GsrSavedFrame& f, int order_mode, const float* features,
                                       const float* dL_dout, int C, float* inst_grads, uint32_t* inst_flag, hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    // instances that contributed nowhere get no record: only their flag words are cleared -- in the plan kernel's launch, or with a fill.  The plan
    // (the blend backward's: the cost of a half tile is the forward's count of the entries it blended) serves every group of the call.
    if (n_band_tiles <= 0) {
        (void)hipMemsetAsync(inst_flag, 0, (size_t)R * 4, st);
        return;
    }
    const uint32_t* tile_order = gsr_launch_bwd_plan(cam, f.block_steps, order_mode ? f.tile_order : nullptr, inst_flag, R, order_mode, st) ? f.tile_order : nullptr;
    const int wave_order = (tile_order && order_mode == 3) ? 1 : 0;
    const int groups16 = gsr_tile_groups(n_band_tiles, 16);
    const bool vec4 = (C % 4 == 0) && (((uintptr_t)features) & 15) == 0;
    for (int c0 = 0; c0 < C;) {
        const int nq = geom_group_nq(C - c0);
#define GSR_FEATURE_GEOM_GROUP(VEC, NQ)                                                                                                                  \
        hipLaunchKernelGGL((feature_geom_walk<VEC, NQ>), dim3(groups16 * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats,      \
                           f.final_T, f.n_contrib, features, dL_dout, C, c0, reinterpret_cast<float4*>(inst_grads),                                      \
                           reinterpret_cast<uint8_t*>(inst_flag), R, tile_order, wave_order, c0 > 0 ? 1 : 0)
        if (vec4) {
#if GSR_FEAT_GEOM_G >= 32
            if (nq == 8) { GSR_FEATURE_GEOM_GROUP(true, 8); } else
#endif
            if (nq == 4) { GSR_FEATURE_GEOM_GROUP(true, 4); }
            else if (nq == 2) { GSR_FEATURE_GEOM_GROUP(true, 2); }
            else { GSR_FEATURE_GEOM_GROUP(true, 1); }
        } else {
#if GSR_FEAT_GEOM_G >= 32
            if (nq == 8) { GSR_FEATURE_GEOM_GROUP(false, 8); } else
#endif
            if (nq == 4) { GSR_FEATURE_GEOM_GROUP(false, 4); }
            else if (nq == 2) { GSR_FEATURE_GEOM_GROUP(false, 2); }
            else { GSR_FEATURE_GEOM_GROUP(false, 1); }
        }
#undef GSR_FEATURE_GEOM_GROUP
        c0 += 4 * nq;
    }
}
