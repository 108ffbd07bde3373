// Per-Gaussian blend-weight statistics of one forward (gsr_contribution_stats, include/gsr.h; no reference counterpart): for every
// Gaussian i, over the pixels p it was blended into, with w_ip = alpha_ip * T_ip (the forward's `alpha * Tl`) and a per-pixel weight E,
//     weight_sum[i] = sum_p E(p) w_ip,   weight_max[i] = max(0, max_p E(p) w_ip),   pixel_count[i] = #{p : E(p) != 0, i contributes to p}.
// The importance scores of the pruning recipes (sum / max of alpha T), the error-weighted densification scores (E = a per-pixel error) and
// hit counts, read from the state the tracking forward keeps instead of a second forward plus a blend backward of sum E C.
//
// Two kernels, NO atomics, every sum in a fixed association order -> two runs give the same bits (the design of render_bwd.hip):
//
//  contrib_walk     one wave64 per 8x8 pixel block, front to back, the forward's structure (render_fwd_wave_bf): ids two batches ahead, the
//                   64-byte record gather one batch ahead, the forward's exact box test, the survivors parked compacted in the wave's LDS, then the
//                   lanes act as pixel lanes with the forward's p2 and alpha (gsr_blend.h) and its testT.  n_contrib is the authority on who
//                   contributed: a pixel takes a valid entry (power <= 0, alpha >= 1/255) exactly when its list position is <= n_contrib[p],
//                   T < 1e-4 is not re-tested, and the wave walks no further than the largest n_contrib of its pixels.  A pixel with
//                   E(p) == 0 -- or outside the image -- takes part with n_contrib = 0.  Per survivor the 64 values E w are summed and
//                   maximised with two DPP chains (totals in lane 63; a lane without a DPP source reads 0, which is the identity of the sum
//                   and of a maximum that is clamped at 0 by definition), the count is popcount(ballot).  Lane 63 parks (sum, max, count)
//                   in an LDS table; after the batch the Gaussian lanes store the touched entries' 16-byte records into the block's SLOT of
//                   the instance's emission index k = goffset + (ty - miny) * w + (tx - minx) (4th quad of the splat record) with plain stores --
//                   a (block, entry) pair is visited once -- plus one flag byte: slots[quad][k], flags[k] byte `quad`.  The launcher clears
//                   the flags (4 R bytes); slots without a flag are never read.
//  contrib_reduce   the instance-run reduce that gsr_reduce.h describes (one wave per 64 consecutive Gaussians of the depth order, the ordered path,
//                   the fold of a chunk owned by one Gaussian, the skipped chunks, its known cost), written out here (see the kernel): the up to
//                   four slot records of an instance combined in slot order, (sum, max, count) per instance.  Then `accumulate` and the
//                   scattered row stores; rows of Gaussians without instances are not touched (the launcher zeroes the arrays when
//                   accumulate == 0).
#include "gsr_internal.h"
#include "gsr_blend.h"
#include "gsr_wave.h"

namespace {

__global__ void __launch_bounds__(64)
contrib_walk(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
             const float4* __restrict__ splats, const uint32_t* __restrict__ n_contrib, const float* __restrict__ pixel_weight /*[H*W] or NULL: 1*/,
             float4* __restrict__ slots /*[4][R] (sum, max, count bits, -)*/, uint8_t* __restrict__ slot_flags /*[R][4]*/, int64_t R) {
    __shared__ float4 s_rec[64 * 2];      // the batch's survivors, compacted: (x, y, a2, b2) (c2, opacity, lane bits, -)
    __shared__ float4 s_out[64];          // per entry of the batch (by lane): (sum, max, count bits, -)
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
    // (unconditional loads from clamped addresses: a load behind a test of another load's value is a serial chain)
    const uint32_t nc = n_contrib[pix];
    const float Ew = pixel_weight ? pixel_weight[pix] : 1.0f;
    const float E = inside ? Ew : 0.0f;
    const uint32_t last = E != 0.0f ? nc : 0u;      // list position (from 1) of the pixel's last contributor; 0: the pixel takes no entry
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
    float4* slot = slots + (int64_t)quad * R;
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
            const float v = contrib ? E * w : 0.0f;
            float s;
            uint32_t m;
            gsrw::wave_sum_max_to_lane63(v, s, m);
            if (lane == 63) s_out[j] = make_float4(s, __uint_as_float(m), __uint_as_float((uint32_t)__popcll(hit)), 0.f);
            touched |= 1ull << j;
        }
        __builtin_amdgcn_wave_barrier();
        if ((touched >> lane) & 1ull) {
            slot[(int64_t)k_emit] = s_out[lane];
            slot_flags[(int64_t)k_emit * 4 + quad] = 1;
        }
        __builtin_amdgcn_wave_barrier();      // the next batch overwrites both tables
    }
}

// (Written out, not gsr_reduce.h's reduce_instance_runs over an ops struct: that form compiled to another schedule of this kernel -- two more s_waitcnt --
// and measured 0.5 - 1 % slower statistics on the MI355X, twice.  The frame below is that header's, line by line: change them together.)
__global__ void __launch_bounds__(64)
contrib_reduce(int P, int64_t R, const uint32_t* __restrict__ order, const uint32_t* __restrict__ offsets, const float4* __restrict__ slots,
               const uint32_t* __restrict__ flags, float* __restrict__ weight_sum, float* __restrict__ weight_max,
               int32_t* __restrict__ pixel_count, int accumulate) {
    __shared__ float s_sum[64];
    __shared__ float s_max[64];
    __shared__ uint32_t s_cnt[64];
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const int64_t jc = j < P ? j : (int64_t)P - 1;
    const uint32_t incl = offsets[jc];
    uint32_t excl = jc > 0 ? offsets[jc - 1] : 0u;
    if (j >= P) excl = incl;                      // (lanes past the last Gaussian own nothing)
    const uint32_t g = order[jc];
    const uint32_t c_begin = (uint32_t)__builtin_amdgcn_readlane((int)excl, 0);
    const uint32_t c_end = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    float acc_s = 0.0f, acc_m = 0.0f;
    uint32_t acc_n = 0u;
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
        float4 rec[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rec[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((f >> (8 * q)) & 0xFFu) rec[q] = slots[(int64_t)q * R + k];
        }
        float s = rec[0].x, m = rec[0].y;
        uint32_t nn = __float_as_uint(rec[0].z);
#pragma unroll
        for (int q = 1; q < 4; ++q) {      // the up to four blocks of the instance's tile, in slot order (a missing slot adds zeros)
            s += rec[q].x;
            m = fmaxf(m, rec[q].y);
            nn += __float_as_uint(rec[q].z);
        }
        // a chunk inside one Gaussian's run: butterfly (the same total in every lane); else the owners add their instances in order
        const uint32_t lo = max(excl, c), hi = min(incl, c + 64u);
        const bool own_all = lo < hi && hi - lo == 64u;
        if (__ballot(own_all) != 0ull) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                s += __shfl_xor(s, off, 64);
                m = fmaxf(m, __shfl_xor(m, off, 64));
                nn += __shfl_xor(nn, off, 64);
            }
            if (own_all) { acc_s += s; acc_m = fmaxf(acc_m, m); acc_n += nn; }
            continue;
        }
        s_sum[lane] = s; s_max[lane] = m; s_cnt[lane] = nn;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lo; i < hi; ++i) {
            acc_s += s_sum[i - c];
            acc_m = fmaxf(acc_m, s_max[i - c]);
            acc_n += s_cnt[i - c];
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (j < P && incl > excl) {
        if (weight_sum) weight_sum[g] = accumulate ? weight_sum[g] + acc_s : acc_s;
        if (weight_max) weight_max[g] = accumulate ? fmaxf(weight_max[g], acc_m) : acc_m;
        if (pixel_count) pixel_count[g] = accumulate ? pixel_count[g] + (int32_t)acc_n : (int32_t)acc_n;
    }
}

}  // namespace

GsrContribScratch gsr_carve_slots(char* base, int64_t R, int nb) {
    GsrContribScratch w;
    const size_t r = (size_t)(R > 0 ? R : 0);
    size_t off = 0;
    w.slots = reinterpret_cast<float4*>(base + off);
    off += gsr_align128(r * 4 * (size_t)nb * sizeof(float4));
    w.flags = reinterpret_cast<uint32_t*>(base + off);
    off += gsr_align128(r * sizeof(uint32_t));
    w.bytes = off;
    return w;
}

void gsr_launch_contribution_stats(const GsrCamDev& cam, int P, int64_t R, const GsrSavedFrame& f, const float* pixel_weight,
                                   const GsrContribScratch& w, float* weight_sum, float* weight_max, int32_t* pixel_count, int accumulate,
                                   hipStream_t st) {
    const int n_band_tiles = gsr_band_tiles(cam);
    if (n_band_tiles <= 0 || P <= 0 || R <= 0) return;
    (void)hipMemsetAsync(w.flags, 0, (size_t)R * 4, st);
    const int groups = gsr_tile_groups(n_band_tiles, 8);
    hipLaunchKernelGGL(contrib_walk, dim3(groups * 32), dim3(64), 0, st, cam, n_band_tiles, f.ranges, f.point_list, f.splats, f.n_contrib,
                       pixel_weight, w.slots, reinterpret_cast<uint8_t*>(w.flags), R);
    hipLaunchKernelGGL(contrib_reduce, dim3((P + 63) / 64), dim3(64), 0, st, P, R, f.order, f.offsets, (const float4*)w.slots,
                       (const uint32_t*)w.flags, weight_sum, weight_max, pixel_count, accumulate);
}
