// A/B measurement variant (compiled only into lib_ab/ with -DGSR_AB_VARIANTS; included by gaussian-splatting_amd/csrc/render_bwd.hip inside its anonymous
// namespace).  Not part of the product library.
// ------------------------------------------------------------------------------------------------
// variant 1 (A/B baseline): wave per 8x8 block, DPP full-wave reductions, one global atomic set per (block, Gaussian)
// into the per-Gaussian record
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
render_bwd_wave(GsrCamDev cam, int n_band_tiles, const uint2* __restrict__ ranges,
                const uint32_t* __restrict__ point_list, const float4* __restrict__ splats,
                const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                const float* __restrict__ dL_dpix, const float* __restrict__ dL_dinvdepth, float* __restrict__ grads) {
    const int b = blockIdx.x;
    const int grp = b >> 5, r32 = b & 31;
    const int tile_local = grp * 8 + (r32 & 7);
    const int quad = r32 >> 3;
    if (tile_local >= n_band_tiles) return;
    const int tile = cam.tile_y0 * cam.gx + tile_local;
    const int tx = tile % cam.gx, ty = tile / cam.gx;
    const int lane = threadIdx.x;
    const int bx0 = tx * GSR_TILE + (quad & 1) * 8, by0 = ty * GSR_TILE + (quad >> 1) * 8;
    if (bx0 >= cam.W || by0 >= cam.H) return;
    const int px = bx0 + (lane & 7), py = by0 + (lane >> 3);
    const bool inside = px < cam.W && py < cam.H;
    const float pxf = (float)px, pyf = (float)py;
    const float x0 = (float)bx0, x1 = (float)min(bx0 + 7, cam.W - 1);
    const float y0 = (float)by0, y1 = (float)min(by0 + 7, cam.H - 1);
    const uint2 range = ranges[tile];
    const int64_t pix = (int64_t)py * cam.W + px;
    const int64_t HW = (int64_t)cam.H * cam.W;
    const float T_final = inside ? final_T[pix] : 0.f;
    const uint32_t last_contrib = inside ? n_contrib[pix] : 0u;
    const float dLr = inside ? dL_dpix[pix] : 0.f;
    const float dLg = inside ? dL_dpix[HW + pix] : 0.f;
    const float dLb = inside ? dL_dpix[2 * HW + pix] : 0.f;
    const float dLd = (inside && dL_dinvdepth) ? dL_dinvdepth[pix] : 0.f;
    const float Tf_bg = -T_final * (cam.bg[0] * dLr + cam.bg[1] * dLg + cam.bg[2] * dLb);
    uint32_t max_contrib = last_contrib;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) max_contrib = max(max_contrib, (uint32_t)__shfl_xor((int)max_contrib, off, 64));
    const uint32_t end = min(range.y - range.x, max_contrib);
    if (end == 0) return;
    BwdPix s = {T_final, 0.f, 0.f, 0.f};
    for (int bstart = (int)((end - 1) & ~63u); bstart >= 0; bstart -= 64) {
        const uint32_t n = min(64u, end - (uint32_t)bstart);
        float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
        float colb = 0.f, invd = 0.f;
        uint32_t id = 0;
        bool keep = false;
        if ((uint32_t)lane < n) {
            id = point_list[range.x + bstart + lane];
            q0 = splats[id * 4 +0];
            q1 = splats[id * 4 +1];
            const float4 q2 = splats[id * 4 +2];
            colb = q2.x;
            invd = q2.w;
            keep = !(min_q_over_box(q0.x, q0.y, q0.z, q0.w, q1.x, x0, x1, y0, y1) > q2.z);
        }
        uint64_t mask = __ballot(keep);
        while (mask) {
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const uint32_t pos0 = (uint32_t)bstart + (uint32_t)j;
            const float gx_ = bcast(q0.x, j), gy_ = bcast(q0.y, j), cA = bcast(q0.z, j), cB = bcast(q0.w, j);
            const float cC = bcast(q1.x, j), op = bcast(q1.y, j), cr = bcast(q1.z, j), cg = bcast(q1.w, j);
            const float cb = bcast(colb, j), idp = bcast(invd, j);
            const uint32_t gid = (uint32_t)__builtin_amdgcn_readlane((int)id, j);
            float g_px, g_py, g_A, g_B, g_C, g_op, g_r, g_g, g_b, g_d;
            const bool active = bwd_step(s, pos0 < last_contrib, pxf, pyf, Tf_bg, dLr, dLg, dLb, dLd, gx_, gy_,
                                         gsrb::conic_diag_to_log2(cA), gsrb::conic_cross_to_log2(cB), gsrb::conic_diag_to_log2(cC), op, cr, cg, cb, idp, g_px, g_py,
                                         g_A, g_B, g_C, g_op, g_r, g_g, g_b, g_d);
            if (__builtin_amdgcn_ballot_w64(active) == 0ull) continue;
            g_px = wave_sum_to_lane63(g_px); g_py = wave_sum_to_lane63(g_py);
            g_A = wave_sum_to_lane63(g_A); g_B = wave_sum_to_lane63(g_B); g_C = wave_sum_to_lane63(g_C);
            g_op = wave_sum_to_lane63(g_op);
            g_r = wave_sum_to_lane63(g_r); g_g = wave_sum_to_lane63(g_g); g_b = wave_sum_to_lane63(g_b);
            g_d = wave_sum_to_lane63(g_d);
            if (lane == 63) {
                float* o = grads + (int64_t)gid * 12;
                float4 u0 = make_float4(g_px, g_py, g_A, g_B), u1 = make_float4(g_C, 0.f, 0.f, 0.f);
                u1.y = g_op;
                moments_to_grads(cA, cB, cC, op, u0, u1);
                atomicAdd(o + 0, u0.x); atomicAdd(o + 1, u0.y);
                atomicAdd(o + 2, u0.z); atomicAdd(o + 3, u0.w); atomicAdd(o + 4, u1.x);
                atomicAdd(o + 5, u1.y);
                atomicAdd(o + 6, g_r); atomicAdd(o + 7, g_g); atomicAdd(o + 8, g_b);
                atomicAdd(o + 9, g_d);
            }
        }
    }
}

