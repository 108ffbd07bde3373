// A/B measurement variants (compiled only into lib_ab/ with -DGSR_AB_VARIANTS; included by gaussian-splatting_amd/csrc/render_bwd.hip inside its anonymous
// namespace, before the variants).  Not part of the product library: what only the variants of this directory use -- the one-pixel-per-lane step of
// rounds 1-2 and the whole-wave reductions it was paired with (gsr_wave.h: reduce4 / reduce2 / wave_sum_to_lane63).
using gsrb::LOG2E;
using gsrb::emission_index;
using gsrb::min_q_over_box;
using gsrw::reduce2;
using gsrw::reduce4;
using gsrw::wave_sum_to_lane63;

__device__ __forceinline__ float bcast(float v, int srclane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), srclane));
}

// per-pixel running state of the back-to-front walk (Appendix A.5).  The reference keeps one running colour per channel
// ("accum_rec") and dots (c - accum) with dL/dpixel afterwards; both are linear in the channel, so the walk here carries
// the already-dotted scalars: accD = <accum, dL/dpix>, lastD = <last colour, dL/dpix> -- 2 VALU ops per step instead of 12.
struct BwdPix {
    float T, accD, lastD, last_alpha;
};

// One (pixel, Gaussian) step: the ten per-pair values of render_bwd.hip (raw moments, see moments_to_grads there), zero when the pixel does not
// take part.  Returns whether it did.
__device__ __forceinline__ bool bwd_step(BwdPix& s, bool take, float pxf, float pyf, float Tf_bg, float dLr, float dLg,
                                         float dLb, float dLd, float gx_, float gy_, float a2, float b2, float c2, float op,
                                         float cr, float cg, float cb, float idp, float& mx, float& my, float& mxx,
                                         float& mxy, float& myy, float& g_op, float& g_r, float& g_g, float& g_b,
                                         float& g_d) {
    const v2f d = (v2f){gx_, gy_} - (v2f){pxf, pyf};
    const float dx = d.x, dy = d.y;
    const float p2 = gsrb::p2(dx, dy, a2, b2, c2);
    const float G = __builtin_amdgcn_exp2f(p2);
    const float alpha = gsrb::alpha_of(op * G);
    const bool active = take & (p2 <= 0.0f) & (alpha >= GSR_ALPHA_MIN);
    const v2f dL01 = {dLr, dLg}, dL23 = {dLb, dLd};
    const v2f cd = (v2f){cr, cg} * dL01 + (v2f){cb, idp} * dL23;
    const float cD = cd.x + cd.y;
    float w = 0.0f, dL_dalpha = 0.0f;
    if (active) {
        const float inv1ma = __builtin_amdgcn_rcpf(1.0f - alpha);
        s.T = s.T * inv1ma;
        w = alpha * s.T;
        s.accD = fmaf(s.last_alpha, s.lastD - s.accD, s.accD);
        s.lastD = cD;
        s.last_alpha = alpha;
        dL_dalpha = fmaf(cD - s.accD, s.T, Tf_bg * inv1ma);      // Tf_bg = -T_final * <bg, dL/dpix>
    }
    const v2f g01 = w * dL01, g23 = w * dL23;
    g_r = g01.x; g_g = g01.y; g_b = g23.x; g_d = g23.y;
    const float m = op * (G * dL_dalpha);
    g_op = m;                            // zeroth moment (see moments_to_grads)
    const v2f md = m * d;                // (m dx, m dy)
    const v2f mxd = md.x * d;            // (m dx^2, m dx dy)
    mx = md.x; my = md.y;
    mxx = mxd.x; mxy = mxd.y;
    myy = md.y * dy;
    return active;
}
