// What the kernels that walk the per-tile splat lists must compute IDENTICALLY (device only): the forward blend (render_fwd.hip) decides which
// entries a wave keeps and which pixels take them; the blend backward (render_bwd.hip), the contribution statistics (contrib.hip) and the per-pixel
// probe (probe.hip) trust its n_contrib and re-derive alpha and the hard masks, which is correct only while those are the forward's bits.  One definition each of the box
// test, the conic pre-scale, the exponent / alpha sequence, the emission index and the placement of a wave per 8x8 pixel block.  The loops, the
// prefetch pipeline, the LDS parking and the per-kernel step bodies stay in their files.  Every helper here compiles to the instructions of the
// code it replaced, kernel by kernel; one that does not is not shared (see Block8).
#pragma once
#include "gsr_internal.h"

namespace gsrb {

constexpr float LOG2E = 1.4426950408889634f;

// Smallest value of q(d) = A dx^2 + 2 B dx dy + C dy^2 over the pixel box [x0,x1]x[y0,y1] for a Gaussian centred
// at (mx,my).  Exact for positive-definite (A,B,C): the minimiser is the centre if it is inside, otherwise it
// lies on an edge facing the centre, where q restricted to the edge is a 1-D parabola with a clamped optimum.
__device__ __forceinline__ float min_q_over_box(float mx, float my, float A, float B, float C, float x0, float x1,
                                                float y0, float y1) {
    const float lx = x0 - mx, hx = x1 - mx, ly = y0 - my, hy = y1 - my;   // box in centre-relative coords
    const bool in_x = (lx <= 0.0f) && (hx >= 0.0f);
    const bool in_y = (ly <= 0.0f) && (hy >= 0.0f);
    float q = 3.0e38f;
    if (in_x && in_y) return 0.0f;
    if (!in_x) {
        const float dx = lx > 0.0f ? lx : hx;                 // facing vertical edge
        const float dy = fminf(hy, fmaxf(ly, -B * dx * __builtin_amdgcn_rcpf(C)));   // clamped optimum along it (tau carries a 0.01 margin: v_rcp_f32's ulp is harmless)
        q = fminf(q, A * dx * dx + 2.0f * B * dx * dy + C * dy * dy);
    }
    if (!in_y) {
        const float dy = ly > 0.0f ? ly : hy;
        const float dx = fminf(hx, fmaxf(lx, -B * dy * __builtin_amdgcn_rcpf(A)));
        q = fminf(q, A * dx * dx + 2.0f * B * dx * dy + C * dy * dy);
    }
    return q;
}

// conic -> log2 units with the sign folded in, done once by the Gaussian lanes: power * log2(e) = a2 dx^2 + b2 dx dy + c2 dy^2 with
// a2 = conic_diag_to_log2(A), b2 = conic_cross_to_log2(B), c2 = conic_diag_to_log2(C)
__device__ __forceinline__ float conic_diag_to_log2(float AC) { return -0.5f * LOG2E * AC; }
__device__ __forceinline__ float conic_cross_to_log2(float B) { return -LOG2E * B; }

// log2(e) * power of a pixel at offset (dx, dy) from the centre: mul, fma, fma -- this operation order is part of the contract
__device__ __forceinline__ float p2(float dx, float dy, float a2, float b2, float c2) {
    const float t = fmaf(b2, dy, a2 * dx);
    return fmaf(dx, t, (c2 * dy) * dy);
}
// the same for two pixels of one row (the blend backward's lanes): the square term is shared, every operation is p2's
__device__ __forceinline__ void p2_pair(float dxA, float dxB, float dy, float a2, float b2, float c2, float& p2A, float& p2B) {
    const float u = (c2 * dy) * dy;
    const float tA = fmaf(b2, dy, a2 * dxA), tB = fmaf(b2, dy, a2 * dxB);
    p2A = fmaf(dxA, tA, u);
    p2B = fmaf(dxB, tB, u);
}
// opacity * G -> alpha (the 0.99 cap), and alpha from the exponent (one v_exp_f32: the conic is in log2 units)
__device__ __forceinline__ float alpha_of(float opG) { return fminf(GSR_ALPHA_MAX, opG); }
__device__ __forceinline__ float alpha(float op, float p2_) { return alpha_of(op * __builtin_amdgcn_exp2f(p2_)); }

// q3 of the splat record = (rect.x bits, rect.y bits, first emission index bits, tiles bits), see preprocess.hip / binning.hip
__device__ __forceinline__ uint32_t emission_index(const float4 q3, uint32_t tx, uint32_t ty) {
    const uint32_t rx = __float_as_uint(q3.x), ry = __float_as_uint(q3.y), goff = __float_as_uint(q3.z);
    const uint32_t minx = rx & 0xFFFFu, w = (rx >> 16) - minx, miny = ry & 0xFFFFu;
    return goff + (ty - miny) * w + (tx - minx);
}

// XCD-aware mapping of the kernels that run one 64-thread workgroup per 8x8 block: workgroup b runs on XCD b % 8 (observed).  The four 8x8
// blocks of a tile share one splat list, so they get ids b, b+8, b+16, b+24 -> same XCD -> they share the gathered records in L2.
struct TileQuad { int tile_local, quad; };
__device__ __forceinline__ TileQuad block8_of_workgroup(int b) {
    const int grp = b >> 5, r32 = b & 31;
    return {grp * 8 + (r32 & 7), r32 >> 3};
}

// One wave per 8x8 pixel block: where quadrant `quad` (bit 0: right half, bit 1: lower half) of tile `tile_local` of the camera's band lies.
// The lane's pixel, `inside` and the box clamped to the image stay written out in the kernels: in a helper they reach the optimiser's early
// passes as a call, and contrib_walk then compiles to other instructions (s_bfe for s_lshr + s_and, a moved v_cvt) -- the bar is none.
struct Block8 {
    int tile, tx, ty;            // tile index in the frame and its grid coordinates
    int bx0, by0;                // the block's first pixel (the block has none if that lies outside the image)
    __device__ __forceinline__ Block8(const GsrCamDev& cam, int tile_local, int quad) {
        tile = cam.tile_y0 * cam.gx + tile_local;
        tx = tile % cam.gx; ty = tile / cam.gx;
        bx0 = tx * GSR_TILE + (quad & 1) * 8; by0 = ty * GSR_TILE + (quad >> 1) * 8;
    }
};

}  // namespace gsrb
