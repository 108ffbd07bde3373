// wave64 / workgroup primitives shared by the binning, sorting and blend kernels (device only): integer DPP scans, workgroup scans, digit matching,
// and the float DPP / permlane reductions of the blend backward and the contribution statistics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsrw {

constexpr int WG_THREADS = 256;
constexpr int WG_WAVES = WG_THREADS / 64;

// Wave-wide inclusive scans with DPP moves (gfx9 family: row_shr inside the 16-lane rows, row_bcast:15 / row_bcast:31
// across them) instead of __shfl_up: a __shfl_up is a ds_bpermute_b32 -- an LDS-crossbar round trip of ~100 cycles that
// the next step depends on, six in a row per scan -- while the DPP forms are plain VALU operand modifiers (the compiler
// fuses most steps into v_add_u32_dpp).  Lanes without a source (row start, masked row) read 0.  All lanes must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_src_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
#define GSR_DPP_SCAN_STEPS(STEP) STEP(0x111, 0xf) STEP(0x112, 0xf) STEP(0x114, 0xf) STEP(0x118, 0xf) STEP(0x142, 0xa) STEP(0x143, 0xc)

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int /*lane*/) {
#define GSR_STEP(C, M) v += dpp_src_u32<C, M>(v);
    GSR_DPP_SCAN_STEPS(GSR_STEP)
#undef GSR_STEP
    return v;
}

__device__ __forceinline__ uint32_t wave_incl_max_u32(uint32_t v) {
#define GSR_STEP(C, M) v = max(v, dpp_src_u32<C, M>(v));
    GSR_DPP_SCAN_STEPS(GSR_STEP)
#undef GSR_STEP
    return v;
}

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v, int /*lane*/) {
#define GSR_STEP(C, M) v += ((uint64_t)dpp_src_u32<C, M>((uint32_t)(v >> 32)) << 32) | dpp_src_u32<C, M>((uint32_t)v);
    GSR_DPP_SCAN_STEPS(GSR_STEP)
#undef GSR_STEP
    return v;
}

// Exclusive scan over the 256 threads of a workgroup of the per-thread totals of DPT values (thread t owns entries
// t*DPT .. t*DPT+DPT-1); returns the exclusive prefix of the thread's first entry.  wsum: 4-entry LDS scratch; two barriers.
template <int DPT>
__device__ __forceinline__ uint32_t block_excl_scan(const uint32_t (&v)[DPT], uint32_t* wsum, int lane, int w) {
    uint32_t tsum = 0;
#pragma unroll
    for (int i = 0; i < DPT; ++i) tsum += v[i];
    const uint32_t incl = wave_incl_scan_u32(tsum, lane);
    __syncthreads();
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t wbase = 0;
#pragma unroll
    for (int k = 0; k < WG_WAVES; ++k)
        if (k < w) wbase += wsum[k];
    return wbase + incl - tsum;
}

// a / b and the remainder for a < 2^24, 0 < b < 2^16 with a quotient < 2^16: one v_rcp_f32 and a +-1 correction instead
// of the ~30-instruction integer division sequence
__device__ __forceinline__ uint32_t div_small(uint32_t a, uint32_t b, uint32_t& rem) {
    uint32_t q = (uint32_t)((float)a * __builtin_amdgcn_rcpf((float)b));
    int r = (int)a - (int)(q * b);
    if (r < 0) { --q; r += (int)b; }
    else if (r >= (int)b) { ++q; r -= (int)b; }
    rem = (uint32_t)r;
    return q;
}

// a * b for a, b < 2^24: v_mul_u32_u24, one issue slot, where the full v_mul_lo_u32 takes four.  The low 32 bits of the product, i.e. exactly
// `a * b` while both operands fit 24 bits (the caller's duty; the host form masks the operands as the instruction does, so a violation shows in tests/simt).
__device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b) {
#ifdef GSR_SIMT_SHIM
    return (a & 0xFFFFFFu) * (b & 0xFFFFFFu);
#else
    return __umul24(a, b);
#endif
}
// div_small for operands that also keep q * b inside 24 x 24 bits (q <= 2^16, b < 2^16): the same quotient and remainder, the product by mul_u24
__device__ __forceinline__ uint32_t div_small24(uint32_t a, uint32_t b, uint32_t& rem) {
    uint32_t q = (uint32_t)((float)a * __builtin_amdgcn_rcpf((float)b));
    int r = (int)a - (int)mul_u24(q, b);
    if (r < 0) { --q; r += (int)b; }
    else if (r >= (int)b) { ++q; r -= (int)b; }
    rem = (uint32_t)r;
    return q;
}

// no instruction: the wave-uniform value exists in an SGPR here, so the optimiser does not fold the expression that made it into its consumers
__device__ __forceinline__ uint32_t pin_sgpr_u32(uint32_t v) {
#if !defined(GSR_SIMT_SHIM)
    asm volatile("" : "+s"(v));
#endif
    return v;
}

// 64-bit mask of the lanes whose `digit` (low `bits` bits significant) equals this lane's, among the lanes in `valid_mask`.
// FOUR VALU instructions per bit: the bit sign-extended by one v_bfe_i32, one v_cmp for the ballot, and "mask & ~(ballot ^ bit)" as one
// v_bitop3_b32 per half (truth table 0x90 = a & ~(b ^ c)).  The plain form ("mask &= bit ? bal : ~bal") compiles to EIGHT (v_and, two v_cmp,
// v_cndmask 0 / -1, two v_xor, two v_and).  Every ranking kernel of the forward's binning chain spends most of its VALU here (emit_scatter: 16 items x 7
// bits per thread and block; bucket_scatter 16 x 6; ds_scatter 16 x 11; ds_segsort 2-3 passes x 9).  Measured, same box, interleaved
// (profiles/r05_ab_candidates.json): depth sort + emission + tile sort 0.182 -> 0.174 ms; bins bit-exact on the GPU suites.
__device__ __forceinline__ uint64_t match_digit(uint32_t digit, int bits, uint64_t valid_mask) {
    uint32_t lo = (uint32_t)valid_mask, hi = (uint32_t)(valid_mask >> 32);
    for (int b = 0; b < bits; ++b) {            // wave-uniform trip count
        const int sx = __builtin_amdgcn_sbfe((int)digit, (unsigned)b, 1u);      // 0 / -1
        const uint64_t bal = __ballot(sx != 0);
        lo = __builtin_amdgcn_bitop3_b32(lo, (uint32_t)bal, (uint32_t)sx, 0x90);
        hi = __builtin_amdgcn_bitop3_b32(hi, (uint32_t)(bal >> 32), (uint32_t)sx, 0x90);
    }
    return ((uint64_t)hi << 32) | lo;
}
// The same mask for a digit width known at compile time: the chain fully unrolled -- the same four VALU per bit, and none of what the rolled loop adds
// to every bit (loop counter, compare, taken branch and the wait state between the v_cmp's SGPR result and its VALU reader).  The first bit reads
// `valid_mask` as the wave-uniform value it is instead of a per-lane copy of it.  Straight-line code, so the chains of neighbouring items can be
// interleaved by the scheduler.  The run-time form above stays for widths without an instantiation.
// (The bit is extracted by a v_bfe_i32 the optimiser cannot see through: with the position a constant it rewrites the builtin into shift-left,
// compare-with-0 and arithmetic shift right -- three VALU for the sign mask and the ballot where v_bfe_i32 + v_cmp_ne are two.)
template <int B>
__device__ __forceinline__ int digit_bit_sx(uint32_t digit) {
#ifdef GSR_SIMT_SHIM
    return __builtin_amdgcn_sbfe((int)digit, (unsigned)B, 1u);
#else
    int sx;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(sx) : "v"(digit), "n"(B));
    return sx;
#endif
}
template <int B, int BITS>
__device__ __forceinline__ void match_digit_step(uint32_t digit, uint32_t& lo, uint32_t& hi) {
    if constexpr (B < BITS) {
        const int sx = digit_bit_sx<B>(digit);      // 0 / -1
        const uint64_t bal = __ballot(sx != 0);
        lo = __builtin_amdgcn_bitop3_b32(lo, (uint32_t)bal, (uint32_t)sx, 0x90);
        hi = __builtin_amdgcn_bitop3_b32(hi, (uint32_t)(bal >> 32), (uint32_t)sx, 0x90);
        match_digit_step<B + 1, BITS>(digit, lo, hi);
    }
}
template <int BITS>
__device__ __forceinline__ uint64_t match_digit(uint32_t digit, uint64_t valid_mask) {
    static_assert(BITS >= 1 && BITS <= 16, "digit width");
    uint32_t lo = (uint32_t)valid_mask, hi = (uint32_t)(valid_mask >> 32);
    match_digit_step<0, BITS>(digit, lo, hi);
    return ((uint64_t)hi << 32) | lo;
}
// BITS = 0: the run-time width (one source for both forms of a ranking kernel)
template <int BITS>
__device__ __forceinline__ uint64_t match_digit_w(uint32_t digit, int bits, uint64_t valid_mask) {
    if constexpr (BITS > 0) return match_digit<BITS>(digit, valid_mask);
    else return match_digit(digit, bits, valid_mask);
}

// Number of lanes below this one that are set in `mask` = popcount(mask & lt_mask), lt_mask = (1 << lane) - 1: v_mbcnt_lo / v_mbcnt_hi apply the
// lane mask themselves -- two VALU instead of two v_and and two v_bcnt.  0 <=> this lane is the lowest one of the mask (the "leader" of the ranking loops).
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask, uint64_t lt_mask) {
#ifdef GSR_SIMT_SHIM
    return (uint32_t)__popcll(mask & lt_mask);
#else
    (void)lt_mask;
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
#endif
}

// ------------------------------------------------------------------------------------------------
// float reductions over the wave (blend backward, contribution statistics)
// ------------------------------------------------------------------------------------------------
#ifdef GSR_SIMT_SHIM      // (tests/simt/: the kernel source compiled for the host, where the two swap builtins are functions of the shim)
typedef uint2 uint2v;
#else
typedef unsigned uint2v __attribute__((ext_vector_type(2)));
#endif

// Every cross-lane add of the walk is ONE v_add_f32_dpp: the DPP moves use the full row mask and bound_ctrl (a lane without a source reads 0; the rows a
// partial row mask would protect only hold partial sums nobody reads: row_bcast:15 results are consumed in lanes 31 / 63, row_bcast:31 in lane 63), and
// the sum is pinned in a register before the branch that consumes it.  (Rounds 2-4 left four of them per step as v_mov 0 + v_mov_dpp + v_add: the
// compiler sinks the add of the last row_shr into the "(lane & 15) == 15" branch -- a DPP move cannot follow it there -- and it cannot fuse a move with a
// partial row mask into a float add, the kept lanes would need -0 + 0 = -0.)  103 -> 95 VALU per step; the consumed lanes add the same values in the same
// order, so the gradients are the bits of the earlier form (tests/test_simt_forward_cpu.py ran both); measured on the GPU, same box, interleaved:
// blend backward 0.342 -> 0.326 ms (profiles/r05_ab_candidates.json).
// dpp_pin: no instruction -- the sum exists in all lanes here, so its add stays next to its DPP move instead of sinking into the consumer's branch, and
// the pins of one stage keep their order
__device__ __forceinline__ void dpp_pin(float& r) {
#if !defined(GSR_SIMT_SHIM)
    asm volatile("" : "+v"(r));
#endif
}
template <int CTRL, int ROW_MASK /*documents which rows consume the result; the move itself takes all rows*/>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true);
    return v + __int_as_float(moved);
}
// The maximum of NON-NEGATIVE floats, taken on their bit patterns: they order like their bits, +0 (what a lane without a source reads) is the smallest
// of them, and an integer maximum needs no NaN canonicalisation of its operands -- one v_max_u32_dpp.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max_bits(uint32_t m) {
    return max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, CTRL, 0xf, 0xf, true));
}

// sum over the 64 lanes; the total is valid in lane 63 only
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    v = dpp_add<0x111, 0xf>(v);   // row_shr:1
    v = dpp_add<0x112, 0xf>(v);   // row_shr:2
    v = dpp_add<0x114, 0xf>(v);   // row_shr:4
    v = dpp_add<0x118, 0xf>(v);   // row_shr:8
    v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 -> rows 1,3
    v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 -> rows 2,3
    return v;
}
// The same chain and, stage by stage beside it, the maximum of the values clamped at 0 (as bits): s = sum(v), m = bits of max(0, max v), both valid in
// lane 63 only.  A lane without a DPP source reads 0: the identity of the sum and of a maximum that is clamped at 0 by definition.
__device__ __forceinline__ void wave_sum_max_to_lane63(float v, float& s, uint32_t& m) {
    s = v;
    m = __float_as_uint(fmaxf(v, 0.0f));
#define GSR_STEP(C, M) s = dpp_add<C, M>(s); m = dpp_max_bits<C>(m);
    GSR_DPP_SCAN_STEPS(GSR_STEP)
#undef GSR_STEP
}

// [a.lo+a.hi | b.lo+b.hi] : lanes 0-31 hold 32 partial sums of a, lanes 32-63 of b
__device__ __forceinline__ float fold32(float a, float b) {
    const uint2v r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
// rows (16 lanes): [p.row0+p.row1 | q.row0+q.row1 | p.row2+p.row3 | q.row2+q.row3]
__device__ __forceinline__ float fold16(float p, float q) {
    const uint2v r = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(q), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
// Four values summed over the wave at once.  Result: lane 15 -> sum(a), lane 31 -> sum(c), lane 47 -> sum(b),
// lane 63 -> sum(d) (other lanes hold partial sums).
__device__ __forceinline__ float reduce4(float a, float b, float c, float d) {
    float v = fold16(fold32(a, b), fold32(c, d));
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    return v;
}

// Two values summed over the wave: lane 31 -> sum(a), lane 63 -> sum(b)
__device__ __forceinline__ float reduce2(float a, float b) {
    float v = fold32(a, b);
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 -> rows 1,3
    return v;
}

}  // namespace gsrw
