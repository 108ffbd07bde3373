// The ranking primitives of gsr_wave.h compiled for the HOST through the SIMT-on-CPU shim (tests/test_simt_ranking_widths_cpu.py): match_digit<BITS>
// against the run-time-width loop form for BITS = 1 .. 11, lanes_below against popcount(mask & lt_mask), and the 24-bit emission arithmetic
// (mul_u24, div_small24) against the full-width forms -- on the digits, valid flags and operands the test hands in.
#define __HIPCC__ 1
#include "hip/hip_runtime.h"
#include "gsr_wave.h"
#include "simt_runtime.h"
using namespace gsrw;

namespace {
constexpr int MAX_BITS = 11;
const uint32_t* g_digit;
const uint8_t* g_valid;
uint64_t* g_loop;      // [MAX_BITS][256]
uint64_t* g_tmpl;      // [MAX_BITS][256]
uint32_t* g_below;     // [MAX_BITS][256][2]: lanes_below, popcount(mask & lt_mask)

template <int BITS>
void one_width(int tid, int lane, uint32_t d, bool valid) {
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint32_t dig = d & ((1u << BITS) - 1u);
    const uint64_t a = match_digit(dig, BITS, __ballot(valid));
    const uint64_t b = match_digit<BITS>(dig, __ballot(valid));
    const uint64_t c = match_digit_w<BITS>(dig, BITS, __ballot(valid)), e = match_digit_w<0>(dig, BITS, __ballot(valid));
    g_loop[(BITS - 1) * 256 + tid] = a;
    g_tmpl[(BITS - 1) * 256 + tid] = (c == b && e == a) ? b : ~b;      // (the dispatching form must pick the same two)
    g_below[((BITS - 1) * 256 + tid) * 2] = lanes_below(b, lt_mask);
    g_below[((BITS - 1) * 256 + tid) * 2 + 1] = (uint32_t)__builtin_popcountll(a & lt_mask);
}
template <int BITS>
void all_widths(int tid, int lane, uint32_t d, bool valid) {
    if constexpr (BITS <= MAX_BITS) {
        one_width<BITS>(tid, lane, d, valid);
        all_widths<BITS + 1>(tid, lane, d, valid);
    }
}
void kern() {
    const int tid = threadIdx.x, lane = tid & 63;
    all_widths<1>(tid, lane, g_digit[tid], g_valid[tid] != 0);
}
}  // namespace

// digit[256], valid[256] (one workgroup of four waves) -> loop[11][256], tmpl[11][256] (the masks of the two forms, width b at row b - 1: the digit's low
// b bits are matched), below[11][256][2].  Returns 0, or 1000 when the workgroup could not run.
extern "C" int simt_ranking_match(const uint32_t* digit, const uint8_t* valid, uint64_t* loop, uint64_t* tmpl, uint32_t* below) {
    g_digit = digit; g_valid = valid; g_loop = loop; g_tmpl = tmpl; g_below = below;
    return simt::run_block(0, 1, 256, [] { kern(); }) ? 0 : 1000;
}

// n (a, b) pairs with a < 2^24, 0 < b < 2^16, a / b < 2^16 -> the number of pairs where div_small24 and div_small (quotient or remainder), or either and
// the integer division, disagree; and n (x, y) pairs below 2^24 -> ... where mul_u24 is not x * y
extern "C" int simt_ranking_arith(int n, const uint32_t* a, const uint32_t* b, const uint32_t* x, const uint32_t* y) {
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        uint32_t r0, r1;
        const uint32_t q0 = div_small(a[i], b[i], r0), q1 = div_small24(a[i], b[i], r1);
        bad += q0 != q1 || r0 != r1 || q0 != a[i] / b[i] || r0 != a[i] % b[i];
        bad += mul_u24(x[i], y[i]) != x[i] * y[i];
    }
    return bad;
}
