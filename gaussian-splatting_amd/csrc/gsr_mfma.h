// The fp32-input matrix instruction of gfx950 behind one name (device only): D = A B + C on a 32 x 32 tile with an inner dimension of 2,
// v_mfma_f32_32x32x2_f32.  One VGPR per operand: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; accumulator register r
// of lane l is the element (row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31).  Every element is the k-ordered chain
//     acc = fmaf(a_k1, b_k1, fmaf(a_k0, b_k0, acc))
// in plain fp32, one rounding per step: the numbers of a VALU fmaf loop at the fp32 vector rate, with the VALU left free.
// Under GSR_SIMT_SHIM (the host build of tests/simt: every lane a fiber) the same arithmetic is written with __shfl, so the host build of a kernel
// that calls this runs the device's numbers.  Every lane of the wave must call it (no exec mask is modelled there, and none is wanted here).
#pragma once
#include <hip/hip_runtime.h>

#ifdef GSR_SIMT_SHIM
__device__ __forceinline__ void gsr_mfma_32x32x2_f32(float a, float b, float (&acc)[16]) {
    const int l = (int)(threadIdx.x & 63u), j = l & 31, h = l >> 5;
    const float b0 = __shfl(b, j), b1 = __shfl(b, j + 32);
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float a0 = __shfl(a, i), a1 = __shfl(a, i + 32);
        acc[r] = fmaf(a1, b1, fmaf(a0, b0, acc[r]));
    }
}
#else
typedef float gsr_f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void gsr_mfma_32x32x2_f32(float a, float b, float (&acc)[16]) {
    gsr_f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = acc[r];
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = c[r];
}
#endif
