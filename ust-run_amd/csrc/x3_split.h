// x3_split.h -- the arithmetic of dtype USTRUN_F32X3 shared by its kernels (x3.hip, wgrad_tap_x3.hip, conv_first.hip): an f32 value as three bf16
// terms, a product of two such values as six bf16 MFMAs with f32 accumulation (see x3.hip's header).
#pragma once
#include "common.h"

namespace ustrun {
namespace {

#define X3_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

// three bf16 terms of four f32 values, each plane as two dwords (four bf16)
__device__ __forceinline__ void split4(const f32x4 v, u32x2& p0, u32x2& p1, u32x2& p2) {
    b16x4 h0, h1, h2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        h0[q] = (__bf16)v[q];
        const float r1 = v[q] - (float)h0[q];          // exact: the low 16 bits of v (+ the rounding carry)
        h1[q] = (__bf16)r1;
        const float r2 = r1 - (float)h1[q];            // exact
        h2[q] = (__bf16)r2;
    }
    p0 = __builtin_bit_cast(u32x2, h0); p1 = __builtin_bit_cast(u32x2, h1); p2 = __builtin_bit_cast(u32x2, h2);
}

// the six products of one fragment pair, small terms first
__device__ __forceinline__ f32x16 mfma6(const b16x8 (&a)[3], const b16x8 (&b)[3], f32x16 c) {
    c = X3_MFMA(a[0], b[2], c, 0, 0, 0);
    c = X3_MFMA(a[1], b[1], c, 0, 0, 0);
    c = X3_MFMA(a[2], b[0], c, 0, 0, 0);
    c = X3_MFMA(a[0], b[1], c, 0, 0, 0);
    c = X3_MFMA(a[1], b[0], c, 0, 0, 0);
    c = X3_MFMA(a[0], b[0], c, 0, 0, 0);
    return c;
}

}  // namespace
}  // namespace ustrun
