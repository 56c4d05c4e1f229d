// What the streaming loss kernels (loss.hip, consistency.hip, labelmap.hip) share: the class limit, the width of a block's partial
// row, the wavefront sum, the grid cap, the 16-byte / one-float plane access, a block's partial row and the item walk.
// ustrun_loss_partials_bytes sizes a buffer of 2048 rows of NS floats; stream_blocks never asks for more than 1024.
#pragma once
#include "common.h"

namespace ustrun {

constexpr int KMAX = 8;
constexpr int NS = 1 + 3 * KMAX;   // per-thread running sums of the widest kernel: ce, I[k], Z[k], Y[k]

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid of a grid-stride kernel with blocks of 256: four items per thread, at most 1024 blocks
static inline int stream_blocks(long work_items) {
    long b = (work_items + 256 * 4 - 1) / (256 * 4);
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// V consecutive floats of a plane: one 16-byte access for V = 4, one float for V = 1
template <int V> __device__ __forceinline__ void ldv(const float* p, float (&o)[V]) {
    if constexpr (V == 4) { const f32x4 t = *(const f32x4*)p; o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w; }
    else o[0] = *p;
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&o)[V]) {
    if constexpr (V == 4) *(f32x4*)p = (f32x4){o[0], o[1], o[2], o[3]};
    else *p = o[0];
}

// the first NC running sums of every thread -> the block's partial row (rows are NS floats apart)
template <int NC> __device__ __forceinline__ void block_row(const float (&acc)[NC], float* __restrict__ partials) {
    __shared__ float red[4][NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NC; ++i) { const float v = wave_sum(acc[i]); if (lane == 0) red[wave][i] = v; }
    __syncthreads();
    if (threadIdx.x < NC)
        partials[(long)blockIdx.x * NS + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// item i of a [N, HW / V] walk -> image and first pixel (32-bit divide: N * HW < 2^32, checked on the host)
template <int V> __device__ __forceinline__ void item_at(long i, int per, long& n, long& hw) {
    n = (unsigned)i / (unsigned)per;
    hw = (i - n * per) * V;
}

}  // namespace ustrun
