// What the streaming loss kernels (loss.hip, consistency.hip) share: the class limit, the width of a block's partial row, the
// wavefront sum and the grid cap.  ustrun_loss_partials_bytes sizes a buffer of 2048 rows of NS floats; stream_blocks never asks
// for more than 1024.
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

}  // namespace ustrun
