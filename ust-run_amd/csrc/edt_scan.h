// The column half of the exact integer Euclidean distance transform, shared by surface.hip (distances between two masks'
// borders) and distmap.hip (dense signed distances of every plane): how a boolean plane is read, and the u16 column scan.
#pragma once
#include "common.h"

namespace ustrun {
namespace {

constexpr int COL_INF = 4096;            // > any distance inside a 1024-pixel column; COL_INF^2 + 1023^2 fits an int
constexpr int SURF_MAX = 1024;           // H, W limit: d2 <= 2 * 1023^2 < 2^21

// the boolean plane of ustrun_dice_counts: (x == c + 1) of a class map, or (x != 0)
__device__ __forceinline__ bool fg_at(const void* m, int is64, int by_class, long base, int c, long e) {
    if (by_class) {
        const long long v = is64 ? ((const long long*)m)[base + e] : (long long)((const float*)m)[base + e];
        return v == c + 1;
    }
    return is64 ? ((const long long*)m)[base + e] != 0 : ((const float*)m)[base + e] != 0.f;
}

// col[map][H][W]: 0 on the pixels of a set, COL_INF elsewhere -> in place, the distance along the column to the nearest pixel of
// the set, capped at COL_INF.  grid (ceil(W / 64), maps), one thread per column: down, then up, 8 rows loaded ahead of the
// dependent chain
__global__ __launch_bounds__(64) void colscan_kernel(int H, int W, unsigned short* __restrict__ col) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    unsigned short* p = col + (long)blockIdx.y * H * W + x;
    int d = COL_INF;
    for (int y0 = 0; y0 < H; y0 += 8) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = y0 + j < H ? p[(long)(y0 + j) * W] : COL_INF;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d = v[j] == 0 ? 0 : min(d + 1, COL_INF);
            if (y0 + j < H) p[(long)(y0 + j) * W] = (unsigned short)d;
        }
    }
    d = COL_INF;
    for (int y0 = H - 1; y0 >= 0; y0 -= 8) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = y0 - j >= 0 ? p[(long)(y0 - j) * W] : COL_INF;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d = min(v[j], min(d + 1, COL_INF));
            if (y0 - j >= 0) p[(long)(y0 - j) * W] = (unsigned short)d;
        }
    }
}

}  // namespace
}  // namespace ustrun
