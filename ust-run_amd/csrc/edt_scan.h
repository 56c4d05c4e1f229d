// The pieces of the exact integer Euclidean distance transform shared by surface.hip (distances between two masks' borders),
// distmap.hip (dense signed distances of every plane) and edt3d.hip (both, for volumes): how a boolean plane is read, the u16
// column scan, and the normalisation of a signed squared distance map (distmap.hip per plane, edt3d.hip per volume).
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
// dependent chain.  colscan_column is one thread's work on the column at p (edt3d.hip walks more maps than a grid's y extent
// holds with it)
__device__ __forceinline__ void colscan_column(int H, int W, unsigned short* __restrict__ p) {
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
__global__ __launch_bounds__(64) void colscan_kernel(int H, int W, unsigned short* __restrict__ col) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    colscan_column(H, W, col + (long)blockIdx.y * H * W + x);
}

// ---- the normalisation of a signed squared distance map (distmap.hip per plane, edt3d.hip per volume: HW is the map's size)
constexpr int MAX_PER_BLOCK = 2048;      // planemax_kernel: pixels per block

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// grid (ceil(HW / 2048), N * K), 256 threads.  mx[plane] = {max d2 over foreground, max d2 over background}, zeroed before
__global__ __launch_bounds__(256) void planemax_kernel(long HW, const int* __restrict__ s2, const int* __restrict__ flags,
                                                      int* __restrict__ mx) {
    const int plane = blockIdx.y;
    if (flags[plane] != 1) return;
    const int* p = s2 + (long)plane * HW;
    int pos = 0, neg = 0;
    const long e0 = (long)blockIdx.x * MAX_PER_BLOCK + threadIdx.x;
#pragma unroll
    for (int j = 0; j < MAX_PER_BLOCK / 256; ++j) {
        const long e = e0 + j * 256;
        const int v = e < HW ? p[e] : 0;
        pos = max(pos, -v);
        neg = max(neg, v);
    }
    pos = wave_max_i32(pos);
    neg = wave_max_i32(neg);
    if ((threadIdx.x & 63) == 0) {
        if (pos > 0) atomicMax(&mx[plane * 2], pos);
        if (neg > 0) atomicMax(&mx[plane * 2 + 1], neg);
    }
}

// grid (ceil(HW / 256), N * K)
__global__ __launch_bounds__(256) void normalise_kernel(long HW, const int* __restrict__ s2, const int* __restrict__ flags,
                                                       const int* __restrict__ mx, float* __restrict__ sdf) {
    const int plane = blockIdx.y;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= HW) return;
    float r = 0.f;
    if (flags[plane] == 1) {
        const int v = s2[(long)plane * HW + e];
        if (v > 0) r = (float)(sqrt((double)v) / sqrt((double)mx[plane * 2 + 1]));
        else if (v < -1) r = (float)-(sqrt((double)-v) / sqrt((double)mx[plane * 2]));       // v == -1: the inner boundary, 0
    }
    sdf[(long)plane * HW + e] = r;
}

}  // namespace
}  // namespace ustrun
