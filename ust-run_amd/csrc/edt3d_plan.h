// The host/device arithmetic of the 3-D distance kernels (edt3d.hip) that is pure integer or f64 bookkeeping: the limits, the
// overflow bound, the percentile ranks, how a long list of rows or maps is folded onto a grid, the radix digits of the select, and
// the two searches (along x inside a row, along z across slices) for one output element.  No HIP type is named here, so
// tests/host/edt3d_plan_check.hip replays every function on the CPU over the ranges its comment claims.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDT3D_HD __host__ __device__ inline
#else
#define EDT3D_HD inline
#endif

namespace ustrun {
namespace edt3d {

constexpr int VOL_MAX = 1024;                        // D, H, W limit
constexpr int64_t VOX_MAX = (int64_t)1 << 27;        // D * H * W limit: a list of both borders has at most 2^28 entries, an int
constexpr int WEIGHT_MAX = 255;
constexpr int64_t D2_MAX = 2147483646;               // 2^31 - 2: every finite d2 stays below G_NONE = USTRUN_DIST_NONE = 2^31 - 1
constexpr int G_NONE = 0x7fffffff;                   // in-slice distance of a row whose slice has no source
constexpr int64_t NK_MAX = 32767;
constexpr int GRID_Y_MAX = 65535;
constexpr int GRID_X_FOLD = 1 << 20;                 // blocks of a folded 1-D grid: the rest of the list is walked in a loop

EDT3D_HD bool sizes_ok(int N, int K, int D, int H, int W) {
    return N > 0 && K > 0 && D >= 1 && H >= 1 && W >= 1 && D <= VOL_MAX && H <= VOL_MAX && W <= VOL_MAX &&
           (int64_t)N * K <= NK_MAX;
}
EDT3D_HD bool voxels_ok(int D, int H, int W) { return (int64_t)D * H * W <= VOX_MAX; }
EDT3D_HD bool weights_ok(int wz, int wy, int wx) {
    return wz >= 1 && wy >= 1 && wx >= 1 && wz <= WEIGHT_MAX && wy <= WEIGHT_MAX && wx <= WEIGHT_MAX;
}
// the largest d2 between two voxels of the volume, in int64: at most 3 * 255^2 * 1023^2 < 2^38
EDT3D_HD int64_t d2_bound(int D, int H, int W, int wz, int wy, int wx) {
    const int64_t a = (int64_t)wz * (D - 1), b = (int64_t)wy * (H - 1), c = (int64_t)wx * (W - 1);
    return a * a + b * b + c * c;
}
EDT3D_HD bool d2_fits(int D, int H, int W, int wz, int wy, int wx) { return d2_bound(D, H, W, wz, wy, wx) <= D2_MAX; }

// numpy's linear percentile 95 of n >= 1 values sits at 0.95 (n - 1), taken in f64: the ranks of its two neighbours
EDT3D_HD int rank95(int n) { return (int)(0.95 * (double)(n - 1)); }          // (>= 0: truncation is floor)
EDT3D_HD int rank95_next(int n) { const int k = rank95(n); return k + 1 < n ? k + 1 : n - 1; }

// a list of `items` (>= 1) walked by a grid of `per` items per block: the block count, at most `cap`; block b takes the groups
// b, b + blocks, b + 2 blocks, ... of `per` items each
EDT3D_HD int fold_blocks(int64_t items, int per, int cap) {
    const int64_t groups = (items + per - 1) / per;
    return (int)(groups < cap ? groups : cap);
}

// the three radix levels of the order-statistic select over values in [0, 2^31): 11 + 10 + 10 bits
constexpr int L1_BITS = 11, L2_BITS = 10, L3_BITS = 10;
EDT3D_HD int digit1(int v) { return v >> (L2_BITS + L3_BITS); }
EDT3D_HD int digit2(int v) { return (v >> L3_BITS) & ((1 << L2_BITS) - 1); }
EDT3D_HD int digit3(int v) { return v & ((1 << L3_BITS) - 1); }
EDT3D_HD int prefix2(int v) { return v >> L3_BITS; }                          // digits 1 and 2 together

// ---- the two searches of the separable transform, one output element each (edt3d.hip's kernels call them per lane)
constexpr int COL_CAP = 4096;                        // edt_scan.h's COL_INF: a column without a source
EDT3D_HD int imin(int a, int b) { return a < b ? a : b; }

// ---- pass 3, one pixel: min over x' of wy2 other[x']^2 + wx2 (x - x')^2 over the finite entries of the row, G_NONE if none
EDT3D_HD int row_min(const unsigned short* other, int x, int W, int wy2, int wx2, bool any) {
    if (!any) return G_NONE;
    const int g = other[x];
    int best = g < COL_CAP ? wy2 * g * g : G_NONE;
    for (int dx = 1; dx < W; ++dx) {
        const int c = wx2 * dx * dx;
        if (c >= best) break;
        const int xl = x - dx, xr = x + dx;
        if (xl < 0 && xr >= W) break;
        if (xl >= 0) { const int v = other[xl]; if (v < COL_CAP) best = imin(best, wy2 * v * v + c); }
        if (xr < W) { const int v = other[xr]; if (v < COL_CAP) best = imin(best, wy2 * v * v + c); }
    }
    return best;
}

// ---- pass 4, one voxel: min over z' of g2(z') + wz2 (z - z')^2, from `best` = the own slice's g2 (G_NONE if it has none).
// p points at the voxel in a map [D][HW].  SIGNED: the map holds the signed values above and `fg` is the voxel's kind
template <bool SIGNED>
EDT3D_HD int z_min(const int* p, int z, int D, long HW, int wz2, int best, bool fg) {
    for (int dz = 1; dz < D; ++dz) {
        const int c = wz2 * dz * dz;
        if (c >= best) break;
        const int zl = z - dz, zr = z + dz;
        if (zl < 0 && zr >= D) break;
        for (int side = 0; side < 2; ++side) {
            const int zz = side ? zr : zl;
            if (zz < 0 || zz >= D) continue;
            int u = p[(long)(zz - z) * HW];
            if (SIGNED) u = ((u < 0) != fg) ? 0 : (u < 0 ? -u : u);        // a voxel of the opposite kind right there: g2 = 0
            if (u != G_NONE) best = imin(best, u + c);
        }
    }
    return best;
}

}  // namespace edt3d
}  // namespace ustrun
