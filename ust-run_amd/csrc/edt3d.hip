// Exact Euclidean distances in volumes [D][H][W] on the device (include/ustrun.h: ustrun_signed_dist2_3d,
// ustrun_sdf_from_dist2_3d, ustrun_surface_metrics_3d): the 3-D twins of distmap.hip and surface.hip -- the signed distance map
// the reference's compute_sdf documents for shape (batch_size, x, y, z) (utils/util.py:208-239), and the per-case surface
// distances medpy's binary.hd / hd95 / asd / assd take from n-dimensional masks with `voxelspacing` (train.py:306-325).
//
//   d2(p, q) = wz^2 dz^2 + wy^2 dy^2 + wx^2 dx^2        integer axis weights in 1..255, exact in int32
//
// Three separable passes; a "map" is one slice [H][W] of one kind (signed: foreground / background; surface: border(P) / border(G)):
//   1 seed / border   col[vol][kind][z][y][x] = 0 on a voxel of the kind, COL_INF elsewhere (u16); whether the volume has a voxel of
//                     each kind (signed), resp. how many border voxels (surface), goes to integer counters
//   2 colscan_fold    edt_scan.h's column scan, unchanged per column, over all N K D 2 maps: more maps than a grid's y extent
//                     holds are walked in a loop
//   3 row pass        one wave per row (z, y): g2[x] = min over x' of wy^2 col[x']^2 + wx^2 (x - x')^2, searched outwards from x
//                     while wx^2 dx^2 can still win.  A row whose map has no finite entry belongs to a slice without that kind:
//                     it gets the sentinel G_NONE.  Rows are a folded 1-D list (N K D H of them)
//   4 z pass          one thread per voxel, lanes on consecutive x: d2 = min over z' of g2(z') + wz^2 (z - z')^2, searched
//                     outwards from z while wz^2 dz^2 can still win; every step reads one coalesced row piece of slice z +- dz
// Whether the VOLUME has a voxel of a kind is pass 1's counter, not a slice's fact: without the opposite kind every voxel
// gets +- USTRUN_DIST_NONE (signed) or no distance exists (surface), whatever single slices looked like.
//
// No intermediate overflows an int.  The launchers refuse volumes with wz^2 (D-1)^2 + wy^2 (H-1)^2 + wx^2 (W-1)^2 > 2^31 - 2
// (edt3d_plan.h: d2_fits, in int64).  A finite column entry is at most H - 1, a row offset at most W - 1, a slice offset at most
// D - 1, so wy^2 col^2, wx^2 dx^2, wz^2 dz^2 and every sum of one of each are at most that bound.  An infinite entry -- COL_INF
// in a column, G_NONE in a slice -- is SKIPPED, never squared, multiplied or added to: COL_INF^2 times a weight squared does not
// fit an int.  The search bounds compare w^2 d^2 (bounded as above) with the best value so far, which is a finite d2 or G_NONE.
//
// ustrun_signed_dist2_3d keeps ONE int32 per voxel between passes 3 and 4: + g2 to the slice's foreground at a background voxel,
// - g2 to the slice's background at a foreground voxel (never 0: the opposite kind is at least one weight away); the sign tells
// the kind, so a voxel of the opposite kind in slice z' stands for g2(z') = 0.
// ustrun_surface_metrics_3d keeps both kinds' g2 (a border voxel of P needs the distance to border(G) and the reverse), appends
// the d2 of every border voxel to that side's list (integer wave-aggregated counter: the order in the list is not fixed, nothing
// order-dependent reads it), and selects the two percentile ranks with a three-level radix select (11 + 10 + 10 bits: d2 < 2^31),
// one block per volume.  The two f64 sums of sqrt(d2) are fixed trees over voxel positions (lane, xor butterfly, waves in order,
// 256-voxel blocks in order, butterfly, waves in order); counters and maxima are integer atomics: two runs give the same bits.
#include "common.h"
#include "edt_scan.h"        // COL_INF, fg_at, colscan_column, planemax_kernel, normalise_kernel
#include "edt3d_plan.h"

namespace ustrun {
namespace {

using namespace edt3d;

static_assert(COL_CAP == COL_INF, "edt3d_plan.h names edt_scan.h's infinite column entry");
constexpr int ROWS_PER_BLOCK = 4;        // row kernels: one wave per row

static inline int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// ---- pass 2: the column scan over `maps` slices [H][W].  grid (ceil(W / 64), min(maps, 65535)), 64 threads
__global__ __launch_bounds__(64) void colscan_fold_kernel(int H, int W, long maps, unsigned short* __restrict__ col) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    for (long m = blockIdx.y; m < maps; m += gridDim.y) colscan_column(H, W, col + m * H * W + x);
}

// Both row kernels: grid (fold_blocks(rows, 4, GRID_X_FOLD)), 256 threads; wave w of block b takes the rows 4 (b + i gridDim.x) + w.
// Row r = (vol * D + z) * H + y lies at offset (r mod D H) W of its volume; col[vol][kind][D H W].
// SIGNED: g[vol][D H W] = + g2 to the slice's foreground / - g2 to its background;  else g[vol][kind][D H W] = g2 to that kind
template <bool SIGNED>
__global__ __launch_bounds__(256) void row_kernel(long rows, int DH, int W, int wy2, int wx2, const unsigned short* __restrict__ col,
                                                 int* __restrict__ g) {
    __shared__ unsigned short row[ROWS_PER_BLOCK][2][VOL_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long DHW = (long)DH * W;
    for (long r0 = (long)blockIdx.x * ROWS_PER_BLOCK; r0 < rows; r0 += (long)gridDim.x * ROWS_PER_BLOCK) {      // uniform per block
        const long r = r0 + wave;
        const long vol = r / DH, off = (r % DH) * W;
        bool fin[2] = {false, false};
        if (r < rows)
            for (int kind = 0; kind < 2; ++kind)
                for (int x = lane; x < W; x += 64) {
                    const unsigned short v = col[(vol * 2 + kind) * DHW + off + x];
                    row[wave][kind][x] = v;
                    fin[kind] |= v < COL_INF;
                }
        const bool any0 = __ballot(fin[0]) != 0, any1 = __ballot(fin[1]) != 0;
        __syncthreads();
        if (r < rows)
            for (int x = lane; x < W; x += 64) {
                if (SIGNED) {
                    const bool fg = row[wave][0][x] == 0;
                    const int v = row_min(row[wave][fg ? 1 : 0], x, W, wy2, wx2, fg ? any1 : any0);
                    g[vol * DHW + off + x] = fg ? -v : v;
                } else {
                    g[(vol * 2) * DHW + off + x] = row_min(row[wave][0], x, W, wy2, wx2, any0);
                    g[(vol * 2 + 1) * DHW + off + x] = row_min(row[wave][1], x, W, wy2, wx2, any1);
                }
            }
        __syncthreads();
    }
}

// ======== ustrun_signed_dist2_3d ========
struct DistWork {
    int* has;                // [NK][2]      1 once a foreground / a background voxel of the volume was seen (zeroed every call)
    unsigned short* col;     // [NK][2][DHW]
    int* g;                  // [NK][DHW]
};
int64_t dist_work_bytes(int64_t NK, int64_t DHW) { return up16(NK * 2 * 4) + up16(NK * 2 * DHW * 2) + up16(NK * DHW * 4); }
DistWork dist_carve(void* work, int64_t NK, int64_t DHW) {
    char* p = (char*)work;
    DistWork w;
    w.has = (int*)p; p += up16(NK * 2 * 4);
    w.col = (unsigned short*)p; p += up16(NK * 2 * DHW * 2);
    w.g = (int*)p;
    return w;
}

// grid (ceil(DHW / 256), N * K)
__global__ __launch_bounds__(256) void seed3d_kernel(const void* mask, int is64, int K, int by_class, long DHW,
                                                    unsigned short* __restrict__ col, int* __restrict__ has) {
    const int vol = blockIdx.y, n = vol / K, c = vol % K;
    const long base = by_class ? (long)n * DHW : (long)vol * DHW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = e < DHW;
    const bool fg = in && fg_at(mask, is64, by_class, base, c, e);
    if (in) {
        unsigned short* o = col + (long)vol * 2 * DHW;
        o[e] = fg ? 0 : COL_INF;
        o[DHW + e] = fg ? COL_INF : 0;
    }
    // only "is there one" is asked of `has`: a wave that already sees the mark set skips the atomic, so the two words of a volume
    // take a handful of atomics instead of one per wave (a stale 0 only costs one more)
    const bool any_fg = __ballot(fg) != 0, any_bg = __ballot(in && !fg) != 0;
    if ((threadIdx.x & 63) == 0) {
        volatile int* seen = has + vol * 2;
        if (any_fg && seen[0] == 0) atomicOr(&has[vol * 2], 1);
        if (any_bg && seen[1] == 0) atomicOr(&has[vol * 2 + 1], 1);
    }
}

// grid (ceil(DHW / 256), N * K)
__global__ __launch_bounds__(256) void signed_z_kernel(int D, long HW, int wz2, const int* __restrict__ g, const int* __restrict__ has,
                                                      int* __restrict__ s2, int* __restrict__ flags) {
    const int vol = blockIdx.y;
    const long DHW = (long)D * HW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= DHW) return;
    const bool has_fg = has[vol * 2] != 0, has_bg = has[vol * 2 + 1] != 0;
    if (e == 0) flags[vol] = has_fg ? (has_bg ? 1 : 2) : 0;
    const int* p = g + (long)vol * DHW + e;
    const int own = *p;
    const bool fg = own < 0;
    int best = USTRUN_DIST_NONE;
    if (fg ? has_bg : has_fg) best = z_min<true>(p, (int)(e / HW), D, HW, wz2, fg ? -own : own, fg);
    s2[(long)vol * DHW + e] = fg ? -best : best;
}

// ======== ustrun_surface_metrics_3d ========
struct SurfWork {
    int* cnt;                // [NK][6]      {|border(P)|, |border(G)|, list fill P, list fill G, max d2 P, max d2 G} (zeroed every call)
    double* blocksum;        // [NK][2][nblk] sum of sqrt(d2) over the side's border voxels of one 256-voxel block
    unsigned short* col;     // [NK][2][DHW]
    int* g;                  // [NK][2][DHW] in-slice g2 to border(P) / border(G)
    int* d2;                 // [NK][2][DHW] side's distances, the first cnt[vol][side] entries
};
int64_t surf_work_bytes(int64_t NK, int64_t DHW) {
    const int64_t nblk = (DHW + 255) / 256;
    return up16(NK * 6 * 4) + up16(NK * 2 * nblk * 8) + up16(NK * 2 * DHW * 2) + 2 * up16(NK * 2 * DHW * 4);
}
SurfWork surf_carve(void* work, int64_t NK, int64_t DHW) {
    const int64_t nblk = (DHW + 255) / 256;
    char* p = (char*)work;
    SurfWork w;
    w.cnt = (int*)p; p += up16(NK * 6 * 4);
    w.blocksum = (double*)p; p += up16(NK * 2 * nblk * 8);
    w.col = (unsigned short*)p; p += up16(NK * 2 * DHW * 2);
    w.g = (int*)p; p += up16(NK * 2 * DHW * 4);
    w.d2 = (int*)p;
    return w;
}

// a foreground voxel with a background 6-neighbour; a neighbour outside the volume is background
__device__ __forceinline__ bool border3d_at(const void* m, int is64, int by_class, long base, int c, long e, int z, int y, int x,
                                            int D, int H, int W) {
    if (!fg_at(m, is64, by_class, base, c, e)) return false;
    if (z == 0 || y == 0 || x == 0 || z == D - 1 || y == H - 1 || x == W - 1) return true;
    const long HW = (long)H * W;
    return !(fg_at(m, is64, by_class, base, c, e - HW) && fg_at(m, is64, by_class, base, c, e + HW) &&
             fg_at(m, is64, by_class, base, c, e - W) && fg_at(m, is64, by_class, base, c, e + W) &&
             fg_at(m, is64, by_class, base, c, e - 1) && fg_at(m, is64, by_class, base, c, e + 1));
}

// grid (ceil(DHW / 256), N * K)
__global__ __launch_bounds__(256) void border3d_kernel(const void* pred, const void* gt, int pi64, int gi64, int K, int by_class,
                                                      int D, int H, int W, unsigned short* __restrict__ col, int* __restrict__ cnt) {
    const int vol = blockIdx.y, n = vol / K, c = vol % K;
    const long HW = (long)H * W, DHW = (long)D * HW, base = by_class ? (long)n * DHW : (long)vol * DHW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    bool bp = false, bg = false;
    if (e < DHW) {
        const int z = (int)(e / HW), y = (int)((e % HW) / W), x = (int)(e % W);
        bp = border3d_at(pred, pi64, by_class, base, c, e, z, y, x, D, H, W);
        bg = border3d_at(gt, gi64, by_class, base, c, e, z, y, x, D, H, W);
        unsigned short* o = col + (long)vol * 2 * DHW;
        o[e] = bp ? 0 : COL_INF;
        o[DHW + e] = bg ? 0 : COL_INF;
    }
    // one atomicAdd per block and side, and none for a block without a border voxel
    __shared__ int wcnt[2][4];
    const int np = __popcll(__ballot(bp)), ng = __popcll(__ballot(bg));
    if ((threadIdx.x & 63) == 0) { wcnt[0][threadIdx.x >> 6] = np; wcnt[1][threadIdx.x >> 6] = ng; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int* w = wcnt[threadIdx.x];
        const int sum = w[0] + w[1] + w[2] + w[3];
        if (sum) atomicAdd(&cnt[vol * 6 + threadIdx.x], sum);
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (ceil(DHW / 256), N * K): block b of a volume takes its voxels 256 b .. 256 b + 255
__global__ __launch_bounds__(256) void surf_z_kernel(int D, long HW, int wz2, const int* __restrict__ g, int* __restrict__ cnt,
                                                    int* __restrict__ d2, double* __restrict__ blocksum) {
    __shared__ double wsum[2][4];
    const int vol = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long DHW = (long)D * HW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    int* c = cnt + vol * 6;
    if (c[0] == 0 || c[1] == 0) return;                  // an empty border: no distance exists (uniform over the volume's blocks)
    for (int side = 0; side < 2; ++side) {
        const int* mine = g + ((long)vol * 2 + side) * DHW;
        const int* other = g + ((long)vol * 2 + 1 - side) * DHW;
        const bool on = e < DHW && mine[e] == 0;         // g2 to the own border is 0 exactly on it
        int best = 0;
        double root = 0.0;
        if (on) {
            best = z_min<false>(other + e, (int)(e / HW), D, HW, wz2, other[e], false);
            root = sqrt((double)best);
        }
        const unsigned long long m = __ballot(on);
        if (m) {
            int at = 0;
            if (lane == 0) at = atomicAdd(&c[2 + side], __popcll(m));
            at = __shfl(at, 0) + __popcll(m & ((1ull << lane) - 1ull));
            if (on && at < DHW) d2[((long)vol * 2 + side) * DHW + at] = best;       // (at < DHW always: at most DHW border voxels)
        }
        int mx = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
        if (lane == 0 && mx > 0) atomicMax(&c[4 + side], mx);
        root = wave_sum_f64(root);
        if (lane == 0) wsum[side][wave] = root;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double* w = wsum[threadIdx.x];
        blocksum[((long)vol * 2 + threadIdx.x) * gridDim.x + blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
}

// The bin of `hist` (nbins = 256 * per) that holds rank `rank`, and the rank inside it: every thread adds `per` bins, thread 0
// walks the 256 partial sums.  Block-wide call; the result is in res[0..1] for every thread afterwards.
__device__ __forceinline__ void find_rank(const int* hist, int per, int rank, int* part, int* res) {
    const int t = threadIdx.x;
    int s = 0;
    for (int j = 0; j < per; ++j) s += hist[t * per + j];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int i = 0, r = rank;
        while (i < 255 && r >= part[i]) r -= part[i++];
        int b = i * per;
        const int last = b + per - 1;
        while (b < last && r >= hist[b]) r -= hist[b++];
        res[0] = b; res[1] = r;
    }
    __syncthreads();
}

// grid (N * K), 256 threads.  out record (40 bytes): int32 {|border(P)|, |border(G)|, d2[k], d2[k+1], max d2 P, max d2 G},
// f64 sum of sqrt(d2) over border(P), f64 the same over border(G)
__global__ __launch_bounds__(256) void select3d_kernel(long DHW, int nblk, const int* __restrict__ d2, const int* __restrict__ cnt,
                                                      const double* __restrict__ blocksum, int* __restrict__ out) {
    __shared__ int hist[1 << L1_BITS];
    __shared__ int hist2[2][1 << L2_BITS];
    __shared__ int part[256];
    __shared__ int res[2];
    __shared__ double wsum[2][4];
    const int vol = blockIdx.x, t = threadIdx.x;
    const int* c = cnt + vol * 6;
    const int n0 = c[0], n1 = c[1], n = n0 + n1;
    const int* l0 = d2 + (long)vol * 2 * DHW;
    const int* l1 = l0 + DHW;
    int* rec = out + (long)vol * 10;
    if (n0 == 0 || n1 == 0) {            // an empty mask: no distance exists; the host applies the reference's rules from the counts
        if (t < 10) rec[t] = t == 0 ? n0 : (t == 1 ? n1 : 0);
        return;
    }
    for (int side = 0; side < 2; ++side) {
        const double* bs = blocksum + ((long)vol * 2 + side) * nblk;
        double acc = 0.0;
        for (int b = t; b < nblk; b += 256) acc += bs[b];
        acc = wave_sum_f64(acc);
        if ((t & 63) == 0) wsum[side][t >> 6] = acc;
    }
    const int k = rank95(n), k1 = rank95_next(n);

    // level 1: the top 11 bits
    for (int i = t; i < (1 << L1_BITS); i += 256) hist[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 256) atomicAdd(&hist[digit1(i < n0 ? l0[i] : l1[i - n0])], 1);
    __syncthreads();
    find_rank(hist, (1 << L1_BITS) / 256, k, part, res);
    int pk = res[0], rk = res[1];
    __syncthreads();
    find_rank(hist, (1 << L1_BITS) / 256, k1, part, res);
    int pk1 = res[0], rk1 = res[1];
    __syncthreads();
    // levels 2 and 3: the next 10 bits among the values that share the prefix found so far
    for (int level = 2; level <= 3; ++level) {
        for (int i = t; i < (2 << L2_BITS); i += 256) (&hist2[0][0])[i] = 0;
        __syncthreads();
        for (int i = t; i < n; i += 256) {
            const int v = i < n0 ? l0[i] : l1[i - n0];
            const int pre = level == 2 ? digit1(v) : prefix2(v), dig = level == 2 ? digit2(v) : digit3(v);
            if (pre == pk) atomicAdd(&hist2[0][dig], 1);
            if (pre == pk1) atomicAdd(&hist2[1][dig], 1);
        }
        __syncthreads();
        find_rank(hist2[0], (1 << L2_BITS) / 256, rk, part, res);
        pk = (pk << L2_BITS) | res[0]; rk = res[1];
        __syncthreads();
        find_rank(hist2[1], (1 << L2_BITS) / 256, rk1, part, res);
        pk1 = (pk1 << L2_BITS) | res[0]; rk1 = res[1];
        __syncthreads();
    }
    if (t == 0) {
        rec[0] = n0; rec[1] = n1; rec[2] = pk; rec[3] = pk1; rec[4] = c[4]; rec[5] = c[5];
        double* sums = (double*)(rec + 6);
        sums[0] = ((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3];
        sums[1] = ((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3];
    }
}

// the checks every launcher shares, sizes before any pointer is used: 0, or 1 + message
int check_volume(const char* who, int N, int K, int D, int H, int W, int wz, int wy, int wx) {
    USTRUN_CHECK(sizes_ok(N, K, D, H, W), "%s: N, K > 0, N * K <= %lld and D, H, W in 1..%d, got N %d K %d D %d H %d W %d", who,
                 (long long)NK_MAX, VOL_MAX, N, K, D, H, W);
    USTRUN_CHECK(voxels_ok(D, H, W), "%s: D * H * W = %lld voxels exceed 2^27 = %lld (D %d H %d W %d)", who,
                 (long long)D * H * W, (long long)VOX_MAX, D, H, W);
    USTRUN_CHECK(weights_ok(wz, wy, wx), "%s: axis weights must be in 1..%d, got wz %d wy %d wx %d", who, WEIGHT_MAX, wz, wy, wx);
    USTRUN_CHECK(d2_fits(D, H, W, wz, wy, wx),
                 "%s: the largest squared distance wz^2 (D-1)^2 + wy^2 (H-1)^2 + wx^2 (W-1)^2 = %lld exceeds 2^31 - 2 "
                 "(D %d H %d W %d wz %d wy %d wx %d)", who, (long long)d2_bound(D, H, W, wz, wy, wx), D, H, W, wz, wy, wx);
    return 0;
}

int launch_colscan(int H, int W, int64_t maps, unsigned short* col, hipStream_t st, const char* name) {
    hipLaunchKernelGGL(colscan_fold_kernel, dim3(cdiv(W, 64), fold_blocks(maps, 1, GRID_Y_MAX)), dim3(64), 0, st, H, W, (long)maps, col);
    USTRUN_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int64_t ustrun_signed_dist2_3d_work_bytes(int N, int K, int D, int H, int W) {
    if (check_volume("signed_dist2_3d_work_bytes", N, K, D, H, W, 1, 1, 1)) return -1;
    return dist_work_bytes((int64_t)N * K, (int64_t)D * H * W);
}

extern "C" int ustrun_signed_dist2_3d(const void* mask, int mask_is_i64, int N, int K, int by_class, int D, int H, int W, int wz,
                                      int wy, int wx, void* work, int64_t work_bytes, int32_t* s2, int32_t* flags,
                                      ustrun_stream_t s) {
    USTRUN_TRY(check_volume("signed_dist2_3d", N, K, D, H, W, wz, wy, wx));
    USTRUN_CHECK(mask && work && s2 && flags, "signed_dist2_3d: null pointer (mask %p work %p s2 %p flags %p)", mask, work,
                 (void*)s2, (void*)flags);
    const int64_t NK = (int64_t)N * K, HW = (int64_t)H * W, DHW = D * HW;
    USTRUN_CHECK(work_bytes >= dist_work_bytes(NK, DHW), "signed_dist2_3d: work buffer of %lld bytes, needs %lld",
                 (long long)work_bytes, (long long)dist_work_bytes(NK, DHW));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)s2 & 3) == 0 && ((uintptr_t)flags & 3) == 0 &&
                 ((uintptr_t)mask & (mask_is_i64 ? 7 : 3)) == 0,
                 "signed_dist2_3d: work must be 16-byte, s2 and flags 4-byte aligned, mask to its element");
    const DistWork w = dist_carve(work, NK, DHW);
    const hipStream_t st = (hipStream_t)s;
    const hipError_t e = hipMemsetAsync(w.has, 0, sizeof(int) * 2 * NK, st);
    USTRUN_CHECK(e == hipSuccess, "signed_dist2_3d: memset failed: %s", hipGetErrorString(e));
    const dim3 voxels(cdiv(DHW, 256), NK);
    hipLaunchKernelGGL(seed3d_kernel, voxels, dim3(256), 0, st, mask, mask_is_i64, K, by_class, (long)DHW, w.col, w.has);
    USTRUN_LAUNCH_CHECK("signed_dist2_3d: seed");
    USTRUN_TRY(launch_colscan(H, W, NK * 2 * D, w.col, st, "signed_dist2_3d: column scan"));
    const int64_t rows = NK * D * H;
    hipLaunchKernelGGL(row_kernel<true>, dim3(fold_blocks(rows, ROWS_PER_BLOCK, GRID_X_FOLD)), dim3(256), 0, st, (long)rows, D * H, W,
                       wy * wy, wx * wx, w.col, w.g);
    USTRUN_LAUNCH_CHECK("signed_dist2_3d: row minimum");
    hipLaunchKernelGGL(signed_z_kernel, voxels, dim3(256), 0, st, D, (long)HW, wz * wz, w.g, w.has, s2, flags);
    USTRUN_LAUNCH_CHECK("signed_dist2_3d: slice minimum");
    return 0;
}

extern "C" int64_t ustrun_sdf_from_dist2_3d_work_bytes(int N, int K, int D, int H, int W) {
    if (check_volume("sdf_from_dist2_3d_work_bytes", N, K, D, H, W, 1, 1, 1)) return -1;
    return up16((int64_t)N * K * 2 * 4);
}

extern "C" int ustrun_sdf_from_dist2_3d(const int32_t* s2, const int32_t* flags, int N, int K, int D, int H, int W, void* work,
                                        int64_t work_bytes, float* sdf, ustrun_stream_t s) {
    USTRUN_TRY(check_volume("sdf_from_dist2_3d", N, K, D, H, W, 1, 1, 1));
    USTRUN_CHECK(s2 && flags && work && sdf, "sdf_from_dist2_3d: null pointer (s2 %p flags %p work %p sdf %p)", (const void*)s2,
                 (const void*)flags, work, (void*)sdf);
    const int64_t NK = (int64_t)N * K, DHW = (int64_t)D * H * W;
    USTRUN_CHECK(work_bytes >= up16(NK * 2 * 4), "sdf_from_dist2_3d: work buffer of %lld bytes, needs %lld", (long long)work_bytes,
                 (long long)up16(NK * 2 * 4));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)s2 & 3) == 0 && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)sdf & 3) == 0,
                 "sdf_from_dist2_3d: work must be 16-byte, s2, flags and sdf 4-byte aligned");
    int* mx = (int*)work;
    const hipStream_t st = (hipStream_t)s;
    const hipError_t e = hipMemsetAsync(mx, 0, sizeof(int) * 2 * NK, st);
    USTRUN_CHECK(e == hipSuccess, "sdf_from_dist2_3d: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(planemax_kernel, dim3(cdiv(DHW, MAX_PER_BLOCK), NK), dim3(256), 0, st, (long)DHW, s2, flags, mx);
    USTRUN_LAUNCH_CHECK("sdf_from_dist2_3d: volume maxima");
    hipLaunchKernelGGL(normalise_kernel, dim3(cdiv(DHW, 256), NK), dim3(256), 0, st, (long)DHW, s2, flags, mx, sdf);
    USTRUN_LAUNCH_CHECK("sdf_from_dist2_3d: normalise");
    return 0;
}

extern "C" int64_t ustrun_surface_metrics_3d_work_bytes(int N, int K, int D, int H, int W) {
    if (check_volume("surface_metrics_3d_work_bytes", N, K, D, H, W, 1, 1, 1)) return -1;
    return surf_work_bytes((int64_t)N * K, (int64_t)D * H * W);
}

extern "C" int ustrun_surface_metrics_3d(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N, int K, int by_class,
                                         int D, int H, int W, int wz, int wy, int wx, void* work, int64_t work_bytes, void* out,
                                         ustrun_stream_t s) {
    USTRUN_TRY(check_volume("surface_metrics_3d", N, K, D, H, W, wz, wy, wx));
    USTRUN_CHECK(pred && gt && work && out, "surface_metrics_3d: null pointer (pred %p gt %p work %p out %p)", pred, gt, work, out);
    const int64_t NK = (int64_t)N * K, HW = (int64_t)H * W, DHW = D * HW;
    USTRUN_CHECK(work_bytes >= surf_work_bytes(NK, DHW), "surface_metrics_3d: work buffer of %lld bytes, needs %lld",
                 (long long)work_bytes, (long long)surf_work_bytes(NK, DHW));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)pred & (pred_is_i64 ? 7 : 3)) == 0 &&
                 ((uintptr_t)gt & (gt_is_i64 ? 7 : 3)) == 0,
                 "surface_metrics_3d: work must be 16-byte and out 8-byte aligned, pred and gt to their element");
    const SurfWork w = surf_carve(work, NK, DHW);
    const hipStream_t st = (hipStream_t)s;
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(int) * 6 * NK, st);
    USTRUN_CHECK(e == hipSuccess, "surface_metrics_3d: memset failed: %s", hipGetErrorString(e));
    const dim3 voxels(cdiv(DHW, 256), NK);
    hipLaunchKernelGGL(border3d_kernel, voxels, dim3(256), 0, st, pred, gt, pred_is_i64, gt_is_i64, K, by_class, D, H, W, w.col, w.cnt);
    USTRUN_LAUNCH_CHECK("surface_metrics_3d: border");
    USTRUN_TRY(launch_colscan(H, W, NK * 2 * D, w.col, st, "surface_metrics_3d: column scan"));
    const int64_t rows = NK * D * H;
    hipLaunchKernelGGL(row_kernel<false>, dim3(fold_blocks(rows, ROWS_PER_BLOCK, GRID_X_FOLD)), dim3(256), 0, st, (long)rows, D * H, W,
                       wy * wy, wx * wx, w.col, w.g);
    USTRUN_LAUNCH_CHECK("surface_metrics_3d: row minimum");
    hipLaunchKernelGGL(surf_z_kernel, voxels, dim3(256), 0, st, D, (long)HW, wz * wz, w.g, w.cnt, w.d2, w.blocksum);
    USTRUN_LAUNCH_CHECK("surface_metrics_3d: slice minimum");
    hipLaunchKernelGGL(select3d_kernel, dim3(NK), dim3(256), 0, st, (long)DHW, (int)voxels.x, w.d2, w.cnt, w.blocksum, (int*)out);
    USTRUN_LAUNCH_CHECK("surface_metrics_3d: select");
    return 0;
}
