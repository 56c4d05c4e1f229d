// What host and device share of the chamfer-distance / binary-morphology kernels (morph.hip): the limits and codes, how a long
// list of rows or maps is folded onto a grid, and the integer arithmetic of the three passes -- the row pass with its chunk
// carry, the city-block (L1) recurrence and the chessboard (L-inf) search, each with the candidates the outside of the box adds.
// No HIP type is named here, so tests/host/morph_plan_check.hip replays every function on the CPU, in the kernels' pass order,
// against a brute force over small boxes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MORPH_HD __host__ __device__ inline
#else
#define MORPH_HD inline
#endif

namespace ustrun {
namespace morph {

constexpr int AXIS_MAX = 1024;                       // D, H, W limit
constexpr int64_t VOX_MAX = (int64_t)1 << 27;        // D * H * W limit
constexpr int64_t NK_MAX = 32767;
constexpr int WIDTH_MAX = 4095;                      // iterations: the cap width + 1 still fits the u16 intermediates' 4096
constexpr int DIST_MAX = 3 * (AXIS_MAX - 1);         // 3069: the largest distance between two voxels of a legal box (L1, rank 3)
constexpr int CAP_INF = 4096;                        // edt_scan.h's COL_INF: "no source"; > DIST_MAX, so no finite distance reaches it
constexpr int GRID_Y_MAX = 65535;
constexpr int GRID_X_FOLD = 1 << 20;                 // blocks of a folded 1-D grid: the rest of the list is walked in a loop
constexpr int ROW_CHUNKS = AXIS_MAX / 64;            // 64-pixel chunks of the longest row

enum { METRIC_L1 = 0, METRIC_LINF = 1 };
enum { OP_DILATE = 0, OP_ERODE = 1, OP_OPEN = 2, OP_CLOSE = 3, OP_BAND = 4 };
enum { OUTSIDE_NONE = 0, OUTSIDE_BG = 1, OUTSIDE_FG = 2 };
enum { KIND_FG = 1, KIND_BG = 2 };                   // bit k: the distance to kind k (0 foreground, 1 background) is wanted

// ---- the limits
MORPH_HD bool rank_ok(int rank, int D) { return rank == 3 || (rank == 2 && D == 1); }
MORPH_HD bool sizes_ok(int N, int K, int D, int H, int W) {
    return N > 0 && K > 0 && D >= 1 && H >= 1 && W >= 1 && D <= AXIS_MAX && H <= AXIS_MAX && W <= AXIS_MAX &&
           (int64_t)N * K <= NK_MAX;
}
MORPH_HD bool voxels_ok(int D, int H, int W) { return (int64_t)D * H * W <= VOX_MAX; }
MORPH_HD bool metric_ok(int metric) { return metric == METRIC_L1 || metric == METRIC_LINF; }
MORPH_HD bool outside_ok(int outside) { return outside >= OUTSIDE_NONE && outside <= OUTSIDE_FG; }
MORPH_HD bool op_ok(int op) { return op >= OP_DILATE && op <= OP_BAND; }
MORPH_HD bool width_ok(int width) { return width >= 1 && width <= WIDTH_MAX; }
MORPH_HD bool border_ok(int b) { return b == 0 || b == 1; }

// a threshold at `width` only asks whether a distance is <= width: every intermediate is clipped at width + 1 (<= CAP_INF)
MORPH_HD int morph_cap(int width) { return width + 1; }
// scipy's border_value: 0 = the outside is background, 1 = the outside is foreground
MORPH_HD int outside_of_border(int border_value) { return border_value ? OUTSIDE_FG : OUTSIDE_BG; }
// is the outside of the box a source of kind k (0 foreground, 1 background)?
MORPH_HD bool outside_is(int outside, int kind) { return outside == (kind ? OUTSIDE_BG : OUTSIDE_FG); }
// the distances one round of an op thresholds; opening and closing are two rounds: (erode, dilate) resp. (dilate, erode)
MORPH_HD int kinds_of(int op) { return op == OP_DILATE ? KIND_FG : (op == OP_ERODE ? KIND_BG : (KIND_FG | KIND_BG)); }
MORPH_HD int first_round(int op) { return op == OP_OPEN ? OP_ERODE : (op == OP_CLOSE ? OP_DILATE : op); }
MORPH_HD int second_round(int op) { return op == OP_OPEN ? OP_DILATE : (op == OP_CLOSE ? OP_ERODE : -1); }
// the thresholded byte: d0 = clipped distance to the foreground, d1 = to the background (an unwanted one is not read)
MORPH_HD int morph_bit(int op, int d0, int d1, int width) {
    const int dil = d0 <= width, ero = d1 > width;
    return op == OP_DILATE ? dil : (op == OP_ERODE ? ero : (dil & !ero));
}
// the signed chamfer distance from the two unclipped distances (CAP_INF: no source); none = USTRUN_DIST_NONE
MORPH_HD int signed_of(int d0, int d1, int none) {
    return d0 == 0 ? -(d1 >= CAP_INF ? none : d1) : (d0 >= CAP_INF ? none : d0);
}

// ---- the grid folding (edt3d_plan.h's rule): `items` (>= 1) walked `per` to a block by at most `cap` blocks; block b takes the
// groups b, b + blocks, b + 2 blocks, ...
MORPH_HD int fold_blocks(int64_t items, int per, int cap) {
    const int64_t groups = (items + per - 1) / per;
    return (int)(groups < cap ? groups : cap);
}
// the last axis: y (rank 2) or z (rank 3).  Line q of a volume holds the entries q + i * last_stride, i < last_len; a volume has
// last_stride lines (W columns resp. H W pillars)
MORPH_HD int last_len(int rank, int D, int H) { return rank == 3 ? D : H; }
MORPH_HD int64_t last_stride(int rank, int H, int W) { return rank == 3 ? (int64_t)H * W : W; }

MORPH_HD int imin(int a, int b) { return a < b ? a : b; }

// ---- pass 1, along x.  The seed is 0 on the set and CAP_INF elsewhere, so BOTH operators are the distance along the row to the
// nearest pixel of the set.  A row is up to 16 chunks of 64 pixels; masks[j] has bit l set where pixel 64 j + l is of the set
// (bits at and past W are clear).  The carry of chunk j is the position of the nearest set pixel in an earlier resp. a later
// chunk: with the outside a source that is position -1 resp. W, without any it is a position too far to matter.
constexpr int POS_FAR = 1 << 20;
MORPH_HD int chunk_carry_left(const unsigned long long* masks, int j, bool outside) {
    for (int jj = j - 1; jj >= 0; --jj)
        if (masks[jj]) return jj * 64 + 63 - __builtin_clzll(masks[jj]);
    return outside ? -1 : -POS_FAR;
}
MORPH_HD int chunk_carry_right(const unsigned long long* masks, int j, int nchunks, int W, bool outside) {
    for (int jj = j + 1; jj < nchunks; ++jj)
        if (masks[jj]) return jj * 64 + __builtin_ctzll(masks[jj]);
    return outside ? W : POS_FAR;
}
// pixel x = 64 j + lane of a chunk with mask `m`: the distance to the nearest set pixel of the row, clipped at cap
MORPH_HD int row_dist(unsigned long long m, int lane, int x, int left, int right, int cap) {
    const unsigned long long lo = m & (~0ull >> (63 - lane)), hi = m >> lane;
    const int pl = lo ? x - lane + 63 - __builtin_clzll(lo) : left;
    const int pr = hi ? x + __builtin_ctzll(hi) : right;
    return imin(imin(x - pl, pr - x), cap);
}

// ---- the L1 operator v'(i) = min over i' of v(i') + |i - i'|: a forward and a backward recurrence d = l1_step(d, v) from
// d = l1_start, the backward one over the forward one's results.  The outside as a source is a 0 one step before index 0 and one
// step past the last index; no outside is the cap there
MORPH_HD int l1_start(bool outside, int cap) { return outside ? 0 : cap; }
MORPH_HD int l1_step(int d, int v, int cap) { return imin(v, imin(d + 1, cap)); }

// ---- the L-inf operator v'(i) = min over i' of max(v(i'), |i - i'|) at entry i of a line of n entries `stride` apart: the first
// r >= 0 with min over |i - i'| <= r of v(i') <= r, searched outwards.  The running minimum starts at v(i), so the search ends
// after at most min(v(i), cap, the outside candidates i + 1 and n - i) steps, two reads each.  The reads of LINF_AHEAD radii are
// issued together, ahead of the dependent chain of minima and tests (as the scans load 8 entries ahead): up to LINF_AHEAD - 1
// radii past the stopping one are read in vain, all inside the line.
constexpr int LINF_AHEAD = 4;
MORPH_HD int linf_at(const unsigned short* p, int64_t stride, int i, int n, int cap, bool outside) {
    const int bound = outside ? imin(cap, imin(i + 1, n - i)) : cap;         // >= 1
    int m = p[(int64_t)i * stride];
    if (m == 0) return 0;
    const int reach = i > n - 1 - i ? i : n - 1 - i;                         // the farthest entry of the line
    for (int r0 = 1; r0 < bound && r0 <= reach; r0 += LINF_AHEAD) {
        int lo[LINF_AHEAD], hi[LINF_AHEAD];
        for (int j = 0; j < LINF_AHEAD; ++j) {
            const int r = r0 + j;
            lo[j] = i - r >= 0 ? p[(int64_t)(i - r) * stride] : CAP_INF;
            hi[j] = i + r < n ? p[(int64_t)(i + r) * stride] : CAP_INF;
        }
        for (int j = 0; j < LINF_AHEAD; ++j) {
            const int r = r0 + j;
            if (r >= bound) return bound;
            m = imin(m, imin(lo[j], hi[j]));
            if (m <= r) return r;
        }
    }
    return imin(bound, m);                  // the whole line has been seen, or every radius below the bound: m > each radius tried
}

}  // namespace morph
}  // namespace ustrun
