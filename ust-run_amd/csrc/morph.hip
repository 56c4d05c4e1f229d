// Chamfer distances and binary morphology of label planes [H][W] and volumes [D][H][W] on the device (include/ustrun.h:
// ustrun_chamfer_dist, ustrun_morph): what the reference's GetBoundary (dataloaders/custom_transforms.py:630-647) takes from
// scipy.ndimage.binary_dilation / binary_erosion with `iterations`, scipy's binary_opening / binary_closing, and
// scipy.ndimage.distance_transform_cdt -- all thresholds or plain values of ONE quantity, the exact integer distance to a set
// under the city-block (L1: the cross) or the chessboard (L-inf: the full structure) metric:
//
//   dilation(A, w)  =  d(p, A) <= w          erosion(A, w)  =  d(p, ~A) > w          band = dilation & ~erosion
//
// with the outside of the box part of A (border_value 1) resp. of ~A (border_value 0) -- DESIGN 31 has the identities.
//
// Both metrics are separable: one 1-D operator per axis, applied in turn to v = 0 on the set, CAP_INF elsewhere (morph_plan.h):
//   L1    v'(i) = min over i' of v(i') + |i - i'|          a forward and a backward recurrence d = min(v, d + 1)
//   L-inf v'(i) = min over i' of max(v(i'), |i - i'|)       a search outwards from i (linf_at)
// "The outside is a source" is a 0 one step before index 0 and past the last index (L1) or the candidates i + 1, n - i (L-inf).
// Two u16 maps per volume, kind 0 = distance to the foreground, kind 1 = to the background; only the wanted kinds are computed.
//
//   1 rowseed   one wave per row (z, y), 4 rows a block, rows a folded 1-D list.  The seed is binary, so along x both operators
//               are the distance to the nearest set pixel of the row: one ballot per 64-pixel chunk and kind, kept in LDS; a lane
//               finds its neighbours in its chunk's mask with clz / ctz and takes the chunk carry (nearest set pixel of an earlier
//               / a later chunk, or the outside) where its own chunk has none.  Reads the mask once, coalesced; writes u16.
//               Whether the volume has a pixel of each kind goes to two flag words (integer atomicOr, skipped once set).
//   2 mid       rank 3 only, along y: one thread per column of a slice, lanes on consecutive x (coalesced), slices a folded list.
//               L1 in place; L-inf from buffer A to buffer B (its search reads what an in-place pass would overwrite).
//   3 last      along y (rank 2) or z (rank 3): one thread per line, lanes on consecutive x resp. (y, x).  L1: forward in place,
//               then the backward recurrence hands each finished distance to the emit; L-inf: the search per entry.  The emit
//               writes the signed int32 distance and the flags (chamfer) or the thresholded byte (morph): no full-size distance
//               map of the morphology entry ever goes to memory.  reduce_parts: the thread walks the K parts of its image and
//               ORs into the byte it wrote itself -- no atomics, no other thread touches that byte.
// Opening and closing are two rounds of 1-3 through a u8 intermediate in `work`.
//
// Work per pixel.  Passes 1 and the L1 recurrences: O(1).  The L-inf search at entry i takes at most min(v(i), cap, outside
// candidates) steps of two reads, v(i) being the entry's own value before the pass -- it never walks past its own result's
// upper bound.  ustrun_morph clips every intermediate at cap = width + 1, so its search is at most `width` steps; for
// ustrun_chamfer_dist cap = CAP_INF and the bound is the distance itself (<= the axis length).  A kind without any source (empty
// plane, no outside) is known from the flag words and skips the search.
//
// Everything is integers; no block waits for another; nothing is allocated; two runs give equal bits.
#include "common.h"
#include "edt_scan.h"        // COL_INF, fg_at
#include "morph_plan.h"

namespace ustrun {
namespace {

using namespace morph;

static_assert(CAP_INF == COL_INF, "morph_plan.h names edt_scan.h's infinite column entry");
static_assert(WIDTH_MAX + 1 <= CAP_INF && DIST_MAX < CAP_INF, "u16 intermediates hold every clipped distance");
constexpr int ROWS_PER_BLOCK = 4;
constexpr int FMT_F32 = 0, FMT_I64 = 1, FMT_U8 = 2;      // how the mask is stored; u8: the intermediate of opening / closing

static inline int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

__device__ __forceinline__ bool set_at(const void* m, int fmt, int by_class, long base, int c, long e) {
    if (fmt == FMT_U8) return ((const unsigned char*)m)[base + e] != 0;
    return fg_at(m, fmt, by_class, base, c, e);
}

struct Geo {
    int K, D, H, W, rank;
    long NK, DHW;
};

// ---- pass 1.  grid (fold_blocks(rows, 4, GRID_X_FOLD)), 256 threads; wave w of block b takes the rows 4 (b + i gridDim.x) + w.
// Row r = (vol * D + z) * H + y lies at offset (r mod D H) W of its volume; buf[vol][kind][D H W]
__global__ __launch_bounds__(256) void rowseed_kernel(const void* mask, int fmt, int K, int by_class, long rows, int DH, int W,
                                                     int kinds, int outside, int cap, unsigned short* __restrict__ buf,
                                                     int* __restrict__ has) {
    __shared__ unsigned long long masks[ROWS_PER_BLOCK][2][ROW_CHUNKS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nch = (W + 63) >> 6;
    const long DHW = (long)DH * W;
    for (long r0 = (long)blockIdx.x * ROWS_PER_BLOCK; r0 < rows; r0 += (long)gridDim.x * ROWS_PER_BLOCK) {
        const long r = r0 + wave;                        // uniform per wave
        const long vol = r / DH, off = (r % DH) * W;
        if (r < rows) {
            const int n = (int)(vol / K), c = (int)(vol % K);
            const long base = by_class ? (long)n * DHW : vol * DHW;
            bool any_fg = false, any_bg = false;
            for (int j = 0; j < nch; ++j) {
                const int x = j * 64 + lane;
                const bool in = x < W;
                const bool fg = in && set_at(mask, fmt, by_class, base, c, off + x);
                const unsigned long long mf = __ballot(fg), mb = __ballot(in && !fg);
                if (lane == 0) { masks[wave][0][j] = mf; masks[wave][1][j] = mb; }
                any_fg |= mf != 0;
                any_bg |= mb != 0;
            }
            if (lane == 0) {                             // a mark already set costs a read, not an atomic
                volatile int* seen = has + vol * 2;
                if (any_fg && seen[0] == 0) atomicOr(&has[vol * 2], 1);
                if (any_bg && seen[1] == 0) atomicOr(&has[vol * 2 + 1], 1);
            }
        }
        wave_lds_sync();                                 // each wave reads only the masks it wrote
        if (r < rows)
            for (int kind = 0; kind < 2; ++kind) {
                if (!((kinds >> kind) & 1)) continue;
                const unsigned long long* m = masks[wave][kind];
                const bool out = outside_is(outside, kind);
                unsigned short* o = buf + (vol * 2 + kind) * DHW + off;
                for (int j = 0; j < nch; ++j) {
                    const int x = j * 64 + lane;
                    const int left = chunk_carry_left(m, j, out), right = chunk_carry_right(m, j, nch, W, out);
                    if (x < W) o[x] = (unsigned short)row_dist(m[j], lane, x, left, right, cap);
                }
            }
        wave_lds_sync();
    }
}

// ---- the L1 recurrences along one line of n entries `stride` apart, in place, 8 entries loaded ahead of the dependent chain
__device__ __forceinline__ void l1_forward(int n, long stride, unsigned short* p, int start, int cap) {
    int d = start;
    for (int i0 = 0; i0 < n; i0 += 8) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i0 + j < n ? p[(long)(i0 + j) * stride] : cap;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d = l1_step(d, v[j], cap);
            if (i0 + j < n) p[(long)(i0 + j) * stride] = (unsigned short)d;
        }
    }
}
__device__ __forceinline__ void l1_backward(int n, long stride, unsigned short* p, int start, int cap) {
    int d = start;
    for (int i0 = n - 1; i0 >= 0; i0 -= 8) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i0 - j >= 0 ? p[(long)(i0 - j) * stride] : cap;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d = l1_step(d, v[j], cap);
            if (i0 - j >= 0) p[(long)(i0 - j) * stride] = (unsigned short)d;
        }
    }
}

// ---- pass 2 (rank 3), along y.  grid (ceil(W / 64), min(maps, 65535)), 64 threads; maps = N K D slices, each with two kinds.
// L1: a in place.  L-inf: a -> b
template <int METRIC>
__global__ __launch_bounds__(64) void mid_kernel(int D, int H, int W, long maps, int kinds, int outside, int cap,
                                                unsigned short* __restrict__ a, unsigned short* __restrict__ b,
                                                const int* __restrict__ has) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const long HW = (long)H * W;
    for (long mp = blockIdx.y; mp < maps; mp += gridDim.y) {
        const long vol = mp / D, z = mp % D;
        for (int kind = 0; kind < 2; ++kind) {
            if (!((kinds >> kind) & 1)) continue;
            const bool out = outside_is(outside, kind);
            const long at = ((vol * 2 + kind) * D + z) * HW + x;
            if (METRIC == METRIC_L1) {
                l1_forward(H, W, a + at, l1_start(out, cap), cap);
                l1_backward(H, W, a + at, l1_start(out, cap), cap);
            } else {
                const bool live = out || has[vol * 2 + kind] != 0;
                for (int y = 0; y < H; ++y) b[at + (long)y * W] = (unsigned short)(live ? linf_at(a + at, W, y, H, cap, out) : cap);
            }
        }
    }
}

// ---- pass 3 and the emit
struct Emit {
    int morph;               // 0: signed distances + flags, 1: the thresholded byte
    int op, width, parts;    // parts: K when the K parts of an image are ORed into one plane, else 1
    unsigned char* out8;     // [units][DHW]
    int* sd;                 // [units][DHW]
    int* flags;              // [units]
};

__device__ __forceinline__ void emit_at(const Emit& e, long at, int c, int d0, int d1) {
    if (e.morph) {
        int bit = morph_bit(e.op, d0, d1, e.width);
        if (c > 0) bit |= e.out8[at];                    // this thread's own earlier store
        e.out8[at] = (unsigned char)bit;
    } else {
        e.sd[at] = signed_of(d0, d1, USTRUN_DIST_NONE);
    }
}

// grid (ceil(lines / 64), min(units, 65535)), 64 threads: one wave a block, so that a batch of planes (W lines each) still
// spreads over the CUs.  unit = a volume, or an image whose e.parts volumes are reduced; line q of a volume holds the entries
// q + i stride, i < n.  src[vol][kind][DHW]
template <int METRIC>
__global__ __launch_bounds__(64) void last_kernel(int n, long stride, long lines, long DHW, long units, int kinds, int outside,
                                                  int cap, unsigned short* __restrict__ src, const int* __restrict__ has, Emit e) {
    const long q = (long)blockIdx.x * 64 + threadIdx.x;
    if (q >= lines) return;
    const bool out0 = outside_is(outside, 0), out1 = outside_is(outside, 1);
    const bool k0 = kinds & KIND_FG, k1 = kinds & KIND_BG;
    for (long unit = blockIdx.y; unit < units; unit += gridDim.y)
        for (int c = 0; c < e.parts; ++c) {
            const long vol = unit * e.parts + c;
            unsigned short* p0 = src + vol * 2 * DHW + q;
            unsigned short* p1 = p0 + DHW;
            const long o = unit * DHW + q;
            if (!e.morph && q == 0) {
                const bool has_fg = has[vol * 2] != 0, has_bg = has[vol * 2 + 1] != 0;
                e.flags[vol] = has_fg ? (has_bg ? 1 : 2) : 0;
            }
            if (METRIC == METRIC_L1) {
                if (k0) l1_forward(n, stride, p0, l1_start(out0, cap), cap);
                if (k1) l1_forward(n, stride, p1, l1_start(out1, cap), cap);
                int d0 = l1_start(out0, cap), d1 = l1_start(out1, cap);
                for (int i0 = n - 1; i0 >= 0; i0 -= 8) {
                    int v0[8], v1[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const bool in = i0 - j >= 0;
                        v0[j] = in && k0 ? p0[(long)(i0 - j) * stride] : cap;
                        v1[j] = in && k1 ? p1[(long)(i0 - j) * stride] : cap;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        d0 = l1_step(d0, v0[j], cap);
                        d1 = l1_step(d1, v1[j], cap);
                        if (i0 - j >= 0) emit_at(e, o + (long)(i0 - j) * stride, c, d0, d1);
                    }
                }
            } else {
                const bool live0 = k0 && (out0 || has[vol * 2] != 0), live1 = k1 && (out1 || has[vol * 2 + 1] != 0);
                for (int i = 0; i < n; ++i) {
                    const int d0 = live0 ? linf_at(p0, stride, i, n, cap, out0) : cap;
                    const int d1 = live1 ? linf_at(p1, stride, i, n, cap, out1) : cap;
                    emit_at(e, o + (long)i * stride, c, d0, d1);
                }
            }
        }
}

// ---- the work buffer: the flag words, buffer A, buffer B (rank 3: the L-inf pass along y cannot run in place), and for opening
// and closing the u8 result of the first round
struct Work {
    int* has;                // [NK][2]   (zeroed every round)
    unsigned short* a;       // [NK][2][DHW]
    unsigned short* b;       // [NK][2][DHW], rank 3
    unsigned char* tmp;      // [NK][DHW], two-round ops
};
int64_t work_bytes_of(int64_t NK, int64_t DHW, int rank, bool two_rounds) {
    return up16(NK * 2 * 4) + up16(NK * 2 * DHW * 2) * (rank == 3 ? 2 : 1) + (two_rounds ? up16(NK * DHW) : 0);
}
Work carve(void* work, int64_t NK, int64_t DHW, int rank) {
    char* p = (char*)work;
    Work w;
    w.has = (int*)p; p += up16(NK * 2 * 4);
    w.a = (unsigned short*)p; p += up16(NK * 2 * DHW * 2);
    w.b = w.a;
    if (rank == 3) { w.b = (unsigned short*)p; p += up16(NK * 2 * DHW * 2); }
    w.tmp = (unsigned char*)p;
    return w;
}

// the checks both entries share, sizes before any pointer is used: 0, or 1 + message
int check_box(const char* who, int N, int K, int rank, int D, int H, int W) {
    USTRUN_CHECK(rank == 2 || rank == 3, "%s: rank must be 2 or 3, got %d", who, rank);
    USTRUN_CHECK(rank_ok(rank, D), "%s: rank 2 takes planes, D must be 1, got %d", who, D);
    USTRUN_CHECK(sizes_ok(N, K, D, H, W), "%s: N, K > 0, N * K <= %lld and D, H, W in 1..%d, got N %d K %d D %d H %d W %d", who,
                 (long long)NK_MAX, AXIS_MAX, N, K, D, H, W);
    USTRUN_CHECK(voxels_ok(D, H, W), "%s: D * H * W = %lld voxels exceed 2^27 = %lld (D %d H %d W %d)", who, (long long)D * H * W,
                 (long long)VOX_MAX, D, H, W);
    return 0;
}

// one round of the three passes over mask -> emit
int run_round(const char* who, const void* mask, int fmt, int by_class, const Geo& g, int metric, int kinds, int outside, int cap,
              const Work& w, const Emit& e, hipStream_t st) {
    const hipError_t err = hipMemsetAsync(w.has, 0, sizeof(int) * 2 * g.NK, st);
    USTRUN_CHECK(err == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(err));
    const int64_t rows = g.NK * g.D * g.H;
    hipLaunchKernelGGL(rowseed_kernel, dim3(fold_blocks(rows, ROWS_PER_BLOCK, GRID_X_FOLD)), dim3(256), 0, st, mask, fmt, g.K, by_class,
                       (long)rows, g.D * g.H, g.W, kinds, outside, cap, w.a, w.has);
    USTRUN_LAUNCH_CHECK("morph: row pass");
    unsigned short* src = w.a;
    if (g.rank == 3) {
        const int64_t maps = g.NK * g.D;
        const dim3 grid(cdiv(g.W, 64), fold_blocks(maps, 1, GRID_Y_MAX));
        if (metric == METRIC_L1) {
            hipLaunchKernelGGL(mid_kernel<METRIC_L1>, grid, dim3(64), 0, st, g.D, g.H, g.W, (long)maps, kinds, outside, cap, w.a, w.b, w.has);
        } else {
            hipLaunchKernelGGL(mid_kernel<METRIC_LINF>, grid, dim3(64), 0, st, g.D, g.H, g.W, (long)maps, kinds, outside, cap, w.a, w.b, w.has);
            src = w.b;
        }
        USTRUN_LAUNCH_CHECK("morph: column pass");
    }
    const int n = last_len(g.rank, g.D, g.H);
    const int64_t stride = last_stride(g.rank, g.H, g.W), lines = stride, units = g.NK / e.parts;
    const dim3 grid(cdiv(lines, 64), fold_blocks(units, 1, GRID_Y_MAX));
    if (metric == METRIC_L1)
        hipLaunchKernelGGL(last_kernel<METRIC_L1>, grid, dim3(64), 0, st, n, (long)stride, (long)lines, g.DHW, (long)units, kinds, outside, cap, src, w.has, e);
    else
        hipLaunchKernelGGL(last_kernel<METRIC_LINF>, grid, dim3(64), 0, st, n, (long)stride, (long)lines, g.DHW, (long)units, kinds, outside, cap, src, w.has, e);
    USTRUN_LAUNCH_CHECK("morph: last pass");
    return 0;
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int64_t ustrun_chamfer_dist_work_bytes(int N, int K, int rank, int D, int H, int W) {
    if (check_box("chamfer_dist_work_bytes", N, K, rank, D, H, W)) return -1;
    return work_bytes_of((int64_t)N * K, (int64_t)D * H * W, rank, false);
}

extern "C" int ustrun_chamfer_dist(const void* mask, int mask_is_i64, int N, int K, int by_class, int rank, int D, int H, int W,
                                   int metric, int outside, void* work, int64_t work_bytes, int32_t* sd, int32_t* flags,
                                   ustrun_stream_t s) {
    USTRUN_TRY(check_box("chamfer_dist", N, K, rank, D, H, W));
    USTRUN_CHECK(metric_ok(metric), "chamfer_dist: metric must be 0 (city-block) or 1 (chessboard), got %d", metric);
    USTRUN_CHECK(outside_ok(outside), "chamfer_dist: outside must be 0 (neither kind), 1 (background) or 2 (foreground), got %d", outside);
    USTRUN_CHECK(mask && work && sd && flags, "chamfer_dist: null pointer (mask %p work %p sd %p flags %p)", mask, work, (void*)sd,
                 (void*)flags);
    Geo g{K, D, H, W, rank, (long)N * K, (long)D * H * W};
    const int64_t need = work_bytes_of(g.NK, g.DHW, rank, false);
    USTRUN_CHECK(work_bytes >= need, "chamfer_dist: work buffer of %lld bytes, needs %lld", (long long)work_bytes, (long long)need);
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)sd & 3) == 0 && ((uintptr_t)flags & 3) == 0 &&
                 ((uintptr_t)mask & (mask_is_i64 ? 7 : 3)) == 0,
                 "chamfer_dist: work must be 16-byte, sd and flags 4-byte aligned, mask to its element");
    const Work w = carve(work, g.NK, g.DHW, rank);
    Emit e{0, 0, 0, 1, nullptr, sd, flags};
    return run_round("chamfer_dist", mask, mask_is_i64 ? FMT_I64 : FMT_F32, by_class ? 1 : 0, g, metric, KIND_FG | KIND_BG, outside, CAP_INF,
                     w, e, (hipStream_t)s);
}

extern "C" int64_t ustrun_morph_work_bytes(int N, int K, int rank, int D, int H, int W, int op) {
    if (check_box("morph_work_bytes", N, K, rank, D, H, W)) return -1;
    if (!op_ok(op)) {
        set_error("morph_work_bytes: op must be 0 (dilation), 1 (erosion), 2 (opening), 3 (closing) or 4 (band), got %d", op);
        return -1;
    }
    return work_bytes_of((int64_t)N * K, (int64_t)D * H * W, rank, second_round(op) >= 0);
}

extern "C" int ustrun_morph(const void* mask, int mask_is_i64, int N, int K, int by_class, int rank, int D, int H, int W, int metric,
                            int op, int width, int border_value, int reduce_parts, void* work, int64_t work_bytes, uint8_t* out,
                            ustrun_stream_t s) {
    USTRUN_TRY(check_box("morph", N, K, rank, D, H, W));
    USTRUN_CHECK(metric_ok(metric), "morph: metric must be 0 (city-block: the cross) or 1 (chessboard: the full structure), got %d", metric);
    USTRUN_CHECK(op_ok(op), "morph: op must be 0 (dilation), 1 (erosion), 2 (opening), 3 (closing) or 4 (band), got %d", op);
    USTRUN_CHECK(width_ok(width), "morph: width (iterations) must be in 1..%d, got %d (iterating until nothing changes is not built)",
                 WIDTH_MAX, width);
    USTRUN_CHECK(border_ok(border_value), "morph: border_value must be 0 or 1, got %d", border_value);
    USTRUN_CHECK(mask && work && out, "morph: null pointer (mask %p work %p out %p)", mask, work, (void*)out);
    Geo g{K, D, H, W, rank, (long)N * K, (long)D * H * W};
    const bool two = second_round(op) >= 0;
    const int64_t need = work_bytes_of(g.NK, g.DHW, rank, two);
    USTRUN_CHECK(work_bytes >= need, "morph: work buffer of %lld bytes, needs %lld", (long long)work_bytes, (long long)need);
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)mask & (mask_is_i64 ? 7 : 3)) == 0,
                 "morph: work must be 16-byte aligned, mask to its element");
    const Work w = carve(work, g.NK, g.DHW, rank);
    const hipStream_t st = (hipStream_t)s;
    const int outside = outside_of_border(border_value), cap = morph_cap(width), parts = reduce_parts ? K : 1;
    const int fmt = mask_is_i64 ? FMT_I64 : FMT_F32;
    if (!two) {
        Emit e{1, op, width, parts, out, nullptr, nullptr};
        return run_round("morph", mask, fmt, by_class ? 1 : 0, g, metric, kinds_of(op), outside, cap, w, e, st);
    }
    Emit e1{1, first_round(op), width, 1, w.tmp, nullptr, nullptr};
    USTRUN_TRY(run_round("morph", mask, fmt, by_class ? 1 : 0, g, metric, kinds_of(e1.op), outside, cap, w, e1, st));
    Emit e2{1, second_round(op), width, parts, out, nullptr, nullptr};
    return run_round("morph", w.tmp, FMT_U8, 0, g, metric, kinds_of(e2.op), outside, cap, w, e2, st);
}
