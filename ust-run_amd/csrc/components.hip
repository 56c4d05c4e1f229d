// Post-processing of a binary prediction on the device (include/ustrun.h: ustrun_post_process): the reference's
// dataloaders/utils.py:193-204 `post_processing` per (sample, part) plane -- fill the holes, label the 8-connected components,
// delete every component smaller than a share of the foreground -- over all N x K planes of a batch at once, integer-exact.
//
//   holes  = background pixels not 4-connected through background to the image border (binary_fill_holes, default structure)
//   F      = P | holes;   total = |F|
//   out    = F without the 8-connected components c with share_den * |c| < share_num * total
//
// Connected components by label equivalence (components.h): a forest over the plane's pixels, pixel e = node e + 1, node 0 the
// virtual outside.  Launches on the stream, each one finished before the next starts -- no block ever waits for another:
//   1 local_kernel<0>  one block per 16 x 64 tile: the BACKGROUND's 4-connected components of the tile, merged in LDS (a wave holds
//                      one tile row: its horizontal runs come from one ballot, unions only join runs of adjacent rows); every
//                      pixel's parent = its tile component's smallest node, or node 0 when that component touches the image border
//   2 merge_kernel     one thread per neighbour pair across a tile edge: unite (atomic minimum on the larger root), unless the
//                      pair beside it joins the same two tile components (components.h: pair_redundant)
//   3 local_kernel<1>  F = foreground | background whose root in forest 1 is not node 0 -> out; F's 8-connected tile components
//                      in LDS as in 1 -> forest 2, each tile component's pixel count at its smallest node, |F| per plane (one
//                      atomic add per block)
//   4 merge_kernel     forest 2, 8 neighbours
//   5 flatten_kernel   every node points at its root; the tile components' counts are added up at the roots (one integer atomic
//                      per tile component, none per pixel)
//   6 filter_kernel    out = 0 where the root's count is below the share
// fill_holes = 0 drops 1-2, share_num = 0 drops the labelling of 3 and 4-6.  Integer atomics only (minimum, add): the forest's
// roots are the components' smallest nodes and the counts are exact, whatever the order -- equal bits on every run.
#include "components_dev.h"            // Shared, Local, fg_at

namespace ustrun {
namespace {

constexpr int PP_MAX = 1024;             // H, W limit, as ustrun_surface_metrics has it

struct PostWork {
    int* hole;       // [NK][HW + 1]  forest 1: background, 4 neighbours, node 0 = outside
    int* comp;       // [NK][HW + 1]  forest 2: F, 8 neighbours
    int* size;       // [NK][HW + 1]  pixels of the tile component at its smallest node, after flatten of the component at its root
    int* total;      // [NK]          |F|  (zeroed every call)
};

static inline int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }
static inline int64_t forest_bytes(int64_t NK, int64_t H, int64_t W) { return up16(NK * (H * W + 1) * 4); }
int64_t post_work_bytes(int64_t NK, int64_t H, int64_t W) { return 3 * forest_bytes(NK, H, W) + up16(NK * 4); }

PostWork post_carve(void* work, int64_t NK, int64_t H, int64_t W) {
    char* p = (char*)work;
    PostWork w;
    w.hole = (int*)p; p += forest_bytes(NK, H, W);
    w.comp = (int*)p; p += forest_bytes(NK, H, W);
    w.size = (int*)p; p += forest_bytes(NK, H, W);
    w.total = (int*)p;
    return w;
}

// grid (tiles, N * K), 256 threads: wave w takes the tile's rows w, w + 4, w + 8, w + 12.
// PASS 0: members = background, 4 neighbours -> forest `dst` with the outside root.  PASS 1: members = F (`holes`: forest 1 after
// its merge, or null = no filling), written to `out`; label = 0 stops there, else 8 neighbours -> forest `dst`, counts, totals.
template <int PASS>
__global__ __launch_bounds__(256) void local_kernel(const void* pred, int is64, int K, int by_class, int H, int W,
                                                   const int* __restrict__ holes, int label, int* __restrict__ dst,
                                                   int* __restrict__ size, int* __restrict__ total, float* __restrict__ out) {
    __shared__ int lab[cc::TILE_PIX];
    __shared__ int cnt[cc::TILE_PIX];
    __shared__ int members;
    constexpr int conn = PASS == 0 ? 4 : 8;
    constexpr int PER = cc::TILE_PIX / 256;
    const int plane = blockIdx.y, n = plane / K, c = plane % K, t = threadIdx.x;
    const int ntx = cc::tiles_x(W), y0 = (int)(blockIdx.x / ntx) * cc::TILE_H, x0 = (int)(blockIdx.x % ntx) * cc::TILE_W;
    const long HW = (long)H * W, base = by_class ? (long)n * HW : (long)plane * HW, fbase = (long)plane * (HW + 1);
    const int lx = t & 63, x = x0 + lx;
    bool in[PER], mem[PER];
    int root[PER];
    if (t == 0) members = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int ly = (t >> 6) + 4 * j, y = y0 + ly, i = ly * cc::TILE_W + lx;
        const long e = (long)y * W + x;
        in[j] = y < H && x < W;
        mem[j] = false;
        if (in[j]) {
            const bool fg = fg_at(pred, is64, by_class, base, c, e);
            if (PASS == 0) mem[j] = !fg;
            else mem[j] = fg || (holes && cc::find<cc::Plain>(holes + fbase, cc::node(e)) != cc::OUTSIDE);
            if (PASS == 1) out[(long)plane * HW + e] = mem[j] ? 1.f : 0.f;
        }
        lab[i] = cc::tile_init(__ballot(mem[j]), ly, lx);          // (a wave holds one tile row)
        cnt[i] = 0;
    }
    if (PASS == 1 && !label) return;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) cc::tile_unite_pixel<Local>(lab, ((t >> 6) + 4 * j) * cc::TILE_W + lx, conn);
    __syncthreads();                                     // the tile's forest is final: plain reads from here on
    int mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int ly = (t >> 6) + 4 * j, y = y0 + ly, i = ly * cc::TILE_W + lx;
        root[j] = mem[j] ? cc::find<cc::Plain>(lab, i) : 0;
        if (!mem[j]) continue;
        if (PASS == 0) {
            if (y == 0 || x == 0 || y == H - 1 || x == W - 1) cnt[root[j]] = 1;      // (every writer stores the same 1)
        } else {
            atomicAdd(&cnt[root[j]], 1);
            ++mine;
        }
    }
    if (PASS == 1) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if ((t & 63) == 0 && mine) atomicAdd(&members, mine);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (!in[j]) continue;
        const int ly = (t >> 6) + 4 * j, i = ly * cc::TILE_W + lx;
        const long at = fbase + cc::node((long)(y0 + ly) * W + x);
        if (PASS == 0) {
            dst[at] = !mem[j] ? -1 : cnt[root[j]] ? cc::OUTSIDE : cc::tile_node(root[j], y0, x0, W);
        } else {
            dst[at] = mem[j] ? cc::tile_node(root[j], y0, x0, W) : -1;
            size[at] = mem[j] && root[j] == i ? cnt[i] : 0;
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        dst[fbase] = cc::OUTSIDE;                       // node 0: the outside's root (forest 2 has it too, with nothing below it)
        if (PASS == 1) size[fbase] = 0;
    }
    if (PASS == 1 && t == 0 && members) atomicAdd(&total[plane], members);
}

// grid (ceil(slots / 256), N * K): one thread per slot of components.h's border-pair enumeration
__global__ __launch_bounds__(256) void merge_kernel(int conn, int H, int W, long slots, int* __restrict__ forest) {
    const long slot = (long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= slots) return;
    int ya, xa, yb, xb, kind, y, x;
    if (!cc::border_pair(conn, H, W, slot, &ya, &xa, &yb, &xb, &kind, &y, &x)) return;
    int* P = forest + (long)blockIdx.y * ((long)H * W + 1);
    const int a = cc::node((long)ya * W + xa), b = cc::node((long)yb * W + xb);
    const auto mem = [&](int v, int u) { return Shared::load(P + cc::node((long)v * W + u)) >= 0; };   // (a member's parent is never negative)
    if (!mem(ya, xa) || !mem(yb, xb) || cc::pair_redundant(kind, y, x, W, mem)) return;
    cc::unite<Shared>(P, a, b);
}

// grid (ceil(HW / 256), N * K).  Roots do not change in this launch (nothing unites); a node below its root adds its tile
// component's count there and then points at it, which other threads climbing through it may or may not see yet.
__global__ __launch_bounds__(256) void flatten_kernel(int H, int W, int* __restrict__ forest, int* __restrict__ size) {
    const long HW = (long)H * W, e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= HW) return;
    const long fbase = (long)blockIdx.y * (HW + 1);
    int* P = forest + fbase;
    const int me = cc::node(e), p = Shared::load(P + me);
    if (p < 0 || p == me) return;
    const int r = cc::find<Shared>(P, me);
    const int c = size[fbase + me];                      // (written by local_kernel<1>; only roots' counts change here)
    if (c > 0) atomicAdd(&size[fbase + r], c);
    if (p != r) __hip_atomic_store(P + me, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(HW / 256), N * K)
__global__ __launch_bounds__(256) void filter_kernel(int H, int W, const int* __restrict__ forest, const int* __restrict__ size,
                                                    const int* __restrict__ total, int num, int den, float* __restrict__ out) {
    const long HW = (long)H * W, e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= HW) return;
    const long fbase = (long)blockIdx.y * (HW + 1);
    const int r = forest[fbase + cc::node(e)];
    if (r < 0) return;
    if (cc::removed(size[fbase + r], total[blockIdx.y], num, den)) out[(long)blockIdx.y * HW + e] = 0.f;
}

int check_sizes(const char* who, int N, int K, int H, int W) {
    USTRUN_CHECK(N > 0 && K > 0, "%s: N, K > 0, got N %d K %d", who, N, K);
    USTRUN_CHECK(H >= 1 && W >= 1 && H <= PP_MAX && W <= PP_MAX, "%s: H and W must be in 1..%d, got %d x %d", who, PP_MAX, H, W);
    USTRUN_CHECK((int64_t)N * K <= 65535, "%s: N * K = %lld planes exceed one launch (65535)", who, (long long)N * K);
    return 0;
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int64_t ustrun_post_process_work_bytes(int N, int K, int H, int W) {
    if (check_sizes("post_process_work_bytes", N, K, H, W)) return -1;
    return post_work_bytes((int64_t)N * K, H, W);
}

extern "C" int ustrun_post_process(const void* pred, int pred_is_i64, int N, int K, int by_class, int H, int W, int fill_holes,
                                   int share_num, int share_den, void* work, int64_t work_bytes, float* out, ustrun_stream_t s) {
    USTRUN_TRY(check_sizes("post_process", N, K, H, W));
    USTRUN_CHECK(pred && work && out, "post_process: bad args");
    USTRUN_CHECK(share_num >= 0 && share_den > 0, "post_process: share_num >= 0 and share_den > 0, got %d / %d", share_num, share_den);
    const int64_t NK = (int64_t)N * K;
    USTRUN_CHECK(work_bytes >= post_work_bytes(NK, H, W), "post_process: work buffer of %lld bytes, needs %lld",
                 (long long)work_bytes, (long long)post_work_bytes(NK, H, W));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)out & 3) == 0, "post_process: work must be 16-byte and out 4-byte aligned");
    const PostWork w = post_carve(work, NK, H, W);
    const hipStream_t st = (hipStream_t)s;
    const dim3 tiles(cc::tiles_x(W) * cc::tiles_y(H), NK), pixels(cdiv((int64_t)H * W, 256), NK);
    if (fill_holes) {
        hipLaunchKernelGGL(local_kernel<0>, tiles, dim3(256), 0, st, pred, pred_is_i64, K, by_class, H, W, (const int*)nullptr, 1,
                           w.hole, (int*)nullptr, (int*)nullptr, (float*)nullptr);
        USTRUN_LAUNCH_CHECK("post_process: background tiles");
        const long slots = cc::border_slots(4, H, W);
        if (slots) {
            hipLaunchKernelGGL(merge_kernel, dim3(cdiv(slots, 256), NK), dim3(256), 0, st, 4, H, W, slots, w.hole);
            USTRUN_LAUNCH_CHECK("post_process: background merge");
        }
    }
    if (share_num) {
        const hipError_t e = hipMemsetAsync(w.total, 0, sizeof(int) * NK, st);
        USTRUN_CHECK(e == hipSuccess, "post_process: memset failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(local_kernel<1>, tiles, dim3(256), 0, st, pred, pred_is_i64, K, by_class, H, W,
                       fill_holes ? (const int*)w.hole : (const int*)nullptr, share_num ? 1 : 0, w.comp, w.size, w.total, out);
    USTRUN_LAUNCH_CHECK("post_process: foreground tiles");
    if (!share_num) return 0;
    const long slots = cc::border_slots(8, H, W);
    if (slots) {
        hipLaunchKernelGGL(merge_kernel, dim3(cdiv(slots, 256), NK), dim3(256), 0, st, 8, H, W, slots, w.comp);
        USTRUN_LAUNCH_CHECK("post_process: foreground merge");
    }
    hipLaunchKernelGGL(flatten_kernel, pixels, dim3(256), 0, st, H, W, w.comp, w.size);
    USTRUN_LAUNCH_CHECK("post_process: flatten");
    hipLaunchKernelGGL(filter_kernel, pixels, dim3(256), 0, st, H, W, (const int*)w.comp, (const int*)w.size, (const int*)w.total,
                       share_num, share_den, out);
    USTRUN_LAUNCH_CHECK("post_process: filter");
    return 0;
}
