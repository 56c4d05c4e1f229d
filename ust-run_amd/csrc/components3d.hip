// Post-processing of a binary prediction as a VOLUME on the device (include/ustrun.h: ustrun_post_process_3d): the reference's
// dataloaders/utils.py:193-204 `post_processing`, whose scipy / skimage calls are n-dimensional, on every (case, part) volume
// [D][H][W] of a batch at once, integer-exact -- the 3-D twin of components.hip.
//
//   holes  = background voxels not 6-connected through background to a face of the volume (binary_fill_holes, default structure)
//   F      = P | holes;   total = |F|
//   out    = F without the 26-connected components c with share_den * |c| < share_num * total, and with `largest` without every
//            component but the largest one (among equal sizes: the one whose smallest voxel index is smallest)
//
// The forest is components.h's over the volume's voxels (components3d.h: voxel e = node e + 1, node 0 the outside).  Inside a
// slice the 6-neighbourhood is the cross and the 26-neighbourhood the 3 x 3 square, so slices are labelled and merged as planes are
// -- the same tile, the same border pairs -- and one launch more per forest unites the pairs between adjacent slices.  Launches on
// the stream, each finished before the next starts; no block waits for another, takes a ticket or spins:
//   1 local_kernel<0>   a block per 16 x 64 tile of a slice (flat index over tiles x slices x volumes, folded: a block walks several
//                       tiles when there are more than LOCAL_BLOCKS_MAX): the BACKGROUND's cross components of the tile in LDS;
//                       parent = the tile component's smallest node, or node 0 when it touches a face of the volume -- an in-plane
//                       border pixel, or any pixel of slices 0 and D - 1
//   2 merge_kernel      one thread per border pair of a slice (components.h: border_pair, pair_redundant), conn 4
//   3 zmerge_kernel     one thread per pair (z, y, x) - (z - 1, y, x), unless redundant (components3d.h: z_pair_redundant)
//   4 local_kernel<1>   F = foreground | background whose root in forest 1 is not node 0 -> out; F's 3 x 3 tile components ->
//                       forest 2, each tile component's voxel count at its smallest node, |F| per volume (one atomic add per block)
//   5 merge_kernel      conn 8
//   6 zmerge_kernel     the nine pairs (z, y, x) - (z - 1, y + dy, x + dx)
//   7 flatten_kernel    every node points at its root; counts are added at the roots (one atomic per tile component)
//   8 largest_kernel    only with `largest`: one 64-bit atomic maximum per root on (size << 32) | (0xffffffff - root)
//   9 filter_kernel     out = 0 where the root's count is below the share, or the root is not the winner
// fill_holes = 0 drops 1-3; share_num = 0 without `largest` drops the labelling of 4 and 5-9.  Integer atomics only (minimum, add,
// maximum): roots are the components' smallest nodes, counts and the winner are exact whatever the order -- equal bits on every run.
//
// Stale reads in 2, 3, 5, 6: a parent read from another XCD's older copy is an older ancestor of the node,
// because parents only decrease along ancestors; `find` then stops at a node that is a root no longer, and the atomic minimum on
// that node -- performed at the device's coherence point -- returns its true parent, with which `unite` goes on.  No union is lost,
// and every loop steps to a strictly smaller index.
#include "components_dev.h"
#include "components3d.h"
#include "edt3d_plan.h"                 // the volume limits: sizes_ok, voxels_ok

namespace ustrun {
namespace {

constexpr int LOCAL_BLOCKS_MAX = 1 << 16;        // blocks of the folded tile grid: 16 M threads, many times what the device holds
constexpr int DBG2_UNITE_ALL = 128;              // ustrun_debug_flags2 bit 7: no z-pair is left out as redundant (A/B runs)

struct Post3Work {
    int* hole;                      // [NK][DHW + 1]  forest 1: background, 6 neighbours, node 0 = outside
    int* comp;                      // [NK][DHW + 1]  forest 2: F, 26 neighbours
    int* size;                      // [NK][DHW + 1]  voxels of the tile component at its smallest node, after flatten of the component at its root
    int* total;                     // [NK]           |F|                                  (zeroed every call, with key: one memset)
    unsigned long long* key;        // [NK]           components3d.h: largest_key of the winner
};

static inline int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }
static inline int64_t forest_bytes(int64_t NK, int64_t DHW) { return up16(NK * (DHW + 1) * 4); }
static inline int64_t tail_bytes(int64_t NK) { return up16(NK * 4) + up16(NK * 8); }
int64_t post3_work_bytes(int64_t NK, int64_t DHW) { return 3 * forest_bytes(NK, DHW) + tail_bytes(NK); }

Post3Work post3_carve(void* work, int64_t NK, int64_t DHW) {
    char* p = (char*)work;
    Post3Work w;
    w.hole = (int*)p; p += forest_bytes(NK, DHW);
    w.comp = (int*)p; p += forest_bytes(NK, DHW);
    w.size = (int*)p; p += forest_bytes(NK, DHW);
    w.total = (int*)p; p += up16(NK * 4);
    w.key = (unsigned long long*)p;
    return w;
}

// grid (min(tiles x D x N x K, LOCAL_BLOCKS_MAX)), 256 threads: wave w takes the tile's rows w, w + 4, w + 8, w + 12.  Tile b of the
// flat list is tile b % tiles of slice (b / tiles) % D of volume b / tiles / D; offsets between volumes in 64 bits, int32 inside one.
// PASS 0: members = background, cross -> forest `dst` with the outside root.  PASS 1: members = F (`holes`: forest 1 after its
// merges, or null = no filling), written to `out`; label = 0 stops there, else 3 x 3 square -> forest `dst`, counts, totals.
template <int PASS>
__global__ __launch_bounds__(256) void local_kernel(const void* pred, int is64, int K, int by_class, int D, int H, int W, long ntiles,
                                                   const int* __restrict__ holes, int label, int* __restrict__ dst,
                                                   int* __restrict__ size, int* __restrict__ total, float* __restrict__ out) {
    __shared__ int lab[cc::TILE_PIX];
    __shared__ int cnt[cc::TILE_PIX];
    __shared__ int members;
    constexpr int conn = PASS == 0 ? 4 : 8;
    constexpr int PER = cc::TILE_PIX / 256;
    const int t = threadIdx.x, lx = t & 63;
    const int ntx = cc::tiles_x(W), per_slice = ntx * cc::tiles_y(H), HW = H * W;
    const long DHW = (long)D * HW;
    const bool labels = PASS == 0 || label;
    for (long b = blockIdx.x; b < ntiles; b += gridDim.x) {
        const int tile = (int)(b % per_slice), z = (int)(b / per_slice % D), vol = (int)(b / per_slice / D), n = vol / K, c = vol % K;
        const int y0 = tile / ntx * cc::TILE_H, x0 = tile % ntx * cc::TILE_W, x = x0 + lx, zoff = z * HW;
        const long base = (by_class ? (long)n : (long)vol) * DHW, fbase = (long)vol * (DHW + 1);
        bool in[PER], mem[PER];
        int root[PER];
        if (t == 0) members = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int ly = (t >> 6) + 4 * j, y = y0 + ly, i = ly * cc::TILE_W + lx;
            const int e = zoff + y * W + x;
            in[j] = y < H && x < W;
            mem[j] = false;
            if (in[j]) {
                const bool fg = fg_at(pred, is64, by_class, base, c, e);
                if (PASS == 0) mem[j] = !fg;
                else mem[j] = fg || (holes && cc::find<cc::Plain>(holes + fbase, cc::node(e)) != cc::OUTSIDE);
                if (PASS == 1) out[(long)vol * DHW + e] = mem[j] ? 1.f : 0.f;
            }
            if (labels) {
                lab[i] = cc::tile_init(__ballot(mem[j]), ly, lx);      // (a wave holds one tile row)
                cnt[i] = 0;
            }
        }
        if (!labels) continue;                               // (no LDS touched: nothing to wait for)
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
                if (cc::on_face(z, y, x, D, H, W)) cnt[root[j]] = 1;                  // (every writer stores the same 1)
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
            const long at = fbase + zoff + cc::node((long)(y0 + ly) * W + x);
            const int rnode = zoff + cc::tile_node(root[j], y0, x0, W);
            if (PASS == 0) {
                dst[at] = !mem[j] ? -1 : cnt[root[j]] ? cc::OUTSIDE : rnode;
            } else {
                dst[at] = mem[j] ? rnode : -1;
                size[at] = mem[j] && root[j] == i ? cnt[i] : 0;
            }
        }
        if (tile == 0 && z == 0 && t == 0) {
            dst[fbase] = cc::OUTSIDE;                       // node 0: the outside's root (forest 2 has it too, with nothing below it)
            if (PASS == 1) size[fbase] = 0;
        }
        if (PASS == 1 && t == 0 && members) atomicAdd(&total[vol], members);
        __syncthreads();                                     // the next tile of this block reuses lab, cnt, members
    }
}

// grid (ceil(D * slots / 256), N * K): one thread per slot of components.h's border-pair enumeration in each slice
__global__ __launch_bounds__(256) void merge_kernel(int conn, int D, int H, int W, long slots, int* __restrict__ forest) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= slots * D) return;
    const int zoff = (int)(idx / slots) * H * W;
    int ya, xa, yb, xb, kind, y, x;
    if (!cc::border_pair(conn, H, W, idx % slots, &ya, &xa, &yb, &xb, &kind, &y, &x)) return;
    int* P = forest + (long)blockIdx.y * ((long)D * H * W + 1);
    const int a = zoff + cc::node((long)ya * W + xa), b = zoff + cc::node((long)yb * W + xb);
    const auto mem = [&](int v, int u) { return Shared::load(P + zoff + cc::node((long)v * W + u)) >= 0; };   // (a member's parent is never negative)
    if (!mem(ya, xa) || !mem(yb, xb) || cc::pair_redundant(kind, y, x, W, mem)) return;
    cc::unite<Shared>(P, a, b);
}

// grid (ceil(slots / 256), N * K): one thread per slot of components3d.h's z-pair enumeration (fan 1 or 9)
__global__ __launch_bounds__(256) void zmerge_kernel(int fan, int prune, int D, int H, int W, long slots, int* __restrict__ forest) {
    const long slot = (long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= slots) return;
    int z, y, x, dy, dx;
    if (!cc::z_pair(fan, H, W, slot, &z, &y, &x, &dy, &dx)) return;
    int* P = forest + (long)blockIdx.y * ((long)D * H * W + 1);
    const auto mem = [&](int w, int v, int u) { return Shared::load(P + cc::vnode(w, v, u, H, W)) >= 0; };
    if (!mem(z, y, x) || !mem(z - 1, y + dy, x + dx) || (prune && cc::z_pair_redundant(z, y, x, dy, dx, mem))) return;
    cc::unite<Shared>(P, cc::vnode(z, y, x, H, W), cc::vnode(z - 1, y + dy, x + dx, H, W));
}

// grid (ceil(DHW / 256), N * K).  Roots do not change in this launch (nothing unites); a node below its root adds its tile
// component's count there and then points at it, which other threads climbing through it may or may not see yet.
__global__ __launch_bounds__(256) void flatten_kernel(int DHW, int* __restrict__ forest, int* __restrict__ size) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= DHW) return;
    const long fbase = (long)blockIdx.y * ((long)DHW + 1);
    int* P = forest + fbase;
    const int me = cc::node(e), p = Shared::load(P + me);
    if (p < 0 || p == me) return;
    const int r = cc::find<Shared>(P, me);
    const int c = size[fbase + me];                      // (written by local_kernel<1>; only roots' counts change here)
    if (c > 0) atomicAdd(&size[fbase + r], c);
    if (p != r) __hip_atomic_store(P + me, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(DHW / 256), N * K): every root offers its key
__global__ __launch_bounds__(256) void largest_kernel(int DHW, const int* __restrict__ forest, const int* __restrict__ size,
                                                     unsigned long long* __restrict__ key) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= DHW) return;
    const long fbase = (long)blockIdx.y * ((long)DHW + 1);
    const int me = cc::node(e);
    if (forest[fbase + me] != me) return;
    __hip_atomic_fetch_max(key + blockIdx.y, cc::largest_key(size[fbase + me], me), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(DHW / 256), N * K)
__global__ __launch_bounds__(256) void filter_kernel(int DHW, const int* __restrict__ forest, const int* __restrict__ size,
                                                    const int* __restrict__ total, const unsigned long long* __restrict__ key,
                                                    int num, int den, int largest, float* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= DHW) return;
    const long fbase = (long)blockIdx.y * ((long)DHW + 1);
    const int r = forest[fbase + cc::node(e)];
    if (r < 0) return;
    if (cc::removed(size[fbase + r], total[blockIdx.y], num, den) || (largest && r != cc::key_root(key[blockIdx.y])))
        out[(long)blockIdx.y * DHW + e] = 0.f;
}

int check_volume(const char* who, int N, int K, int D, int H, int W) {
    USTRUN_CHECK(edt3d::sizes_ok(N, K, D, H, W), "%s: N, K > 0, N * K <= %lld and D, H, W in 1..%d, got N %d K %d D %d H %d W %d", who,
                 (long long)edt3d::NK_MAX, edt3d::VOL_MAX, N, K, D, H, W);
    USTRUN_CHECK(edt3d::voxels_ok(D, H, W), "%s: D * H * W = %lld voxels exceed 2^27 = %lld (D %d H %d W %d)", who,
                 (long long)D * H * W, (long long)edt3d::VOX_MAX, D, H, W);
    return 0;
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int64_t ustrun_post_process_3d_work_bytes(int N, int K, int D, int H, int W) {
    if (check_volume("post_process_3d_work_bytes", N, K, D, H, W)) return -1;
    return post3_work_bytes((int64_t)N * K, (int64_t)D * H * W);
}

extern "C" int ustrun_post_process_3d(const void* pred, int pred_is_i64, int N, int K, int by_class, int D, int H, int W,
                                      int fill_holes, int share_num, int share_den, int largest, void* work, int64_t work_bytes,
                                      float* out, ustrun_stream_t s) {
    USTRUN_TRY(check_volume("post_process_3d", N, K, D, H, W));
    USTRUN_CHECK(share_num >= 0 && share_den > 0, "post_process_3d: share_num >= 0 and share_den > 0, got %d / %d", share_num, share_den);
    USTRUN_CHECK(pred && work && out, "post_process_3d: null pointer (pred %p work %p out %p)", pred, work, (void*)out);
    const int64_t NK = (int64_t)N * K, DHW = (int64_t)D * H * W;
    USTRUN_CHECK(work_bytes >= post3_work_bytes(NK, DHW), "post_process_3d: work buffer of %lld bytes, needs %lld",
                 (long long)work_bytes, (long long)post3_work_bytes(NK, DHW));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)pred & (pred_is_i64 ? 7 : 3)) == 0,
                 "post_process_3d: work must be 16-byte and out 4-byte aligned, pred to its element");
    const Post3Work w = post3_carve(work, NK, DHW);
    const hipStream_t st = (hipStream_t)s;
    const int prune = !(g_debug_flags2 & DBG2_UNITE_ALL), label = share_num || largest;
    const long ntiles = (long)cc::tiles_x(W) * cc::tiles_y(H) * D * NK;
    const dim3 tiles(ntiles < LOCAL_BLOCKS_MAX ? ntiles : LOCAL_BLOCKS_MAX), voxels(cdiv(DHW, 256), NK);
    if (fill_holes) {
        hipLaunchKernelGGL(local_kernel<0>, tiles, dim3(256), 0, st, pred, pred_is_i64, K, by_class, D, H, W, ntiles, (const int*)nullptr,
                           1, w.hole, (int*)nullptr, (int*)nullptr, (float*)nullptr);
        USTRUN_LAUNCH_CHECK("post_process_3d: background tiles");
        const long slots = cc::border_slots(4, H, W), zslots = cc::z_slots(1, D, H, W);
        if (slots) {
            hipLaunchKernelGGL(merge_kernel, dim3(cdiv(slots * D, 256), NK), dim3(256), 0, st, 4, D, H, W, slots, w.hole);
            USTRUN_LAUNCH_CHECK("post_process_3d: background merge");
        }
        if (zslots) {
            hipLaunchKernelGGL(zmerge_kernel, dim3(cdiv(zslots, 256), NK), dim3(256), 0, st, 1, prune, D, H, W, zslots, w.hole);
            USTRUN_LAUNCH_CHECK("post_process_3d: background z-merge");
        }
    }
    if (label) {
        const hipError_t e = hipMemsetAsync(w.total, 0, tail_bytes(NK), st);       // totals and keys
        USTRUN_CHECK(e == hipSuccess, "post_process_3d: memset failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(local_kernel<1>, tiles, dim3(256), 0, st, pred, pred_is_i64, K, by_class, D, H, W, ntiles,
                       fill_holes ? (const int*)w.hole : (const int*)nullptr, label, w.comp, w.size, w.total, out);
    USTRUN_LAUNCH_CHECK("post_process_3d: foreground tiles");
    if (!label) return 0;
    const long slots = cc::border_slots(8, H, W), zslots = cc::z_slots(9, D, H, W);
    if (slots) {
        hipLaunchKernelGGL(merge_kernel, dim3(cdiv(slots * D, 256), NK), dim3(256), 0, st, 8, D, H, W, slots, w.comp);
        USTRUN_LAUNCH_CHECK("post_process_3d: foreground merge");
    }
    if (zslots) {
        hipLaunchKernelGGL(zmerge_kernel, dim3(cdiv(zslots, 256), NK), dim3(256), 0, st, 9, prune, D, H, W, zslots, w.comp);
        USTRUN_LAUNCH_CHECK("post_process_3d: foreground z-merge");
    }
    hipLaunchKernelGGL(flatten_kernel, voxels, dim3(256), 0, st, (int)DHW, w.comp, w.size);
    USTRUN_LAUNCH_CHECK("post_process_3d: flatten");
    if (largest) {
        hipLaunchKernelGGL(largest_kernel, voxels, dim3(256), 0, st, (int)DHW, (const int*)w.comp, (const int*)w.size, w.key);
        USTRUN_LAUNCH_CHECK("post_process_3d: largest key");
    }
    hipLaunchKernelGGL(filter_kernel, voxels, dim3(256), 0, st, (int)DHW, (const int*)w.comp, (const int*)w.size, (const int*)w.total,
                       (const unsigned long long*)w.key, share_num, share_den, largest, out);
    USTRUN_LAUNCH_CHECK("post_process_3d: filter");
    return 0;
}
