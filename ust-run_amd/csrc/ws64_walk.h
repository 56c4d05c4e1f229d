// ws64_walk.h -- the work plan of the 64 -> 64 streaming convolution (conv_ws64_bf16.hip) and the cursor a block walks over its share of
// it.  Pure integer code without device-only constructs: the three builds of the kernel use it, and tests/host/ws64_walk_check.hip
// compiles it for the host and pins it over whole ranges of shapes.
#pragma once
#include "common.h"

namespace ustrun {

constexpr int WS_TW = 32;          // strip width in pixels

// Uniform plan: every strip is cut into sy segments of seg rows, item = (image, segment, strip), ipb items per block.
// Flat plan (L > 0; the consumer / producer build only): the strips' 8-row steps form ONE sequence of N * sx * steps steps and
// block b takes steps [b L, (b + 1) L) of it, whatever strips they fall in -- equal work per block at ANY image count (81 images of
// 256^2: 648 strips over 256 CUs are 3 rounds of items with the last one half empty, but 81 steps per block exactly).  L >= steps,
// so a strip is cut at most once: item slot = 2 strip + (the piece does not start at the strip's first row).
struct WsPlan { int sx, sy, seg, items, ipb, L, steps; unsigned long long* dbg; };

struct Cur {            // one group of 8 input rows of one item (or nothing)
    int valid, item, img, x0, ybeg, S, k;
    int left;           // flat plan: steps of the block's range behind this item
};

// Group k of `item` for a block whose items end at it1 (uniform plan), or -- flat -- the first piece of block blk: wherever step
// blk * L falls (item and it1 are not looked at).  The one place that divides.
__host__ __device__ __forceinline__ Cur ws_decode(const WsPlan& p, int N, int H, int blk, int it1, int item, int k, bool flat) {
    Cur c;
    c.k = k; c.left = 0;
    if (flat) {
        const int total = N * p.sx * p.steps;
        const int pos = blk * p.L, end = min(pos + p.L, total);
        const int strip = pos / p.steps, st = pos - strip * p.steps;
        c.valid = pos < end;
        c.img = strip / p.sx;
        c.x0 = (strip - c.img * p.sx) * WS_TW;
        c.ybeg = st * 8;
        c.S = max(min(p.steps - st, end - pos), 1);
        c.left = max(end - pos - c.S, 0);
        c.item = strip * 2 + (st != 0 ? 1 : 0);
        return c;
    }
    c.valid = item < it1;
    item = min(item, it1 - 1);                 // (geometry stays inside the tensor when there is nothing left)
    c.item = item;
    const int per = p.sx * p.sy;
    c.img = item / per;
    const int rem = item - c.img * per;
    const int ys = rem / p.sx;
    c.x0 = (rem - ys * p.sx) * WS_TW;
    c.ybeg = ys * p.seg;
    const int rows = min(p.seg, H - c.ybeg);
    c.S = (rows + 7) >> 3;
    return c;
}

// the next group: same item, or the next item by counting (strip, segment, image) up -- no divisions on the producers'
// path between two barriers (the division-based decode runs once, for the block's first item)
__host__ __device__ __forceinline__ Cur ws_advance(const WsPlan& p, int H, int it1, const Cur& c, bool flat) {
    Cur n = c;
    const bool same = c.k < c.S;
    if (flat) {             // the next piece starts at the next strip's first row and ends with the strip or with the block's range
        const bool has = c.left > 0;
        int x0 = c.x0 + WS_TW, img = c.img;
        const bool wrapx = x0 >= p.sx * WS_TW;
        x0 = wrapx ? 0 : x0;
        img = wrapx ? img + 1 : img;
        const int S = min(p.steps, c.left);
        if (same) n.k = c.k + 1;
        else if (has) { n.item = (c.item | 1) + 1; n.img = img; n.x0 = x0; n.ybeg = 0; n.S = S; n.left = c.left - S; n.k = 0; }
        else { n.valid = 0; n.k = 0; }
        return c.valid ? n : c;
    }
    const int item = min(c.item + 1, it1 - 1);
    const bool has = c.item + 1 < it1;
    int x0 = c.x0 + WS_TW, ybeg = c.ybeg, img = c.img;
    const bool wrapx = x0 >= p.sx * WS_TW;
    x0 = wrapx ? 0 : x0;
    ybeg = wrapx ? ybeg + p.seg : ybeg;
    const bool wrapy = ybeg >= p.sy * p.seg;
    ybeg = wrapy ? 0 : ybeg;
    img = wrapy ? img + 1 : img;
    const int rows = min(p.seg, H - ybeg);
    if (same) n.k = c.k + 1;
    else if (has) { n.item = item; n.img = img; n.x0 = x0; n.ybeg = ybeg; n.S = (rows + 7) >> 3; n.k = 0; }
    else { n.valid = 0; n.k = 0; }
    return c.valid ? n : c;
}

// the same sequence through a fresh decode per item (two divisions): the uniform plan's walk in the four-wave and the eight-wave build
__host__ __device__ __forceinline__ Cur ws_advance_div(const WsPlan& p, int N, int H, int blk, int it1, const Cur& c) {
    if (!c.valid) return c;
    if (c.k < c.S) { Cur n = c; n.k = c.k + 1; return n; }
    return ws_decode(p, N, H, blk, it1, c.item + 1, 0, false);
}

// segments per strip: whole waves of blocks over the 256 CUs, few bubbles (one staging-only iteration per item) -- or, where that
// leaves a round of items half empty, the flat plan: equal step counts per block.  cp_build: the launch runs the consumer /
// producer build (the only one that walks the flat plan); keep_uniform: the caller asks for the uniform plan anyway (A/B runs).
inline WsPlan ws_plan(int N, int H, int W, bool cp_build, bool keep_uniform) {
    WsPlan p;
    p.sx = cdiv(W, WS_TW);
    const int steps = cdiv(H, 8);
    double best = 1e30;
    p.sy = 1;
    for (int sy = 1; sy <= steps; ++sy) {
        const int per = cdiv(steps, sy);
        if (cdiv(steps, per) != sy) continue;                 // (no empty segments)
        const long items = (long)N * p.sx * sy;
        const long ipb = (items + 255) / 256;
        const double cost = (double)ipb * (per + 1.5);
        if (cost < best - 1e-9) { best = cost; p.sy = sy; }
    }
    p.seg = cdiv(steps, p.sy) * 8;
    p.items = N * p.sx * p.sy;
    p.ipb = (p.items + 255) / 256;
    p.L = 0; p.steps = steps;
    p.dbg = nullptr;
    // the flat plan: L steps per block, its range touching at most cdiv(L - 1, steps) + 1 strips
    const long total = (long)N * p.sx * steps;
    const int L = (int)((total + 255) / 256);
    if (cp_build && !keep_uniform && L >= steps && total < (1L << 30)) {
        const double cost = L + 1.5 * (cdiv(L - 1, steps) + 1);
        if (cost < 0.97 * best) p.L = L;
    }
    return p;
}
inline int ws_grid(int N, const WsPlan& p) {
    return p.L > 0 ? (int)cdiv((long)N * p.sx * p.steps, (long)p.L) : cdiv(p.items, p.ipb);
}
// statistics rows of a launch: two (one per consumer-wave pair) per item; flat plan: per slot, two slots per strip
inline int ws_stat_rows(int N, const WsPlan& p) { return p.L > 0 ? N * p.sx * 4 : p.items * 2; }

}  // namespace ustrun
