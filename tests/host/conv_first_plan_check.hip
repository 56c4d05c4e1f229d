// conv_first_plan_check.hip -- host-only check of the strip plans, the item decodes and the streaming-eligibility predicate of the first
// convolution (ust-run_amd/csrc/conv_first_plan.h) over whole ranges of shapes (tests/test_conv_first_plan_host.py builds and runs it;
// no GPU, no device code is called).  Exit status 0 = every check passed.  With the argument "rows" it also prints the forward's grid
// of every swept shape ("rows N H W grid"): the Python side compares them with what the library reports and promises.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ust-run_amd/csrc/conv_first_plan.h"

using namespace ustrun;

static long g_fail = 0;
static void fail(const char* what, int N, int H, int W, long a, long b) {
    if (g_fail++ < 20) std::printf("FAIL %s (N = %d, %d x %d): %ld, %ld\n", what, N, H, W, a, b);
}

static const int Ws[] = {16, 17, 33, 37, 70, 100, 256}, Hs[] = {3, 5, 8, 9, 19, 40, 136, 288};

// a dense NCHW f32 source of C channels
static ustrun_src_t nchw(int C, int H, int W) {
    ustrun_src_t s = {};
    s.ptr = (const void*)16; s.C = C; s.H = H; s.W = W; s.f32 = 1;
    s.sW = 1; s.sH = W; s.sC = (int64_t)H * W; s.sN = (int64_t)C * H * W;
    return s;
}

// weight gradient: the plan's bounds, no empty segment, the items' (image, strip, row) triples cover the batch exactly once
static long check_wgrad(int N, int H, int W, int dy_esz, std::vector<int>& cover) {
    const ustrun_src_t s = nchw(3, H, W);
    if (!conv_first_wgrad_stream_ok(s, N, H, W, dy_esz)) return 0;
    const CfWgradPlan p = conv_first_wgrad_plan(N, H, W);
    if (p.blocks > 1024 || p.blocks < 1 || (long)p.blocks * 4 < p.items) fail("wgrad blocks", N, H, W, p.blocks, p.items);
    if (p.items > 4096 || p.items != (long)N * p.strips * p.nseg) fail("wgrad items", N, H, W, p.items, p.nseg);
    if ((int64_t)p.blocks * 32 * 64 * 4 > (int64_t)1024 * 32 * 64 * 4) fail("wgrad slabs beyond the partials bound", N, H, W, p.blocks, 1024);
    if (p.strips != cdiv(W, CF_WG_TW) || p.seg_rows < 1 || (long)(p.nseg - 1) * p.seg_rows >= H || (long)p.nseg * p.seg_rows < H)
        fail("wgrad empty segment", N, H, W, p.nseg, p.seg_rows);
    cover.assign((size_t)N * p.strips * H, 0);
    for (int item = 0; item < (int)p.items; ++item) {
        const CfWgradItem it = conv_first_wgrad_item(p.strips, p.nseg, p.seg_rows, H, item);
        if (it.img < 0 || it.img >= N || it.x0 % CF_WG_TW || it.x0 < 0 || it.x0 >= W || it.r0 < 0 || it.r0 >= it.r1 || it.r1 > H) {
            fail("wgrad decode", N, H, W, item, it.r0);
            continue;
        }
        if (item % p.strips != it.x0 / CF_WG_TW) fail("wgrad: strip is not the fastest index", N, H, W, item, it.x0);
        for (int y = it.r0; y < it.r1; ++y) ++cover[((size_t)it.img * p.strips + it.x0 / CF_WG_TW) * H + y];
    }
    for (size_t i = 0; i < cover.size(); ++i)
        if (cover[i] != 1) { fail("wgrad items do not cover (image, strip, row) once", N, H, W, (long)i, cover[i]); break; }
    return p.items;
}

// forward: the grid, its share per image, the items' 8-row steps cover every row of every strip once
static long check_fwd(int N, int H, int W, bool print, std::vector<int>& cover) {
    const CfFwdPlan p = conv_first_fwd_plan(N, H, W);
    const int grid = conv_first_fwd_grid(N, p);
    if (print) std::printf("rows %d %d %d %d\n", N, H, W, grid);
    if (p.seg_rows != stream_seg_rows(N, H, W) || p.strips != cdiv(W, CF_FWD_TW) || p.segs != cdiv(H, p.seg_rows)) fail("fwd plan", N, H, W, p.segs, p.seg_rows);
    if (p.seg_rows < CF_FWD_TH || p.seg_rows > 64 || p.seg_rows % CF_FWD_TH) fail("fwd seg_rows", N, H, W, p.seg_rows, 0);
    if (grid != N * p.segs * p.strips || grid % N || grid < 1) fail("fwd grid", N, H, W, grid, N);
    cover.assign((size_t)N * p.strips * H, 0);
    long steps = 0;
    for (int item = 0; item < grid; ++item) {
        const CfFwdItem it = conv_first_fwd_item(p, H, item);
        if (it.img < 0 || it.img >= N || it.x0 % CF_FWD_TW || it.x0 < 0 || it.x0 >= W || it.r0 < 0 || it.r0 >= it.r1 || it.r1 > H || it.nsteps < 1 ||
            it.nsteps != cdiv(it.r1 - it.r0, CF_FWD_TH)) {
            fail("fwd decode", N, H, W, item, it.nsteps);
            continue;
        }
        if (it.img != item / (grid / N)) fail("fwd: an image's rows are not contiguous", N, H, W, item, it.img);
        for (int s = 0; s < it.nsteps; ++s)                                     // step s: rows r0 + 8 s .. + 7, cut at the segment's end
            for (int y = it.r0 + CF_FWD_TH * s; y < min(it.r1, it.r0 + CF_FWD_TH * (s + 1)); ++y) ++cover[((size_t)it.img * p.strips + it.x0 / CF_FWD_TW) * H + y];
        steps += it.nsteps;
    }
    for (size_t i = 0; i < cover.size(); ++i)
        if (cover[i] != 1) { fail("fwd steps do not cover (image, strip, row) once", N, H, W, (long)i, cover[i]); break; }
    return steps;
}

static void expect_wgrad(int N, int H, int W, int strips, int nseg, int seg_rows, long items, int blocks) {
    const CfWgradPlan p = conv_first_wgrad_plan(N, H, W);
    if (p.strips != strips || p.nseg != nseg || p.seg_rows != seg_rows) fail("pinned wgrad plan", N, H, W, p.nseg, p.seg_rows);
    if (p.items != items || p.blocks != blocks) fail("pinned wgrad items / blocks", N, H, W, p.items, p.blocks);
}
static void expect_fwd(int N, int H, int W, int seg_rows, int grid) {
    const CfFwdPlan p = conv_first_fwd_plan(N, H, W);
    if (p.seg_rows != seg_rows || conv_first_fwd_grid(N, p) != grid) fail("pinned fwd plan", N, H, W, p.seg_rows, conv_first_fwd_grid(N, p));
}

int main(int argc, char** argv) {
    const bool print = argc > 1 && !std::strcmp(argv[1], "rows");
    std::vector<int> cover;
    long shapes = 0, ok16 = 0, ok32 = 0, items = 0, steps = 0;
    for (int N = 1; N <= 96; ++N)
        for (int W : Ws)
            for (int H : Hs) {
                const long i16 = check_wgrad(N, H, W, 2, cover), i32 = check_wgrad(N, H, W, 4, cover);
                ok16 += i16 > 0; ok32 += i32 > 0; items += i16 + i32;
                steps += check_fwd(N, H, W, print, cover);
                ++shapes;
            }
    std::printf("sweep: N = 1..96 x 7 widths x 8 heights, %ld shapes\n", shapes);
    std::printf("weight gradient: %ld shapes stream with 16-bit dY, %ld with f32 dY, %ld items\n", ok16, ok32, items);
    std::printf("forward: %ld steps\n", steps);

    // the predicate: what it must refuse
    {
        ustrun_src_t s = nchw(3, 64, 64);
        if (!conv_first_wgrad_stream_ok(s, 4, 64, 64, 2)) fail("predicate: dense NCHW refused", 4, 64, 64, 0, 0);
        ustrun_src_t t = s; t.sW = 2;
        if (conv_first_wgrad_stream_ok(t, 4, 64, 64, 2)) fail("predicate: pixel stride 2", 4, 64, 64, 0, 0);
        t = s; t.f32 = 0;
        if (conv_first_wgrad_stream_ok(t, 4, 64, 64, 2)) fail("predicate: 16-bit source", 4, 64, 64, 0, 0);
        t = s; t.sH = 80; t.sC = 64 * 80; t.sN = 3 * 64 * 80;                       // a row pitch above W, dense above the row: the kernel strides rows by sH
        if (!conv_first_wgrad_stream_ok(t, 4, 64, 64, 2)) fail("predicate: row pitch above W refused", 4, 64, 64, 0, 0);
        t = s; t.sN = s.sN + 1;
        if (conv_first_wgrad_stream_ok(t, 4, 64, 64, 2)) fail("predicate: image stride != C sC", 4, 64, 64, 0, 0);
        t = s; t.sC = s.sC + 64; t.sN = 3 * t.sC;
        if (conv_first_wgrad_stream_ok(t, 4, 64, 64, 2)) fail("predicate: channel stride != H sH", 4, 64, 64, 0, 0);
        s = nchw(3, 256, 256);                                                      // dY bytes: 2^31 at N = 128 (f32) / 256 (16-bit)
        if (!conv_first_wgrad_stream_ok(s, 127, 256, 256, 4) || conv_first_wgrad_stream_ok(s, 128, 256, 256, 4)) fail("predicate: f32 dY at 2^31 bytes", 128, 256, 256, 0, 0);
        if (!conv_first_wgrad_stream_ok(s, 255, 256, 256, 2) || conv_first_wgrad_stream_ok(s, 256, 256, 256, 2)) fail("predicate: 16-bit dY at 2^31 bytes", 256, 256, 256, 0, 0);
        s = nchw(1, 8, 16 * 4097);                                                  // more strips than items
        if (conv_first_wgrad_stream_ok(s, 1, 8, 16 * 4097, 2)) fail("predicate: 4097 items", 1, 8, 16 * 4097, 0, 0);
        s = nchw(1, 8, 16 * 4096);
        if (!conv_first_wgrad_stream_ok(s, 1, 8, 16 * 4096, 2)) fail("predicate: 4096 items refused", 1, 8, 16 * 4096, 0, 0);
    }

    // the workload's shapes (3 x 256 x 256), as literals
    expect_wgrad(16, 256, 256, 16, 16, 16, 4096, 1024);
    expect_wgrad(64, 256, 256, 16, 4, 64, 4096, 1024);
    expect_fwd(16, 256, 256, 32, 1024);
    expect_fwd(64, 256, 256, 64, 2048);
    std::printf("pinned: weight gradient and forward plans at N = 16 and 64, 3 x 256 x 256\n");

    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
