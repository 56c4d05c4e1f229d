// Host-only replay of ust-run_amd/csrc/morph_plan.h (tests/test_morph_plan_host.py): the helpers of the chamfer / morphology
// kernels, called in the kernels' pass order -- row pass with its chunk carry, L1 recurrence or L-inf search along y, then along z --
// over small boxes, against a brute force over all pairs in 64-bit integers; then the thresholds, the grid folding and the limits.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../ust-run_amd/csrc/morph_plan.h"

using namespace ustrun::morph;

static int failures = 0;
#define EXPECT(cond, ...)                         \
    do {                                          \
        if (!(cond)) {                            \
            if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            ++failures;                           \
        }                                         \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

struct Box { int rank, D, H, W; };

// brute force: the distance of every voxel to the set, all pairs, int64; `outside`: the outside of the box is part of the set.
// rank 2: z is no axis (D == 1 and no border along it)
static std::vector<int64_t> brute(const Box& b, const std::vector<char>& set, int metric, bool outside) {
    const int64_t none = (int64_t)1 << 40;
    std::vector<int64_t> out((size_t)b.D * b.H * b.W, none);
    for (int z = 0; z < b.D; ++z)
        for (int y = 0; y < b.H; ++y)
            for (int x = 0; x < b.W; ++x) {
                int64_t best = none;
                for (int zz = 0; zz < b.D; ++zz)
                    for (int yy = 0; yy < b.H; ++yy)
                        for (int xx = 0; xx < b.W; ++xx) {
                            if (!set[((size_t)zz * b.H + yy) * b.W + xx]) continue;
                            const int64_t dz = llabs((long long)z - zz), dy = llabs((long long)y - yy), dx = llabs((long long)x - xx);
                            const int64_t d = metric == METRIC_L1 ? dz + dy + dx : (dz > dy ? (dz > dx ? dz : dx) : (dy > dx ? dy : dx));
                            if (d < best) best = d;
                        }
                if (outside) {
                    int64_t o = x + 1 < b.W - x ? x + 1 : b.W - x;
                    const int64_t oy = y + 1 < b.H - y ? y + 1 : b.H - y;
                    if (oy < o) o = oy;
                    if (b.rank == 3) { const int64_t oz = z + 1 < b.D - z ? z + 1 : b.D - z; if (oz < o) o = oz; }
                    if (o < best) best = o;
                }
                out[((size_t)z * b.H + y) * b.W + x] = best;
            }
    return out;
}

// the kernels' passes over one kind of one volume: a = buffer A, bb = buffer B; returns the final distances
static std::vector<int> replay(const Box& b, const std::vector<char>& set, int metric, bool outside, int cap) {
    const long HW = (long)b.H * b.W, DHW = HW * b.D;
    std::vector<unsigned short> a((size_t)DHW), bb((size_t)DHW);
    const int nch = (b.W + 63) >> 6;
    // pass 1: one "wave" per row -- a ballot per chunk, then every lane of every chunk
    for (long r = 0; r < (long)b.D * b.H; ++r) {
        unsigned long long masks[ROW_CHUNKS] = {0};
        for (int j = 0; j < nch; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const int x = j * 64 + lane;
                if (x < b.W && set[(size_t)(r * b.W + x)]) masks[j] |= 1ull << lane;
            }
        for (int j = 0; j < nch; ++j) {
            const int left = chunk_carry_left(masks, j, outside), right = chunk_carry_right(masks, j, nch, b.W, outside);
            for (int lane = 0; lane < 64; ++lane) {
                const int x = j * 64 + lane;
                if (x < b.W) a[(size_t)(r * b.W + x)] = (unsigned short)row_dist(masks[j], lane, x, left, right, cap);
            }
        }
    }
    bool any = outside;
    for (char s : set) any |= s != 0;
    unsigned short* src = a.data();
    // pass 2 (rank 3): along y, per slice and column
    if (b.rank == 3) {
        for (int z = 0; z < b.D; ++z)
            for (int x = 0; x < b.W; ++x) {
                unsigned short* p = a.data() + z * HW + x;
                if (metric == METRIC_L1) {
                    int d = l1_start(outside, cap);
                    for (int y = 0; y < b.H; ++y) { d = l1_step(d, p[(long)y * b.W], cap); p[(long)y * b.W] = (unsigned short)d; }
                    d = l1_start(outside, cap);
                    for (int y = b.H - 1; y >= 0; --y) { d = l1_step(d, p[(long)y * b.W], cap); p[(long)y * b.W] = (unsigned short)d; }
                } else {
                    for (int y = 0; y < b.H; ++y) bb[(size_t)(z * HW + x + (long)y * b.W)] = (unsigned short)(any ? linf_at(p, b.W, y, b.H, cap, outside) : cap);
                }
            }
        if (metric == METRIC_LINF) src = bb.data();
    }
    // pass 3: along the last axis
    const int n = last_len(b.rank, b.D, b.H);
    const long stride = (long)last_stride(b.rank, b.H, b.W), lines = stride;
    std::vector<int> out((size_t)DHW);
    for (long q = 0; q < lines; ++q) {
        unsigned short* p = src + q;
        if (metric == METRIC_L1) {
            int d = l1_start(outside, cap);
            for (int i = 0; i < n; ++i) { d = l1_step(d, p[i * stride], cap); p[i * stride] = (unsigned short)d; }
            d = l1_start(outside, cap);
            for (int i = n - 1; i >= 0; --i) { d = l1_step(d, p[i * stride], cap); out[(size_t)(q + i * stride)] = d; }
        } else {
            for (int i = 0; i < n; ++i) out[(size_t)(q + i * stride)] = any ? linf_at(p, stride, i, n, cap, outside) : cap;
        }
    }
    return out;
}

static void check_box(const Box& b, double density, int& boxes) {
    const size_t n = (size_t)b.D * b.H * b.W;
    std::vector<char> set(n);
    for (size_t i = 0; i < n; ++i) set[i] = density >= 1.0 ? 1 : (rnd() / 4294967296.0 < density);
    const int caps[] = {CAP_INF, morph_cap(1), morph_cap(2), morph_cap(5), morph_cap(WIDTH_MAX)};
    for (int metric = 0; metric < 2; ++metric)
        for (int outside = 0; outside < 2; ++outside) {
            const std::vector<int64_t> want = brute(b, set, metric, outside != 0);
            for (int cap : caps) {
                const std::vector<int> got = replay(b, set, metric, outside != 0, cap);
                for (size_t i = 0; i < n; ++i) {
                    const int64_t w = want[i] < cap ? want[i] : cap;
                    EXPECT(got[i] == w, "rank %d box %dx%dx%d density %.2f metric %d outside %d cap %d voxel %zu: got %d want %lld", b.rank,
                           b.D, b.H, b.W, density, metric, outside, cap, i, got[i], (long long)w);
                }
            }
        }
    ++boxes;
}

int main() {
    // ---- the passes against the brute force
    const Box shapes[] = {{2, 1, 1, 1}, {2, 1, 1, 7}, {2, 1, 7, 1}, {2, 1, 9, 13}, {2, 1, 5, 70}, {2, 1, 3, 130}, {2, 1, 12, 64},
                          {3, 1, 5, 6}, {3, 2, 9, 4}, {3, 5, 6, 7}, {3, 3, 4, 66}, {3, 1, 1, 1}};
    const double densities[] = {0.0, 0.03, 0.3, 0.9, 1.0};
    int boxes = 0;
    for (const Box& b : shapes)
        for (double dens : densities) check_box(b, dens, boxes);
    // one pixel in each corner of a plane wider than two chunks
    {
        const Box b{2, 1, 4, 131};
        const int at[4] = {0, 130, 3 * 131, 3 * 131 + 130};
        for (int c = 0; c < 4; ++c) {
            std::vector<char> set((size_t)4 * 131, 0);
            set[at[c]] = 1;
            for (int metric = 0; metric < 2; ++metric) {
                const std::vector<int64_t> want = brute(b, set, metric, false);
                const std::vector<int> got = replay(b, set, metric, false, CAP_INF);
                for (size_t i = 0; i < set.size(); ++i) EXPECT(got[i] == want[i], "corner %d metric %d pixel %zu: got %d want %lld", c, metric, i, got[i], (long long)want[i]);
            }
        }
    }
    // ---- the chunk carry on its own: a row of 1024 with single set pixels
    {
        for (int trial = 0; trial < 200; ++trial) {
            const int W = 1 + rnd() % 1024, nch = (W + 63) >> 6, npix = rnd() % 4;
            unsigned long long masks[ROW_CHUNKS] = {0};
            std::vector<int> pos;
            for (int k = 0; k < npix; ++k) { const int x = rnd() % W; pos.push_back(x); masks[x >> 6] |= 1ull << (x & 63); }
            for (int outside = 0; outside < 2; ++outside)
                for (int x = 0; x < W; ++x) {
                    int want = CAP_INF;
                    for (int p : pos) want = imin(want, abs(x - p));
                    if (outside) want = imin(want, imin(x + 1, W - x));
                    const int j = x >> 6;
                    const int got = row_dist(masks[j], x & 63, x, chunk_carry_left(masks, j, outside), chunk_carry_right(masks, j, nch, W, outside), CAP_INF);
                    EXPECT(got == want, "carry: W %d x %d outside %d: got %d want %d", W, x, outside, got, want);
                }
        }
    }
    // ---- thresholds and codes
    EXPECT(morph_bit(OP_DILATE, 3, 0, 3) == 1 && morph_bit(OP_DILATE, 4, 0, 3) == 0, "dilation threshold");
    EXPECT(morph_bit(OP_ERODE, 0, 4, 3) == 1 && morph_bit(OP_ERODE, 0, 3, 3) == 0, "erosion threshold");
    EXPECT(morph_bit(OP_BAND, 2, 0, 3) == 1 && morph_bit(OP_BAND, 0, 4, 3) == 0 && morph_bit(OP_BAND, 4, 0, 3) == 0 && morph_bit(OP_BAND, 0, 3, 3) == 1, "band");
    EXPECT(signed_of(0, 5, 0x7fffffff) == -5 && signed_of(7, 0, 0x7fffffff) == 7, "signs");
    EXPECT(signed_of(0, CAP_INF, 0x7fffffff) == -0x7fffffff && signed_of(CAP_INF, 0, 0x7fffffff) == 0x7fffffff, "sentinels");
    EXPECT(kinds_of(OP_DILATE) == KIND_FG && kinds_of(OP_ERODE) == KIND_BG && kinds_of(OP_BAND) == 3, "kinds");
    EXPECT(first_round(OP_OPEN) == OP_ERODE && second_round(OP_OPEN) == OP_DILATE && first_round(OP_CLOSE) == OP_DILATE &&
           second_round(OP_CLOSE) == OP_ERODE && second_round(OP_BAND) < 0 && first_round(OP_BAND) == OP_BAND, "rounds");
    EXPECT(outside_of_border(0) == OUTSIDE_BG && outside_of_border(1) == OUTSIDE_FG, "border codes");
    EXPECT(outside_is(OUTSIDE_BG, 1) && !outside_is(OUTSIDE_BG, 0) && outside_is(OUTSIDE_FG, 0) && !outside_is(OUTSIDE_FG, 1) &&
           !outside_is(OUTSIDE_NONE, 0) && !outside_is(OUTSIDE_NONE, 1), "outside kinds");
    // ---- the grid folding: every group is taken exactly once
    {
        const int64_t items[] = {1, 3, 4, 5, 65535, 65536, 75000, 600000, ((int64_t)1 << 22) + 5, 32767ll * 1024};
        const int pers[] = {1, 4};
        const int capsf[] = {GRID_Y_MAX, GRID_X_FOLD};
        for (int64_t it : items)
            for (int per : pers)
                for (int cap : capsf) {
                    const int blocks = fold_blocks(it, per, cap);
                    const int64_t groups = (it + per - 1) / per;
                    EXPECT(blocks >= 1 && blocks <= cap && blocks <= groups, "fold: %lld items per %d cap %d -> %d blocks", (long long)it, per, cap, blocks);
                    int64_t taken = 0;                  // block b walks b, b + blocks, ...: count the groups below `groups`
                    for (int b = 0; b < blocks; b += (blocks > 4096 ? blocks / 64 : 1)) taken += (groups - b + blocks - 1) / blocks;
                    if (blocks <= 4096) EXPECT(taken == groups, "fold: %lld groups, %lld taken", (long long)groups, (long long)taken);
                }
    }
    // ---- the limits
    EXPECT(rank_ok(2, 1) && !rank_ok(2, 2) && rank_ok(3, 1) && rank_ok(3, 7) && !rank_ok(1, 1) && !rank_ok(4, 1), "rank");
    EXPECT(sizes_ok(1, 1, 1, 1, 1) && sizes_ok(32767, 1, 1024, 1024, 1024) && !sizes_ok(32768, 1, 1, 1, 1) && !sizes_ok(1, 1, 1025, 1, 1) &&
           !sizes_ok(1, 1, 1, 0, 1) && !sizes_ok(0, 1, 1, 1, 1) && !sizes_ok(1, 1, 1, 1, 1025) && !sizes_ok(181, 182, 1, 1, 1), "sizes");
    EXPECT(voxels_ok(128, 1024, 1024) && !voxels_ok(129, 1024, 1024), "voxels");
    EXPECT(width_ok(1) && width_ok(4095) && !width_ok(0) && !width_ok(4096) && !width_ok(-1), "width");
    EXPECT(morph_cap(WIDTH_MAX) == CAP_INF && DIST_MAX < CAP_INF && DIST_MAX == 3069, "cap");
    EXPECT(metric_ok(0) && metric_ok(1) && !metric_ok(2) && !metric_ok(-1) && outside_ok(0) && outside_ok(2) && !outside_ok(3) &&
           !outside_ok(-1) && op_ok(0) && op_ok(4) && !op_ok(5) && !op_ok(-1) && border_ok(0) && border_ok(1) && !border_ok(2), "codes");
    EXPECT(last_len(2, 1, 9) == 9 && last_len(3, 5, 9) == 5 && last_stride(2, 9, 13) == 13 && last_stride(3, 9, 13) == 117, "last axis");

    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("all checks passed: %d boxes x 2 metrics x 2 outside x 5 caps\n", boxes);
    return 0;
}
