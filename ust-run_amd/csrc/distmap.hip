// Signed distance maps of label planes on the device (include/ustrun.h: ustrun_signed_dist2, ustrun_sdf_from_dist2): what the
// reference's compute_sdf (utils/util.py:208-239) takes from two scipy.ndimage.distance_transform_edt calls per image on the
// host, for all N x K planes of a batch, in exact integer arithmetic up to the final normalisation.
//
//   s2(p) = + min over foreground q of |p - q|^2   at a background pixel p
//           - min over background q of |p - q|^2   at a foreground pixel p        (q inside the image only: scipy's convention)
//
// ustrun_signed_dist2, three launches over all planes:
//   1 seed_kernel     col[plane][0] = 0 on foreground, col[plane][1] = 0 on background, COL_INF elsewhere (u16)
//   2 colscan_kernel  (edt_scan.h) both maps in place: distance along the column to the nearest pixel of that kind
//   3 signed_row_kernel  one wave per row, one lane per pixel: d2 = min over x' of col_opposite[x']^2 + (x - x')^2, searched
//                     outwards from x while (x - x')^2 can still win (exact: what is left out is >= the minimum).  A row whose
//                     opposite map has no finite entry belongs to a plane without that kind (a pixel of it anywhere in the plane
//                     would give its column a finite entry in every row): no search, +- USTRUN_DIST_NONE.  Row 0 writes the flag.
// ustrun_sdf_from_dist2, two launches (edt_scan.h: planemax_kernel, normalise_kernel, shared with edt3d.hip): the integer maxima of both signs per plane (atomicMax: exact, order-free), then
//   sdf = sqrt(neg) / sqrt(maxneg) - sqrt(pos) / sqrt(maxpos) per pixel in f64, rounded to f32 once.
// No floating-point reduction anywhere: two runs give the same bits.
#include "common.h"
#include "edt_scan.h"        // COL_INF, SURF_MAX, fg_at, colscan_kernel, planemax_kernel, normalise_kernel

namespace ustrun {
namespace {

constexpr int ROWS_PER_BLOCK = 4;        // signed_row_kernel: one wave per row
constexpr int64_t MAX_PLANES = 65535 / 2;

static inline int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

int64_t dist_work_bytes(int64_t NK, int64_t H, int64_t W) { return up16(NK * 2 * H * W * 2); }      // col[NK][2][HW] u16
int64_t sdf_work_bytes(int64_t NK) { return up16(NK * 2 * 4); }                                     // {maxpos, maxneg}[NK] int32

bool sizes_ok(int N, int K, int H, int W) {
    return N > 0 && K > 0 && H >= 1 && W >= 1 && H <= SURF_MAX && W <= SURF_MAX && (int64_t)N * K <= MAX_PLANES;
}

// grid (ceil(HW / 256), N * K)
__global__ __launch_bounds__(256) void seed_kernel(const void* mask, int is64, int K, int by_class, int H, int W,
                                                  unsigned short* __restrict__ col) {
    const int plane = blockIdx.y, n = plane / K, c = plane % K;
    const long HW = (long)H * W, base = by_class ? (long)n * HW : (long)plane * HW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= HW) return;
    const bool fg = fg_at(mask, is64, by_class, base, c, e);
    unsigned short* o = col + (long)plane * 2 * HW;
    o[e] = fg ? 0 : COL_INF;
    o[HW + e] = fg ? COL_INF : 0;
}

// grid (ceil(H / 4), N * K), 256 threads: wave w takes row 4 * blockIdx.x + w
__global__ __launch_bounds__(256) void signed_row_kernel(int H, int W, const unsigned short* __restrict__ col, int* __restrict__ s2,
                                                        int* __restrict__ flags) {
    __shared__ unsigned short row[ROWS_PER_BLOCK][2][SURF_MAX];
    const int plane = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.x * ROWS_PER_BLOCK + wave;
    const long HW = (long)H * W;
    bool fin[2] = {false, false};        // the row's map of that kind has a finite entry <=> the plane has a pixel of that kind
    if (y < H)
        for (int side = 0; side < 2; ++side)
            for (int x = lane; x < W; x += 64) {
                const unsigned short v = col[((long)plane * 2 + side) * HW + (long)y * W + x];
                row[wave][side][x] = v;
                fin[side] |= v < COL_INF;
            }
    const bool has_fg = __ballot(fin[0]) != 0, has_bg = __ballot(fin[1]) != 0;
    __syncthreads();
    if (y >= H) return;
    if (y == 0 && lane == 0) flags[plane] = has_fg ? (has_bg ? 1 : 2) : 0;
    int* out = s2 + (long)plane * HW + (long)y * W;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        if (x >= W) continue;
        const bool fg = row[wave][0][x] == 0;
        const unsigned short* other = row[wave][fg ? 1 : 0];
        int best = USTRUN_DIST_NONE;
        if (fg ? has_bg : has_fg) {
            const int g = other[x];
            best = g * g;
            for (int dx = 1; dx * dx < best; ++dx) {
                const int xl = x - dx, xr = x + dx;
                if (xl < 0 && xr >= W) break;
                if (xl >= 0) { const int v = other[xl]; best = min(best, v * v + dx * dx); }
                if (xr < W) { const int v = other[xr]; best = min(best, v * v + dx * dx); }
            }
        }
        out[x] = fg ? -best : best;
    }
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int64_t ustrun_signed_dist2_work_bytes(int N, int K, int H, int W) {
    if (!sizes_ok(N, K, H, W)) {
        set_error("signed_dist2_work_bytes: N, K > 0, N * K <= %lld and H, W in 1..%d, got N %d K %d H %d W %d",
                  (long long)MAX_PLANES, SURF_MAX, N, K, H, W);
        return -1;
    }
    return dist_work_bytes((int64_t)N * K, H, W);
}

extern "C" int ustrun_signed_dist2(const void* mask, int mask_is_i64, int N, int K, int by_class, int H, int W, void* work,
                                   int64_t work_bytes, int32_t* s2, int32_t* flags, ustrun_stream_t s) {
    USTRUN_CHECK(mask && work && s2 && flags, "signed_dist2: null pointer (mask %p work %p s2 %p flags %p)", mask, work,
                 (void*)s2, (void*)flags);
    USTRUN_CHECK(sizes_ok(N, K, H, W), "signed_dist2: N, K > 0, N * K <= %lld and H, W in 1..%d, got N %d K %d H %d W %d",
                 (long long)MAX_PLANES, SURF_MAX, N, K, H, W);
    const int64_t NK = (int64_t)N * K;
    USTRUN_CHECK(work_bytes >= dist_work_bytes(NK, H, W), "signed_dist2: work buffer of %lld bytes, needs %lld",
                 (long long)work_bytes, (long long)dist_work_bytes(NK, H, W));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)s2 & 3) == 0 && ((uintptr_t)flags & 3) == 0,
                 "signed_dist2: work must be 16-byte, s2 and flags 4-byte aligned");
    unsigned short* col = (unsigned short*)work;
    const hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(seed_kernel, dim3(cdiv((int64_t)H * W, 256), NK), dim3(256), 0, st, mask, mask_is_i64, K, by_class, H, W, col);
    USTRUN_LAUNCH_CHECK("signed_dist2: seed");
    hipLaunchKernelGGL(colscan_kernel, dim3(cdiv(W, 64), NK * 2), dim3(64), 0, st, H, W, col);
    USTRUN_LAUNCH_CHECK("signed_dist2: column scan");
    hipLaunchKernelGGL(signed_row_kernel, dim3(cdiv(H, ROWS_PER_BLOCK), NK), dim3(256), 0, st, H, W, col, s2, flags);
    USTRUN_LAUNCH_CHECK("signed_dist2: row minimum");
    return 0;
}

extern "C" int64_t ustrun_sdf_from_dist2_work_bytes(int N, int K, int H, int W) {
    if (!sizes_ok(N, K, H, W)) {
        set_error("sdf_from_dist2_work_bytes: N, K > 0, N * K <= %lld and H, W in 1..%d, got N %d K %d H %d W %d",
                  (long long)MAX_PLANES, SURF_MAX, N, K, H, W);
        return -1;
    }
    return sdf_work_bytes((int64_t)N * K);
}

extern "C" int ustrun_sdf_from_dist2(const int32_t* s2, const int32_t* flags, int N, int K, int H, int W, void* work,
                                     int64_t work_bytes, float* sdf, ustrun_stream_t s) {
    USTRUN_CHECK(s2 && flags && work && sdf, "sdf_from_dist2: null pointer (s2 %p flags %p work %p sdf %p)", (const void*)s2,
                 (const void*)flags, work, (void*)sdf);
    USTRUN_CHECK(sizes_ok(N, K, H, W), "sdf_from_dist2: N, K > 0, N * K <= %lld and H, W in 1..%d, got N %d K %d H %d W %d",
                 (long long)MAX_PLANES, SURF_MAX, N, K, H, W);
    const int64_t NK = (int64_t)N * K, HW = (int64_t)H * W;
    USTRUN_CHECK(work_bytes >= sdf_work_bytes(NK), "sdf_from_dist2: work buffer of %lld bytes, needs %lld", (long long)work_bytes,
                 (long long)sdf_work_bytes(NK));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)s2 & 3) == 0 && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)sdf & 3) == 0,
                 "sdf_from_dist2: work must be 16-byte, s2, flags and sdf 4-byte aligned");
    int* mx = (int*)work;
    const hipStream_t st = (hipStream_t)s;
    const hipError_t e = hipMemsetAsync(mx, 0, sizeof(int) * 2 * NK, st);
    USTRUN_CHECK(e == hipSuccess, "sdf_from_dist2: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(planemax_kernel, dim3(cdiv(HW, MAX_PER_BLOCK), NK), dim3(256), 0, st, (long)HW, s2, flags, mx);
    USTRUN_LAUNCH_CHECK("sdf_from_dist2: plane maxima");
    hipLaunchKernelGGL(normalise_kernel, dim3(cdiv(HW, 256), NK), dim3(256), 0, st, (long)HW, s2, flags, mx, sdf);
    USTRUN_LAUNCH_CHECK("sdf_from_dist2: normalise");
    return 0;
}
