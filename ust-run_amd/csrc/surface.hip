// Surface-distance metrics of the validation path on the device (include/ustrun.h: ustrun_surface_metrics): what the
// reference takes from medpy.metric.binary (hd95, asd; train.py:306-325) per (sample, part), up to the final square roots of
// the two order statistics, in exact integer arithmetic.
//
//   border(A)   = A & ~erode(A), 4-neighbour cross, outside the image = background
//   sds(A, B)   = Euclidean distance from every pixel of border(A) to the nearest pixel of border(B)
//   hd95        = percentile 95 (linear) of sds(P,G) u sds(G,P);   asd = mean(sds(P,G))
//
// Four launches over all N x K planes, both sides (0: prediction, 1: ground truth) in each:
//   1 border_kernel   col[plane][side][y][x] = 0 on a border pixel, COL_INF elsewhere (u16)
//   2 colscan_kernel  (edt_scan.h, shared with distmap.hip) in place: distance along the column to the nearest border pixel of that side, capped at COL_INF
//   3 rowmin_kernel   one wave per row: at every border pixel x of one side, d2 = min over x' of col_other[x']^2 + (x-x')^2,
//                     searched outwards from x until (x-x')^2 can no longer win (exact: the candidates left out are >= the minimum);
//                     the values are appended to that side's list (integer wave-aggregated counter: the order in the list is
//                     not fixed, nothing order-dependent reads it), the row's sum of sqrt(d2) over border(P) goes to rowsum[y]
//   4 select_kernel   one block per plane: two-level histogram select (11 + 10 bits: d2 < 2^21 for H, W <= 1024) of the ranks
//                     k = floor(0.95 (n-1)) and min(k+1, n-1) of the union, and the row sums added in row order
// The f64 sum is a fixed tree (lane's pixels in x order, xor butterfly, rows in y order, butterfly, waves in order): no
// floating-point atomics, two runs give the same bits.
#include "common.h"
#include "edt_scan.h"        // COL_INF, SURF_MAX, fg_at, colscan_kernel

namespace ustrun {
namespace {

constexpr int L1_BITS = 11, L2_BITS = 10;
constexpr int ROWS_PER_BLOCK = 4;        // rowmin_kernel: one wave per row

struct SurfWork {
    double* rowsum;          // [NK][H]      sum of sqrt(d2) over the row's border(P) pixels
    int* d2;                 // [NK][2][HW]  side's distances, the first cnt[plane][side] entries
    int* cnt;                // [NK][2]      |border(P)|, |border(G)|  (zeroed every call)
    unsigned short* col;     // [NK][2][HW]
};

static inline int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

int64_t surf_work_bytes(int64_t NK, int64_t H, int64_t W) {
    return up16(NK * H * 8) + up16(NK * 2 * H * W * 4) + up16(NK * 2 * 4) + up16(NK * 2 * H * W * 2);
}

SurfWork surf_carve(void* work, int64_t NK, int64_t H, int64_t W) {
    char* p = (char*)work;
    SurfWork w;
    w.rowsum = (double*)p; p += up16(NK * H * 8);
    w.d2 = (int*)p; p += up16(NK * 2 * H * W * 4);
    w.cnt = (int*)p; p += up16(NK * 2 * 4);
    w.col = (unsigned short*)p;
    return w;
}

__device__ __forceinline__ bool border_at(const void* m, int is64, int by_class, long base, int c, int y, int x, int H, int W) {
    const long e = (long)y * W + x;
    if (!fg_at(m, is64, by_class, base, c, e)) return false;
    if (y == 0 || x == 0 || y == H - 1 || x == W - 1) return true;       // a neighbour outside the image is background
    return !(fg_at(m, is64, by_class, base, c, e - W) && fg_at(m, is64, by_class, base, c, e + W) &&
             fg_at(m, is64, by_class, base, c, e - 1) && fg_at(m, is64, by_class, base, c, e + 1));
}

// grid (ceil(HW / 256), N * K)
__global__ __launch_bounds__(256) void border_kernel(const void* pred, const void* gt, int pi64, int gi64, int K, int by_class,
                                                    int H, int W, unsigned short* __restrict__ col) {
    const int plane = blockIdx.y, n = plane / K, c = plane % K;
    const long HW = (long)H * W, base = by_class ? (long)n * HW : (long)plane * HW;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= HW) return;
    const int y = (int)(e / W), x = (int)(e % W);
    unsigned short* o = col + (long)plane * 2 * HW;
    o[e] = border_at(pred, pi64, by_class, base, c, y, x, H, W) ? 0 : COL_INF;
    o[HW + e] = border_at(gt, gi64, by_class, base, c, y, x, H, W) ? 0 : COL_INF;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (ceil(H / 4), N * K), 256 threads: wave w takes row 4 * blockIdx.x + w
__global__ __launch_bounds__(256) void rowmin_kernel(int H, int W, const unsigned short* __restrict__ col, int* __restrict__ d2,
                                                    int* __restrict__ cnt, double* __restrict__ rowsum) {
    __shared__ unsigned short row[ROWS_PER_BLOCK][2][SURF_MAX];
    const int plane = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.x * ROWS_PER_BLOCK + wave;
    const long HW = (long)H * W;
    if (y < H)
        for (int side = 0; side < 2; ++side)
            for (int x = lane; x < W; x += 64) row[wave][side][x] = col[((long)plane * 2 + side) * HW + (long)y * W + x];
    __syncthreads();
    if (y >= H) return;
    double acc = 0.0;
    for (int side = 0; side < 2; ++side) {
        const unsigned short* mine = row[wave][side];
        const unsigned short* other = row[wave][1 - side];
        int* list = d2 + ((long)plane * 2 + side) * HW;
        for (int x0 = 0; x0 < W; x0 += 64) {
            const int x = x0 + lane;
            const bool on = x < W && mine[x] == 0;
            int best = 0;
            if (on) {
                const int g = other[x];
                best = g * g;
                for (int dx = 1; dx * dx < best; ++dx) {
                    const int xl = x - dx, xr = x + dx;
                    if (xl < 0 && xr >= W) break;
                    if (xl >= 0) { const int v = other[xl]; best = min(best, v * v + dx * dx); }
                    if (xr < W) { const int v = other[xr]; best = min(best, v * v + dx * dx); }
                }
                if (side == 0) acc += sqrt((double)best);
            }
            const unsigned long long m = __ballot(on);
            if (m) {
                int at = 0;
                if (lane == 0) at = atomicAdd(&cnt[plane * 2 + side], __popcll(m));
                at = __shfl(at, 0) + __popcll(m & ((1ull << lane) - 1ull));
                if (on && at < HW) list[at] = best;          // (at < HW always: a plane has at most HW border pixels)
            }
        }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) rowsum[(long)plane * H + y] = acc;
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

// grid (N * K), 256 threads.  out record: int32 {|border(P)|, |border(G)|, d2[k], d2[k+1]}, f64 sum of sqrt(d2) over border(P)
__global__ __launch_bounds__(256) void select_kernel(int H, int W, const int* __restrict__ d2, const int* __restrict__ cnt,
                                                    const double* __restrict__ rowsum, int* __restrict__ out) {
    __shared__ int hist[1 << L1_BITS];
    __shared__ int hist2[2][1 << L2_BITS];
    __shared__ int part[256];
    __shared__ int res[2];
    __shared__ double wsum[4];
    const int plane = blockIdx.x, t = threadIdx.x;
    const long HW = (long)H * W;
    const int n0 = cnt[plane * 2], n1 = cnt[plane * 2 + 1], n = n0 + n1;
    const int* l0 = d2 + (long)plane * 2 * HW;
    const int* l1 = l0 + HW;
    int* rec = out + (long)plane * 6;
    if (n0 == 0 || n1 == 0) {            // an empty mask: no distance exists; the host applies the reference's rules from the counts
        if (t == 0) { rec[0] = n0; rec[1] = n1; rec[2] = 0; rec[3] = 0; *(double*)(rec + 4) = 0.0; }
        return;
    }
    double acc = 0.0;
    for (int y = t; y < H; y += 256) acc += rowsum[(long)plane * H + y];
    acc = wave_sum_f64(acc);
    if ((t & 63) == 0) wsum[t >> 6] = acc;

    const int vmax = (1 << (L1_BITS + L2_BITS)) - 1;
    for (int i = t; i < (1 << L1_BITS); i += 256) hist[i] = 0;
    for (int i = t; i < (2 << L2_BITS); i += 256) (&hist2[0][0])[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const int v = min(i < n0 ? l0[i] : l1[i - n0], vmax);
        atomicAdd(&hist[v >> L2_BITS], 1);
    }
    __syncthreads();
    const int k = (int)floor(0.95 * (double)(n - 1));          // numpy's linear method: position 0.95 (n - 1), in f64
    const int k1 = min(k + 1, n - 1);
    find_rank(hist, (1 << L1_BITS) / 256, k, part, res);
    const int bk = res[0], rk = res[1];
    __syncthreads();
    find_rank(hist, (1 << L1_BITS) / 256, k1, part, res);
    const int bk1 = res[0], rk1 = res[1];
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const int v = min(i < n0 ? l0[i] : l1[i - n0], vmax);
        const int hi = v >> L2_BITS, lo = v & ((1 << L2_BITS) - 1);
        if (hi == bk) atomicAdd(&hist2[0][lo], 1);
        if (hi == bk1) atomicAdd(&hist2[1][lo], 1);
    }
    __syncthreads();
    find_rank(hist2[0], (1 << L2_BITS) / 256, rk, part, res);
    const int vk = (bk << L2_BITS) | res[0];
    __syncthreads();
    find_rank(hist2[1], (1 << L2_BITS) / 256, rk1, part, res);
    const int vk1 = (bk1 << L2_BITS) | res[0];
    if (t == 0) {
        rec[0] = n0; rec[1] = n1; rec[2] = vk; rec[3] = vk1;
        *(double*)(rec + 4) = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int64_t ustrun_surface_metrics_work_bytes(int N, int K, int H, int W) {
    if (N <= 0 || K <= 0 || H < 1 || W < 1 || H > SURF_MAX || W > SURF_MAX) {
        set_error("surface_metrics_work_bytes: N, K > 0 and H, W in 1..%d, got N %d K %d H %d W %d", SURF_MAX, N, K, H, W);
        return -1;
    }
    return surf_work_bytes((int64_t)N * K, H, W);
}

extern "C" int ustrun_surface_metrics(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N, int K,
                                      int by_class, int H, int W, void* work, int64_t work_bytes, void* out,
                                      ustrun_stream_t s) {
    USTRUN_CHECK(pred && gt && work && out && N > 0 && K > 0, "surface_metrics: bad args");
    USTRUN_CHECK(H >= 1 && W >= 1 && H <= SURF_MAX && W <= SURF_MAX, "surface_metrics: H and W must be in 1..%d, got %d x %d",
                 SURF_MAX, H, W);
    const int64_t NK = (int64_t)N * K;
    USTRUN_CHECK(NK <= 65535 / 2, "surface_metrics: N * K = %lld planes exceed one launch (32767)", (long long)NK);
    USTRUN_CHECK(work_bytes >= surf_work_bytes(NK, H, W), "surface_metrics: work buffer of %lld bytes, needs %lld",
                 (long long)work_bytes, (long long)surf_work_bytes(NK, H, W));
    USTRUN_CHECK(((uintptr_t)work & 15) == 0 && ((uintptr_t)out & 7) == 0,
                 "surface_metrics: work must be 16-byte and out 8-byte aligned");
    const SurfWork w = surf_carve(work, NK, H, W);
    const hipStream_t st = (hipStream_t)s;
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(int) * 2 * NK, st);
    USTRUN_CHECK(e == hipSuccess, "surface_metrics: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(border_kernel, dim3(cdiv((int64_t)H * W, 256), NK), dim3(256), 0, st, pred, gt, pred_is_i64, gt_is_i64, K,
                       by_class, H, W, w.col);
    USTRUN_LAUNCH_CHECK("surface_metrics: border");
    hipLaunchKernelGGL(colscan_kernel, dim3(cdiv(W, 64), NK * 2), dim3(64), 0, st, H, W, w.col);
    USTRUN_LAUNCH_CHECK("surface_metrics: column scan");
    hipLaunchKernelGGL(rowmin_kernel, dim3(cdiv(H, ROWS_PER_BLOCK), NK), dim3(256), 0, st, H, W, w.col, w.d2, w.cnt, w.rowsum);
    USTRUN_LAUNCH_CHECK("surface_metrics: row minimum");
    hipLaunchKernelGGL(select_kernel, dim3(NK), dim3(256), 0, st, H, W, w.d2, w.cnt, w.rowsum, (int*)out);
    USTRUN_LAUNCH_CHECK("surface_metrics: select");
    return 0;
}
