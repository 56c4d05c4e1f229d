// labelmap.hip -- losses and metrics of a general label-map segmenter: class-weighted cross-entropy over a label map with ignored
// pixels (K up to 256: one pass over the planes with an online log-sum-exp, no per-class registers), K x K confusion matrices
// (K up to 32: one private LDS histogram per wave, integer atomics at the end of a block's range), four per-plane sums for the
// sigmoid-map losses of utils/metrics.py, and colour decoding through a palette.  The float reductions follow loss.hip and
// consistency.hip (stream_reduce.h): wavefront shuffle -> LDS -> one partial row per block -> fixed-order f64 finalize, so a
// repeated call is bit-identical; the only atomics are integer adds, which are exact and order-free.
#include "stream_reduce.h"

namespace ustrun {
namespace {

constexpr int CE_KMAX = USTRUN_CE_MAP_KMAX, CF_KMAX = USTRUN_CONFUSION_KMAX, PAL_KMAX = USTRUN_COLORIZE_KMAX;
typedef __attribute__((ext_vector_type(2))) long long i64x2;

template <int V> __device__ __forceinline__ void ld_targets(const long long* p, long long (&t)[V]) {
    if constexpr (V == 4) { const i64x2 a = *(const i64x2*)p, b = *(const i64x2*)(p + 2); t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y; }
    else t[0] = *p;
}

// ---- class-weighted cross-entropy over a label map --------------------------------------------------------------------------
struct CeCfg { int N, K, HW, has_ignore, ignore_negative, by_weight, by_count; long long ignore_index; float scale; };

__device__ __forceinline__ bool ce_ignored(const CeCfg& c, long long t) {
    return (c.has_ignore && t == c.ignore_index) || (c.ignore_negative && t < 0);
}
// the class weights (all ones for NULL) in LDS; every thread of the block calls this
__device__ __forceinline__ void stage_weights(const float* __restrict__ weight, int K, float* wl) {
    for (int k = threadIdx.x; k < K; k += 256) wl[k] = weight ? weight[k] : 1.f;
    __syncthreads();
}

// partial row: S = sum w[t] (lse - x_t), sum w[t], valid pixels, out-of-range targets
template <int V>
__global__ __launch_bounds__(256) void ce_map_fwd_kernel(const CeCfg c, const float* __restrict__ logits, const long long* __restrict__ target,
                                                        const float* __restrict__ weight, float* __restrict__ lse_out,
                                                        float* __restrict__ partials) {
    __shared__ float wl[CE_KMAX];
    stage_weights(weight, c.K, wl);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int per = c.HW / V;
    const long items = (long)c.N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        long long t[V];
        ld_targets<V>(target + n * c.HW + hw, t);
        float m[V], s[V], xt[V], l[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { m[v] = -INFINITY; s[v] = 0.f; xt[v] = 0.f; }
        const float* p = logits + n * c.K * c.HW + hw;
#pragma unroll 4
        for (int k = 0; k < c.K; ++k) {
            float x[V];
            ldv<V>(p + (long)k * c.HW, x);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                // online log-sum-exp: s = sum exp(x_j - m) over the classes seen, m their maximum; one expf per value
                const float d = x[v] - m[v], e = expf(-fabsf(d));
                if (d > 0.f) { s[v] = s[v] * e + 1.f; m[v] = x[v]; }
                else s[v] += e;
                if (t[v] == k) xt[v] = x[v];
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            l[v] = m[v] + logf(s[v]);
            if (ce_ignored(c, t[v])) continue;
            if (t[v] < 0 || t[v] >= c.K) { acc[3] += 1.f; continue; }
            const float w = wl[t[v]];
            acc[0] += w * (l[v] - xt[v]);
            acc[1] += w;
            acc[2] += 1.f;
        }
        if (lse_out) stv<V>(lse_out + n * c.HW + hw, l);
    }
    block_row<4>(acc, partials);
}

// the partial rows added in a fixed order in double; out[0] = scale * S [/ sum w] [/ count]
__global__ __launch_bounds__(1024) void ce_map_finalize_kernel(const CeCfg c, const float* __restrict__ partials, int rows, float* __restrict__ out) {
    __shared__ double red[256][4];
    const int col = threadIdx.x & 3, rg = threadIdx.x >> 2;
    double v = 0.0;
    for (int r = rg; r < rows; r += 256) v += (double)partials[(long)r * NS + col];
    red[rg][col] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < 256; ++r)
        for (int j = 0; j < 4; ++j) tot[j] += red[r][j];
    double loss = (double)c.scale * tot[0];
    if (c.by_weight) loss /= tot[1];
    if (c.by_count) loss /= tot[2];
    out[0] = (float)loss;
    for (int j = 0; j < 4; ++j) out[1 + j] = (float)tot[j];
}

template <int V>
__global__ __launch_bounds__(256) void ce_map_bwd_kernel(const CeCfg c, const float* __restrict__ logits, const long long* __restrict__ target,
                                                        const float* __restrict__ weight, const float* __restrict__ lse,
                                                        const float* __restrict__ fwd_out, const float* __restrict__ g,
                                                        float* __restrict__ dlogits) {
    __shared__ float wl[CE_KMAX];
    stage_weights(weight, c.K, wl);
    float coef = g[0] * c.scale;
    if (c.by_weight) coef /= fwd_out[2];
    if (c.by_count) coef /= fwd_out[3];
    const int per = c.HW / V;
    const long items = (long)c.N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        long long t[V];
        ld_targets<V>(target + n * c.HW + hw, t);
        float l[V], f[V];
        ldv<V>(lse + n * c.HW + hw, l);
        bool valid[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            valid[v] = !ce_ignored(c, t[v]) && t[v] >= 0 && t[v] < c.K;
            f[v] = valid[v] ? coef * wl[t[v]] : 0.f;
        }
        const long base = n * c.K * c.HW + hw;
#pragma unroll 4
        for (int k = 0; k < c.K; ++k) {
            float x[V];
            ldv<V>(logits + base + (long)k * c.HW, x);
#pragma unroll
            for (int v = 0; v < V; ++v) x[v] = valid[v] ? f[v] * (expf(x[v] - l[v]) - (t[v] == k ? 1.f : 0.f)) : 0.f;      // exactly 0 off the valid pixels
            stv<V>(dlogits + base + (long)k * c.HW, x);
        }
    }
}

// ---- confusion matrices -----------------------------------------------------------------------------------------------------
// a label as an index: int64 as it is; f32 only where it holds an integer (anything else, NaN included, is out of range)
__device__ __forceinline__ long long label_at(const void* p, int is_i64, long i) {
    if (is_i64) return ((const long long*)p)[i];
    const float f = ((const float*)p)[i];
    if (!(f > -16777216.f && f < 16777216.f)) return -1;
    const long long v = (long long)f;
    return (float)v == f ? v : -1;
}

// grid: per_img blocks per image, never across two images.  Each wave owns a K*K histogram in LDS (an image of one class puts all
// 64 lanes on one bin: a wave whose lanes agree adds its count with one LDS atomic); the block's non-zero bins go to global memory
// with integer atomics.
__global__ __launch_bounds__(256) void confusion_kernel(const void* __restrict__ pred, const void* __restrict__ gt, int pi64, int gi64, int K, int HW,
                                                       int per_img, int has_ignore, long long ignore_index, int* __restrict__ counts,
                                                       int* __restrict__ skipped) {
    __shared__ int hist[4][CF_KMAX * CF_KMAX];
    __shared__ int skip_s;
    const int KK = K * K, wave = threadIdx.x >> 6;
    for (int b = threadIdx.x; b < 4 * CF_KMAX * CF_KMAX; b += 256) (&hist[0][0])[b] = 0;
    if (threadIdx.x == 0) skip_s = 0;
    __syncthreads();
    const int n = blockIdx.x / per_img, blk = blockIdx.x - n * per_img;
    const long base = (long)n * HW;
    int skip = 0;
    // every lane of a wave runs the same number of rounds (the ballot below needs the whole wave)
    for (long e0 = blk * 256 + wave * 64; e0 < HW; e0 += per_img * 256) {
        const long e = e0 + (threadIdx.x & 63);
        int bin = -1;
        if (e < HW) {
            const long long g = label_at(gt, gi64, base + e), p = label_at(pred, pi64, base + e);
            if ((has_ignore && g == ignore_index) || g < 0 || g >= K || p < 0 || p >= K) ++skip;
            else bin = (int)g * K + (int)p;
        }
        const int first = __builtin_amdgcn_readfirstlane(bin);
        if (__all(bin == first)) {
            if ((threadIdx.x & 63) == 0 && first >= 0) atomicAdd(&hist[wave][first], 64);
        } else if (bin >= 0) atomicAdd(&hist[wave][bin], 1);
    }
    if (skip) atomicAdd(&skip_s, skip);
    __syncthreads();
    for (int b = threadIdx.x; b < KK; b += 256) {
        const int v = hist[0][b] + hist[1][b] + hist[2][b] + hist[3][b];
        if (v) atomicAdd(&counts[(long)n * KK + b], v);
    }
    if (threadIdx.x == 0 && skip_s) atomicAdd(&skipped[n], skip_s);
}

// ---- per-plane sums for the sigmoid-map losses -------------------------------------------------------------------------------
// s and log(1 - s), log s from the log-sigmoid, as activate() in consistency.hip
__device__ __forceinline__ float sig(float x) {
    const float ea = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + ea) : ea / (1.f + ea);
}
// bce_with_logits(x, t) = max(x, 0) - x t + log(1 + exp(-|x|))
__device__ __forceinline__ float bce_logits(float x, float t) { return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))); }

// grid: K * per_plane blocks; block b walks plane b / per_plane over every image.  Partial row: sum s t, sum s, sum t, sum (1 + t) bce
template <int V>
__global__ __launch_bounds__(256) void plane_sums_fwd_kernel(const float* __restrict__ x, const float* __restrict__ t, int N, int K, int HW, int act,
                                                            int has_ignore, float ignore_value, int per_plane, float* __restrict__ partials) {
    const int k = blockIdx.x / per_plane, blk = blockIdx.x - k * per_plane;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int per = HW / V;
    const long items = (long)N * per;
    for (long i = (long)blk * 256 + threadIdx.x; i < items; i += (long)per_plane * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float xv[V], tv[V];
        const long at = (n * K + k) * HW + hw;
        ldv<V>(x + at, xv);
        ldv<V>(t + at, tv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (has_ignore && tv[v] == ignore_value) continue;
            const float s = act == USTRUN_LOSS_SIGMOID ? sig(xv[v]) : xv[v];
            acc[0] += s * tv[v]; acc[1] += s; acc[2] += tv[v];
            if (act == USTRUN_LOSS_SIGMOID) acc[3] += (1.f + tv[v]) * bce_logits(xv[v], tv[v]);
        }
    }
    block_row<4>(acc, partials);
}

// one block per plane: its per_plane partial rows added in a fixed order in double -> out[k][0..3]
__global__ __launch_bounds__(256) void plane_sums_finalize_kernel(const float* __restrict__ partials, int per_plane, float* __restrict__ out) {
    __shared__ double red[64][4];
    const int k = blockIdx.x, col = threadIdx.x & 3, rg = threadIdx.x >> 2;
    double v = 0.0;
    for (int r = rg; r < per_plane; r += 64) v += (double)partials[((long)k * per_plane + r) * NS + col];
    red[rg][col] = v;
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int r = 0; r < 64; ++r) t += red[r][threadIdx.x];
        out[k * 4 + threadIdx.x] = (float)t;
    }
}

// dx = ((coef[k][0] t + coef[k][1]) ds/dx + coef[k][2] (1 + t)(s - t)), 0 where t is ignored; ds/dx = s (1 - s) or 1
template <int V>
__global__ __launch_bounds__(256) void plane_sums_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, int N, int K, int HW, int act,
                                                            int has_ignore, float ignore_value, const float* __restrict__ coef,
                                                            float* __restrict__ dx) {
    const int per = HW / V;
    const long items = (long)N * K * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long nk, hw;
        item_at<V>(i, per, nk, hw);
        const int k = (int)(nk % K);
        const float a = coef[k * 3], b = coef[k * 3 + 1], c = coef[k * 3 + 2];
        float xv[V], tv[V];
        ldv<V>(x + nk * HW + hw, xv);
        ldv<V>(t + nk * HW + hw, tv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (has_ignore && tv[v] == ignore_value) { xv[v] = 0.f; continue; }
            if (act == USTRUN_LOSS_SIGMOID) {
                const float s = sig(xv[v]);
                xv[v] = (a * tv[v] + b) * s * (1.f - s) + c * (1.f + tv[v]) * (s - tv[v]);
            } else xv[v] = a * tv[v] + b;
        }
        stv<V>(dx + nk * HW + hw, xv);
    }
}

// ---- colour decoding ----------------------------------------------------------------------------------------------------------
// out[n][c][hw] = palette[l][c] / 255 for a label in [0, K), l / 255 in all three channels otherwise.  One pixel per lane: this is
// a visualisation pass over one label map, not a step of any training loop.
__global__ __launch_bounds__(256) void colorize_kernel(const void* __restrict__ labels, int is_i64, int N, int HW, const unsigned char* __restrict__ palette,
                                                      int K, float* __restrict__ out) {
    __shared__ float pal[PAL_KMAX * 3];
    for (int j = threadIdx.x; j < K * 3; j += 256) pal[j] = (float)palette[j] / 255.0f;
    __syncthreads();
    const long total = (long)N * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = i / HW, hw = i - n * HW;
        float raw;
        long long l;
        if (is_i64) { l = ((const long long*)labels)[i]; raw = (float)l; }
        else { raw = ((const float*)labels)[i]; l = label_at(labels, 0, i); }
        float* o = out + n * 3 * HW + hw;
        const bool in = l >= 0 && l < K;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[(long)ch * HW] = in ? pal[l * 3 + ch] : raw / 255.0f;
    }
}

int ce_cfg(CeCfg* c, const char* who, int N, int K, int HW, int has_ignore, int64_t ignore_index, int ignore_negative, float scale,
           int by_weight, int by_count) {
    USTRUN_CHECK(K >= 1 && K <= CE_KMAX, "%s: %d classes (1..%d)", who, K, CE_KMAX);
    USTRUN_CHECK(N > 0 && HW > 0 && (long)N * HW < (1L << 32), "%s: bad shape N=%d K=%d HW=%d", who, N, K, HW);
    *c = CeCfg{N, K, HW, has_ignore != 0, ignore_negative != 0, by_weight != 0, by_count != 0, (long long)ignore_index, scale};
    return 0;
}

int planes_ok(const char* who, int N, int K, int HW, int act) {
    USTRUN_CHECK(K >= 1 && K <= KMAX, "%s: %d planes (1..%d)", who, K, KMAX);
    USTRUN_CHECK(N > 0 && HW > 0 && (long)N * K * HW < (1L << 32), "%s: bad shape N=%d K=%d HW=%d", who, N, K, HW);
    USTRUN_CHECK(act == USTRUN_LOSS_SOFTMAX || act == USTRUN_LOSS_SIGMOID, "%s: bad activation %d", who, act);
    return 0;
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int ustrun_ce_map_fwd(const float* logits, const int64_t* target, const float* weight_dev, int N, int K, int HW, int has_ignore,
                                 int64_t ignore_index, int ignore_negative, float scale, int by_weight, int by_count, float* out, float* lse,
                                 float* partials, int64_t partials_bytes, ustrun_stream_t s) {
    USTRUN_CHECK(logits && target && out, "ce_map_fwd: null pointer");
    CeCfg c;
    USTRUN_TRY(ce_cfg(&c, "ce_map_fwd", N, K, HW, has_ignore, ignore_index, ignore_negative, scale, by_weight, by_count));
    USTRUN_CHECK(partials && partials_bytes >= ustrun_loss_partials_bytes(1, 1, 1), "ce_map_fwd: partials too small");
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    const bool vec = HW % 4 == 0 && al16(logits) && al16(target) && al16(lse);
    const int rows = stream_blocks(vec ? npix / 4 : npix);
    if (vec) hipLaunchKernelGGL(ce_map_fwd_kernel<4>, dim3(rows), dim3(256), 0, st, c, logits, (const long long*)target, weight_dev, lse, partials);
    else hipLaunchKernelGGL(ce_map_fwd_kernel<1>, dim3(rows), dim3(256), 0, st, c, logits, (const long long*)target, weight_dev, lse, partials);
    USTRUN_LAUNCH_CHECK("ce_map_fwd");
    hipLaunchKernelGGL(ce_map_finalize_kernel, dim3(1), dim3(1024), 0, st, c, partials, rows, out);
    USTRUN_LAUNCH_CHECK("ce_map_finalize");
    return 0;
}

extern "C" int ustrun_ce_map_bwd(const float* logits, const int64_t* target, const float* weight_dev, const float* lse, int N, int K, int HW,
                                 int has_ignore, int64_t ignore_index, int ignore_negative, float scale, int by_weight, int by_count,
                                 const float* fwd_out, const float* gout_dev, float* dlogits, ustrun_stream_t s) {
    USTRUN_CHECK(logits && target && lse && fwd_out && gout_dev && dlogits, "ce_map_bwd: null pointer");
    CeCfg c;
    USTRUN_TRY(ce_cfg(&c, "ce_map_bwd", N, K, HW, has_ignore, ignore_index, ignore_negative, scale, by_weight, by_count));
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    const bool vec = HW % 4 == 0 && al16(logits) && al16(target) && al16(lse) && al16(dlogits);
    if (vec) hipLaunchKernelGGL(ce_map_bwd_kernel<4>, dim3(stream_blocks(npix / 4)), dim3(256), 0, st, c, logits, (const long long*)target, weight_dev,
                                lse, fwd_out, gout_dev, dlogits);
    else hipLaunchKernelGGL(ce_map_bwd_kernel<1>, dim3(stream_blocks(npix)), dim3(256), 0, st, c, logits, (const long long*)target, weight_dev, lse,
                            fwd_out, gout_dev, dlogits);
    USTRUN_LAUNCH_CHECK("ce_map_bwd");
    return 0;
}

extern "C" int ustrun_confusion(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N, int K, int64_t HW, int has_ignore,
                                int64_t ignore_index, int32_t* counts, int32_t* skipped, ustrun_stream_t s) {
    USTRUN_CHECK(pred && gt && counts && skipped, "confusion: null pointer");
    USTRUN_CHECK(K >= 1 && K <= CF_KMAX, "confusion: %d classes (1..%d)", K, CF_KMAX);
    USTRUN_CHECK(HW > 0 && HW < (1LL << 31), "confusion: HW %lld (1..2^31-1: a bin is an int32)", (long long)HW);
    USTRUN_CHECK(N > 0 && N <= 65536, "confusion: N %d (1..65536)", N);
    const hipStream_t st = (hipStream_t)s;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)N * K * K, st);
    if (e == hipSuccess) e = hipMemsetAsync(skipped, 0, sizeof(int32_t) * (size_t)N, st);
    USTRUN_CHECK(e == hipSuccess, "confusion: memset failed: %s", hipGetErrorString(e));
    // 16 rounds of 256 pixels per block, at most about 2048 blocks in all
    long per_img = (HW + 4095) / 4096;
    const long cap = 2048 / N > 1 ? 2048 / N : 1;
    if (per_img > cap) per_img = cap;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)(per_img * N)), dim3(256), 0, st, pred, gt, pred_is_i64, gt_is_i64, K, (int)HW, (int)per_img,
                       has_ignore, (long long)ignore_index, counts, skipped);
    USTRUN_LAUNCH_CHECK("confusion");
    return 0;
}

extern "C" int ustrun_plane_sums_fwd(const float* x, const float* t, int N, int K, int HW, int act, int has_ignore, float ignore_value, float* out,
                                     float* partials, int64_t partials_bytes, ustrun_stream_t s) {
    USTRUN_CHECK(x && t && out, "plane_sums_fwd: null pointer");
    USTRUN_TRY(planes_ok("plane_sums_fwd", N, K, HW, act));
    USTRUN_CHECK(partials && partials_bytes >= ustrun_loss_partials_bytes(1, 1, 1), "plane_sums_fwd: partials too small");
    const hipStream_t st = (hipStream_t)s;
    const bool vec = HW % 4 == 0 && al16(x) && al16(t);
    int per_plane = stream_blocks(vec ? (long)N * HW / 4 : (long)N * HW);
    if (per_plane > 2048 / KMAX) per_plane = 2048 / KMAX;            // K * per_plane rows fit the partials buffer
    if (vec) hipLaunchKernelGGL(plane_sums_fwd_kernel<4>, dim3(K * per_plane), dim3(256), 0, st, x, t, N, K, HW, act, has_ignore, ignore_value, per_plane,
                                partials);
    else hipLaunchKernelGGL(plane_sums_fwd_kernel<1>, dim3(K * per_plane), dim3(256), 0, st, x, t, N, K, HW, act, has_ignore, ignore_value, per_plane,
                            partials);
    USTRUN_LAUNCH_CHECK("plane_sums_fwd");
    hipLaunchKernelGGL(plane_sums_finalize_kernel, dim3(K), dim3(256), 0, st, partials, per_plane, out);
    USTRUN_LAUNCH_CHECK("plane_sums_finalize");
    return 0;
}

extern "C" int ustrun_plane_sums_bwd(const float* x, const float* t, int N, int K, int HW, int act, int has_ignore, float ignore_value,
                                     const float* coef_dev, float* dx, ustrun_stream_t s) {
    USTRUN_CHECK(x && t && coef_dev && dx, "plane_sums_bwd: null pointer");
    USTRUN_TRY(planes_ok("plane_sums_bwd", N, K, HW, act));
    const hipStream_t st = (hipStream_t)s;
    const long n = (long)N * K * HW;
    const bool vec = HW % 4 == 0 && al16(x) && al16(t) && al16(dx);
    if (vec) hipLaunchKernelGGL(plane_sums_bwd_kernel<4>, dim3(stream_blocks(n / 4)), dim3(256), 0, st, x, t, N, K, HW, act, has_ignore, ignore_value,
                                coef_dev, dx);
    else hipLaunchKernelGGL(plane_sums_bwd_kernel<1>, dim3(stream_blocks(n)), dim3(256), 0, st, x, t, N, K, HW, act, has_ignore, ignore_value, coef_dev,
                            dx);
    USTRUN_LAUNCH_CHECK("plane_sums_bwd");
    return 0;
}

extern "C" int ustrun_colorize(const void* labels, int labels_is_i64, int N, int HW, const uint8_t* palette_dev, int K, float* out,
                               ustrun_stream_t s) {
    USTRUN_CHECK(labels && palette_dev && out, "colorize: null pointer");
    USTRUN_CHECK(K >= 1 && K <= PAL_KMAX, "colorize: %d colours (1..%d)", K, PAL_KMAX);
    USTRUN_CHECK(N > 0 && HW > 0, "colorize: bad shape N=%d HW=%d", N, HW);
    hipLaunchKernelGGL(colorize_kernel, dim3(stream_blocks((long)N * HW)), dim3(256), 0, (hipStream_t)s, labels, labels_is_i64, N, HW, palette_dev, K,
                       out);
    USTRUN_LAUNCH_CHECK("colorize");
    return 0;
}
