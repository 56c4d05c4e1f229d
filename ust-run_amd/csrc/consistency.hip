// consistency.hip -- the semi-supervised loss toolkit of utils/losses.py: pair consistency between two logit tensors (squared
// error map, KL mean, soft Dice), entropy of a probability map, focal loss, six sums over two flat arrays, row-wise symmetric KL.
// All of it streams f32 NCHW [N,K,HW] once and is HBM-bound: a lane takes V = 4 consecutive pixels of every plane with one
// 16-byte access each (V = 1 when HW % 4 != 0 or a pointer is not 16-byte aligned: same arithmetic), grid-stride blocks of
// 256; reductions go wavefront shuffle -> LDS -> one partial row per block -> single-block f64 finalize in a fixed order.
// Backward kernels recompute the probabilities from the logits; nothing but the reduced sums is kept between the two passes.
#include "stream_reduce.h"

namespace ustrun {
namespace {

constexpr float DICE_SMOOTH = 1e-5f;      // losses.py:10,21
constexpr float ENT_EPS = 1e-6f;          // losses.py:32,60,272,279

template <int V, int KN> __device__ __forceinline__ void ld_planes(const float* t, long n, int K, int HW, long hw, float (&x)[KN][V]) {
#pragma unroll
    for (int k = 0; k < KN; ++k) if (k < K) ldv<V>(t + (n * K + k) * HW + hw, x[k]);
}
template <int V, int KN> __device__ __forceinline__ void st_planes(float* t, long n, int K, int HW, long hw, const float (&x)[KN][V]) {
#pragma unroll
    for (int k = 0; k < KN; ++k) if (k < K) stv<V>(t + (n * K + k) * HW + hw, x[k]);
}

// KN: the class bound a kernel is built for (2, 4 or KMAX; the host picks the smallest that holds K): the per-pixel arrays, and
// with them the registers of a lane, scale with it.
// probabilities and their logarithms of one pixel; the logarithm comes from the log-softmax / log-sigmoid, never from log(p)
template <int V, int KN> __device__ __forceinline__ void activate(int act, int K, const float (&x)[KN][V], int v, float* p, float* lp) {
    if (act == USTRUN_LOSS_SOFTMAX) {
        float mx = -INFINITY, se = 0.f;
#pragma unroll
        for (int k = 0; k < KN; ++k) if (k < K) mx = fmaxf(mx, x[k][v]);
#pragma unroll
        for (int k = 0; k < KN; ++k) if (k < K) { p[k] = expf(x[k][v] - mx); se += p[k]; }
        const float inv = 1.f / se, lse = logf(se);
#pragma unroll
        for (int k = 0; k < KN; ++k) if (k < K) { p[k] *= inv; lp[k] = x[k][v] - mx - lse; }
    } else {
#pragma unroll
        for (int k = 0; k < KN; ++k)
            if (k < K) {
                const float xv = x[k][v], ea = expf(-fabsf(xv));
                p[k] = xv >= 0.f ? 1.f / (1.f + ea) : ea / (1.f + ea);
                lp[k] = fminf(xv, 0.f) - log1pf(ea);
            }
    }
}
// gradient of the logits from the gradient G of the probabilities of one pixel
template <int KN> __device__ __forceinline__ void through_act(int act, int K, const float* p, float* G) {
    if (act == USTRUN_LOSS_SOFTMAX) {
        float gp = 0.f;
#pragma unroll
        for (int k = 0; k < KN; ++k) if (k < K) gp += G[k] * p[k];
#pragma unroll
        for (int k = 0; k < KN; ++k) if (k < K) G[k] = p[k] * (G[k] - gp);
    } else {
#pragma unroll
        for (int k = 0; k < KN; ++k) if (k < K) G[k] = G[k] * p[k] * (1.f - p[k]);
    }
}

// ---- pair consistency ----------------------------------------------------------------------------------------------------
template <int V, int KIND, int KN>
__global__ __launch_bounds__(256) void cons_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int K, int HW,
                                                      int act, float* __restrict__ out, float* __restrict__ partials) {
    constexpr int NC = KIND == USTRUN_CONS_SOFT_DICE ? NS : 1;
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.f;
    const int per = HW / V;
    const long items = (long)N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float xa[KN][V], xb[KN][V];
        ld_planes<V, KN>(a, n, K, HW, hw, xa);
        ld_planes<V, KN>(b, n, K, HW, hw, xb);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float pa[KN], la[KN], pb[KN], lb[KN];
            activate<V, KN>(act, K, xa, v, pa, la);
            activate<V, KN>(act, K, xb, v, pb, lb);
#pragma unroll
            for (int k = 0; k < KN; ++k)
                if (k < K) {
                    if constexpr (KIND == USTRUN_CONS_MSE_MAP) { const float d = pa[k] - pb[k]; xa[k][v] = d * d; }
                    else if constexpr (KIND == USTRUN_CONS_KL_MEAN) acc[0] += pb[k] * (lb[k] - la[k]);      // pb = 0: 0 * finite
                    else { acc[1 + k] += pa[k] * pb[k]; acc[1 + KMAX + k] += pa[k]; acc[1 + 2 * KMAX + k] += pb[k]; }
                }
        }
        if constexpr (KIND == USTRUN_CONS_MSE_MAP) st_planes<V, KN>(out, n, K, HW, hw, xa);
    }
    if constexpr (KIND != USTRUN_CONS_MSE_MAP) block_row<NC>(acc, partials);
}

template <int V, int KIND, int KN>
__global__ __launch_bounds__(256) void cons_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int K, int HW,
                                                      int act, const float* __restrict__ sums, const float* __restrict__ g,
                                                      float* __restrict__ da, float* __restrict__ db) {
    float c1[KN], c2[KN], gs = 0.f;       // soft Dice: dL/dpa_k = c1[k] pb_k + c2[k] (and a <-> b); KL: gs = upstream / count
    if constexpr (KIND == USTRUN_CONS_KL_MEAN) gs = g[0] / ((float)N * (float)K * (float)HW);
    if constexpr (KIND == USTRUN_CONS_SOFT_DICE) {
#pragma unroll
        for (int k = 0; k < KN; ++k)
            if (k < K) {
                const float I = sums[1 + k], D = sums[1 + KMAX + k] + sums[1 + 2 * KMAX + k] + DICE_SMOOTH;
                c1[k] = g[0] * -2.f / D / K;
                c2[k] = g[0] * (2.f * I + DICE_SMOOTH) / (D * D) / K;
            }
    }
    const int per = HW / V;
    const long items = (long)N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float xa[KN][V], xb[KN][V], gm[KN][V];
        ld_planes<V, KN>(a, n, K, HW, hw, xa);
        ld_planes<V, KN>(b, n, K, HW, hw, xb);
        if constexpr (KIND == USTRUN_CONS_MSE_MAP) ld_planes<V, KN>(g, n, K, HW, hw, gm);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float pa[KN], la[KN], pb[KN], lb[KN], Ga[KN], Gb[KN];
            activate<V, KN>(act, K, xa, v, pa, la);
            activate<V, KN>(act, K, xb, v, pb, lb);
            if constexpr (KIND == USTRUN_CONS_KL_MEAN) {
                // side a enters through log pa: softmax d(log pa_k)/da_j = [k = j] - pa_j, sigmoid d(log pa_k)/da_k = 1 - pa_k
                float gl = 0.f;
#pragma unroll
                for (int k = 0; k < KN; ++k) if (k < K) { Ga[k] = -pb[k] * gs; gl += Ga[k]; Gb[k] = (lb[k] - la[k] + 1.f) * gs; }
#pragma unroll
                for (int k = 0; k < KN; ++k)
                    if (k < K) Ga[k] = act == USTRUN_LOSS_SOFTMAX ? Ga[k] - pa[k] * gl : Ga[k] * (1.f - pa[k]);
                through_act<KN>(act, K, pb, Gb);
            } else {
#pragma unroll
                for (int k = 0; k < KN; ++k)
                    if (k < K) {
                        if constexpr (KIND == USTRUN_CONS_MSE_MAP) { Ga[k] = 2.f * (pa[k] - pb[k]) * gm[k][v]; Gb[k] = -Ga[k]; }
                        else { Ga[k] = c1[k] * pb[k] + c2[k]; Gb[k] = c1[k] * pa[k] + c2[k]; }
                    }
                through_act<KN>(act, K, pa, Ga);
                through_act<KN>(act, K, pb, Gb);
            }
#pragma unroll
            for (int k = 0; k < KN; ++k) if (k < K) { xa[k][v] = Ga[k]; xb[k][v] = Gb[k]; }
        }
        if (da) st_planes<V, KN>(da, n, K, HW, hw, xa);
        if (db) st_planes<V, KN>(db, n, K, HW, hw, xb);
    }
}

// ---- entropy of a probability map ----------------------------------------------------------------------------------------
// log(p + 1e-6) without the rounding of the sum: at p = 1 the f32 sum is 1 + 2^-20 and its logarithm 5% off, which is the whole
// entropy of a one-class map.  s + e = p + 1e-6 exactly (TwoSum), log(s + e) = log s + e / s up to e^2.
__device__ __forceinline__ float log_eps(float p) {
    const float s = p + ENT_EPS, bb = s - p, e = (p - (s - bb)) + (ENT_EPS - bb);
    return logf(s) + e / s;
}

template <int V, bool MEAN, int KN>
__global__ __launch_bounds__(256) void entropy_fwd_kernel(const float* __restrict__ p, int N, int K, int HW, float factor,
                                                         float* __restrict__ out, float* __restrict__ partials) {
    float acc[1] = {0.f};
    const int per = HW / V;
    const long items = (long)N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float x[KN][V], e[V];
        ld_planes<V, KN>(p, n, K, HW, hw, x);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KN; ++k) if (k < K) s += x[k][v] * log_eps(x[k][v]);
            e[v] = -s * factor;
            acc[0] += e[v];
        }
        if constexpr (!MEAN) stv<V>(out + n * HW + hw, e);
    }
    if constexpr (MEAN) block_row<1>(acc, partials);
}

template <int V, bool MEAN, int KN>
__global__ __launch_bounds__(256) void entropy_bwd_kernel(const float* __restrict__ p, int N, int K, int HW, float factor,
                                                         const float* __restrict__ g, float* __restrict__ dp) {
    const float gs = MEAN ? g[0] / ((float)N * (float)HW) : 0.f;
    const int per = HW / V;
    const long items = (long)N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float x[KN][V], u[V];
        ld_planes<V, KN>(p, n, K, HW, hw, x);
        if constexpr (!MEAN) ldv<V>(g + n * HW + hw, u);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float up = (MEAN ? gs : u[v]) * factor;
#pragma unroll
            for (int k = 0; k < KN; ++k)
                if (k < K) x[k][v] = -(log_eps(x[k][v]) + x[k][v] / (x[k][v] + ENT_EPS)) * up;
        }
        st_planes<V, KN>(dp, n, K, HW, hw, x);
    }
}

// ---- focal loss ----------------------------------------------------------------------------------------------------------
struct FocalCfg { int N, K, HW, has_alpha, mean; float gamma; float alpha[KMAX]; };

// (1 - pt)^gamma alpha_t of one pixel, and the log-softmax; 0 for a target outside [0, K)
template <int V, int KN> __device__ __forceinline__ float focal_factor(const FocalCfg& c, const float (&x)[KN][V], int v, long long t, float* p,
                                                              float* lpt) {
    float lp[KN], lt = 0.f, at = 0.f;
    activate<V, KN>(USTRUN_LOSS_SOFTMAX, c.K, x, v, p, lp);
#pragma unroll
    for (int k = 0; k < KN; ++k) if (k < c.K && t == k) { lt = lp[k]; at = c.has_alpha ? c.alpha[k] : 1.f; }
    *lpt = lt;
    return powf(1.f - expf(lt), c.gamma) * at;       // pt = exp(log pt), as losses.py:141 forms it
}

template <int V, int KN>
__global__ __launch_bounds__(256) void focal_fwd_kernel(const FocalCfg c, const float* __restrict__ logits, const long long* __restrict__ target,
                                                       float* __restrict__ partials) {
    float acc[1] = {0.f};
    const int per = c.HW / V;
    const long items = (long)c.N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float x[KN][V];
        ld_planes<V, KN>(logits, n, c.K, c.HW, hw, x);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float p[KN], lt;
            const float f = focal_factor<V, KN>(c, x, v, target[n * c.HW + hw + v], p, &lt);
            acc[0] -= f * lt;
        }
    }
    block_row<1>(acc, partials);
}

template <int V, int KN>
__global__ __launch_bounds__(256) void focal_bwd_kernel(const FocalCfg c, const float* __restrict__ logits, const long long* __restrict__ target,
                                                       const float* __restrict__ g, float* __restrict__ dlogits) {
    const float gs = c.mean ? g[0] / ((float)c.N * (float)c.HW) : g[0];
    const int per = c.HW / V;
    const long items = (long)c.N * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        long n, hw;
        item_at<V>(i, per, n, hw);
        float x[KN][V];
        ld_planes<V, KN>(logits, n, c.K, c.HW, hw, x);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float p[KN], lt;
            const long long t = target[n * c.HW + hw + v];
            const float f = focal_factor<V, KN>(c, x, v, t, p, &lt) * gs;      // the factor is a constant of the gradient (detached pt)
#pragma unroll
            for (int k = 0; k < KN; ++k) if (k < c.K) x[k][v] = f * (p[k] - (t == k ? 1.f : 0.f));
        }
        st_planes<V, KN>(dlogits, n, c.K, c.HW, hw, x);
    }
}

// ---- six sums over two flat arrays -----------------------------------------------------------------------------------------
__device__ __forceinline__ void pair_add(float a, float b, float (&acc)[6]) {
    const float d = a - b;
    acc[0] += a * b; acc[1] += a * a; acc[2] += b * b; acc[3] += a; acc[4] += b; acc[5] += d * d;
}
template <int V>
__global__ __launch_bounds__(256) void pair_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                       float* __restrict__ partials) {
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long nv = n / V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        float x[V], y[V];
        ldv<V>(a + i * V, x);
        ldv<V>(b + i * V, y);
#pragma unroll
        for (int v = 0; v < V; ++v) pair_add(x[v], y[v], acc);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - nv * V) pair_add(a[nv * V + threadIdx.x], b[nv * V + threadIdx.x], acc);
    block_row<6>(acc, partials);
}

// d loss / da_i = ka[0] a_i + ka[1] b_i + ka[2], d loss / db_i = kb[0] a_i + kb[1] b_i + kb[2]
__device__ __forceinline__ void pair_coef(int kind, long n, const float* sums, float g, float (&ka)[3], float (&kb)[3]) {
    const float I = sums[0];
    if (kind == USTRUN_PAIR_MSE) {
        const float c = 2.f * g / (float)n;
        ka[0] = c; ka[1] = -c; ka[2] = 0.f; kb[0] = -c; kb[1] = c; kb[2] = 0.f;
    } else if (kind == USTRUN_PAIR_DICE_SQ) {
        const float D = sums[1] + sums[2] + DICE_SMOOTH, r = 2.f * (2.f * I + DICE_SMOOTH) / (D * D) * g, q = -2.f / D * g;
        ka[0] = r; ka[1] = q; ka[2] = 0.f; kb[0] = q; kb[1] = r; kb[2] = 0.f;
    } else {
        const float D = sums[3] + sums[4] + DICE_SMOOTH, r = (2.f * I + DICE_SMOOTH) / (D * D) * g, q = -2.f / D * g;
        ka[0] = 0.f; ka[1] = q; ka[2] = r; kb[0] = q; kb[1] = 0.f; kb[2] = r;
    }
}
template <int V>
__global__ __launch_bounds__(256) void pair_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, int kind,
                                                      const float* __restrict__ sums, const float* __restrict__ g,
                                                      float* __restrict__ da, float* __restrict__ db) {
    float ka[3], kb[3];
    pair_coef(kind, n, sums, g[0], ka, kb);
    const long nv = n / V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        float x[V], y[V], u[V], w[V];
        ldv<V>(a + i * V, x);
        ldv<V>(b + i * V, y);
#pragma unroll
        for (int v = 0; v < V; ++v) { u[v] = ka[0] * x[v] + ka[1] * y[v] + ka[2]; w[v] = kb[0] * x[v] + kb[1] * y[v] + kb[2]; }
        if (da) stv<V>(da + i * V, u);
        if (db) stv<V>(db + i * V, w);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - nv * V) {
        const long i = nv * V + threadIdx.x;
        const float x = a[i], y = b[i];
        if (da) da[i] = ka[0] * x + ka[1] * y + ka[2];
        if (db) db[i] = kb[0] * x + kb[1] * y + kb[2];
    }
}

// ---- compute_kl_loss: softmax over the C contiguous values of a row, one lane per row, any C ---------------------------------
struct RowStat { float mx, inv, lse; };      // p_c = exp(x_c - mx) * inv (not exp(log p_c): that carries the rounding of a logarithm of size 20), log p_c = x_c - mx - lse
__device__ __forceinline__ RowStat row_stat(const float* __restrict__ x, int C) {
    float mx = -INFINITY;
    double se = 0.0;                 // row sums in double: a row may be long, and one lane adds it in order
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, x[c]);
    for (int c = 0; c < C; ++c) se += (double)expf(x[c] - mx);
    return RowStat{mx, (float)(1.0 / se), (float)log(se)};
}
__global__ __launch_bounds__(256) void row_kl_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long rows, int C,
                                                        float* __restrict__ partials) {
    float acc[1] = {0.f};
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        const float *x = a + r * C, *y = b + r * C;
        const RowStat sa = row_stat(x, C), sb = row_stat(y, C);
        double row = 0.0;
        for (int c = 0; c < C; ++c) {
            const float ua = x[c] - sa.mx, ub = y[c] - sb.mx, la = ua - sa.lse, lb = ub - sb.lse;
            row += (double)((expf(ub) * sb.inv - expf(ua) * sa.inv) * (lb - la));        // pb (lb - la) + pa (la - lb)
        }
        acc[0] += (float)row;
    }
    block_row<1>(acc, partials);
}
// f = sum_c (p_c - q_c)(lp_c - lq_c):  df/da_j = p_j (d_j - sum_c p_c d_c) + (p_j - q_j) - p_j sum_c (p_c - q_c),  d = lp - lq
__global__ __launch_bounds__(256) void row_kl_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long rows, int C,
                                                        const float* __restrict__ g, float* __restrict__ da, float* __restrict__ db) {
    const float gs = g[0] / (2.f * (float)rows * (float)C);
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        const float *x = a + r * C, *y = b + r * C;
        const RowStat sa = row_stat(x, C), sb = row_stat(y, C);
        double spd = 0.0, sqd = 0.0, sp = 0.0, sq = 0.0;
        for (int c = 0; c < C; ++c) {
            const float ua = x[c] - sa.mx, ub = y[c] - sb.mx, la = ua - sa.lse, lb = ub - sb.lse, p = expf(ua) * sa.inv, q = expf(ub) * sb.inv;
            spd += (double)(p * (la - lb)); sqd += (double)(q * (lb - la)); sp += (double)p; sq += (double)q;
        }
        const float fpd = (float)spd, fqd = (float)sqd, dpq = (float)(sp - sq);
        for (int c = 0; c < C; ++c) {
            const float ua = x[c] - sa.mx, ub = y[c] - sb.mx, la = ua - sa.lse, lb = ub - sb.lse, p = expf(ua) * sa.inv, q = expf(ub) * sb.inv;
            if (da) da[r * C + c] = gs * (p * ((la - lb) - fpd) + (p - q) - p * dpq);
            if (db) db[r * C + c] = gs * (q * ((lb - la) - fqd) + (q - p) + q * dpq);
        }
    }
}

// ---- single-block finalize: the partial rows added in a fixed order in double ---------------------------------------------------
enum { FIN_SCALE = 0, FIN_SOFT_DICE = 1, FIN_PAIR = 2 };
struct FinCfg { int what, K; double scale; };      // FIN_SCALE: out[0] = total[0] * scale; FIN_PAIR: scale = 1 / n

__global__ __launch_bounds__(1024) void finalize_kernel(const float* __restrict__ partials, int rows, int ncols, const FinCfg c,
                                                       float* __restrict__ out) {
    __shared__ double tot[32];
    __shared__ double red[32][33];
    const int col = threadIdx.x & 31, rg = threadIdx.x >> 5;      // 32 columns (ncols used) x 32 row lanes
    double v = 0.0;
    if (col < ncols)
        for (int r = rg; r < rows; r += 32) v += (double)partials[(long)r * NS + col];
    red[rg][col] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
        for (int k = 0; k < 32; ++k) t += red[k][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (c.what == FIN_SCALE) out[0] = (float)(tot[0] * c.scale);
    else if (c.what == FIN_SOFT_DICE) {
        double loss = 0.0;
        for (int k = 0; k < KMAX; ++k) {
            const double I = tot[1 + k], A = tot[1 + KMAX + k], B = tot[1 + 2 * KMAX + k];
            if (k < c.K) loss += 1.0 - (2.0 * I + (double)DICE_SMOOTH) / (A + B + (double)DICE_SMOOTH);
            out[1 + k] = (float)I; out[1 + KMAX + k] = (float)A; out[1 + 2 * KMAX + k] = (float)B;
        }
        out[0] = (float)(loss / c.K);
    } else {
        for (int i = 0; i < 6; ++i) out[i] = (float)tot[i];
        out[6] = (float)(1.0 - (2.0 * tot[0] + (double)DICE_SMOOTH) / (tot[1] + tot[2] + (double)DICE_SMOOTH));
        out[7] = (float)(1.0 - (2.0 * tot[0] + (double)DICE_SMOOTH) / (tot[3] + tot[4] + (double)DICE_SMOOTH));
        out[8] = (float)(tot[5] * c.scale);
    }
}

int finalize(const float* partials, int rows, int ncols, int what, int K, double scale, float* out, hipStream_t st, const char* who) {
    const FinCfg c = {what, K, scale};
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1024), 0, st, partials, rows, ncols, c, out);
    USTRUN_LAUNCH_CHECK(who);
    return 0;
}

int shape_ok(const char* who, int N, int K, int HW) {
    USTRUN_CHECK(K >= 1 && K <= KMAX, "%s: %d classes (1..%d)", who, K, KMAX);
    USTRUN_CHECK(N > 0 && HW > 0 && (long)N * HW < (1L << 32), "%s: bad shape N=%d K=%d HW=%d", who, N, K, HW);
    return 0;
}
int partials_ok(const char* who, const float* partials, int64_t bytes) {
    USTRUN_CHECK(partials && bytes >= ustrun_loss_partials_bytes(1, 1, 1), "%s: partials too small", who);
    return 0;
}

// the build of a kernel for the smallest class bound that holds K (the bound is the kernel's last template argument)
template <class Kern> Kern by_k(int K, Kern k2, Kern k4, Kern k8) { return K <= 2 ? k2 : K <= 4 ? k4 : k8; }
#define BY_K(K, name, ...) by_k(K, name<__VA_ARGS__, 2>, name<__VA_ARGS__, 4>, name<__VA_ARGS__, KMAX>)

// launches k4 (four pixels per lane) when the 16-byte path applies, k1 otherwise
template <class Kern, class... A> void launch_v(bool vec, Kern k4, Kern k1, long npix, hipStream_t st, A... args) {
    if (vec) hipLaunchKernelGGL(k4, dim3(stream_blocks(npix / 4)), dim3(256), 0, st, args...);
    else hipLaunchKernelGGL(k1, dim3(stream_blocks(npix)), dim3(256), 0, st, args...);
}

int focal_cfg(FocalCfg* c, const char* who, int N, int K, int HW, float gamma, const float* alpha_host, int mean) {
    USTRUN_TRY(shape_ok(who, N, K, HW));
    c->N = N; c->K = K; c->HW = HW; c->has_alpha = alpha_host != nullptr; c->mean = mean; c->gamma = gamma;
    for (int k = 0; k < KMAX; ++k) c->alpha[k] = (alpha_host && k < K) ? alpha_host[k] : 1.f;
    return 0;
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int ustrun_consistency_fwd(const float* a, const float* b, int N, int K, int HW, int act, int kind, float* out,
                                      float* partials, int64_t partials_bytes, ustrun_stream_t s) {
    USTRUN_CHECK(a && b && out, "consistency_fwd: null pointer");
    USTRUN_TRY(shape_ok("consistency_fwd", N, K, HW));
    USTRUN_CHECK(act == USTRUN_LOSS_SOFTMAX || act == USTRUN_LOSS_SIGMOID, "consistency_fwd: bad activation %d", act);
    USTRUN_CHECK(kind >= USTRUN_CONS_MSE_MAP && kind <= USTRUN_CONS_SOFT_DICE, "consistency_fwd: bad kind %d", kind);
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    if (kind == USTRUN_CONS_MSE_MAP) {
        const bool vec = HW % 4 == 0 && al16(a) && al16(b) && al16(out);
        launch_v(vec, BY_K(K, cons_fwd_kernel, 4, USTRUN_CONS_MSE_MAP), BY_K(K, cons_fwd_kernel, 1, USTRUN_CONS_MSE_MAP), npix, st, a, b, N, K, HW, act,
                 out, (float*)nullptr);
        USTRUN_LAUNCH_CHECK("consistency_fwd");
        return 0;
    }
    USTRUN_TRY(partials_ok("consistency_fwd", partials, partials_bytes));
    const bool vec = HW % 4 == 0 && al16(a) && al16(b);
    const int rows = stream_blocks(vec ? npix / 4 : npix);
    if (kind == USTRUN_CONS_KL_MEAN)
        launch_v(vec, BY_K(K, cons_fwd_kernel, 4, USTRUN_CONS_KL_MEAN), BY_K(K, cons_fwd_kernel, 1, USTRUN_CONS_KL_MEAN), npix, st, a, b, N, K, HW, act,
                 (float*)nullptr, partials);
    else
        launch_v(vec, BY_K(K, cons_fwd_kernel, 4, USTRUN_CONS_SOFT_DICE), BY_K(K, cons_fwd_kernel, 1, USTRUN_CONS_SOFT_DICE), npix, st, a, b, N, K, HW,
                 act, (float*)nullptr, partials);
    USTRUN_LAUNCH_CHECK("consistency_fwd");
    if (kind == USTRUN_CONS_KL_MEAN) return finalize(partials, rows, 1, FIN_SCALE, K, 1.0 / ((double)npix * K), out, st, "consistency_finalize");
    return finalize(partials, rows, NS, FIN_SOFT_DICE, K, 0.0, out, st, "consistency_finalize");
}

extern "C" int ustrun_consistency_bwd(const float* a, const float* b, int N, int K, int HW, int act, int kind, const float* sums,
                                      const float* gout_dev, float* da, float* db, ustrun_stream_t s) {
    USTRUN_CHECK(a && b && gout_dev && (da || db), "consistency_bwd: null pointer");
    USTRUN_TRY(shape_ok("consistency_bwd", N, K, HW));
    USTRUN_CHECK(act == USTRUN_LOSS_SOFTMAX || act == USTRUN_LOSS_SIGMOID, "consistency_bwd: bad activation %d", act);
    USTRUN_CHECK(kind >= USTRUN_CONS_MSE_MAP && kind <= USTRUN_CONS_SOFT_DICE, "consistency_bwd: bad kind %d", kind);
    USTRUN_CHECK(kind != USTRUN_CONS_SOFT_DICE || sums, "consistency_bwd: the soft Dice needs the forward's sums");
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    const bool vec = HW % 4 == 0 && al16(a) && al16(b) && al16(da) && al16(db) && (kind != USTRUN_CONS_MSE_MAP || al16(gout_dev));
    if (kind == USTRUN_CONS_MSE_MAP)
        launch_v(vec, BY_K(K, cons_bwd_kernel, 4, USTRUN_CONS_MSE_MAP), BY_K(K, cons_bwd_kernel, 1, USTRUN_CONS_MSE_MAP), npix, st, a, b, N, K, HW, act,
                 sums, gout_dev, da, db);
    else if (kind == USTRUN_CONS_KL_MEAN)
        launch_v(vec, BY_K(K, cons_bwd_kernel, 4, USTRUN_CONS_KL_MEAN), BY_K(K, cons_bwd_kernel, 1, USTRUN_CONS_KL_MEAN), npix, st, a, b, N, K, HW, act,
                 sums, gout_dev, da, db);
    else
        launch_v(vec, BY_K(K, cons_bwd_kernel, 4, USTRUN_CONS_SOFT_DICE), BY_K(K, cons_bwd_kernel, 1, USTRUN_CONS_SOFT_DICE), npix, st, a, b, N, K, HW,
                 act, sums, gout_dev, da, db);
    USTRUN_LAUNCH_CHECK("consistency_bwd");
    return 0;
}

extern "C" int ustrun_entropy_fwd(const float* p, int N, int K, int HW, float factor, int mean, float* out, float* partials,
                                  int64_t partials_bytes, ustrun_stream_t s) {
    USTRUN_CHECK(p && out, "entropy_fwd: null pointer");
    USTRUN_TRY(shape_ok("entropy_fwd", N, K, HW));
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    if (!mean) {
        const bool vec = HW % 4 == 0 && al16(p) && al16(out);
        launch_v(vec, BY_K(K, entropy_fwd_kernel, 4, false), BY_K(K, entropy_fwd_kernel, 1, false), npix, st, p, N, K, HW, factor, out, (float*)nullptr);
        USTRUN_LAUNCH_CHECK("entropy_fwd");
        return 0;
    }
    USTRUN_TRY(partials_ok("entropy_fwd", partials, partials_bytes));
    const bool vec = HW % 4 == 0 && al16(p);
    launch_v(vec, BY_K(K, entropy_fwd_kernel, 4, true), BY_K(K, entropy_fwd_kernel, 1, true), npix, st, p, N, K, HW, factor, (float*)nullptr, partials);
    USTRUN_LAUNCH_CHECK("entropy_fwd");
    return finalize(partials, stream_blocks(vec ? npix / 4 : npix), 1, FIN_SCALE, K, 1.0 / (double)npix, out, st, "entropy_finalize");
}

extern "C" int ustrun_entropy_bwd(const float* p, int N, int K, int HW, float factor, int mean, const float* gout_dev, float* dp,
                                  ustrun_stream_t s) {
    USTRUN_CHECK(p && gout_dev && dp, "entropy_bwd: null pointer");
    USTRUN_TRY(shape_ok("entropy_bwd", N, K, HW));
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    const bool vec = HW % 4 == 0 && al16(p) && al16(dp) && (mean || al16(gout_dev));
    if (mean) launch_v(vec, BY_K(K, entropy_bwd_kernel, 4, true), BY_K(K, entropy_bwd_kernel, 1, true), npix, st, p, N, K, HW, factor, gout_dev, dp);
    else launch_v(vec, BY_K(K, entropy_bwd_kernel, 4, false), BY_K(K, entropy_bwd_kernel, 1, false), npix, st, p, N, K, HW, factor, gout_dev, dp);
    USTRUN_LAUNCH_CHECK("entropy_bwd");
    return 0;
}

extern "C" int ustrun_focal_fwd(const float* logits, const int64_t* target, int N, int K, int HW, float gamma, const float* alpha_host,
                                int mean, float* out, float* partials, int64_t partials_bytes, ustrun_stream_t s) {
    USTRUN_CHECK(logits && target && out, "focal_fwd: null pointer");
    FocalCfg c;
    USTRUN_TRY(focal_cfg(&c, "focal_fwd", N, K, HW, gamma, alpha_host, mean));
    USTRUN_TRY(partials_ok("focal_fwd", partials, partials_bytes));
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    const bool vec = HW % 4 == 0 && al16(logits);
    launch_v(vec, BY_K(K, focal_fwd_kernel, 4), BY_K(K, focal_fwd_kernel, 1), npix, st, c, logits, (const long long*)target, partials);
    USTRUN_LAUNCH_CHECK("focal_fwd");
    return finalize(partials, stream_blocks(vec ? npix / 4 : npix), 1, FIN_SCALE, K, mean ? 1.0 / (double)npix : 1.0, out, st, "focal_finalize");
}

extern "C" int ustrun_focal_bwd(const float* logits, const int64_t* target, int N, int K, int HW, float gamma, const float* alpha_host,
                                int mean, const float* gout_dev, float* dlogits, ustrun_stream_t s) {
    USTRUN_CHECK(logits && target && gout_dev && dlogits, "focal_bwd: null pointer");
    FocalCfg c;
    USTRUN_TRY(focal_cfg(&c, "focal_bwd", N, K, HW, gamma, alpha_host, mean));
    const hipStream_t st = (hipStream_t)s;
    const long npix = (long)N * HW;
    const bool vec = HW % 4 == 0 && al16(logits) && al16(dlogits);
    launch_v(vec, BY_K(K, focal_bwd_kernel, 4), BY_K(K, focal_bwd_kernel, 1), npix, st, c, logits, (const long long*)target, gout_dev, dlogits);
    USTRUN_LAUNCH_CHECK("focal_bwd");
    return 0;
}

extern "C" int ustrun_pair_sums(const float* a, const float* b, int64_t n, float* out, float* partials, int64_t partials_bytes,
                                ustrun_stream_t s) {
    USTRUN_CHECK(a && b && out && n > 0, "pair_sums: bad args");
    USTRUN_TRY(partials_ok("pair_sums", partials, partials_bytes));
    const hipStream_t st = (hipStream_t)s;
    const bool vec = al16(a) && al16(b);
    launch_v(vec, pair_sums_kernel<4>, pair_sums_kernel<1>, (long)n, st, a, b, (long)n, partials);
    USTRUN_LAUNCH_CHECK("pair_sums");
    return finalize(partials, stream_blocks(vec ? n / 4 : n), 6, FIN_PAIR, 1, 1.0 / (double)n, out, st, "pair_sums_finalize");
}

extern "C" int ustrun_pair_sums_bwd(const float* a, const float* b, int64_t n, int kind, const float* sums, const float* gout_dev,
                                    float* da, float* db, ustrun_stream_t s) {
    USTRUN_CHECK(a && b && sums && gout_dev && (da || db) && n > 0, "pair_sums_bwd: bad args");
    USTRUN_CHECK(kind >= USTRUN_PAIR_DICE_SQ && kind <= USTRUN_PAIR_MSE, "pair_sums_bwd: bad kind %d", kind);
    const hipStream_t st = (hipStream_t)s;
    const bool vec = al16(a) && al16(b) && al16(da) && al16(db);
    launch_v(vec, pair_bwd_kernel<4>, pair_bwd_kernel<1>, (long)n, st, a, b, (long)n, kind, sums, gout_dev, da, db);
    USTRUN_LAUNCH_CHECK("pair_sums_bwd");
    return 0;
}

extern "C" int ustrun_row_kl_fwd(const float* a, const float* b, int64_t rows, int C, float* out, float* partials,
                                 int64_t partials_bytes, ustrun_stream_t s) {
    USTRUN_CHECK(a && b && out && rows > 0 && C > 0, "row_kl_fwd: bad args");
    USTRUN_TRY(partials_ok("row_kl_fwd", partials, partials_bytes));
    const hipStream_t st = (hipStream_t)s;
    const int blocks = stream_blocks((long)rows);
    hipLaunchKernelGGL(row_kl_fwd_kernel, dim3(blocks), dim3(256), 0, st, a, b, (long)rows, C, partials);
    USTRUN_LAUNCH_CHECK("row_kl_fwd");
    return finalize(partials, blocks, 1, FIN_SCALE, 1, 0.5 / ((double)rows * C), out, st, "row_kl_finalize");
}

extern "C" int ustrun_row_kl_bwd(const float* a, const float* b, int64_t rows, int C, const float* gout_dev, float* da, float* db,
                                 ustrun_stream_t s) {
    USTRUN_CHECK(a && b && gout_dev && (da || db) && rows > 0 && C > 0, "row_kl_bwd: bad args");
    hipLaunchKernelGGL(row_kl_bwd_kernel, dim3(stream_blocks((long)rows)), dim3(256), 0, (hipStream_t)s, a, b, (long)rows, C, gout_dev, da,
                       db);
    USTRUN_LAUNCH_CHECK("row_kl_bwd");
    return 0;
}
