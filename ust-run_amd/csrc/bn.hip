// bn.hip -- train-mode BatchNorm2d statistics, and the BatchNorm+ReLU(+MaxPool) backward passes.
// All kernels here are HBM-bound streams over NHWC activations (4 channels = 16 B per lane) with
// fixed-order two-level reductions (block partials, then an f64 finalize) so results are
// reproducible run to run.
#include "common.h"
#include "loader.h"
#include "bn_bwd.h"

namespace ustrun {
namespace {

// ---- forward statistics -------------------------------------------------------------------
// block = 32 channels x 8 row lanes; stat[row][2][C] -> mean, biased var -> scale/shift
// Stage 1 for long statistics tables: block (cb, sp) sums its row range [sp*R, sp*R+R) of its 32 columns
// in f64 and parks the two sums IN PLACE, each as a (hi, lo) float pair, in its OWN cells: row sp*R holds
// the sum (q=0 cell: hi, q=1 cell: lo), row sp*R+1 the sum of squares.  Only this block reads those cells,
// and it does so before the barrier that precedes the writes.
// A shorter TAIL pass may follow the `passes` equal ones (BnTail: its rows start where theirs end; R = 0: too few rows for a first
// stage, the finalize sums them directly -- each pass goes through exactly the arithmetic a call of its own would).
__global__ __launch_bounds__(256) void bn_stat_stage1_kernel(float* stat, int rows, int C, int R, int passes, BnTail tail) {
    __shared__ double red[2][8][32];
    stat += (long)blockIdx.z * rows * 2 * C;            // blockIdx.z = forward pass (its own rows)
    if ((int)blockIdx.z == passes) { rows = tail.rows; R = tail.R; }      // the tail pass: its own rows and split
    if ((int)blockIdx.y * R >= rows) return;            // (grid.y covers the larger of the two split counts)
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl, r0 = blockIdx.y * R, r1 = min(rows, r0 + R);
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        int r = r0 + rg;
        for (; r + 24 < r1; r += 32) {               // four rows' loads issued before the first add, sums in ascending row order
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = stat[((long)(r + 8 * u) * 2 + 0) * C + c]; b[u] = stat[((long)(r + 8 * u) * 2 + 1) * C + c]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { s1 += (double)a[u]; s2 += (double)b[u]; }
        }
        for (; r < r1; r += 8) {
            s1 += (double)stat[((long)r * 2 + 0) * C + c];
            s2 += (double)stat[((long)r * 2 + 1) * C + c];
        }
    }
    red[0][rg][cl] = s1; red[1][rg][cl] = s2;
    __syncthreads();
    if (rg < 2 && c < C) {                   // rg 0 -> sum into row r0, rg 1 -> sum of squares into row r0+1
        double v = 0.0;
        for (int k = 0; k < 8; ++k) v += red[rg][k][cl];
        const float hi = (float)v, lo = __builtin_isfinite(hi) ? (float)(v - (double)hi) : 0.f;      // (an inf sum stays inf: inf - inf would park a NaN)
        stat[((long)(r0 + rg) * 2 + 0) * C + c] = hi;
        stat[((long)(r0 + rg) * 2 + 1) * C + c] = lo;
    }
}

// Both stages in ONE launch (the U-Net forward: 52 x 2 launches of ~7.5 us per step were launch latency, not work): block
// (cb, sp, g) does stage 1 for its row range, then takes a ticket for its channel block; the block that draws the last
// ticket -- every stage-1 sum of that channel block is then parked and visible (agent-scope release by the writers before
// the ticket, acquire by the reader after it) -- finalizes the channel block's passes one after the other with the very
// summation order of bn_finalize_kernel<true> (eight row lanes per pass, lanes added in ascending order), so the constants
// are bit-identical to the two-launch form.  tickets[cb] returns to 0 for the next launch on the same stream.
__global__ __launch_bounds__(256) void bn_stat_fused_kernel(float* stat, int rows, int C, double count, int R,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* rm, float* rv, int64_t* nbt, float momentum, float eps,
                                                            int update, float* scale, float* shift, float* mean, float* rstd,
                                                            int passes, long astride, unsigned* tickets) {
    constexpr int PPR = 4;                                 // passes finalized per round (their loads in flight together)
    __shared__ double red[2][PPR][8][32];
    __shared__ bool last;
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    {
        float* st = stat + (long)blockIdx.z * rows * 2 * C;
        const int r0 = blockIdx.y * R, r1 = min(rows, r0 + R);
        double s1 = 0.0, s2 = 0.0;
        for (int r = r0 + rg; r < r1; r += 8) {
            s1 += (double)st[((long)r * 2 + 0) * C + c];
            s2 += (double)st[((long)r * 2 + 1) * C + c];
        }
        red[0][0][rg][cl] = s1; red[1][0][rg][cl] = s2;
        __syncthreads();
        if (rg < 2) {
            double v = 0.0;
            for (int k = 0; k < 8; ++k) v += red[rg][0][k][cl];
            const float hi = (float)v, lo = __builtin_isfinite(hi) ? (float)(v - (double)hi) : 0.f;
            // write-through (sc1) stores, drained by every storing wave before the barrier in front of the ticket: no agent
            // release -- that is a write-back of the XCD's L2 (MI355X_MICROARCH.md, fence table), which the convolution has
            // just filled with dirty output lines: with it this kernel cost the step 0.6 ms MORE than the two launches
            __hip_atomic_store(st + ((long)(r0 + rg) * 2 + 0) * C + c, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(st + ((long)(r0 + rg) * 2 + 1) * C + c, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned total = gridDim.y * gridDim.z;
        const unsigned t = __hip_atomic_fetch_add(tickets + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == total - 1;
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");        // (the other blocks' parked sums: not from this CU's L1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          //  and every load of them below is an sc1 load as well)
    __syncthreads();
    double run_m = 0.0, run_v = 0.0;
    if (update && rg == 0) { run_m = (double)rm[c]; run_v = (double)rv[c]; }
    // a row lane holds the splits rg, rg + 8, .. (at most four: the launcher splits a table into <= 32 ranges) of up to PPR
    // passes: every load of the round is issued before the first sum
    for (int g0 = 0; g0 < passes; g0 += PPR) {
        float v[PPR][4][4];
#pragma unroll
        for (int q = 0; q < PPR; ++q) {
            const float* st = stat + (long)(g0 + q < passes ? g0 + q : 0) * rows * 2 * C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sp = rg + 8 * k;
                const bool ok = g0 + q < passes && sp * R < rows;
                const long a0 = (long)(sp * R) * 2 * C + c, a1 = (long)(sp * R + 1) * 2 * C + c;
                const long z = ok ? 0 : -1;               // (absent: the block's own first cell, value unused)
                const float x0 = __hip_atomic_load(st + (a0 & ~z) , __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const float x1 = __hip_atomic_load(st + ((a0 + C) & ~z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const float x2 = __hip_atomic_load(st + (a1 & ~z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const float x3 = __hip_atomic_load(st + ((a1 + C) & ~z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[q][k][0] = ok ? x0 : 0.f; v[q][k][1] = ok ? x1 : 0.f;
                v[q][k][2] = ok ? x2 : 0.f; v[q][k][3] = ok ? x3 : 0.f;
            }
        }
        __syncthreads();                                       // (red: the previous round's sums are consumed)
#pragma unroll
        for (int q = 0; q < PPR; ++q) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                      // (x + 0.0 leaves x: absent splits do not change the sums)
                s1 += (double)v[q][k][0] + (double)v[q][k][1];
                s2 += (double)v[q][k][2] + (double)v[q][k][3];
            }
            red[0][q][rg][cl] = s1; red[1][q][rg][cl] = s2;
        }
        __syncthreads();
        if (rg == 0) {
            for (int q = 0; q < PPR && g0 + q < passes; ++q) {
                double t1 = 0.0, t2 = 0.0;
                for (int k = 0; k < 8; ++k) { t1 += red[0][q][k][cl]; t2 += red[1][q][k][cl]; }
                const double m = t1 / count;
                double var = t2 / count - m * m;
                if (var < 0.0) var = 0.0;
                const double rs = 1.0 / sqrt(var + (double)eps);
                const long o = (long)(g0 + q) * astride + c;
                scale[o] = (float)((double)gamma[c] * rs);
                shift[o] = (float)((double)beta[c] - m * (double)gamma[c] * rs);
                mean[o] = (float)m; rstd[o] = (float)rs;
                if (update) {
                    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
                    run_m = (double)(float)((1.0 - momentum) * run_m + momentum * m);
                    run_v = (double)(float)((1.0 - momentum) * run_v + momentum * unb);
                }
            }
        }
    }
    if (update && rg == 0) { rm[c] = (float)run_m; rv[c] = (float)run_v; }
    if (update && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += passes;
    if (threadIdx.x == 0) __hip_atomic_store(tickets + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `passes` forward passes batched into one launch: pass g owns rows [g*rows, (g+1)*rows) of stat and the constants at
// scale/shift/mean/rstd + g*astride; the running buffers receive the passes' updates one after the other, exactly as
// `passes` separate calls would apply them.
template <bool PRE>
__global__ void bn_finalize_kernel(const float* __restrict__ stat, int rows, int C, double count, int R,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* rm, float* rv, int64_t* nbt, float momentum, float eps, int update,
                                   float* scale, float* shift, float* mean, float* rstd, int passes, long astride, BnTail tail) {
    __shared__ double red[2][32][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;      // 32 channels x 32 row lanes
    const int full = passes;                                     // the equal passes; then the tail, if any
    const int rows_f = rows, R_f = R;
    const double count_f = count;
    if (tail.rows > 0) ++passes;
    const int c = blockIdx.x * 32 + cl;
    double run_m = 0.0, run_v = 0.0;
    if (update && rg == 0 && c < C) { run_m = (double)rm[c]; run_v = (double)rv[c]; }
    // The 32 row lanes work on up to four passes at once, eight lanes per pass (the passes' row sums are independent;
    // only the running-buffer update is sequential): one round of loads instead of one per pass.  A pass always gets
    // eight lanes, so its sums are formed in the same order whether it comes alone or batched with others.
    constexpr int LPP = 8, PPR = 32 / LPP;                        // lanes per pass, passes per round
    const int gl = rg / LPP, lane = rg % LPP;
    for (int g0 = 0; g0 < passes; g0 += PPR) {
        const int g = g0 + gl;
        double s1 = 0.0, s2 = 0.0;
        if (c < C && g < passes) {
            const float* st = stat + (long)g * rows_f * 2 * C;
            rows = g < full ? rows_f : tail.rows; R = g < full ? R_f : tail.R;
            if (PRE && R > 0) {       // stage-1 doubles parked at rows sp*R / sp*R+1, columns of this channel block
                // at most 32 splits (the launcher's R), i.e. four per lane: all sixteen loads issued before the first sum (one
                // split per trip was four dependent memory round trips in a 7 us kernel); x + 0.0 leaves x, so the absent
                // splits' zeros do not change the sums
                float v[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sp = lane + LPP * k;
                    const bool ok = sp * R < rows;
                    const long a0 = ok ? (long)(sp * R) * 2 * C + c : c, a1 = ok ? (long)(sp * R + 1) * 2 * C + c : c;
                    const float x0 = st[a0], x1 = st[a0 + C], x2 = st[a1], x3 = st[a1 + C];
                    v[k][0] = ok ? x0 : 0.f; v[k][1] = ok ? x1 : 0.f; v[k][2] = ok ? x2 : 0.f; v[k][3] = ok ? x3 : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s1 += (double)v[k][0] + (double)v[k][1];
                    s2 += (double)v[k][2] + (double)v[k][3];
                }
                for (int sp = lane + 4 * LPP; sp * R < rows; sp += LPP) {       // (a table split finer than the launcher does)
                    const long a0 = (long)(sp * R) * 2 * C + c, a1 = (long)(sp * R + 1) * 2 * C + c;
                    s1 += (double)st[a0] + (double)st[a0 + C];
                    s2 += (double)st[a1] + (double)st[a1 + C];
                }
            } else {
#pragma unroll 8
                for (int r = lane; r < rows; r += LPP) {        // (unrolled: the loads of eight rows in flight together)
                    s1 += (double)st[((long)r * 2 + 0) * C + c];
                    s2 += (double)st[((long)r * 2 + 1) * C + c];
                }
            }
        }
        red[0][rg][cl] = s1; red[1][rg][cl] = s2;
        __syncthreads();
        if (rg == 0 && c < C) {
            for (int q = 0; q < PPR && g0 + q < passes; ++q) {     // the round's passes, in order
                double t1 = 0.0, t2 = 0.0;
                for (int k = 0; k < LPP; ++k) { t1 += red[0][q * LPP + k][cl]; t2 += red[1][q * LPP + k][cl]; }
                count = g0 + q < full ? count_f : tail.count;
                const double m = t1 / count;
                double var = t2 / count - m * m;
                if (var < 0.0) var = 0.0;
                const double rs = 1.0 / sqrt(var + (double)eps);
                const long o = (long)(g0 + q) * astride + c;
                scale[o] = (float)((double)gamma[c] * rs);
                shift[o] = (float)((double)beta[c] - m * (double)gamma[c] * rs);
                mean[o] = (float)m; rstd[o] = (float)rs;
                if (update) {    // through float after every pass, as the stored buffer of separate calls would be
                    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
                    run_m = (double)(float)((1.0 - momentum) * run_m + momentum * m);
                    run_v = (double)(float)((1.0 - momentum) * run_v + momentum * unb);
                }
            }
        }
        __syncthreads();
    }
    if (update && rg == 0 && c < C) { rm[c] = (float)run_m; rv[c] = (float)run_v; }
    if (update && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += passes;
}

__global__ void bn_eval_affine_kernel(int C, const float* gamma, const float* beta, const float* rm,
                                      const float* rv, float eps, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const float sc = gamma[c] * (1.0f / sqrtf(rv[c] + eps));
        scale[c] = sc; shift[c] = beta[c] - rm[c] * sc;
    }
}

// eval mode: the 18 layers' constants in ONE launch (blockIdx.y = layer x pass), instead of 18 five-microsecond ones
struct EvalAffineJobs {
    const float *gamma[18], *beta[18], *rm[18], *rv[18];
    float* aff[18];          // layer's table: pass g at aff + g * 4C: {scale[C], shift[C], running_mean[C], rstd[C]}
    int C[18];
};
__global__ void bn_eval_affine_multi_kernel(const EvalAffineJobs j, float eps, int passes) {
    const int l = blockIdx.y / passes, g = blockIdx.y % passes, C = j.C[l];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const float rs = 1.0f / sqrtf(j.rv[l][c] + eps);
        const float sc = j.gamma[l][c] * rs;
        float* a = j.aff[l] + 4L * C * g;
        a[c] = sc; a[C + c] = j.beta[l][c] - j.rm[l][c] * sc;
        a[2 * C + c] = j.rm[l][c]; a[3 * C + c] = rs;       // mean, rstd: what the frozen backward's dgamma needs
    }
}

// a = relu(y*scale+shift) materialised (NHWC -> NHWC or NCHW)
__global__ void bn_relu_apply_kernel(const float* __restrict__ y, int esz, const float* __restrict__ scale,
                                     const float* __restrict__ shift, long npix, int C, int HW,
                                     float* __restrict__ out, int nchw) {
    const long total = npix * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long p = e / C; const int c = (int)(e - p * C);
        float v = ld1(y, e, esz);
        if (scale) v = fmaxf(v * scale[c] + shift[c], 0.f);
        if (nchw) { const long n = p / HW; const long hw = p - n * HW; out[(n * C + c) * HW + hw] = v; }
        else out[e] = v;
    }
}

// a = relu(y*scale+shift) in the 16-bit storage type, NHWC -> NHWC, per-pass constants: the operand of a DoubleConv's second
// convolution written out once (8 channels = 16 bytes per lane, four pixels in flight per thread) where applying BatchNorm + ReLU
// per staged item costs that convolution and its weight gradient more than this pass does (unet.hip: the levels from 256 channels)
__global__ __launch_bounds__(256) void act16_kernel(const elt_t* __restrict__ y, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, int relu, int gN, long gstride,
                                                    long npix, int HW, int C, elt_t* __restrict__ out) {
    const int CV = C / 8, PPB = 256 / CV;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    if (pl >= PPB) return;
    constexpr int U = 4;
    const long stride = (long)gridDim.x * PPB;
    for (long p0 = (long)blockIdx.x * PPB + pl; p0 < npix; p0 += U * stride) {
        bf16x8 r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const long p = p0 + u * stride; r[u] = *(const bf16x8*)(y + (p < npix ? p : npix - 1) * C + cv * 8); }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long p = p0 + u * stride;
            if (p >= npix) break;
            const int grp = gN > 0 ? (int)((unsigned)((unsigned)p / (unsigned)HW) / (unsigned)gN) : 0;      // (pixels < 2^32: host check)
            const float* ps = scale + grp * gstride + cv * 8;
            const float* pb = shift + grp * gstride + cv * 8;
            const f32x4 s0 = *(const f32x4*)ps, s1 = *(const f32x4*)(ps + 4), b0 = *(const f32x4*)pb, b1 = *(const f32x4*)(pb + 4);
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float a = (float)r[u][j] * (j < 4 ? s0[j & 3] : s1[j & 3]) + (j < 4 ? b0[j & 3] : b1[j & 3]);
                a = relu ? fmaxf(a, 0.f) : a;
                o[j] = (elt_t)a;
            }
            *(bf16x8*)(out + p * C + cv * 8) = o;
        }
    }
}

// pooled activation p[n][y][x][c] = max over the 2x2 window of relu(s*y + b): the Down block's MaxPool2d input,
// materialised once (a quarter of y) so that the Down convolution and its weight gradient read a plain tensor by
// LDS-DMA instead of pooling four pixels per staged item in an issue-bound kernel.  8 channels (ESZ = 2) or 4
// (ESZ = 4) per thread; batched passes pick their constants per image.
template <int ESZ>
__global__ __launch_bounds__(256) void pool_act_kernel(const float* __restrict__ y, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, int relu, int gN, long gstride,
                                                      int N, int H, int W, int C, float* __restrict__ out,
                                                      elt_t* __restrict__ act) {
    constexpr int V = ESZ == 2 ? 8 : 4;             // channels per thread: one 16-byte load per window pixel
    const int Hp = H / 2, Wp = W / 2, CV = C / V;
    // a thread keeps its channel group (256 % CV == 0 for the power-of-two channel counts; else it re-derives it)
    const long npix = (long)N * Hp * Wp;
    const int PPB = 256 / CV > 0 ? 256 / CV : 1;
    const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
    if (pl >= PPB) return;
    float sc[V], sh[V];
    // the constants are (re)loaded every pixel, unconditionally (L1 hits): a "reload when the pass changes" branch kept the
    // compiler from overlapping one pixel's loads with the next one's
#pragma unroll 2
    for (long p = (long)blockIdx.x * PPB + pl; p < npix; p += (long)gridDim.x * PPB) {
        const unsigned up = (unsigned)p, t = up / (unsigned)Wp;      // 32-bit divides (pooled pixels < 2^32: host check)
        const int px = (int)(up - t * (unsigned)Wp), n = (int)(t / (unsigned)Hp), py = (int)(t - (unsigned)n * (unsigned)Hp);
        const int grp = gN > 0 ? n / gN : 0;
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
            const f32x4 s4 = scale ? *(const f32x4*)(scale + grp * gstride + cv * V + 4 * h) : (f32x4){1.f, 1.f, 1.f, 1.f};
            const f32x4 b4 = scale ? *(const f32x4*)(shift + grp * gstride + cv * V + 4 * h) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) { sc[4 * h + k] = s4[k]; sh[4 * h + k] = b4[k]; }
        }
        const long base = (((long)n * H + 2 * py) * W + 2 * px) * C + cv * V;
        float v[4][V];
        if (ESZ == 2) {
            bf16x8 r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = *(const bf16x8*)((const elt_t*)y + base + ((q >> 1) * (long)W + (q & 1)) * C);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < V; ++j) v[q][j] = (float)r[q][j % 8];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 r = *(const f32x4*)(y + base + ((q >> 1) * (long)W + (q & 1)) * C);
#pragma unroll
                for (int j = 0; j < V; ++j) v[q][j] = r[j % 4];
            }
        }
        float m[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float a = v[q][j] * sc[j] + sh[j];
                a = relu ? fmaxf(a, 0.f) : a;
                v[q][j] = a;
                m[j] = q == 0 ? a : fmaxf(m[j], a);
            }
        }
        if (ESZ == 2 && act) {                      // the window's four activated pixels, as the concat convolution will read them
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bf16x8 a8;
#pragma unroll
                for (int j = 0; j < 8; ++j) a8[j] = (elt_t)v[q][j % V];
                *(bf16x8*)(act + base + ((q >> 1) * (long)W + (q & 1)) * C) = a8;
            }
        }
        const long ob = (((long)n * Hp + py) * Wp + px) * C + cv * V;
        if (ESZ == 2) {                                     // one 16-byte store
            bf16x8 o8;
#pragma unroll
            for (int j = 0; j < 8; ++j) o8[j] = (elt_t)m[j % V];
            *(bf16x8*)((elt_t*)out + ob) = o8;
        } else {
#pragma unroll
            for (int h = 0; h < V / 4; ++h) st4t<ESZ>(out, ob + 4 * h, (f32x4){m[4 * h], m[4 * h + 1], m[4 * h + 2], m[4 * h + 3]});
        }
    }
}

// plain MaxPool2d(2) backward (stand-alone Down block): dx = dp routed to the first maximum of each window (torch's
// tie rule: row-major scan, strict >), zero elsewhere, incl. the odd last row/column the pooling drops
template <int ESZ>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ x, int N, int H,
                                                         int W, int C, float* __restrict__ dx) {
    const int Hp = H / 2, Wp = W / 2;
    const long total = (long)N * H * W * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C); long t = e / C;
        const int ix = (int)(t % W); t /= W;
        const int iy = (int)(t % H); const int n = (int)(t / H);
        const int py = iy >> 1, px = ix >> 1;
        float g = 0.f;
        if (py < Hp && px < Wp) {
            const long b = (((long)n * H + 2 * py) * W + 2 * px) * C + c;
            int best = 0; float bv = ld1(x, b, ESZ);
            const float v1 = ld1(x, b + C, ESZ), v2 = ld1(x, b + (long)W * C, ESZ), v3 = ld1(x, b + (long)W * C + C, ESZ);
            if (v1 > bv) { bv = v1; best = 1; }
            if (v2 > bv) { bv = v2; best = 2; }
            if (v3 > bv) { bv = v3; best = 3; }
            if (best == ((iy & 1) * 2 + (ix & 1))) g = ld1(dp, (((long)n * Hp + py) * Wp + px) * C + c, ESZ);
        }
        st1(dx, e, g, ESZ);
    }
}

// ---- backward -------------------------------------------------------------------------------
// (the kernels: bn_bwd.h)
// 8-channel kernels: bf16, no pooling, C / 8 a power of two <= 256 (every layer of the U-Net and of ResNet-50/101);
// ustrun_debug_flags bit 12 (4096) keeps the 4-channel kernels (A/B runs)
static bool x8_ok(int C, bool pool, int dtype) {
    if (g_debug_flags & 4096) return false;
    const int g8 = C / 8;
    return dtype == USTRUN_D16 && !pool && C % 8 == 0 && g8 >= 1 && g8 <= 256 && (g8 & (g8 - 1)) == 0;
}

// ustrun_debug_last_bn_variant: 0x424E0000 ('BN') | pass (0 reduce, 1 apply, 2 frozen) << 8 | element bytes << 4 | even windows << 2 |
// pooled << 1 | eight channels per lane; per calling thread
thread_local int g_last_bn_variant = 0;
void note_bn_variant(int pass, int esz, bool even, bool pool, bool x8) {
    g_last_bn_variant = 0x424E0000 | pass << 8 | esz << 4 | (even ? 4 : 0) | (pool ? 2 : 0) | (x8 ? 1 : 0);
}

int group_size(int C4) { int g = 1; while (g < C4 && g < 256) g <<= 1; return g; }

int reduce_blocks(long nwin, int G) {
    const int PL = 256 / G;
    long b = (nwin + (long)PL * 8 - 1) / ((long)PL * 8);   // >= 8 windows per thread
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

// What the launchers of the three stream passes share: the build that serves a call, and its grid.
struct BnBwdPlan {
    bool pool, even, x8;
    int G, blocks;          // channel groups per block (C / 8 with x8); grid x
    long nwin;              // windows (pixels, or 2x2 pooling windows) per pass
    PassOff po;
};

// pass: BN_REDUCE / BN_APPLY / BN_FROZEN.  sums: the launch leaves partial rows -- the passes' rows share the 1024-row table, so
// the grid is the reduce pass's; without them it is the apply pass's.
int bn_bwd_plan(BnBwdPlan& p, int pass, int N, int H, int W, int C, int dtype, int passes, bool has_da, bool has_dp, bool sums,
                long act_elems, long pool_elems, long aff_stride) {
    static const char* const names[] = {"bn_bwd_reduce", "bn_bwd_apply", "bn_bwd_frozen"};
    const char* nm = names[pass];
    USTRUN_CHECK(dtype_ok(dtype), "%s: dtype %d not built", nm, dtype);
    USTRUN_CHECK(N > 0 && H > 0 && W > 0 && C % 4 == 0 && C > 0 && passes >= 1 && (!sums || passes <= 64),
                 "%s: N=%d H=%d W=%d C=%d (must be a multiple of 4) passes=%d", nm, N, H, W, C, passes);
    // (H < 2 or W < 2: the pooled map has no elements, and window_dz loads dp[c] whether or not the window has a pooled cell)
    USTRUN_CHECK(!has_dp || (H >= 2 && W >= 2), "%s: pooled windows need H, W >= 2 (%dx%d)", nm, H, W);
    p.pool = has_dp;
    p.even = p.pool && !(H & 1) && !(W & 1);
    p.x8 = x8_ok(C, p.pool, dtype) && has_da;
    p.G = p.x8 ? C / 8 : group_size(C / 4);
    p.nwin = p.pool ? (long)N * ((H + 1) / 2) * ((W + 1) / 2) : (long)N * H * W;
    USTRUN_CHECK(p.nwin < (1L << 31), "%s: %ld windows per pass", nm, p.nwin);
    if (sums) {
        p.blocks = reduce_blocks(p.nwin, p.G);
        if (p.blocks > 1024 / passes) p.blocks = 1024 / passes;
    } else {
        const int PL = 256 / p.G;
        const long b = (p.nwin + (long)PL * 4 - 1) / ((long)PL * 4);
        p.blocks = b > 4096 ? 4096 : (int)b;
    }
    p.po = {act_elems, pool_elems, aff_stride, sums ? (long)p.blocks * 2 * C : 0, pass == BN_FROZEN ? 0 : 3L * C};
    note_bn_variant(pass, act_esz(dtype), p.even, p.pool, p.x8);
    return 0;
}

// the 4-channel kernels' <POOL, ESZ, EVEN> from (pool, dtype, even): f(std::bool_constant, std::integral_constant<int>, std::bool_constant)
template <typename F>
void bn_bwd_dispatch(int dtype, const BnBwdPlan& p, F&& f) {
    auto by_esz = [&](auto pool, auto even) {
        if (dtype == USTRUN_D16) f(pool, std::integral_constant<int, 2>{}, even);
        else f(pool, std::integral_constant<int, 4>{}, even);
    };
    if (p.even) by_esz(std::true_type{}, std::true_type{});
    else if (p.pool) by_esz(std::true_type{}, std::false_type{});
    else by_esz(std::false_type{}, std::false_type{});
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

namespace ustrun {
int bn_finalize_passes(float* stat, int mtiles, int passes, int C, int64_t count, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                       int update_running, float* scale, float* shift, float* mean, float* rstd, long astride, hipStream_t s,
                       unsigned* tickets, int tail_rows, int64_t tail_count) {
    USTRUN_CHECK(stat && gamma && beta && scale && shift && mean && rstd, "bn_finalize: null pointer");
    USTRUN_CHECK(tail_rows >= 0 && tail_rows <= mtiles && (tail_rows == 0 || tail_count > 0), "bn_finalize: tail of %d rows", tail_rows);
    BnTail tail = {tail_rows, 0, (double)tail_count};
    if (tail_rows >= 96 && C % 32 == 0) {       // the split a call of its own would choose for these rows
        tail.R = cdiv(tail_rows, 32);
        while (tail_rows % tail.R == 1) ++tail.R;
    }
    if (tail_rows > 0) tickets = nullptr;       // (the one-launch form knows no tail)
    USTRUN_CHECK(!update_running || (running_mean && running_var), "bn_finalize: running buffers missing");
    USTRUN_CHECK(mtiles > 0 && passes > 0 && C > 0 && count > 0, "bn_finalize: empty");
    // Two stages from 96 rows up (the first one rewrites `stat` in place): one block per 32 channels pulls the whole table
    // through ONE CU (262 KB for 256 rows x 4 passes: 24 us measured, 368 launches per step), the staged form spreads it over
    // 32 x passes blocks per channel block (6 + 5.5 us).
    if (mtiles >= 96 && C % 32 == 0) {
        int R = cdiv(mtiles, 32);
        while (mtiles % R == 1) ++R;         // every split needs two rows to park its sums in
        if (tickets && cdiv(mtiles, R) <= 32) {       // (zeroed by the caller once; C / 32 <= BN_TICKETS counters, back at zero when the launch retires)
            USTRUN_CHECK(C / 32 <= BN_TICKETS, "bn_finalize: %d channels exceed the ticket table", C);
            hipLaunchKernelGGL(bn_stat_fused_kernel, dim3(C / 32, cdiv(mtiles, R), passes), dim3(256), 0, s, (float*)stat, mtiles,
                               C, (double)count, R, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                               update_running, scale, shift, mean, rstd, passes, astride, tickets);
            USTRUN_LAUNCH_CHECK("bn_stat_fused");
            return 0;
        }
        // the tail's split is its own (fewer rows, smaller R): it can need MORE y-blocks than the equal passes (ADVICE r5:
        // 144 rows -> R 5 -> 29 blocks, a 96-row tail -> R 3 -> 32), so the grid covers both and each block checks its range
        const int ysplits = std::max(cdiv(mtiles, R), tail.R > 0 ? cdiv(tail.rows, tail.R) : 0);
        hipLaunchKernelGGL(bn_stat_stage1_kernel, dim3(C / 32, ysplits, passes + (tail.R > 0 ? 1 : 0)), dim3(256), 0, s,
                           (float*)stat, mtiles, C, R, passes, tail);
        USTRUN_LAUNCH_CHECK("bn_stat_stage1");
        hipLaunchKernelGGL(bn_finalize_kernel<true>, dim3(C / 32), dim3(1024), 0, s, stat, mtiles, C, (double)count, R, gamma,
                           beta, running_mean, running_var, num_batches_tracked, momentum, eps, update_running, scale, shift,
                           mean, rstd, passes, astride, tail);
    } else {
        hipLaunchKernelGGL(bn_finalize_kernel<false>, dim3(cdiv(C, 32)), dim3(1024), 0, s, stat, mtiles, C, (double)count, 0,
                           gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, update_running, scale,
                           shift, mean, rstd, passes, astride, tail);
    }
    USTRUN_LAUNCH_CHECK("bn_finalize");
    return 0;
}
}  // namespace ustrun

extern "C" int ustrun_bn_finalize(float* stat, int mtiles, int C, int64_t count, const float* gamma,
                                  const float* beta, float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, float momentum, float eps, int update_running,
                                  float* scale, float* shift, float* mean, float* rstd, ustrun_stream_t s) {
    return bn_finalize_passes(stat, mtiles, 1, C, count, gamma, beta, running_mean, running_var, num_batches_tracked, momentum,
                              eps, update_running, scale, shift, mean, rstd, 0, (hipStream_t)s);
}

extern "C" int ustrun_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                                     const float* running_var, float eps, float* scale, float* shift,
                                     ustrun_stream_t s) {
    USTRUN_CHECK(C > 0 && gamma && beta && running_mean && running_var && scale && shift, "bn_eval_affine: bad args");
    hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)s, C, gamma, beta,
                       running_mean, running_var, eps, scale, shift);
    USTRUN_LAUNCH_CHECK("bn_eval_affine");
    return 0;
}

namespace ustrun {
// used by the U-Net forward in eval mode
int bn_eval_affine_layers(int nlayers, const int* C, const float* const* gamma, const float* const* beta,
                          const float* const* rm, const float* const* rv, float* const* aff, float eps, int passes,
                          hipStream_t s) {
    USTRUN_CHECK(nlayers > 0 && nlayers <= 18 && passes >= 1, "bn_eval_affine_layers: %d layers", nlayers);
    EvalAffineJobs j;
    int cmax = 0;
    for (int l = 0; l < nlayers; ++l) {
        USTRUN_CHECK(gamma[l] && beta[l] && rm[l] && rv[l] && aff[l] && C[l] > 0, "bn_eval_affine_layers: null pointer");
        j.gamma[l] = gamma[l]; j.beta[l] = beta[l]; j.rm[l] = rm[l]; j.rv[l] = rv[l]; j.aff[l] = aff[l]; j.C[l] = C[l];
        cmax = C[l] > cmax ? C[l] : cmax;
    }
    hipLaunchKernelGGL(bn_eval_affine_multi_kernel, dim3(cdiv(cmax, 256), nlayers * passes), dim3(256), 0, s, j, eps, passes);
    USTRUN_LAUNCH_CHECK("bn_eval_affine_layers");
    return 0;
}
}  // namespace ustrun

extern "C" int ustrun_bn_relu_apply(const void* y, const float* scale, const float* shift, int64_t npix, int C,
                                    int HW, float* out, int out_nchw, int dtype, ustrun_stream_t s) {
    USTRUN_CHECK(dtype_ok(dtype), "bn_relu_apply: dtype %d not built", dtype);
    USTRUN_CHECK(y && out && npix > 0 && C > 0 && HW > 0, "bn_relu_apply: bad args");
    int blocks = cdiv(npix * C, 256 * 4);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, (const float*)y, act_esz(dtype), scale,
                       shift, (long)npix, C, HW, out, out_nchw);
    USTRUN_LAUNCH_CHECK("bn_relu_apply");
    return 0;
}

extern "C" int ustrun_act16(const ustrun_src_t* src, int N, void* out, int dtype, ustrun_stream_t s) {
    USTRUN_CHECK(dtype == USTRUN_D16, "act16: 16-bit storage only (dtype %d)", dtype);
    USTRUN_CHECK(src && src->ptr && src->scale && src->shift && out && N > 0, "act16: bad args");
    const int C = src->C, H = src->H, W = src->W;
    USTRUN_CHECK(src->sC == 1 && src->sW == C && src->sH == (int64_t)W * C && src->sN == (int64_t)H * W * C && !src->pool &&
                 !src->off_y && !src->off_x && !src->f32, "act16: source must be a plain contiguous NHWC activation");
    USTRUN_CHECK(C % 8 == 0 && C / 8 <= 256, "act16: C=%d unsupported", C);       // (256 / (C/8) pixels per block; spare threads idle)
    const long npix = (long)N * H * W;
    USTRUN_CHECK(npix < (1L << 32), "act16: %ld pixels", npix);
    const int ppb = 256 / (C / 8);
    long nb = (npix + ppb * 8 - 1) / (ppb * 8);
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(act16_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)s, (const elt_t*)src->ptr, src->scale, src->shift,
                       src->relu, src->gN, (long)src->gstride, npix, H * W, C, (elt_t*)out);
    USTRUN_LAUNCH_CHECK("act16");
    return 0;
}

extern "C" int ustrun_pool_act(const ustrun_src_t* src, int N, void* out, int dtype, ustrun_stream_t s) {
    return ustrun_pool_act2(src, N, out, nullptr, dtype, s);
}

extern "C" int ustrun_pool_act2(const ustrun_src_t* src, int N, void* out, void* act, int dtype, ustrun_stream_t s) {
    USTRUN_CHECK(dtype_ok(dtype), "pool_act: dtype %d not built", dtype);
    USTRUN_CHECK(src && src->ptr && out && N > 0, "pool_act: bad args");
    USTRUN_CHECK(!act || (dtype == USTRUN_D16 && !(src->H & 1) && !(src->W & 1)),
                 "pool_act: the un-pooled activation needs 16-bit storage and even extents (%dx%d)", src->H, src->W);
    const int C = src->C, H = src->H, W = src->W, V = dtype == USTRUN_D16 ? 8 : 4;
    USTRUN_CHECK(C % V == 0 && H >= 2 && W >= 2, "pool_act: C=%d extent %dx%d unsupported", C, H, W);
    USTRUN_CHECK(src->sC == 1 && src->sW == C && src->sH == (int64_t)W * C && src->sN == (int64_t)H * W * C && !src->pool &&
                 !src->off_y && !src->off_x && !src->f32, "pool_act: source must be a plain contiguous NHWC activation");
    USTRUN_CHECK((src->scale == nullptr) == (src->shift == nullptr), "pool_act: scale/shift must come together");
    USTRUN_CHECK(C / V <= 256, "pool_act: C=%d too wide", C);
    const long npix = (long)N * (H / 2) * (W / 2);
    USTRUN_CHECK(npix < (1L << 32), "pool_act: %ld pooled pixels", npix);
    const int ppb = 256 / (C / V);
    long nb = (npix + ppb * 4 - 1) / (ppb * 4);             // about four pixels per thread
    if (nb > 16384) nb = 16384;
    if (nb < 1) nb = 1;
    const int blocks = (int)nb;
    const int gN = src->scale ? src->gN : 0;
    if (dtype == USTRUN_D16)
        hipLaunchKernelGGL(pool_act_kernel<2>, dim3(blocks), dim3(256), 0, (hipStream_t)s, (const float*)src->ptr, src->scale,
                           src->shift, src->relu, gN, (long)src->gstride, N, H, W, C, (float*)out, (elt_t*)act);
    else
        hipLaunchKernelGGL(pool_act_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)s, (const float*)src->ptr, src->scale,
                           src->shift, src->relu, gN, (long)src->gstride, N, H, W, C, (float*)out, (elt_t*)nullptr);
    USTRUN_LAUNCH_CHECK("pool_act");
    return 0;
}

extern "C" int ustrun_maxpool_bwd(const void* dp, const void* x, int N, int H, int W, int C, void* dx, int dtype,
                                  ustrun_stream_t s) {
    USTRUN_CHECK(dtype_ok(dtype), "maxpool_bwd: dtype %d not built", dtype);
    USTRUN_CHECK(dp && x && dx && N > 0 && H >= 2 && W >= 2 && C > 0, "maxpool_bwd: bad args");
    const long total = (long)N * H * W * C;
    long nb = (total + 1023) / 1024;
    if (nb > 8192) nb = 8192;
    if (dtype == USTRUN_D16)
        hipLaunchKernelGGL(maxpool_bwd_kernel<2>, dim3((int)nb), dim3(256), 0, (hipStream_t)s, (const float*)dp, (const float*)x, N, H,
                           W, C, (float*)dx);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<4>, dim3((int)nb), dim3(256), 0, (hipStream_t)s, (const float*)dp, (const float*)x, N, H,
                           W, C, (float*)dx);
    USTRUN_LAUNCH_CHECK("maxpool_bwd");
    return 0;
}

extern "C" int64_t ustrun_bn_bwd_partials_bytes(int64_t npix, int C) {
    (void)npix;
    return (int64_t)1024 * 2 * C * sizeof(float);
}

namespace ustrun {
// `passes` forward passes in one launch each: tensors of pass g start g*act_elems (g*pool_elems for dp) elements
// further, its constants g*aff_stride floats further (scale/shift/mean/rstd), its coefficients at coef + g*3C.
// dgamma/dbeta receive the passes' contributions in order.
int bn_bwd_reduce_passes(const void* da, const void* dp, const void* y, const float* scale, const float* shift,
                         const float* mean, const float* rstd, const float* gamma, int N, int H, int W, int C, float* dgamma,
                         float* dbeta, int accumulate, float* coef, float* partials, int64_t partials_bytes, int dtype,
                         int passes, long act_elems, long pool_elems, long aff_stride, hipStream_t s) {
    USTRUN_CHECK((da || dp) && y && scale && shift && mean && rstd && gamma && coef && partials, "bn_bwd_reduce: null pointer");
    USTRUN_CHECK(partials_bytes >= ustrun_bn_bwd_partials_bytes((int64_t)N * H * W, C), "bn_bwd_reduce: partials too small");
    BnBwdPlan p;
    USTRUN_TRY(bn_bwd_plan(p, BN_REDUCE, N, H, W, C, dtype, passes, da != nullptr, dp != nullptr, true, act_elems, pool_elems, aff_stride));
    const dim3 grid(p.blocks, passes);
    if (p.x8)
        hipLaunchKernelGGL(bn_bwd_reduce_x8_kernel, grid, dim3(256), 0, s, (const elt_t*)da, (const elt_t*)y, scale, shift, p.nwin, C, p.G,
                           partials, p.po);
    else
        bn_bwd_dispatch(dtype, p, [&](auto P, auto E, auto V) {
            hipLaunchKernelGGL((bn_bwd_reduce_kernel<decltype(P)::value, decltype(E)::value, decltype(V)::value>), grid, dim3(256), 0, s,
                               (const float*)da, (const float*)dp, (const float*)y, scale, shift, N, H, W, C, p.G, partials, p.po);
        });
    USTRUN_LAUNCH_CHECK("bn_bwd_reduce");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<false>, dim3(cdiv(C, 32)), dim3(1024), 0, s, partials, p.blocks, C, (double)N * H * W, gamma,
                       mean, rstd, dgamma, dbeta, accumulate, coef, passes, p.po, 2L * C, 0L, 0);
    USTRUN_LAUNCH_CHECK("bn_bwd_finalize");
    return 0;
}

int bn_bwd_apply_passes(const void* da, const void* dp, const void* y, const float* scale, const float* shift,
                        const float* coef, int N, int H, int W, int C, void* dy, int dtype, int passes, long act_elems,
                        long pool_elems, long aff_stride, hipStream_t s) {
    USTRUN_CHECK((da || dp) && y && scale && shift && coef && dy, "bn_bwd_apply: null pointer");
    BnBwdPlan p;
    USTRUN_TRY(bn_bwd_plan(p, BN_APPLY, N, H, W, C, dtype, passes, da != nullptr, dp != nullptr, false, act_elems, pool_elems, aff_stride));
    const dim3 grid(p.blocks, passes);
    if (p.x8)
        hipLaunchKernelGGL(bn_bwd_apply_x8_kernel, grid, dim3(256), 0, s, (const elt_t*)da, (const elt_t*)y, scale, shift, coef, p.nwin, C,
                           p.G, (elt_t*)dy, p.po);
    else
        bn_bwd_dispatch(dtype, p, [&](auto P, auto E, auto V) {
            hipLaunchKernelGGL((bn_bwd_apply_kernel<decltype(P)::value, decltype(E)::value, decltype(V)::value>), grid, dim3(256), 0, s,
                               (const float*)da, (const float*)dp, (const float*)y, scale, shift, coef, N, H, W, C, p.G, (float*)dy, p.po);
        });
    USTRUN_LAUNCH_CHECK("bn_bwd_apply");
    return 0;
}

// Frozen BatchNorm's backward, one launch for all passes (+ the finalize when the parameters want gradients): see
// bn_bwd_frozen_kernel.  dgamma == nullptr: no rows, no finalize, `partials` untouched.
int bn_bwd_frozen_passes(const void* da, const void* dp, const void* y, const float* scale, const float* shift, const float* mean,
                         const float* rstd, int N, int H, int W, int C, void* dy, float* dgamma, float* dbeta, int accumulate,
                         float* partials, int64_t partials_bytes, int dtype, int passes, long act_elems, long pool_elems,
                         long aff_stride, hipStream_t s) {
    USTRUN_CHECK((da || dp) && y && scale && shift && dy, "bn_bwd_frozen: null pointer");
    const bool sums = dgamma != nullptr;
    USTRUN_CHECK(sums == (dbeta != nullptr), "bn_bwd_frozen: dgamma and dbeta come together");
    USTRUN_CHECK(!sums || (mean && rstd && partials), "bn_bwd_frozen: the sums need mean, rstd and the partials scratch");
    USTRUN_CHECK(!sums || partials_bytes >= ustrun_bn_bwd_partials_bytes((int64_t)N * H * W, C), "bn_bwd_frozen: partials too small");
    USTRUN_CHECK(!dp || (H >= 2 && W >= 2), "bn_bwd_frozen: pooled windows need H, W >= 2 (%dx%d)", H, W);
    BnBwdPlan p;
    USTRUN_TRY(bn_bwd_plan(p, BN_FROZEN, N, H, W, C, dtype, passes, da != nullptr, dp != nullptr, sums, act_elems, pool_elems, aff_stride));
    const dim3 grid(p.blocks, passes);
    auto with_sums = [&](auto f) { if (sums) f(std::true_type{}); else f(std::false_type{}); };
    if (p.x8)
        with_sums([&](auto S) {
            hipLaunchKernelGGL(bn_bwd_frozen_x8_kernel<decltype(S)::value>, grid, dim3(256), 0, s, (const elt_t*)da, (const elt_t*)y, scale,
                               shift, p.nwin, C, p.G, (elt_t*)dy, partials, p.po);
        });
    else
        bn_bwd_dispatch(dtype, p, [&](auto P, auto E, auto V) {
            with_sums([&](auto S) {
                hipLaunchKernelGGL((bn_bwd_frozen_kernel<decltype(P)::value, decltype(E)::value, decltype(V)::value, decltype(S)::value>), grid,
                                   dim3(256), 0, s, (const float*)da, (const float*)dp, (const float*)y, scale, shift, N, H, W, C, p.G,
                                   (float*)dy, partials, p.po);
            });
        });
    USTRUN_LAUNCH_CHECK("bn_bwd_frozen");
    if (sums) {         // no coefficient table: dy does not depend on the sums
        hipLaunchKernelGGL((bn_bwd_finalize_kernel<false, false>), dim3(cdiv(C, 32)), dim3(1024), 0, s, partials, p.blocks, C, 0.0,
                           (const float*)nullptr, mean, rstd, dgamma, dbeta, accumulate, (float*)nullptr, passes, p.po, 2L * C, 0L, 0);
        USTRUN_LAUNCH_CHECK("bn_bwd_finalize");
    }
    return 0;
}

int bn_bwd_finalize_rows(const float* partials, int rows, long rstride, long roff, int C, int64_t count, const float* gamma,
                         const float* mean, const float* rstd, float* dgamma, float* dbeta, int accumulate, float* coef,
                         int passes, long aff_stride, hipStream_t s) {
    USTRUN_CHECK(partials && rows > 0 && C > 0 && gamma && mean && rstd && coef && passes >= 1, "bn_bwd_finalize_rows: bad args");
    const PassOff po = {0, 0, aff_stride, (long)rows * rstride, 3L * C};
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<false>, dim3(cdiv(C, 32)), dim3(1024), 0, s, partials, rows, C, (double)count, gamma, mean,
                       rstd, dgamma, dbeta, accumulate, coef, passes, po, rstride, roff, 0);
    USTRUN_LAUNCH_CHECK("bn_bwd_finalize");
    return 0;
}

// rows a convolution epilogue wrote (the forward-statistics table format: [pass][rows][2][C]) -> the same finalize; long tables
// go through the forward statistics' in-place stage 1 first
int bn_bwd_finalize_stat(float* stat, int rows, int passes, int C, int64_t count, const float* gamma, const float* mean,
                         const float* rstd, long aff_stride, float* dgamma, float* dbeta, int accumulate, float* coef, hipStream_t s) {
    USTRUN_CHECK(stat && rows > 0 && passes >= 1 && C > 0 && gamma && mean && rstd && coef, "bn_bwd_finalize_stat: bad args");
    const PassOff po = {0, 0, aff_stride, (long)rows * 2 * C, 3L * C};
    if (rows >= 96 && C % 32 == 0) {
        int R = cdiv(rows, 32);
        while (rows % R == 1) ++R;
        hipLaunchKernelGGL(bn_stat_stage1_kernel, dim3(C / 32, cdiv(rows, R), passes), dim3(256), 0, s, stat, rows, C, R, passes, BnTail{0, 0, 0.0});
        USTRUN_LAUNCH_CHECK("bn_stat_stage1");
        hipLaunchKernelGGL(bn_bwd_finalize_kernel<true>, dim3(C / 32), dim3(1024), 0, s, stat, rows, C, (double)count, gamma, mean, rstd,
                           dgamma, dbeta, accumulate, coef, passes, po, 2L * C, 0L, R);
    } else {
        hipLaunchKernelGGL(bn_bwd_finalize_kernel<false>, dim3(cdiv(C, 32)), dim3(1024), 0, s, stat, rows, C, (double)count, gamma, mean,
                           rstd, dgamma, dbeta, accumulate, coef, passes, po, 2L * C, 0L, 0);
    }
    USTRUN_LAUNCH_CHECK("bn_bwd_finalize");
    return 0;
}

// layer 17's apply pass without a stored da: see bn_bwd_apply_head_x8_kernel.  dlogits [passes][N][K][H][W] f32, head_w [K][C]
bool bn_bwd_apply_head_ok(int C, int K, int dtype) { return x8_ok(C, false, dtype) && K >= 1 && K <= HEAD_KMAX; }
int bn_bwd_apply_head_passes(const float* dlogits, const float* head_w, const void* y, const float* scale, const float* shift,
                             const float* coef, int N, int H, int W, int C, int K, void* dy, int dtype, int passes,
                             long act_elems, long aff_stride, hipStream_t s) {
    USTRUN_CHECK(dlogits && head_w && y && scale && shift && coef && dy, "bn_bwd_apply_head: null pointer");
    USTRUN_CHECK(bn_bwd_apply_head_ok(C, K, dtype), "bn_bwd_apply_head: C=%d K=%d dtype %d not served", C, K, dtype);
    USTRUN_CHECK(N > 0 && H > 0 && W > 0 && passes >= 1, "bn_bwd_apply_head: bad extent");
    USTRUN_CHECK(!(((uintptr_t)head_w | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)coef) & 15) && aff_stride % 4 == 0,
                 "bn_bwd_apply_head: constants must be 16-byte aligned");
    const long npix = (long)N * H * W;
    USTRUN_CHECK(npix < (1L << 31), "bn_bwd_apply_head: %ld pixels per pass", npix);
    const int G = C / 8, PL = 256 / G;
    long blocks = (npix + (long)PL * 4 - 1) / ((long)PL * 4);
    if (blocks > 4096) blocks = 4096;
    const PassOff po = {act_elems, 0, aff_stride, 0, 3L * C};
#define USTRUN_BN_AH(KT)                                                                                                           \
    hipLaunchKernelGGL(bn_bwd_apply_head_x8_kernel<KT>, dim3((int)blocks, passes), dim3(256), 0, s, dlogits, head_w, (const elt_t*)y, \
                       scale, shift, coef, npix, H * W, C, G, K, (elt_t*)dy, po)
    if (K == 2) USTRUN_BN_AH(2); else if (K == 4) USTRUN_BN_AH(4); else USTRUN_BN_AH(0);
#undef USTRUN_BN_AH
    USTRUN_LAUNCH_CHECK("bn_bwd_apply_head");
    return 0;
}
}  // namespace ustrun

extern "C" int ustrun_bn_bwd_apply_head(const float* dlogits, const float* head_w, const void* y, const float* scale,
                                        const float* shift, const float* coef, int N, int H, int W, int C, int K, void* dy,
                                        int dtype, int passes, int64_t aff_stride, ustrun_stream_t s) {
    return bn_bwd_apply_head_passes(dlogits, head_w, y, scale, shift, coef, N, H, W, C, K, dy, dtype, passes, (long)N * H * W * C,
                                    (long)aff_stride, (hipStream_t)s);
}

extern "C" int ustrun_bn_bwd_finalize_stat(float* stat, int rows_per_pass, int passes, int C, int64_t count, const float* gamma,
                                           const float* mean, const float* rstd, int64_t aff_stride, float* dgamma, float* dbeta,
                                           int accumulate, float* coef, ustrun_stream_t s) {
    return bn_bwd_finalize_stat(stat, rows_per_pass, passes, C, count, gamma, mean, rstd, (long)aff_stride, dgamma, dbeta, accumulate,
                                coef, (hipStream_t)s);
}

extern "C" int ustrun_bn_bwd_reduce(const void* da, const void* dp, const void* y, const float* scale,
                                    const float* shift, const float* mean, const float* rstd, const float* gamma,
                                    int N, int H, int W, int C, float* dgamma, float* dbeta, int accumulate,
                                    float* coef, float* partials, int64_t partials_bytes, int dtype,
                                    ustrun_stream_t s) {
    return bn_bwd_reduce_passes(da, dp, y, scale, shift, mean, rstd, gamma, N, H, W, C, dgamma, dbeta, accumulate, coef,
                                partials, partials_bytes, dtype, 1, 0, 0, 0, (hipStream_t)s);
}

extern "C" int ustrun_bn_bwd_apply(const void* da, const void* dp, const void* y, const float* scale,
                                   const float* shift, const float* coef, int N, int H, int W, int C, void* dy,
                                   int dtype, ustrun_stream_t s) {
    return bn_bwd_apply_passes(da, dp, y, scale, shift, coef, N, H, W, C, dy, dtype, 1, 0, 0, 0, (hipStream_t)s);
}

extern "C" int ustrun_bn_bwd_frozen(const void* da, const void* dp, const void* y, const float* scale, const float* shift,
                                    const float* mean, const float* rstd, int N, int H, int W, int C, void* dy, float* dgamma,
                                    float* dbeta, int accumulate, float* partials, int64_t partials_bytes, int dtype,
                                    ustrun_stream_t s) {
    return bn_bwd_frozen_passes(da, dp, y, scale, shift, mean, rstd, N, H, W, C, dy, dgamma, dbeta, accumulate, partials,
                                partials_bytes, dtype, 1, 0, 0, 0, (hipStream_t)s);
}

extern "C" int ustrun_bn_bwd_frozen_passes(const void* da, const void* dp, const void* y, const float* scale, const float* shift,
                                           const float* mean, const float* rstd, int N, int H, int W, int C, void* dy,
                                           float* dgamma, float* dbeta, int accumulate, float* partials, int64_t partials_bytes,
                                           int dtype, int passes, int64_t aff_stride, ustrun_stream_t s) {
    return bn_bwd_frozen_passes(da, dp, y, scale, shift, mean, rstd, N, H, W, C, dy, dgamma, dbeta, accumulate, partials,
                                partials_bytes, dtype, passes, (long)N * H * W * C, (long)N * (H / 2) * (W / 2) * C, (long)aff_stride,
                                (hipStream_t)s);
}

extern "C" int ustrun_bn_eval_consts(int C, const float* gamma, const float* beta, const float* running_mean,
                                     const float* running_var, float eps, float* aff, ustrun_stream_t s) {
    USTRUN_CHECK(C > 0 && aff, "bn_eval_consts: bad args");
    const int c1[1] = {C};
    const float* const g1[1] = {gamma}; const float* const b1[1] = {beta};
    const float* const m1[1] = {running_mean}; const float* const v1[1] = {running_var};
    float* const a1[1] = {aff};
    return bn_eval_affine_layers(1, c1, g1, b1, m1, v1, a1, eps, 1, (hipStream_t)s);
}

extern "C" int ustrun_debug_last_bn_variant(void) { return g_last_bn_variant; }
