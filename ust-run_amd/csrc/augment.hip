// Data augmentation of resident uint8 batches (include/ustrun.h: ustrun_aug_*): what the reference does per sample
// in PIL / scipy on its loader workers (dataloaders/custom_transforms.py), per batch on the device.
//
// Every stage reads uint8 HWC and writes uint8 HWC where the reference quantises, so a stage's result differs from the
// reference's by at most the one rounding it shares with it:
//   gather        pool rows -> batch buffers, 16-byte moves
//   scale_crop    PIL's 8-bit resample (22-bit fixed-point coefficients formed in double, as Resample.c does; horizontal pass,
//                 uint8, vertical pass, uint8) evaluated only inside the crop window; nearest for the label
//   rotate        PIL's affine transform: bilinear in double + truncation for the image, the 16.16 fixed-point walk for the
//                 label (integer arithmetic: exact); the horizontal flip that follows is folded into the output column
//   elastic_field hash -> uniform(-1, 1) -> separable Gaussian through LDS (column strips, then rows), taps in LDS
//   elastic_warp  scipy map_coordinates: linear + constant 0 for the image, nearest + clamped for the label
//   strong        brightness, contrast (per-image integer luma sum: one block per image, wave shuffles, then LDS, fixed order --
//                 integer, so order-free anyway), reflection-padded Gaussian blur in f32
//   finish        x / 127.5 - 1 into NCHW f32, label bytes as floats
// No kernel here uses atomics; two runs give the same bits.
#include "common.h"
#include <math.h>

namespace ustrun {
namespace {

constexpr int AUG_MAX = 1024;            // H, W limit of every entry
constexpr int BLUR_RMAX = 63;            // blur radius limit (the reference's: 12, 14, 19)
constexpr int FIELD_RMAX = 160;          // smoothing radius limit: int(4 * 0.08 * 500 + 0.5)
constexpr int FIELD_COLS = 16;           // pass 1: columns per block
constexpr int FIELD_ROWS = 4;            // pass 2: rows per block

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ double bits_f64(const int32_t* p) {
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)p[1] << 32) | (unsigned)p[0]));
}

// ---------------------------------------------------------------------------------------------------------------- gather
// grid (blocks, B)
__global__ __launch_bounds__(256) void gather_kernel(const uint8_t* __restrict__ pool, const int32_t* __restrict__ idx, long n_pool,
                                                    long bytes, int vec, uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const long i = idx[b];
    if (i < 0 || i >= n_pool) return;
    const uint8_t* s = pool + i * bytes;
    uint8_t* d = out + (long)b * bytes;
    const long n16 = vec ? bytes / 16 : 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n16; e += (long)gridDim.x * 256)
        ((uint4*)d)[e] = ((const uint4*)s)[e];
    for (long e = n16 * 16 + (long)blockIdx.x * 256 + threadIdx.x; e < bytes; e += (long)gridDim.x * 256) d[e] = s[e];
}

// ------------------------------------------------------------------------------------------------------------ scale + crop
// PIL Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, output index xx of `out` from `in` samples
__device__ __forceinline__ void pil_coeffs(int xx, int in, int out, int& xmin, int& n, int k[3]) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    n = xmax - xmin;
    if (n > 3) n = 3;                     // (support <= 1.5 for every enlargement and for w = in: at most 3 samples)
    double w[3] = {0.0, 0.0, 0.0}, ww = 0.0;
    for (int x = 0; x < n; ++x) {
        double a = (x + xmin - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        w[x] = a < 1.0 ? 1.0 - a : 0.0;
        ww += w[x];
    }
    for (int x = 0; x < 3; ++x) {
        const double v = (x < n && ww != 0.0) ? w[x] / ww : 0.0;
        k[x] = (int)(v < 0.0 ? -0.5 + v * 4194304.0 : 0.5 + v * 4194304.0);          // 1 << 22
    }
}
// PIL ImagingScaleAffine: the source index of output x is (int) of a RUNNING sum, xo = in / out / 2, then xo += in / out per
// output sample, in double.  Where (x + 0.5) in / out is an integer (the centre column of an odd w) the sum's rounding decides the
// index, so the sum is repeated here: at most 1.5 x 1024 dependent adds, only for gated samples.
__device__ __forceinline__ int pil_nearest(int x, int in, int out) {
    const double a = (double)in / (double)out;
    double xo = a * 0.5;
    for (int i = 0; i < x; ++i) xo = __dadd_rn(xo, a);
    return (int)xo;
}
__device__ __forceinline__ int clip8_22(int s) { return clampi(s >> 22, 0, 255); }

// grid (ceil(P * P / 256), B)
__global__ __launch_bounds__(256) void scale_crop_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                        const int32_t* __restrict__ params, int stride, int Hs, int Ws, int C, int Cl,
                                                        int P, uint8_t* __restrict__ img_out, uint8_t* __restrict__ lab_out) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P * P) return;
    const int oy = e / P, ox = e % P;
    const int32_t* p = params + (long)b * stride;
    const bool on = p[0] != 0;
    const int w = on ? p[1] : Ws, h = on ? p[2] : Hs, pad = p[3], fill = p[6];
    const int px = ox + p[4] - pad, py = oy + p[5] - pad;
    const bool inside = px >= 0 && px < w && py >= 0 && py < h;
    const uint8_t* si = img + (long)b * Hs * Ws * C;
    uint8_t* di = img_out + ((long)b * P * P + e) * C;
    if (!inside) {
        for (int c = 0; c < C; ++c) di[c] = 0;
    } else if (w == Ws && h == Hs) {
        for (int c = 0; c < C; ++c) di[c] = si[((long)py * Ws + px) * C + c];
    } else {
        int xmin = px, xn = 1, xk[3] = {4194304, 0, 0}, ymin = py, yn = 1, yk[3] = {4194304, 0, 0};
        if (w != Ws) pil_coeffs(px, Ws, w, xmin, xn, xk);       // (PIL skips a pass whose size does not change)
        if (h != Hs) pil_coeffs(py, Hs, h, ymin, yn, yk);
        for (int c = 0; c < C; ++c) {
            int acc = 1 << 21;
            for (int j = 0; j < yn; ++j) {
                const int sy = clampi(ymin + j, 0, Hs - 1);
                int hv;
                if (w != Ws) {
                    int s = 1 << 21;
                    for (int i = 0; i < xn; ++i) s += (int)si[((long)sy * Ws + clampi(xmin + i, 0, Ws - 1)) * C + c] * xk[i];
                    hv = clip8_22(s);
                } else {
                    hv = si[((long)sy * Ws + px) * C + c];
                }
                acc += hv * yk[j];
            }
            di[c] = (uint8_t)(h != Hs ? clip8_22(acc) : (acc - (1 << 21)) >> 22);
        }
    }
    if (lab) {
        uint8_t* dl = lab_out + ((long)b * P * P + e) * Cl;
        if (!inside) {
            for (int c = 0; c < Cl; ++c) dl[c] = (uint8_t)((fill >> (8 * c)) & 255);
        } else {
            const int sx = w == Ws ? px : clampi(pil_nearest(px, Ws, w), 0, Ws - 1);
            const int sy = h == Hs ? py : clampi(pil_nearest(py, Hs, h), 0, Hs - 1);
            const uint8_t* sl = lab + ((long)b * Hs * Ws + (long)sy * Ws + sx) * Cl;
            for (int c = 0; c < Cl; ++c) dl[c] = sl[c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- rotate + flip
// grid (ceil(H * W / 256), B)
__global__ __launch_bounds__(256) void rotate_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                    const int32_t* __restrict__ params, int stride, int H, int W, int C, int Cl,
                                                    uint8_t* __restrict__ img_out, uint8_t* __restrict__ lab_out) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= H * W) return;
    const int32_t* p = params + (long)b * stride;
    const int y = e / W, xo = e % W;
    const int x = p[1] ? W - 1 - xo : xo;         // column of the rotated image this output pixel shows
    const uint8_t* si = img + (long)b * H * W * C;
    uint8_t* di = img_out + ((long)b * H * W + e) * C;
    uint8_t* dl = lab ? lab_out + ((long)b * H * W + e) * Cl : nullptr;
    if (!p[0]) {
        for (int c = 0; c < C; ++c) di[c] = si[((long)y * W + x) * C + c];
        if (lab) for (int c = 0; c < Cl; ++c) dl[c] = lab[((long)b * H * W + (long)y * W + x) * Cl + c];
        return;
    }
    // image: PIL Geometry.c affine_transform + bilinear_filter8 (no contraction: the products and sums round as C's do)
    const double a0 = bits_f64(p + 10), a1 = bits_f64(p + 12), a2 = bits_f64(p + 14);
    const double a3 = bits_f64(p + 16), a4 = bits_f64(p + 18), a5 = bits_f64(p + 20);
    const double xc = x + 0.5, yc = y + 0.5;
    double xin = __dadd_rn(__dadd_rn(__dmul_rn(a0, xc), __dmul_rn(a1, yc)), a2);
    double yin = __dadd_rn(__dadd_rn(__dmul_rn(a3, xc), __dmul_rn(a4, yc)), a5);
    if (xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H) {
        for (int c = 0; c < C; ++c) di[c] = 0;
    } else {
        xin -= 0.5; yin -= 0.5;
        const double fx = floor(xin), fy = floor(yin);
        const int ix = (int)fx, iy = (int)fy;
        const double dx = xin - fx, dy = yin - fy;
        const int x0 = clampi(ix, 0, W - 1), x1 = clampi(ix + 1, 0, W - 1), y0 = clampi(iy, 0, H - 1);
        const bool row2 = iy + 1 >= 0 && iy + 1 < H;
        for (int c = 0; c < C; ++c) {
            const double p00 = si[((long)y0 * W + x0) * C + c], p01 = si[((long)y0 * W + x1) * C + c];
            const double v1 = __dadd_rn(p00, __dmul_rn(p01 - p00, dx));
            double v2 = v1;
            if (row2) {
                const double p10 = si[((long)(iy + 1) * W + x0) * C + c], p11 = si[((long)(iy + 1) * W + x1) * C + c];
                v2 = __dadd_rn(p10, __dmul_rn(p11 - p10, dx));
            }
            di[c] = (uint8_t)(int)__dadd_rn(v1, __dmul_rn(v2 - v1, dy));
        }
    }
    if (lab) {      // PIL affine_fixed: xx = a2 + x a0 + y a1 in 16.16, arithmetic shift
        const int sx = (p[6] + x * p[4] + y * p[5]) >> 16, sy = (p[9] + x * p[7] + y * p[8]) >> 16;
        if (sx >= 0 && sx < W && sy >= 0 && sy < H) {
            const uint8_t* sl = lab + ((long)b * H * W + (long)sy * W + sx) * Cl;
            for (int c = 0; c < Cl; ++c) dl[c] = sl[c];
        } else {
            for (int c = 0; c < Cl; ++c) dl[c] = (uint8_t)((p[2] >> (8 * c)) & 255);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- elastic field
// counter-based generator: two rounds of the 64-bit finaliser of MurmurHash3 over (seed, plane, pixel); the top 24 bits
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z ^= z >> 33; z *= 0xff51afd7ed558ccdULL; z ^= z >> 33; z *= 0xc4ceb9fe1a85ec53ULL; z ^= z >> 33;
    return z;
}
__device__ __forceinline__ float hash_uniform(unsigned long long seed, unsigned plane, unsigned pixel) {
    const unsigned long long k = mix64(seed + 0x9e3779b97f4a7c15ULL * ((unsigned long long)plane + 1));
    const unsigned long long v = mix64(k ^ (0xd1b54a32d192ed03ULL * ((unsigned long long)pixel + 1)));
    return (float)(v >> 40) * (2.0f / 16777216.0f) - 1.0f;        // [-1, 1)
}

// grid (ceil(H * W / 256), 2 * B): the generator's values as the field entry reads them
__global__ __launch_bounds__(256) void noise_kernel(unsigned long long seed, int HW, float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < HW) out[(long)blockIdx.y * HW + e] = hash_uniform(seed, blockIdx.y, (unsigned)e);
}

// the normalised taps of scipy's _gaussian_kernel1d (float64 there; f32 here after the normalisation) into LDS
__device__ __forceinline__ void gaussian_taps(float* taps, double* scratch, int r, double sigma) {
    const int k = 2 * r + 1;
    for (int t = threadIdx.x; t < k; t += blockDim.x) {
        const double x = t - r;
        scratch[t] = exp(-0.5 / (sigma * sigma) * x * x);
    }
    __syncthreads();
    double s = 0.0;
    for (int t = 0; t < k; ++t) s += scratch[t];               // the same order in every thread
    for (int t = threadIdx.x; t < k; t += blockDim.x) taps[t] = (float)(scratch[t] / s);
    __syncthreads();
}

// pass 1, along axis 0 (rows): grid (ceil(W / 16), 2 * B), 256 threads = 16 columns x 16 row lanes; the strip of all H rows
// (+ r zero rows each side) sits in LDS as [H + 2r][16] floats: a wave reads 4 consecutive rows x 16 columns = 64 consecutive
// words, conflict-free.  dynamic LDS: (H + 2r) * 16 floats
__global__ __launch_bounds__(256) void field_pass1_kernel(const float* __restrict__ noise, unsigned long long seed,
                                                         const int32_t* __restrict__ params, int stride, int H, int W, int r,
                                                         double sigma, float* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) float strip[];
    __shared__ float taps[2 * FIELD_RMAX + 1];
    __shared__ double scratch[2 * FIELD_RMAX + 1];
    const int plane = blockIdx.y, b = plane >> 1;
    if (!params[(long)b * stride]) return;
    gaussian_taps(taps, scratch, r, sigma);
    const int x0 = blockIdx.x * FIELD_COLS, cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int x = x0 + cx;
    const long base = (long)plane * H * W;
    for (int y = ry; y < H + 2 * r; y += 16) {
        const int sy = y - r;
        float v = 0.f;
        if (sy >= 0 && sy < H && x < W)
            v = noise ? noise[base + (long)sy * W + x] : hash_uniform(seed, (unsigned)plane, (unsigned)(sy * W + x));
        strip[y * FIELD_COLS + cx] = v;
    }
    __syncthreads();
    if (x >= W) return;
    const int k = 2 * r + 1;
    for (int y = ry; y < H; y += 16) {
        float acc = 0.f;
        for (int t = 0; t < k; ++t) acc += taps[t] * strip[(y + t) * FIELD_COLS + cx];
        work[base + (long)y * W + x] = acc;
    }
}

// pass 2, along axis 1 (columns), then * alpha: grid (ceil(H / 4), 2 * B), 256 threads = 4 rows x 64 lanes; rows in LDS as
// [4][W + 2r] floats, a wave reads 64 consecutive words.  dynamic LDS: 4 * (W + 2r) floats
__global__ __launch_bounds__(256) void field_pass2_kernel(const float* __restrict__ work, const int32_t* __restrict__ params,
                                                         int stride, int H, int W, int r, double sigma, float alpha,
                                                         float* __restrict__ field) {
    extern __shared__ __attribute__((aligned(16))) float rows[];
    __shared__ float taps[2 * FIELD_RMAX + 1];
    __shared__ double scratch[2 * FIELD_RMAX + 1];
    const int plane = blockIdx.y, b = plane >> 1;
    if (!params[(long)b * stride]) return;
    gaussian_taps(taps, scratch, r, sigma);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.x * FIELD_ROWS + wave;
    const int LW = W + 2 * r;
    const long base = (long)plane * H * W;
    for (int x = lane; x < LW; x += 64) {
        const int sx = x - r;
        rows[wave * LW + x] = (y < H && sx >= 0 && sx < W) ? work[base + (long)y * W + sx] : 0.f;
    }
    __syncthreads();
    if (y >= H) return;
    const int k = 2 * r + 1;
    for (int x = lane; x < W; x += 64) {
        float acc = 0.f;
        for (int t = 0; t < k; ++t) acc += taps[t] * rows[wave * LW + x + t];
        field[base + (long)y * W + x] = acc * alpha;
    }
}

// ------------------------------------------------------------------------------------------------------------ elastic warp
// grid (ceil(H * W / 256), B)
__global__ __launch_bounds__(256) void warp_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                  const float* __restrict__ field, const int32_t* __restrict__ params, int stride,
                                                  int H, int W, int C, int Cl, uint8_t* __restrict__ img_out,
                                                  uint8_t* __restrict__ lab_out) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= H * W) return;
    const uint8_t* si = img + (long)b * H * W * C;
    uint8_t* di = img_out + ((long)b * H * W + e) * C;
    uint8_t* dl = lab ? lab_out + ((long)b * H * W + e) * Cl : nullptr;
    if (!params[(long)b * stride]) {
        for (int c = 0; c < C; ++c) di[c] = si[(long)e * C + c];
        if (lab) for (int c = 0; c < Cl; ++c) dl[c] = lab[((long)b * H * W + e) * Cl + c];
        return;
    }
    const int i = e / W, j = e % W;
    const double rr = (double)i + (double)field[((long)b * 2) * H * W + e];
    const double cc = (double)j + (double)field[((long)b * 2 + 1) * H * W + e];
    // scipy NI_GeometricTransform, order 1, mode 'constant' (cval 0): no interpolation beyond the edges.  The reference passes
    // a uint8 array, so map_coordinates itself produces uint8, rounded to nearest; its later astype(np.uint8) changes nothing
    if (rr < 0.0 || rr > (double)(H - 1) || cc < 0.0 || cc > (double)(W - 1)) {
        for (int c = 0; c < C; ++c) di[c] = 0;
    } else {
        const double fr = floor(rr), fc = floor(cc);
        const int r0 = (int)fr, c0 = (int)fc;
        const double tr = rr - fr, tc = cc - fc;
        const int r1 = r0 + 1 < H ? r0 + 1 : r0, c1 = c0 + 1 < W ? c0 + 1 : c0;       // (weight 0 when clamped: rr = H - 1 exactly)
        for (int c = 0; c < C; ++c) {
            const double p00 = si[((long)r0 * W + c0) * C + c], p01 = si[((long)r0 * W + c1) * C + c];
            const double p10 = si[((long)r1 * W + c0) * C + c], p11 = si[((long)r1 * W + c1) * C + c];
            const double v = (1.0 - tr) * ((1.0 - tc) * p00 + tc * p01) + tr * ((1.0 - tc) * p10 + tc * p11);
            di[c] = (uint8_t)clampi((int)(v + 0.5), 0, 255);          // (map_coordinates returns its INPUT's dtype: it rounds)
        }
    }
    if (lab) {      // order 0, mode 'nearest': clamp the coordinate, then floor(c + 0.5)
        const double rn = rr < 0.0 ? 0.0 : (rr > (double)(H - 1) ? (double)(H - 1) : rr);
        const double cn = cc < 0.0 ? 0.0 : (cc > (double)(W - 1) ? (double)(W - 1) : cc);
        const int sr = clampi((int)floor(rn + 0.5), 0, H - 1), sc = clampi((int)floor(cn + 0.5), 0, W - 1);
        const uint8_t* sl = lab + ((long)b * H * W + (long)sr * W + sc) * Cl;
        for (int c = 0; c < Cl; ++c) dl[c] = sl[c];
    }
}

// ------------------------------------------------------------------------------------------------------------------ strong
// PIL Blend.c: the result of blending `lo` (the degenerate image's value) with pixel v at alpha, in float as C evaluates it
__device__ __forceinline__ int pil_blend(int lo, int v, float alpha) {
    if (alpha == 0.0f) return lo;
    if (alpha == 1.0f) return v;
    const float t = __fadd_rn((float)lo, __fmul_rn(alpha, (float)(v - lo)));
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}
__device__ __forceinline__ int pil_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// one block of 1024 threads per image: brightness, the luma sum of the brightened image, contrast -> mid (uint8)
__global__ __launch_bounds__(1024) void enhance_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ params, int stride,
                                                      int HW, int C, uint8_t* __restrict__ mid) {
    __shared__ unsigned long long wsum[16];
    __shared__ int s_mean;
    const int b = blockIdx.x;
    const int32_t* p = params + (long)b * stride;
    const uint8_t* s = img + (long)b * HW * C;
    uint8_t* d = mid + (long)b * HW * C;
    if (!(p[0] & 1)) return;                             // (the blur kernels then read the input itself)
    const float vb = __int_as_float(p[1]), vc = __int_as_float(p[2]);
    unsigned long long sum = 0;
    for (int e = threadIdx.x; e < HW; e += 1024) {
        if (C == 3) {
            sum += pil_luma(pil_blend(0, s[e * 3], vb), pil_blend(0, s[e * 3 + 1], vb), pil_blend(0, s[e * 3 + 2], vb));
        } else {
            sum += pil_blend(0, s[e], vb);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; ++w) t += wsum[w];
        s_mean = (int)((double)t / (double)HW + 0.5);    // ImageEnhance.Contrast: int(ImageStat.Stat(L).mean[0] + 0.5)
    }
    __syncthreads();
    const int mean = s_mean;
    for (int e = threadIdx.x; e < HW * C; e += 1024) d[e] = (uint8_t)pil_blend(mean, pil_blend(0, s[e], vb), vc);
}

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ void blur_taps(float* taps, double* scratch, int r, double sigma) {
    const int k = 2 * r + 1;
    for (int t = threadIdx.x; t < k; t += blockDim.x) {
        const double x = t - r;
        scratch[t] = exp(-(x * x) / (2.0 * sigma * sigma));
    }
    __syncthreads();
    double s = 0.0;
    for (int t = 0; t < k; ++t) s += scratch[t];
    for (int t = threadIdx.x; t < k; t += blockDim.x) taps[t] = (float)(scratch[t] / s);
    __syncthreads();
}

// (gate bit 0: brightness + contrast, bit 1: blur)
// down: mid (uint8) / 255 -> tmp (f32), k taps along y with reflection.  grid (ceil(H * W * C / 256), B)
__global__ __launch_bounds__(256) void blur_down_kernel(const uint8_t* __restrict__ mid, const uint8_t* __restrict__ img, const int32_t* __restrict__ params, int stride,
                                                       int H, int W, int C, int r, float* __restrict__ tmp) {
    __shared__ float taps[2 * BLUR_RMAX + 1];
    __shared__ double scratch[2 * BLUR_RMAX + 1];
    const int b = blockIdx.y;
    const int32_t* p = params + (long)b * stride;
    if (!(p[0] & 2)) return;
    blur_taps(taps, scratch, r, (double)__int_as_float(p[3]));
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int WC = W * C;
    if (e >= H * WC) return;
    const int y = e / WC, xc = e % WC;
    const uint8_t* s = ((p[0] & 1) ? mid : img) + (long)b * H * WC + xc;
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) acc += taps[t] * ((float)s[(long)reflect(y + t - r, H) * WC] / 255.0f);
    tmp[(long)b * H * WC + e] = acc;
}

// across: tmp (f32) -> out (uint8) = trunc(255 * sum); without the blur bit the sample is copied.  grid as above
__global__ __launch_bounds__(256) void blur_across_kernel(const float* __restrict__ tmp, const uint8_t* __restrict__ mid,
                                                         const uint8_t* __restrict__ img,
                                                         const int32_t* __restrict__ params, int stride, int H, int W, int C, int r,
                                                         uint8_t* __restrict__ out) {
    __shared__ float taps[2 * BLUR_RMAX + 1];
    __shared__ double scratch[2 * BLUR_RMAX + 1];
    const int b = blockIdx.y;
    const int32_t* p = params + (long)b * stride;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int WC = W * C;
    if (!(p[0] & 2)) {
        if (e < H * WC) out[(long)b * H * WC + e] = ((p[0] & 1) ? mid : img)[(long)b * H * WC + e];
        return;
    }
    blur_taps(taps, scratch, r, (double)__int_as_float(p[3]));
    if (e >= H * WC) return;
    const int y = e / WC, xc = e % WC, x = xc / C, c = xc % C;
    const float* s = tmp + ((long)b * H + y) * WC + c;
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) acc += taps[t] * s[reflect(x + t - r, W) * C];
    const float v = acc * 255.0f;
    out[(long)b * H * WC + e] = (uint8_t)(v <= 0.f ? 0 : (v >= 255.f ? 255 : (int)v));
}

// ------------------------------------------------------------------------------------------------------------------ finish
// a lane owns 4 adjacent pixels: reads 4 C bytes, writes one float4 per channel plane.  grid (ceil(HW / 4 / 256), B)
__global__ __launch_bounds__(256) void finish_image_kernel(const uint8_t* __restrict__ src, int HW, int C, float* __restrict__ dst) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int e0 = q * 4;
    if (e0 >= HW) return;
    const uint8_t* s = src + (long)b * HW * C;
    float* d = dst + (long)b * C * HW;
    if (e0 + 4 <= HW && (HW & 3) == 0) {
        uint8_t v[12];
        if (C == 1) {
            *(uchar4*)v = *(const uchar4*)(s + e0);
        } else {
            for (int i = 0; i < 4 * C; ++i) v[i] = s[(long)e0 * C + i];
        }
        for (int c = 0; c < C; ++c) {
            float4 o;
            o.x = (float)v[c] / 127.5f - 1.0f; o.y = (float)v[C + c] / 127.5f - 1.0f;
            o.z = (float)v[2 * C + c] / 127.5f - 1.0f; o.w = (float)v[3 * C + c] / 127.5f - 1.0f;
            *(float4*)(d + (long)c * HW + e0) = o;
        }
    } else {
        for (int e = e0; e < HW && e < e0 + 4; ++e)
            for (int c = 0; c < C; ++c) d[(long)c * HW + e] = (float)s[(long)e * C + c] / 127.5f - 1.0f;
    }
}

// bytes -> floats, 4 per lane.  n = total elements
__global__ __launch_bounds__(256) void bytes_to_float_kernel(const uint8_t* __restrict__ src, long n, float* __restrict__ dst) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const long e0 = q * 4;
    if (e0 >= n) return;
    if (e0 + 4 <= n) {
        const uchar4 v = *(const uchar4*)(src + e0);
        float4 o; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
        *(float4*)(dst + e0) = o;
    } else {
        for (long e = e0; e < n; ++e) dst[e] = src[e];
    }
}

int check_dims(const char* who, int B, int H, int W, int C, int Cl) {
    USTRUN_CHECK(B > 0 && B <= 65535, "%s: batch %d outside [1, 65535]", who, B);
    USTRUN_CHECK(H > 0 && W > 0 && H <= AUG_MAX && W <= AUG_MAX, "%s: extent %d x %d outside [1, %d]", who, H, W, AUG_MAX);
    USTRUN_CHECK(C == 1 || C == 3, "%s: %d image channels (1 or 3)", who, C);
    USTRUN_CHECK(Cl == 1 || Cl == 3, "%s: %d label channels (1 or 3)", who, Cl);
    return 0;
}

int field_radius(int H, double* sigma) {
    *sigma = (double)H * 0.08;
    return (int)(4.0 * *sigma + 0.5);
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int ustrun_aug_gather(const uint8_t* images, const uint8_t* labels, const int32_t* idx, int64_t n_pool, int32_t B,
                                 int64_t img_bytes, int64_t lab_bytes, uint8_t* img_out, uint8_t* lab_out, ustrun_stream_t stream) {
    USTRUN_CHECK(images && idx && img_out, "aug_gather: null pointer");
    USTRUN_CHECK(B > 0 && B <= 65535 && n_pool > 0 && img_bytes > 0 && lab_bytes >= 0, "aug_gather: bad sizes (B %d, pool %lld)", B,
                 (long long)n_pool);
    USTRUN_CHECK(!lab_bytes || (labels && lab_out), "aug_gather: null label pointer");
    hipStream_t st = (hipStream_t)stream;
    auto aligned = [](const void* a, const void* b, int64_t n) { return ((uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && n % 16 == 0) ? 1 : 0; };
    gather_kernel<<<dim3(cdiv(cdiv(img_bytes, 16), 256) > 64 ? 64 : cdiv(cdiv(img_bytes, 16), 256), B), 256, 0, st>>>(
        images, idx, n_pool, img_bytes, aligned(images, img_out, img_bytes), img_out);
    if (lab_bytes)
        gather_kernel<<<dim3(cdiv(cdiv(lab_bytes, 16), 256) > 64 ? 64 : cdiv(cdiv(lab_bytes, 16), 256), B), 256, 0, st>>>(
            labels, idx, n_pool, lab_bytes, aligned(labels, lab_out, lab_bytes), lab_out);
    USTRUN_LAUNCH_CHECK("aug_gather");
    return 0;
}

extern "C" int ustrun_aug_scale_crop(const uint8_t* img, const uint8_t* lab, const int32_t* params, int32_t stride, int32_t B,
                                     int32_t Hs, int32_t Ws, int32_t C, int32_t Cl, int32_t P, uint8_t* img_out, uint8_t* lab_out,
                                     ustrun_stream_t stream) {
    USTRUN_CHECK(img && params && img_out && (!lab || lab_out), "aug_scale_crop: null pointer");
    USTRUN_TRY(check_dims("aug_scale_crop", B, Hs, Ws, C, Cl));
    USTRUN_CHECK(P > 0 && P <= AUG_MAX && stride >= 8, "aug_scale_crop: patch %d outside [1, %d] or row stride %d < 8", P, AUG_MAX, stride);
    scale_crop_kernel<<<dim3(cdiv((int64_t)P * P, 256), B), 256, 0, (hipStream_t)stream>>>(img, lab, params, stride, Hs, Ws, C, Cl, P,
                                                                                         img_out, lab_out);
    USTRUN_LAUNCH_CHECK("aug_scale_crop");
    return 0;
}

extern "C" int ustrun_aug_rotate(const uint8_t* img, const uint8_t* lab, const int32_t* params, int32_t stride, int32_t B, int32_t H,
                                 int32_t W, int32_t C, int32_t Cl, uint8_t* img_out, uint8_t* lab_out, ustrun_stream_t stream) {
    USTRUN_CHECK(img && params && img_out && (!lab || lab_out), "aug_rotate: null pointer");
    USTRUN_TRY(check_dims("aug_rotate", B, H, W, C, Cl));
    USTRUN_CHECK(stride >= 22, "aug_rotate: row stride %d < 22", stride);
    rotate_kernel<<<dim3(cdiv((int64_t)H * W, 256), B), 256, 0, (hipStream_t)stream>>>(img, lab, params, stride, H, W, C, Cl, img_out,
                                                                                     lab_out);
    USTRUN_LAUNCH_CHECK("aug_rotate");
    return 0;
}

extern "C" int ustrun_aug_elastic_field(const float* noise, int64_t seed, const int32_t* params, int32_t stride, int32_t B, int32_t H,
                                        int32_t W, float* field, float* work, ustrun_stream_t stream) {
    USTRUN_CHECK(params && field && work, "aug_elastic_field: null pointer");
    USTRUN_CHECK(H == W, "aug_elastic_field: %d x %d: the reference's elastic transform indexes consistently only for square patches", H, W);
    USTRUN_TRY(check_dims("aug_elastic_field", B, H, W, 1, 1));
    USTRUN_CHECK(2 * B <= 65535 && stride >= 1, "aug_elastic_field: batch %d too large or stride %d < 1", B, stride);
    double sigma;
    const int r = field_radius(H, &sigma);
    USTRUN_CHECK(r >= 1 && r <= FIELD_RMAX, "aug_elastic_field: smoothing radius %d outside [1, %d]", r, FIELD_RMAX);
    hipStream_t st = (hipStream_t)stream;
    const int lds1 = (H + 2 * r) * FIELD_COLS * 4, lds2 = FIELD_ROWS * (W + 2 * r) * 4;      // <= 86 KB / 22 KB
    USTRUN_TRY(ensure_dynamic_lds((const void*)field_pass1_kernel, lds1, "aug_elastic_field"));
    field_pass1_kernel<<<dim3(cdiv(W, FIELD_COLS), 2 * B), 256, lds1, st>>>(noise, (unsigned long long)seed, params, stride, H, W, r,
                                                                           sigma, work);
    field_pass2_kernel<<<dim3(cdiv(H, FIELD_ROWS), 2 * B), 256, lds2, st>>>(work, params, stride, H, W, r, sigma, (float)(2 * H), field);
    USTRUN_LAUNCH_CHECK("aug_elastic_field");
    return 0;
}

extern "C" int ustrun_aug_elastic_noise(int64_t seed, int32_t B, int32_t H, int32_t W, float* noise, ustrun_stream_t stream) {
    USTRUN_CHECK(noise, "aug_elastic_noise: null pointer");
    USTRUN_TRY(check_dims("aug_elastic_noise", B, H, W, 1, 1));
    USTRUN_CHECK(2 * B <= 65535, "aug_elastic_noise: batch %d too large", B);
    noise_kernel<<<dim3(cdiv((int64_t)H * W, 256), 2 * B), 256, 0, (hipStream_t)stream>>>((unsigned long long)seed, H * W, noise);
    USTRUN_LAUNCH_CHECK("aug_elastic_noise");
    return 0;
}

extern "C" int ustrun_aug_elastic_warp(const uint8_t* img, const uint8_t* lab, const float* field, const int32_t* params, int32_t stride,
                                       int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cl, uint8_t* img_out, uint8_t* lab_out,
                                       ustrun_stream_t stream) {
    USTRUN_CHECK(img && field && params && img_out && (!lab || lab_out), "aug_elastic_warp: null pointer");
    USTRUN_CHECK(H == W, "aug_elastic_warp: %d x %d: the reference's elastic transform indexes consistently only for square patches", H, W);
    USTRUN_TRY(check_dims("aug_elastic_warp", B, H, W, C, Cl));
    USTRUN_CHECK(stride >= 1, "aug_elastic_warp: row stride %d < 1", stride);
    warp_kernel<<<dim3(cdiv((int64_t)H * W, 256), B), 256, 0, (hipStream_t)stream>>>(img, lab, field, params, stride, H, W, C, Cl, img_out,
                                                                                   lab_out);
    USTRUN_LAUNCH_CHECK("aug_elastic_warp");
    return 0;
}

extern "C" int64_t ustrun_aug_strong_work_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
    const int64_t n = (int64_t)B * H * W * C;
    return ((n + 15) & ~(int64_t)15) + n * 4;             // the enhanced bytes, then the f32 rows of the first blur pass
}

extern "C" int ustrun_aug_strong(const uint8_t* img, const int32_t* params, int32_t stride, int32_t B, int32_t H, int32_t W, int32_t C,
                                 int32_t r, uint8_t* img_out, void* work, int64_t work_bytes, ustrun_stream_t stream) {
    USTRUN_CHECK(img && params && img_out && work, "aug_strong: null pointer");
    USTRUN_TRY(check_dims("aug_strong", B, H, W, C, 1));
    USTRUN_CHECK(r >= 0 && r <= BLUR_RMAX && r < H && r < W, "aug_strong: blur radius %d outside [0, %d] or >= the extent %d x %d", r,
                 BLUR_RMAX, H, W);
    USTRUN_CHECK(stride >= 4, "aug_strong: row stride %d < 4", stride);
    USTRUN_CHECK(work_bytes >= ustrun_aug_strong_work_bytes(B, H, W, C), "aug_strong: work buffer of %lld bytes, %lld needed",
                 (long long)work_bytes, (long long)ustrun_aug_strong_work_bytes(B, H, W, C));
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)B * H * W * C;
    uint8_t* mid = (uint8_t*)work;
    float* tmp = (float*)((char*)work + ((n + 15) & ~(int64_t)15));
    enhance_kernel<<<B, 1024, 0, st>>>(img, params, stride, H * W, C, mid);
    const dim3 grid(cdiv((int64_t)H * W * C, 256), B);
    blur_down_kernel<<<grid, 256, 0, st>>>(mid, img, params, stride, H, W, C, r, tmp);
    blur_across_kernel<<<grid, 256, 0, st>>>(tmp, mid, img, params, stride, H, W, C, r, img_out);
    USTRUN_LAUNCH_CHECK("aug_strong");
    return 0;
}

extern "C" int ustrun_aug_finish(const uint8_t* weak, const uint8_t* strong, const uint8_t* lab, int32_t B, int32_t H, int32_t W, int32_t C,
                                 int32_t Cl, float* xw, float* xs, float* y, ustrun_stream_t stream) {
    USTRUN_CHECK(weak && xw && (!strong || xs) && (!lab || y), "aug_finish: null pointer");
    USTRUN_TRY(check_dims("aug_finish", B, H, W, C, Cl));
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    const dim3 grid(cdiv(cdiv(HW, 4), 256), B);
    finish_image_kernel<<<grid, 256, 0, st>>>(weak, HW, C, xw);
    if (strong) finish_image_kernel<<<grid, 256, 0, st>>>(strong, HW, C, xs);
    if (lab) {
        const int64_t n = (int64_t)B * HW * Cl;
        bytes_to_float_kernel<<<cdiv(cdiv(n, 4), 256), 256, 0, st>>>(lab, n, y);
    }
    USTRUN_LAUNCH_CHECK("aug_finish");
    return 0;
}
