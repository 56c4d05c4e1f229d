// Segmentation overlays of `test.py --save_img` (include/ustrun.h: ustrun_render_*): what the reference draws per
// image on the host (utils/util.py:299-390), per batch on the device, so that three bytes per pixel reach the host.
//
//   range    per-image min / max over all channels: one block per image, wave shuffles, then LDS (min / max: any order is exact)
//   mask     range rule -> v (f32, each step rounded on its own: no contraction), part colour + halving in double, truncation
//   contour  (img - min) / (max - min) * 255 (f32, three rounded steps), 3 x 3 dilation minus the map per part, drawn in the
//            reference's order, round half to even
// A lane owns up to 4 adjacent pixels of ONE row: one 16-byte load per channel plane and one 12-byte store where W % 4 == 0 and the
// buffers are 16-byte aligned, a scalar path otherwise.  Every access is inside [0, H) x [0, W) of image n < N.  No atomics.
#include "common.h"
#include <math.h>

namespace ustrun {
namespace {

constexpr int RENDER_MAX = 8192;         // H, W limit of every entry
constexpr int MASK_PARTS = 5, CONTOUR_PARTS = 4;

// util.py:368 color_list (mask), util.py:348 color_pred_list (contour; util.py:347 color_gt is mask colour 0)
__device__ __forceinline__ void mask_colour(int i, int c[3]) {
    c[0] = (i == 0 || i == 3 || i == 4) ? 255 : 0;
    c[1] = (i == 1 || i == 3) ? 255 : 0;
    c[2] = (i == 2 || i == 4) ? 255 : 0;
}

// ------------------------------------------------------------------------------------------------------------------- range
// grid N, 1024 threads
__global__ __launch_bounds__(1024) void range_kernel(const float* __restrict__ img, long n, int vec, float* __restrict__ range) {
    __shared__ float wmin[16], wmax[16];
    const float* s = img + (long)blockIdx.x * n;
    float lo = INFINITY, hi = -INFINITY;
    const long n4 = vec ? n / 4 : 0;
    for (long e = threadIdx.x; e < n4; e += 1024) {
        const float4 v = ((const float4*)s)[e];
        lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    for (long e = n4 * 4 + threadIdx.x; e < n; e += 1024) {
        lo = fminf(lo, s[e]);
        hi = fmaxf(hi, s[e]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0) {
        wmin[threadIdx.x >> 6] = lo;
        wmax[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            lo = fminf(lo, wmin[w]);
            hi = fmaxf(hi, wmax[w]);
        }
        range[(long)blockIdx.x * 2] = lo;
        range[(long)blockIdx.x * 2 + 1] = hi;
    }
}

// ---------------------------------------------------------------------------------------------------- the lane's 4 pixels
// quad q of image n: row y, columns x0 .. x0 + cnt - 1
struct Quad { int y, x0, cnt; };
__device__ __forceinline__ bool quad_of(int H, int W, Quad& q) {
    const int QW = (W + 3) >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * QW) return false;
    q.y = i / QW;
    q.x0 = (i % QW) * 4;
    q.cnt = W - q.x0 < 4 ? W - q.x0 : 4;
    return true;
}

// the image's C planes at the quad -> px[pixel][channel], one channel repeated to three
__device__ __forceinline__ void load_quad(const float* __restrict__ img, int n, int C, int H, int W, const Quad& q, int vec,
                                          float px[4][3]) {
    const float* s = img + ((long)n * C * H + q.y) * W + q.x0;
    const long plane = (long)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        alignas(16) float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            if (vec) {
                *(float4*)v = *(const float4*)(s + c * plane);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < q.cnt) v[j] = s[c * plane + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j][c] = c < C ? v[j] : px[j][0];
    }
}

__device__ __forceinline__ void store_quad(uint8_t* __restrict__ out, int n, int H, int W, const Quad& q, int vec, const uint8_t o[12]) {
    uint8_t* d = out + (((long)n * H + q.y) * W + q.x0) * 3;
    if (vec) {
        uint3 w;
        w.x = o[0] | (o[1] << 8) | (o[2] << 16) | ((unsigned)o[3] << 24);
        w.y = o[4] | (o[5] << 8) | (o[6] << 16) | ((unsigned)o[7] << 24);
        w.z = o[8] | (o[9] << 8) | (o[10] << 16) | ((unsigned)o[11] << 24);
        *(uint3*)d = w;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < q.cnt * 3) d[j] = o[j];
    }
}

__device__ __forceinline__ uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// -------------------------------------------------------------------------------------------------------------------- mask
// the lowest part index covering each of the quad's pixels, or -1: one 16-byte load per part plane (two for a label quad)
__device__ __forceinline__ void mask_parts(const void* __restrict__ pred, int kind, int n, int P, int H, int W, const Quad& q, int vec,
                                           int part[4]) {
    const long e = (long)q.y * W + q.x0, plane = (long)H * W;
    for (int j = 0; j < 4; ++j) part[j] = -1;
    if (kind == 1) {
        const long long* s = (const long long*)pred + (long)n * plane + e;
        alignas(16) long long l[4] = {0, 0, 0, 0};
        if (vec) {
            *(longlong2*)&l[0] = *(const longlong2*)s;
            *(longlong2*)&l[2] = *(const longlong2*)(s + 2);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < q.cnt) l[j] = s[j];
        }
        for (int j = 0; j < 4; ++j)
            if (l[j] >= 1 && l[j] <= P) part[j] = (int)l[j] - 1;
        return;
    }
    for (int i = P - 1; i >= 0; --i) {
        const float* s = (const float*)pred + ((long)n * P + i) * plane + e;
        alignas(16) float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            *(float4*)v = *(const float4*)s;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < q.cnt) v[j] = s[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v[j] == 1.0f) part[j] = i;
    }
}

// grid (ceil(H * ceil(W / 4) / 256), N)
__global__ __launch_bounds__(256) void mask_kernel(const float* __restrict__ img, const float* __restrict__ range,
                                                  const void* __restrict__ pred, int kind, int C, int P, int H, int W, int vec,
                                                  uint8_t* __restrict__ out) {
    Quad q;
    if (!quad_of(H, W, q)) return;
    const int n = blockIdx.y;
    const float lo = range[n * 2], hi = range[n * 2 + 1];
    const int rule = lo < -0.5f ? 0 : (hi < 1.5f ? 1 : 2);
    float px[4][3];
    load_quad(img, n, C, H, W, q, vec, px);
    uint8_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int parts[4];
    mask_parts(pred, kind, n, P, H, W, q, vec, parts);
#pragma unroll
    for (int j = 0; j < 4; ++j) {              // (a pixel beyond the row computes on zeros and is not stored)
        const int part = parts[j];
        int col[3] = {0, 0, 0};
        if (part >= 0) mask_colour(part, col);
        const double factor = part >= 0 ? 0.5 : 1.0;
        for (int c = 0; c < 3; ++c) {
            const float x = px[j][c];
            const float v = rule == 0 ? __fmul_rn(__fadd_rn(x, 1.0f), 127.5f) : (rule == 1 ? __fmul_rn(x, 255.0f) : x);
            // (f32 v + 255 can round across an integer: the reference adds in float64, where the sum and the halving are exact)
            const double r = ((double)v + (double)col[c]) * factor;
            o[j * 3 + c] = r >= 255.0 ? 255 : (r > 0.0 ? (uint8_t)(int)r : 0);      // truncation; NaN -> 0
        }
    }
    store_quad(out, n, H, W, q, vec, o);
}

// ----------------------------------------------------------------------------------------------------------------- contour
// foreground bits of pixel (y, x): bit i = part i; outside the image: background
__device__ __forceinline__ unsigned fg_bits(const void* __restrict__ map, int kind, int n, int P, int H, int W, int y, int x) {
    if (y < 0 || y >= H || x < 0 || x >= W) return 0u;
    const long e = (long)y * W + x, plane = (long)H * W;
    if (kind == 1) {
        const long long l = ((const long long*)map)[(long)n * plane + e];
        return (l >= 1 && l <= P) ? 1u << ((int)l - 1) : 0u;
    }
    unsigned b = 0;
    for (int i = 0; i < P; ++i)
        if (((const float*)map)[((long)n * P + i) * plane + e] > 0.0f) b |= 1u << i;
    return b;
}

// contour bits of the quad's pixels: (OR over the 3 x 3 neighbourhood) & ~centre.  18 reads for 4 pixels
__device__ __forceinline__ void contour_bits(const void* __restrict__ map, int kind, int n, int P, int H, int W, const Quad& q,
                                             unsigned out[4]) {
    unsigned col[6], ctr[6];                        // columns x0 - 1 .. x0 + 4: OR over the three rows, and the middle row
    for (int k = 0; k < 6; ++k) {
        const int x = q.x0 - 1 + k;
        const unsigned m = fg_bits(map, kind, n, P, H, W, q.y, x);
        ctr[k] = m;
        col[k] = m | fg_bits(map, kind, n, P, H, W, q.y - 1, x) | fg_bits(map, kind, n, P, H, W, q.y + 1, x);
    }
    for (int j = 0; j < 4; ++j) out[j] = (col[j] | col[j + 1] | col[j + 2]) & ~ctr[j + 1];
}

// grid as mask_kernel
__global__ __launch_bounds__(256) void contour_kernel(const float* __restrict__ img, const float* __restrict__ range,
                                                     const void* __restrict__ pred, const void* __restrict__ gt, int kind, int C,
                                                     int P, int H, int W, int vec, uint8_t* __restrict__ out) {
    Quad q;
    if (!quad_of(H, W, q)) return;
    const int n = blockIdx.y;
    const float lo = range[n * 2], hi = range[n * 2 + 1];
    const float span = __fsub_rn(hi, lo);
    float px[4][3];
    load_quad(img, n, C, H, W, q, vec, px);
    unsigned cp[4], cg[4];
    contour_bits(pred, kind, n, P, H, W, q, cp);
    contour_bits(gt, kind, n, P, H, W, q, cg);
    uint8_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {              // (a pixel beyond the row computes on zeros and is not stored)
        int part = -1;                              // the last contour drawn: pred i = mask colour i + 1, gt = mask colour 0
        for (int i = 0; i < P; ++i) {
            if (cp[j] >> i & 1u) part = i + 1;
            if (cg[j] >> i & 1u) part = 0;
        }
        if (part >= 0) {
            int col[3];
            mask_colour(part, col);
            for (int c = 0; c < 3; ++c) o[j * 3 + c] = (uint8_t)col[c];
        } else if (span != 0.0f) {                  // (a constant image: 0, where the reference divides 0 by 0)
            for (int c = 0; c < 3; ++c) {
                const float v = __fmul_rn(__fdiv_rn(__fsub_rn(px[j][c], lo), span), 255.0f);
                o[j * 3 + c] = v >= 255.0f ? 255 : (v > 0.0f ? clamp8((int)rintf(v)) : 0);
            }
        }
    }
    store_quad(out, n, H, W, q, vec, o);
}

int check_dims(const char* who, int N, int C, int P, int pmax, int kind, int H, int W) {
    USTRUN_CHECK(N > 0 && N <= 65535, "%s: batch %d outside [1, 65535]", who, N);
    USTRUN_CHECK(H > 0 && W > 0 && H <= RENDER_MAX && W <= RENDER_MAX, "%s: extent %d x %d outside [1, %d]", who, H, W, RENDER_MAX);
    USTRUN_CHECK(C == 1 || C == 3, "%s: %d image channels (1 or 3)", who, C);
    USTRUN_CHECK(P >= 1 && P <= pmax, "%s: %d parts outside [1, %d]", who, P, pmax);
    USTRUN_CHECK(kind == 0 || kind == 1, "%s: prediction kind %d (0: f32 planes, 1: int64 labels)", who, kind);
    return 0;
}

int aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int ustrun_render_range(const float* img, int32_t N, int32_t C, int32_t H, int32_t W, float* range, ustrun_stream_t stream) {
    USTRUN_CHECK(img && range, "render_range: null pointer");
    USTRUN_TRY(check_dims("render_range", N, C, 1, 1, 0, H, W));
    const long n = (long)C * H * W;
    range_kernel<<<N, 1024, 0, (hipStream_t)stream>>>(img, n, aligned16(img) && n % 4 == 0, range);
    USTRUN_LAUNCH_CHECK("render_range");
    return 0;
}

extern "C" int ustrun_render_mask(const float* img, const float* range, const void* pred, int32_t pred_kind, int32_t N, int32_t C,
                                  int32_t P, int32_t H, int32_t W, uint8_t* out, ustrun_stream_t stream) {
    USTRUN_CHECK(img && range && pred && out, "render_mask: null pointer");
    USTRUN_TRY(check_dims("render_mask", N, C, P, MASK_PARTS, pred_kind, H, W));
    const int vec = W % 4 == 0 && aligned16(img) && aligned16(pred) && aligned16(out);
    mask_kernel<<<dim3(cdiv((int64_t)H * cdiv(W, 4), 256), N), 256, 0, (hipStream_t)stream>>>(img, range, pred, pred_kind, C, P, H, W,
                                                                                            vec, out);
    USTRUN_LAUNCH_CHECK("render_mask");
    return 0;
}

extern "C" int ustrun_render_contour(const float* img, const float* range, const void* pred, const void* gt, int32_t kind, int32_t N,
                                     int32_t C, int32_t P, int32_t H, int32_t W, uint8_t* out, ustrun_stream_t stream) {
    USTRUN_CHECK(img && range && pred && gt && out, "render_contour: null pointer");
    USTRUN_TRY(check_dims("render_contour", N, C, P, CONTOUR_PARTS, kind, H, W));
    const int vec = W % 4 == 0 && aligned16(img) && aligned16(out);
    contour_kernel<<<dim3(cdiv((int64_t)H * cdiv(W, 4), 256), N), 256, 0, (hipStream_t)stream>>>(img, range, pred, gt, kind, C, P, H, W,
                                                                                               vec, out);
    USTRUN_LAUNCH_CHECK("render_contour");
    return 0;
}
