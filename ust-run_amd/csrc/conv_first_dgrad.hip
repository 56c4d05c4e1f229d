// conv_first_dgrad.hip -- input gradient of the network's first convolution (inc.conv0, unet_parts.py:16: 3x3, padding 1, no
// bias; Cin = 1..4 image channels, Cout = the base width) and the feature-gradient add of the whole-network backward.
//
//   dx[n][c][y][x] = sum_{co,kh,kw} dy[n][y + 1 - kh][x + 1 - kw][co] * w[co][c][kh][kw]
//
// With 9 * Cin <= 36 output values per pixel against Cout inputs this is no matrix-core problem either way round: the layer
// reads Cout * esz bytes per pixel, writes 4 * Cin and does 18 * Cin * Cout flop -- at 64 channels 13.5 VALU cycles per pixel and CU
// beside 18-36 cycles of HBM time, so a direct f32 stencil on the VALU is enough, and it keeps the products exact for every
// storage type (stored value x f32 weight, f32 accumulation in one fixed order).
//
//  * block = a 16 x 16 pixel tile of one image, 256 threads.  dy passes through LDS 32 channels at a time, as f32 whatever the
//    storage type (the 18 x 18 halo tile: 128 B per pixel + 16 B pad, rows padded so that the four strip rows of a wave fall on
//    the same banks: ds_read_b128 is then conflict-free); the chunk's 9 * Cin * 32 weights sit beside it as [tap][c][co].
//  * lane = a vertical strip of 4 output pixels, wave = every fourth group of 4 channels of the chunk: a dy value read from LDS
//    serves up to three pixels of the strip, a (wave-uniform: broadcast) weight read serves all four.
//  * the four waves' sums meet in LDS at the end and are added in wave order; dx is written NCHW, overwritten.
#include "common.h"

namespace ustrun {
namespace {

constexpr int DT = 16;                        // the tile: DT x DT output pixels per block
constexpr int DHALO = DT + 2;
constexpr int DCH = 32;                       // channels of dy staged per chunk (f32 in LDS)
constexpr int DPIX = DCH * 4 + 16;            // bytes per halo pixel
constexpr int DROW = DHALO * DPIX + 32;       // bytes per halo row: 4 * DROW = 0 mod 256 (the strip rows of a wave share banks)
constexpr int DTILE = DHALO * DROW;
static_assert((4 * DROW) % 256 == 0 && DROW % 16 == 0, "dgrad tile pitch");

template <int ESZ, int CIN>
__global__ __launch_bounds__(256) void conv_first_dgrad_kernel(const void* __restrict__ dy, const float* __restrict__ w,
                                                              int H, int W, int Cout, float* __restrict__ dx,
                                                              int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) char tile[DTILE];                   // later: the waves' sums [4][CIN][256]
    __shared__ __attribute__((aligned(16))) float wl[9 * CIN][DCH];
    static_assert(DTILE >= 4 * CIN * DT * DT * 4, "the final sum lives in the tile's memory");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (tiles_y * tiles_x);
    const int rem = blockIdx.x - img * tiles_y * tiles_x;
    const int y0 = (rem / tiles_x) * DT, x0 = (rem % tiles_x) * DT;
    const int col = lane & 15, sr = lane >> 4;                // the strip: output rows 4 sr .. 4 sr + 3 of column col
    float acc[4][CIN];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < CIN; ++c) acc[p][c] = 0.f;

    constexpr int IPP = DCH / 4;                              // 4-channel items per halo pixel
    constexpr int ITEMS = (DHALO * DHALO * IPP + 255) / 256;
    for (int c0 = 0; c0 < Cout; c0 += DCH) {
        const int cc = min(DCH, Cout - c0), ng = cc >> 2;     // channels / 4-channel groups of this chunk
        // ---- stage: every load of the chunk first (zeros outside the image and past the chunk's channels), then the LDS stores
        f32x4 v[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int e = tid + 256 * i;
            const int hp = e / IPP, g = e - hp * IPP;
            const int hy = hp / DHALO, hx = hp - hy * DHALO;
            const int gy = y0 + hy - 1, gx = x0 + hx - 1;
            v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (hp < DHALO * DHALO && g < ng && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const long o = (((long)img * H + gy) * W + gx) * Cout + c0 + 4 * g;
                if (ESZ == 4) {
                    v[i] = *(const f32x4*)((const float*)dy + o);
                } else {
                    const bf16x4 h = *(const bf16x4*)((const elt_t*)dy + o);
                    v[i] = (f32x4){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                }
            }
        }
        __syncthreads();                                      // (every wave is done with the previous chunk)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int e = tid + 256 * i;
            const int hp = e / IPP, g = e - hp * IPP;
            const int hy = hp / DHALO, hx = hp - hy * DHALO;
            if (hp < DHALO * DHALO) *(f32x4*)(tile + hy * DROW + hx * DPIX + g * 16) = v[i];
        }
        for (int t = tid; t < 9 * CIN * DCH; t += 256) {      // w[co][c][tap] -> wl[tap * CIN + c][co - c0]
            const int co = t % DCH, k = t / DCH, c = k % CIN, tap = k / CIN;
            wl[k][co] = co < cc ? w[((long)(c0 + co) * CIN + c) * 9 + tap] : 0.f;
        }
        __syncthreads();
        // ---- compute: halo row 4 sr + r (r = 0..5) feeds output rows p = r - 2 + kh of the strip, halo column col + 2 - kw
        for (int g = wave; g < ng; g += 4) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                f32x4 wv[3][CIN];
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int c = 0; c < CIN; ++c) wv[kh][c] = *(const f32x4*)&wl[(kh * 3 + kw) * CIN + c][4 * g];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    const f32x4 d = *(const f32x4*)(tile + (4 * sr + r) * DROW + (col + 2 - kw) * DPIX + g * 16);
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int kh = p + 2 - r;             // dy row y + 1 - kh = halo row (4 sr + p) + 2 - kh
                        if (kh < 0 || kh > 2) continue;
#pragma unroll
                        for (int c = 0; c < CIN; ++c) {
                            float a = acc[p][c];
                            a = fmaf(d[0], wv[kh][c][0], a); a = fmaf(d[1], wv[kh][c][1], a);
                            a = fmaf(d[2], wv[kh][c][2], a); a = fmaf(d[3], wv[kh][c][3], a);
                            acc[p][c] = a;
                        }
                    }
                }
            }
        }
    }
    // ---- the four waves' sums, added in wave order
    __syncthreads();
    float* red = (float*)tile;                                // [wave][c][pixel]
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < CIN; ++c) red[(wave * CIN + c) * (DT * DT) + (4 * sr + p) * DT + col] = acc[p][c];
    __syncthreads();
    for (int e = tid; e < CIN * DT * DT; e += 256) {
        const int c = e / (DT * DT), pix = e - c * (DT * DT);
        const int oy = y0 + pix / DT, ox = x0 + pix % DT;
        if (oy < H && ox < W) {
            float s = red[e];
#pragma unroll
            for (int q = 1; q < 4; ++q) s += red[q * CIN * DT * DT + e];
            dx[(((long)img * CIN + c) * H + oy) * W + ox] = s;
        }
    }
}

// da[n][hw][c] (storage type, NHWC) = (add ? da : 0) + dfeat[n][c][hw] (f32, NCHW): 64 pixels x 64 channels per block through LDS
template <int ESZ>
__global__ __launch_bounds__(256) void feat_grad_add_kernel(const float* __restrict__ dfeat, void* __restrict__ da, int HW, int C,
                                                           int add, int tiles) {
    __shared__ float t[64][65];
    const int img = blockIdx.x / tiles, p0 = (blockIdx.x - img * tiles) * 64;
    const int np = min(64, HW - p0);
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int cc = min(64, C - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * cc; e += 256) {
            const int c = e >> 6, p = e & 63;
            if (p < np) t[p][c] = dfeat[((long)img * C + c0 + c) * HW + p0 + p];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < np * cc; e += 256) {
            const int p = e / cc, c = e - p * cc;
            const long o = ((long)img * HW + p0 + p) * C + c0 + c;
            if (ESZ == 4) {
                float* d = (float*)da + o;
                *d = add ? *d + t[p][c] : t[p][c];
            } else {
                elt_t* d = (elt_t*)da + o;
                *d = (elt_t)(add ? (float)*d + t[p][c] : t[p][c]);
            }
        }
    }
}

}  // namespace

int feat_grad_add(const float* dfeat, void* da, int N, int HW, int C, int add, int dtype, hipStream_t st) {
    USTRUN_CHECK(dfeat && da && N > 0 && HW > 0 && C > 0, "feat_grad_add: bad arguments");
    const int tiles = cdiv(HW, 64);
    USTRUN_CHECK((long)N * tiles < (1L << 31), "feat_grad_add: %d images x %d tiles", N, tiles);
    if (dtype == USTRUN_D16)
        hipLaunchKernelGGL(feat_grad_add_kernel<2>, dim3(N * tiles), dim3(256), 0, st, dfeat, da, HW, C, add, tiles);
    else
        hipLaunchKernelGGL(feat_grad_add_kernel<4>, dim3(N * tiles), dim3(256), 0, st, dfeat, da, HW, C, add, tiles);
    USTRUN_LAUNCH_CHECK("feat_grad_add");
    return 0;
}

}  // namespace ustrun

using namespace ustrun;

extern "C" int ustrun_conv_first_dgrad(const void* dy, const float* w, int N, int H, int W, int Cout, int Cin, float* dx,
                                       int dtype, ustrun_stream_t s) {
    USTRUN_CHECK(dtype_ok(dtype), "conv_first_dgrad: dtype %d not built", dtype);
    USTRUN_CHECK(Cin >= 1 && Cin <= 4, "conv_first_dgrad: Cin=%d (1..4 input channels are built)", Cin);
    USTRUN_CHECK(Cout >= 8 && Cout <= 64 && Cout % 8 == 0, "conv_first_dgrad: Cout=%d (a multiple of 8 up to 64)", Cout);
    USTRUN_CHECK(N > 0 && H > 0 && W > 0, "conv_first_dgrad: bad extent N=%d %dx%d", N, H, W);
    USTRUN_CHECK(dy && w && dx, "conv_first_dgrad: null pointer");
    const int tx = cdiv(W, DT), ty = cdiv(H, DT);
    USTRUN_CHECK((long)N * tx * ty < (1L << 31), "conv_first_dgrad: %d images x %d x %d tiles", N, ty, tx);
    const dim3 grid(N * tx * ty), block(256);
    // (USTRUN_F32X3 stores f32 and this layer is not bound by the matrix cores: it runs the f32 build)
#define USTRUN_FD(E, CI) hipLaunchKernelGGL((conv_first_dgrad_kernel<E, CI>), grid, block, 0, (hipStream_t)s, dy, w, H, W, Cout, dx, tx, ty)
#define USTRUN_FDC(E) do { if (Cin == 1) USTRUN_FD(E, 1); else if (Cin == 2) USTRUN_FD(E, 2); else if (Cin == 3) USTRUN_FD(E, 3); else USTRUN_FD(E, 4); } while (0)
    if (dtype == USTRUN_D16) USTRUN_FDC(2); else USTRUN_FDC(4);
#undef USTRUN_FDC
#undef USTRUN_FD
    USTRUN_LAUNCH_CHECK("conv_first_dgrad");
    return 0;
}
