// conv_stem_dgrad.hip -- input gradient of the DeepLabV2-ResNet stem (Conv2d(3, 64, 7, stride=2, padding=3, bias=False),
// networks/backbone/resnet.py:124,160): the gradient of the network's input image.
//
//   dx[n][c][iy][ix] = sum_{co,ky,kx} w[co][c][ky][kx] * dy[n][(iy + 3 - ky) / 2][(ix + 3 - kx) / 2][co]
//
// over the taps for which iy + 3 - ky and ix + 3 - kx are even and the output pixel exists.  2352 FMAs per input pixel against
// (Cout / 4) * esz bytes read and 12 written: VALU work by more than 10x, so -- as for the U-Net's first convolution
// (conv_first_dgrad.hip) -- a direct f32 stencil: stored value x f32 weight, f32 accumulation in one fixed order, no atomics.
//
//  * the 2 x 2 input pixels of a quad (stem_dgrad_plan.h) read the same 4 x 4 outputs and split the 49 taps between them by parity,
//    so a lane that owns whole quads walks all 49 taps x 3 channels whatever its position: no parity divergence inside a wave.
//  * block = a 32 x 32 input tile (16 x 16 quads) of one image, 256 threads.  Its 19 x 19 dy patch passes through LDS 32 channels at
//    a time, as f32 whatever the storage type, zeros outside the output map (144 B per pixel, rows padded so that the four strip
//    rows of a wave fall on the same banks: ds_read_b128 is conflict-free); the chunk's 147 x 32 weights sit beside it as
//    [tap][c][co].  73.5 KB per block: two blocks per CU.
//  * lane = a vertical strip of 4 quads (8 x 2 input pixels: 48 sums), wave = every fourth group of 4 channels of the chunk: a dy
//    value read from LDS serves several quads of the strip, a (wave-uniform: broadcast) weight read all four: per patch column and
//    column parity 7 dy reads and 21 weight reads for 336 FMAs.
//  * the four waves' sums meet in LDS at the end and are added in wave order; dx is written NCHW, overwritten.
#include "common.h"
#include "stem_dgrad_plan.h"

namespace ustrun {
namespace {

constexpr int SCI = 3;                                // input channels
constexpr int STAPS = SD_K * SD_K;
constexpr int SCH = 32;                               // channels of dy staged per chunk (f32 in LDS)
constexpr int SPIX = SCH * 4 + 16;                    // bytes per patch pixel
constexpr int SROW = SD_PATCH * SPIX + 16;            // bytes per patch row: 4 * SROW = 0 mod 256 (the strip rows of a wave share banks)
constexpr int STILE = SD_PATCH * SROW;
constexpr int SWP = SCH + 4;                          // floats per weight row (the transposing stores spread over the banks)
constexpr int SQS = 4;                                // quads per lane (a vertical strip)
static_assert((4 * SROW) % 256 == 0 && SROW % 16 == 0 && SPIX % 16 == 0, "stem dgrad patch pitch");
static_assert(SD_Q * SD_Q == 64 * SQS && SD_Q == 16, "one wave covers the tile: 16 quad columns x 4 strips of 4 quads");
static_assert(2 * (STILE + STAPS * SCI * SWP * 4) <= 160 * 1024, "two blocks per CU");

template <int ESZ>
__global__ __launch_bounds__(256, 2) void conv_stem_dgrad_kernel(const void* __restrict__ dy, const float* __restrict__ w, int H, int W,
                                                             int Ho, int Wo, int Cout, float* __restrict__ dx, int tiles_x,
                                                             int tiles_y) {
    __shared__ __attribute__((aligned(16))) char tile[STILE];                   // later: the waves' sums [4][SCI][SD_T * SD_T]
    __shared__ __attribute__((aligned(16))) float wl[STAPS * SCI][SWP];
    static_assert(STILE >= 4 * SCI * SD_T * SD_T * 4, "the final sum lives in the patch's memory");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / (tiles_y * tiles_x);
    const int rem = blockIdx.x - img * tiles_y * tiles_x;
    const int y0 = (rem / tiles_x) * SD_T, x0 = (rem % tiles_x) * SD_T;
    const int py0 = sd_patch_origin(y0), px0 = sd_patch_origin(x0);
    const int col = lane & 15, sr = lane >> 4;                // the strip: quad rows 4 sr .. 4 sr + 3 of quad column col
    float acc[SQS][2][2][SCI];                                // [quad][row parity][column parity][channel]
#pragma unroll
    for (int j = 0; j < SQS; ++j)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < SCI; ++c) acc[j][p >> 1][p & 1][c] = 0.f;

    constexpr int IPP = SCH / 4;                              // 4-channel items per patch pixel
    constexpr int ITEMS = (SD_PATCH * SD_PATCH * IPP + 255) / 256;
    for (int c0 = 0; c0 < Cout; c0 += SCH) {
        const int cc = min(SCH, Cout - c0), ng = cc >> 2;     // channels / 4-channel groups of this chunk
        // ---- stage: every load of the chunk first (zeros outside the output map and past the chunk's channels), then the LDS stores
        f32x4 v[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int e = tid + 256 * i;
            const int hp = e / IPP, g = e - hp * IPP;
            const int hy = hp / SD_PATCH, hx = hp - hy * SD_PATCH;
            const int gy = py0 + hy, gx = px0 + hx;
            v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (hp < SD_PATCH * SD_PATCH && g < ng && gy >= 0 && gy < Ho && gx >= 0 && gx < Wo) {
                const long o = (((long)img * Ho + gy) * Wo + gx) * Cout + c0 + 4 * g;
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
            const int hy = hp / SD_PATCH, hx = hp - hy * SD_PATCH;
            if (hp < SD_PATCH * SD_PATCH) *(f32x4*)(tile + hy * SROW + hx * SPIX + g * 16) = v[i];
        }
        for (int t = tid; t < STAPS * SCI * SCH; t += 256) {  // w[co][c][tap] (read along its rows) -> wl[tap * SCI + c][co - c0]
            const int co = t / (STAPS * SCI), k = t - co * (STAPS * SCI), c = k / STAPS, tap = k - c * STAPS;
            wl[tap * SCI + c][co] = co < cc ? w[(long)(c0 + co) * (STAPS * SCI) + k] : 0.f;
        }
        __syncthreads();
        // ---- compute: patch column col + e and patch rows 4 sr + r (r = 0..6) feed, through tap (ky, kx), the pixels of parity
        // (sd_tap_parity(ky), sd_tap_parity(kx)) of the quads whose patch index for that tap they are.  The column parity px is
        // unrolled (it selects registers), the patch column e is a loop: its body -- 7 dy and 21 weight reads for 336 FMAs -- is what the
        // compiler may hoist at once
        for (int g = wave; g < ng; g += 4) {
#pragma unroll
            for (int px = 0; px < 2; ++px) {
#pragma unroll 1
                for (int e = 0; e <= SD_DMAX - SD_DMIN; ++e) {
                    const int kx = sd_tap_of(px, e + SD_DMIN);
                    if (kx < 0) continue;                     // (an even pixel reads three of the four columns)
                    f32x4 d[SQS + SD_DMAX - SD_DMIN];
#pragma unroll
                    for (int r = 0; r < SQS + SD_DMAX - SD_DMIN; ++r)
                        d[r] = *(const f32x4*)(tile + (SQS * sr + r) * SROW + (col + e) * SPIX + g * 16);
#pragma unroll
                    for (int ky = 0; ky < SD_K; ++ky) {
                        const int py = sd_tap_parity(ky);
                        f32x4 wv[SCI];
#pragma unroll
                        for (int c = 0; c < SCI; ++c) wv[c] = *(const f32x4*)&wl[(ky * SD_K + kx) * SCI + c][4 * g];
#pragma unroll
                        for (int j = 0; j < SQS; ++j) {
                            const f32x4 dv = d[sd_patch_index(j, ky)];
#pragma unroll
                            for (int c = 0; c < SCI; ++c) {
                                float a = acc[j][py][px][c];
                                a = fmaf(dv[0], wv[c][0], a); a = fmaf(dv[1], wv[c][1], a);
                                a = fmaf(dv[2], wv[c][2], a); a = fmaf(dv[3], wv[c][3], a);
                                acc[j][py][px][c] = a;
                            }
                        }
                    }
                }
            }
        }
    }
    // ---- the four waves' sums, added in wave order
    __syncthreads();
    float* red = (float*)tile;                                // [wave][c][pixel of the tile]
#pragma unroll
    for (int j = 0; j < SQS; ++j)
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int c = 0; c < SCI; ++c)
                *(f32x2*)&red[(wave * SCI + c) * (SD_T * SD_T) + (2 * (SQS * sr + j) + py) * SD_T + 2 * col] =
                    (f32x2){acc[j][py][0][c], acc[j][py][1][c]};
    __syncthreads();
    for (int e = tid; e < SCI * SD_T * SD_T; e += 256) {
        const int c = e / (SD_T * SD_T), pix = e - c * (SD_T * SD_T);
        const int oy = y0 + pix / SD_T, ox = x0 + pix % SD_T;
        if (oy < H && ox < W) {
            float s = red[e];
#pragma unroll
            for (int q = 1; q < 4; ++q) s += red[q * SCI * SD_T * SD_T + e];
            dx[(((long)img * SCI + c) * H + oy) * W + ox] = s;
        }
    }
}

}  // namespace
}  // namespace ustrun

using namespace ustrun;

extern "C" int ustrun_conv_stem_dgrad(const void* dy, const float* w, int N, int H, int W, int Cout, int Cin, float* dx, int dtype,
                                      ustrun_stream_t s) {
    USTRUN_CHECK(dtype_ok(dtype), "conv_stem_dgrad: dtype %d not built", dtype);
    USTRUN_CHECK(Cin == SCI, "conv_stem_dgrad: Cin=%d (3 input channels are built)", Cin);
    USTRUN_CHECK(Cout >= 8 && Cout <= 64 && Cout % 8 == 0, "conv_stem_dgrad: Cout=%d (a multiple of 8 up to 64)", Cout);
    USTRUN_CHECK(N > 0 && H > 0 && W > 0, "conv_stem_dgrad: bad extent N=%d %dx%d", N, H, W);
    USTRUN_CHECK(dy && w && dx, "conv_stem_dgrad: null pointer");
    const int tx = sd_tiles(W), ty = sd_tiles(H);
    USTRUN_CHECK((long)N * tx * ty < (1L << 31), "conv_stem_dgrad: %d images x %d x %d tiles", N, ty, tx);
    const dim3 grid(N * tx * ty), block(256);
    const int Ho = sd_out_extent(H), Wo = sd_out_extent(W);
    // (USTRUN_F32X3 stores f32 and this layer is not bound by the matrix cores: it runs the f32 build)
    if (dtype == USTRUN_D16)
        hipLaunchKernelGGL(conv_stem_dgrad_kernel<2>, grid, block, 0, (hipStream_t)s, dy, w, H, W, Ho, Wo, Cout, dx, tx, ty);
    else
        hipLaunchKernelGGL(conv_stem_dgrad_kernel<4>, grid, block, 0, (hipStream_t)s, dy, w, H, W, Ho, Wo, Cout, dx, tx, ty);
    USTRUN_LAUNCH_CHECK("conv_stem_dgrad");
    return 0;
}
