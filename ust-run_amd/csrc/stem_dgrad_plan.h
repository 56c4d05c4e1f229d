// stem_dgrad_plan.h -- the tap and parity arithmetic of the 7x7 / stride-2 / padding-3 stem convolution's input gradient
// (conv_stem_dgrad.hip).  Per axis, input pixel i receives through tap k from the output pixel o = (i + 3 - k) / 2 where i + 3 - k is
// even and o lies in [0, Ho).  With i = 2 q + p (quad q, parity p) the taps of parity p are k = 3 + p - 2 d and o = q + d, d = -1..2:
// an even pixel has the three odd taps (d = -1, 0, 1), an odd pixel the four even ones, and BOTH pixels of a quad read the same four
// outputs q - 1 .. q + 2.  A tile of SD_T input pixels (SD_Q quads) per axis therefore reads SD_Q + 3 outputs from q0 - 1 on.
// Pure integer code without device-only constructs: the kernel reads its indices from here and tests/host/stem_dgrad_plan_check.hip
// compiles it for the host and compares it with brute force over whole ranges of extents.
#pragma once
#include "common.h"

namespace ustrun {

constexpr int SD_K = 7, SD_PAD = 3;                  // the geometry is fixed: kernel 7, stride 2, padding 3
constexpr int SD_T = 32;                             // the tile: SD_T x SD_T input pixels per block ...
constexpr int SD_Q = SD_T / 2;                       // ... = SD_Q x SD_Q quads of 2 x 2 pixels
constexpr int SD_PATCH = SD_Q + 3;                   // dy pixels a tile reads per axis
constexpr int SD_DMIN = -1, SD_DMAX = 2;             // a quad q reads the outputs q + d, d = SD_DMIN .. SD_DMAX

// output extent of the convolution: (H + 2 * 3 - 7) / 2 + 1
__host__ __device__ constexpr int sd_out_extent(int H) { return (H - 1) / 2 + 1; }
// tiles per axis
__host__ __device__ constexpr int sd_tiles(int H) { return (H + SD_T - 1) / SD_T; }
// the dy patch of the tile whose first input pixel is t0 (a multiple of SD_T): outputs [origin, origin + SD_PATCH); the origin is -1
// for the first tile and the patch may pass Ho: what lies outside [0, Ho) is staged as zeros
__host__ __device__ constexpr int sd_patch_origin(int t0) { return t0 / 2 + SD_DMIN; }

// parity of the input pixels tap k serves (k odd: even pixels) and the offset d of the output it reads from: o = q + d
__host__ __device__ constexpr int sd_tap_parity(int k) { return (k + 1) & 1; }
__host__ __device__ constexpr int sd_tap_shift(int k) { return (SD_PAD + sd_tap_parity(k) - k) / 2; }      // (the numerator is even)
// the tap through which a pixel of parity p reads the output q + d; -1: none (p = 0, d = 2)
__host__ __device__ constexpr int sd_tap_of(int p, int d) { return (SD_PAD + p - 2 * d >= 0 && SD_PAD + p - 2 * d < SD_K) ? SD_PAD + p - 2 * d : -1; }
// patch-relative index the quad lq of a tile (0 .. SD_Q - 1) reads through tap k: 0 .. SD_PATCH - 1
__host__ __device__ constexpr int sd_patch_index(int lq, int k) { return lq + sd_tap_shift(k) - SD_DMIN; }

// the taps of input pixel i and the outputs they read, those inside [0, Ho) only, by rising k
struct SdTaps { int n, k[4], o[4]; };
__host__ __device__ inline SdTaps sd_pixel_taps(int i, int Ho) {
    SdTaps t = {};
    for (int k = 0; k < SD_K; ++k) {
        if (sd_tap_parity(k) != (i & 1)) continue;
        const int o = (i >> 1) + sd_tap_shift(k);
        if (o < 0 || o >= Ho) continue;
        t.k[t.n] = k; t.o[t.n] = o; ++t.n;
    }
    return t;
}

}  // namespace ustrun
