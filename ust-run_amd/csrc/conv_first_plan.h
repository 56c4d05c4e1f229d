// conv_first_plan.h -- the strip plans of the first convolution's streaming kernels (conv_first.hip), the decode of a work item and the
// one predicate for "the streaming weight gradient may run".  Pure integer code without device-only constructs: the kernels, the host
// side and the dispatcher (ops.hip) all read the plan from here, and tests/host/conv_first_plan_check.hip compiles it for the host and
// pins it over whole ranges of shapes.
#pragma once
#include "common.h"

namespace ustrun {

constexpr int CF_FWD_TW = 32, CF_FWD_TH = 8;       // forward: strip width, rows per step
constexpr int CF_WG_TW = 16;                       // weight gradient: strip width (one row of it = one MFMA k-step)
constexpr int CF_WG_ITEMS = 4096, CF_WG_WAVES = 4; // weight gradient: at most 4096 items, one per wave -> at most 1024 blocks (slabs)

// ---- forward: a block owns a 32-pixel-wide strip of seg_rows rows of one image, item = (image, segment, strip), strip fastest ------
struct CfFwdPlan { int strips, segs, seg_rows; };
struct CfFwdItem { int img, x0, r0, r1, nsteps; };

// rows per block: 64 where that still gives every CU four blocks, else shorter segments
inline int stream_seg_rows(int N, int H, int W) {
    int seg = 64;
    while (seg > CF_FWD_TH && (long)N * cdiv(W, CF_FWD_TW) * cdiv(H, seg) < 1024) seg >>= 1;
    return seg;
}
inline CfFwdPlan conv_first_fwd_plan(int N, int H, int W) {
    CfFwdPlan p;
    p.strips = cdiv(W, CF_FWD_TW);
    p.seg_rows = stream_seg_rows(N, H, W);
    p.segs = cdiv(H, p.seg_rows);
    return p;
}
// blocks of a launch = statistics rows it writes
inline int conv_first_fwd_grid(int N, const CfFwdPlan& p) { return N * p.segs * p.strips; }

__host__ __device__ __forceinline__ CfFwdItem conv_first_fwd_item(const CfFwdPlan& p, int H, int item) {
    CfFwdItem it;
    const int sx = item % p.strips, sy = (item / p.strips) % p.segs;
    it.img = item / (p.strips * p.segs);
    it.x0 = sx * CF_FWD_TW; it.r0 = sy * p.seg_rows; it.r1 = min(H, it.r0 + p.seg_rows);
    it.nsteps = (it.r1 - it.r0 + CF_FWD_TH - 1) / CF_FWD_TH;
    return it;
}

// ---- weight gradient: a wave owns a 16-pixel-wide strip of seg_rows rows of one image, four items per block, one slab per block ----
struct CfWgradPlan { int strips, nseg, seg_rows, blocks; long items; };
struct CfWgradItem { int img, x0, r0, r1; };

inline CfWgradPlan conv_first_wgrad_plan(int N, int H, int W) {
    CfWgradPlan p;
    p.strips = cdiv(W, CF_WG_TW);
    long segs = CF_WG_ITEMS / ((long)N * p.strips);
    if (segs > H / 8) segs = H / 8;
    if (segs < 1) segs = 1;
    p.seg_rows = cdiv(H, segs);
    p.nseg = cdiv(H, p.seg_rows);
    p.items = (long)N * p.strips * p.nseg;
    p.blocks = cdiv(p.items, CF_WG_WAVES);
    return p;
}

// (strip fastest: the four waves of a block read four neighbouring 2 KB pieces of the same dY rows)
__host__ __device__ __forceinline__ CfWgradItem conv_first_wgrad_item(int strips, int nseg, int seg_rows, int H, int item) {
    CfWgradItem it;
    const int sx = item % strips, sg = (item / strips) % nseg;
    it.img = item / (nseg * strips);
    it.x0 = sx * CF_WG_TW; it.r0 = sg * seg_rows; it.r1 = min(H, it.r0 + seg_rows);
    return it;
}

// The streaming weight-gradient kernel may run: unit pixel stride, f32 source, dense NCHW strides (one buffer resource spans the
// tensor and the kernel's 32-bit offsets are image-major), both tensors under 2^31 - 64 bytes (the resources' range checks), and a
// plan of at most 4096 items (conv_first_wgrad_partials_bytes() holds 1024 slabs).
inline bool conv_first_wgrad_stream_ok(const ustrun_src_t& s, int N, int H, int W, int dy_esz) {
    const long xbytes = (long)N * s.sN * 4, dybytes = (long)N * H * W * 64 * dy_esz;
    return s.sW == 1 && s.f32 && s.sN == (int64_t)s.C * s.sC && s.sC == (int64_t)H * s.sH && xbytes < (1L << 31) - 64 &&
           dybytes < (1L << 31) - 64 && conv_first_wgrad_plan(N, H, W).items <= CF_WG_ITEMS;
}

}  // namespace ustrun
