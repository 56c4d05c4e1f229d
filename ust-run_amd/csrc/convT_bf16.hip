// convT_bf16.hip -- ConvTranspose2d(k=2, s=2) forward and input-gradient on the bf16 matrix cores.
// Replaces nn.ConvTranspose2d in Up (reference networks/unet_parts.py:50-52) and its autograd backward.
//
// With stride == kernel the four taps never overlap, so both directions are plain GEMMs over the
// LOW-resolution pixel grid m = (n, y, x):
//   forward   u[n, 2y+dy, 2x+dx, co] = bias[co] + sum_ci act(a[m, ci]) w[ci, co, dy, dx]
//             -> [M x Cin] x [Cin x 4*Cout], columns ordered (tap, co), scatter epilogue
//   dgrad     da[m, ci] = sum_{tap, co} du[n, 2y+dy, 2x+dx, co] w[ci, co, dy, dx]
//             -> [M x 4*Cout] x [4*Cout x Cin], the K axis ordered (tap, co), gather loader
// A rows are 128 consecutive pixels (no halo, no tile waste at any extent), staged global -> registers ->
// [BatchNorm affine + ReLU in f32] -> bf16 -> XOR-swizzled LDS one chunk ahead of the MFMAs; weights are
// [tap][K/8][N][8] bf16 tiles fetched by LDS-DMA.  The epilogue transposes through per-wave LDS scratch and
// stores 16 bytes per lane (see conv_halo_bf16.hip).  The high-resolution pixel of (m, tap) is
// 4m - 2x + 2*dy*W + dx, so only x = m mod W is ever needed.
// Which build serves a launch, its tiles, LDS bytes and variant code: convT_plan.h.
#include "common.h"
#include "loader.h"
#include "convT_plan.h"

namespace ustrun {
namespace {

constexpr int OOBV = (int)0x80000000;           // a buffer offset that reads zeros and stores nothing
__device__ __forceinline__ int fastmod(int v, int d, float inv) {      // v mod d for 0 <= v < 2^22, d < 2^16
    const int q = (int)(((float)v + 0.5f) * inv);
    int r = v - q * d;
    if (r < 0) r += d;
    if (r >= d) r -= d;
    return r;
}
template <int BK> __device__ __forceinline__ int swz(int p) { return BK == 64 ? ((p >> 1) & 7) : ((p >> 2) & 3); }
// element offset of weight column n in K-row 0 of the packed [K/8][ncols][8] matrix (the forward's columns are (tap, co): [tap][K/8][Cout][8])
template <int MODE> __device__ __forceinline__ long weight_col(const IgemmArgs& a, int n) {
    if (MODE != 0) return (long)n * 8;
    const int tap = n / a.Cout, co = n - tap * a.Cout;
    return ((long)tap * (a.Cin / 8) * a.Cout + co) * 8;
}
// one k-step (16-byte channel group ch of the chunk): two 32-column weight fragments (the MFMA's A operand: D[column][pixel]) x MI pixel sub-tiles
template <class G> __device__ __forceinline__ void mfma_step(f32x16 (&acc)[G::MI][2], const char* Acur, int prow0, int ch, bf16x8 b0, bf16x8 b1) {
#pragma unroll
    for (int i = 0; i < G::MI; ++i) {
        const int p = prow0 + 32 * i;
        const bf16x8 af = *(const bf16x8*)(Acur + p * G::ROWB + ((ch ^ swz<G::BK>(p)) * 16));
        acc[i][0] = USTRUN_MFMA_32x32x16(b0, af, acc[i][0], 0, 0, 0);
        acc[i][1] = USTRUN_MFMA_32x32x16(b1, af, acc[i][1], 0, 0, 0);
    }
}

// ---- the activation stage.  Items: pixel = (tid + 256 i) / CPR, 8-channel group c8 = tid % CPR.
// Round 4: 32-bit, TILE-RELATIVE addressing through a buffer resource whose base is the tile's first (gradient: lowest) source
// row -- the per-tile setup of this kernel was ~2300 instructions per wave in front of 64 MFMAs, most of them 64-bit index
// arithmetic and divisions (profiles/r04_pmc_convT_up4.txt).  The source is dense NHWC (the plan checks), so a forward item
// is px * Cin elements behind the tile base; a gradient item is (4 px - 2 x + 2 W) * Cin behind the base (4 m0 - 2 W) * Cin,
// which keeps the offset non-negative; rows past M fall behind the tensor's end and read zeros by the range check.
template <class G, bool DG> struct ActStage {
    int avoff[G::AIT];                          // byte offsets behind the tile base
    bf16x8 av[G::AIT];
    f32x4 asc0, asc1, ash0, ash1;
    __amdgpu_buffer_rsrc_t ars;
    int c8; bool aff, relu; long goff;          // channel group; BatchNorm (+ ReLU) on load; the pass's offset into the constants
    __device__ __forceinline__ void init(const IgemmArgs& a, int tid, int m0, int x0r, int W, float invW) {
        c8 = tid % G::CPR;
        const long a_total = DG ? (long)a.M * 4 * a.Cin : (long)a.M * a.Cin;               // source elements
        const long a_base = DG ? ((long)4 * m0 - 2 * W) * a.Cin : (long)m0 * a.Cin;        // (negative for the first gradient tile: never dereferenced)
#pragma unroll
        for (int i = 0; i < G::AIT; ++i) {
            const int px = (tid + 256 * i) / G::CPR;
            if (DG) {
                const int x = fastmod(x0r + px, W, invW);
                avoff[i] = ((4 * px - 2 * x + 2 * W) * a.Cin + 8 * c8) * 2;
            } else {
                avoff[i] = (px * a.Cin + 8 * c8) * 2;
            }
            if (m0 + px >= a.M) avoff[i] = OOBV;    // (the gradient's rows past M end up behind the tensor anyway; the forward's last tile needs it
        }                                           //  only when another pass's rows follow in memory -- cheap either way)
        const long a_left = (a_total - a_base) * 2;
        ars = buffer_behind((const elt_t*)a.src[0].ptr + a_base, a_left);
        aff = !DG && a.src[0].scale != nullptr;
        // batched passes: a tile never straddles two passes (the plan checks), its pass picks the BatchNorm constants
        goff = (!DG && a.src[0].gN > 0) ? (long)(m0 / (a.src[0].gN * a.Hb * a.Wb)) * a.src[0].gstride : 0;
        relu = !DG && a.src[0].relu;
    }
    __device__ __forceinline__ void load(const IgemmArgs& a, int c, int W) {      // chunk c: global -> registers
        int koffb;                              // wave-uniform byte offset of the chunk: rides in the scalar offset
        if (DG) {
            const int k0 = c * G::BK, tap = k0 / a.Cin, kk = k0 - tap * a.Cin;
            koffb = (((tap >> 1) * 2 * W + (tap & 1)) * a.Cin + kk) * 2;
        } else {
            koffb = c * G::BK * 2;
            if (aff) {
                const int koff = c * G::BK + 8 * c8;
                asc0 = *(const f32x4*)(a.src[0].scale + goff + koff); asc1 = *(const f32x4*)(a.src[0].scale + goff + koff + 4);
                ash0 = *(const f32x4*)(a.src[0].shift + goff + koff); ash1 = *(const f32x4*)(a.src[0].shift + goff + koff + 4);
            }
        }
#pragma unroll
        for (int i = 0; i < G::AIT; ++i) av[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ars, avoff[i], koffb, 0));
    }
    __device__ __forceinline__ void write(char* Adst, int tid) const {            // registers -> [affine + ReLU] -> swizzled LDS tile
#pragma unroll
        for (int i = 0; i < G::AIT; ++i) {
            const int px = (tid + 256 * i) / G::CPR;
            bf16x8 h = av[i];
            if (aff) h = affine8(av[i], asc0, asc1, ash0, ash1, relu);            // (wave-uniform)
            u32x4 u = __builtin_bit_cast(u32x4, h);
            const bool ok = avoff[i] != OOBV;             // a select, not a branch (rows past M: the affine of a zero is not zero)
#pragma unroll
            for (int q = 0; q < 4; ++q) u[q] = ok ? u[q] : 0u;
            *(bf16x8*)(Adst + px * G::ROWB + ((c8 ^ swz<G::BK>(px)) * 16)) = __builtin_bit_cast(bf16x8, u);
        }
    }
};

// ---- the weight feed through LDS: the B tile of chunk c = rows c*CPR .. +CPR of the [K/8][ncols][8] matrix by LDS-DMA; col = the thread's
// (fixed) column in K-row 0, brow = elements per K/8 row ----
template <class G> __device__ __forceinline__ void dma_weights(const elt_t* col, long brow, int c, char* dst, int tid, int wave) {
#pragma unroll
    for (int i = 0; i < G::BIT; ++i) {
        const int o = (tid + 256 * i) / G::BN;
        __builtin_amdgcn_global_load_lds((gptr_t*)(col + (long)(c * G::CPR + o) * brow), (lptr_t*)(dst + (wave * 64 + 256 * i) * 16), 16, 0, 0);
    }
}
// ---- the weight feed through registers (BREG, round 3, as in conv_halo_bf16.hip): the packed weight layout [K/8][N][8] IS the
// B-fragment layout, so each wave loads the fragments of its 64 columns straight from L2 one stage (two k-steps = 4 MI MFMAs) ahead:
// fragment (k-step ks of the stage, column half j) = K-row c*CPR + 2 ks + lh, column colw + 32 j + l31.  Inline asm (hipcc must not
// fold them into its own vmcnt bookkeeping); the kernel counts them by hand ----
template <class G, int MODE> struct WeightsReg {
    bf16x8 bnx[2][2];
    int bvoff;
    long brow;
    __amdgpu_buffer_rsrc_t wrs;
    __device__ __forceinline__ void init(const IgemmArgs& a, int colw, int l31, int lh) {
        brow = (long)a.Cout * 8;
        wrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, 0x7fffffff, 0x00020000);
        bvoff = (int)((weight_col<MODE>(a, colw + l31) + (long)lh * brow) * 2);
    }
    __device__ __forceinline__ void load(int c, int stg) {       // stage stg (k-steps 2 stg, 2 stg + 1) of chunk c -> bnx
        const int s0 = __builtin_amdgcn_readfirstlane((int)(((long)(c * G::CPR + 4 * stg) * brow) * 2));
        const int s1 = __builtin_amdgcn_readfirstlane((int)(((long)(c * G::CPR + 4 * stg + 2) * brow) * 2));
        asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %4, %5, %6 offen\n\tbuffer_load_dwordx4 %1, %4, %5, %6 offen offset:512\n\t"
                     "buffer_load_dwordx4 %2, %4, %5, %7 offen\n\tbuffer_load_dwordx4 %3, %4, %5, %7 offen offset:512"
                     : "=&v"(bnx[0][0]), "=&v"(bnx[0][1]), "=&v"(bnx[1][0]), "=&v"(bnx[1][1])
                     : "v"(bvoff), "s"(wrs), "s"(s0), "s"(s1) : "memory");
    }
};

// ---- the accumulators start from the bias.  The product is D[column][pixel]: lane = pixel l31 of a 32-pixel sub-tile, registers 4g .. 4g + 3
// of accumulator j = columns 32 j + 8 g + 4 lh + 0..3 -- four consecutive channels of one pixel, so the epilogue packs them with two
// cvt_pk and parks them with ONE ds_write_b64 (round 4: the kernel spent ~1800 VALU instructions per wave and tile beside its 64
// MFMAs -- SQ counters in profiles/r04_pmc_convT_up4.txt -- a quarter of them 2-byte LDS scatter of the other orientation).  The
// bias of a column is a property of the REGISTER now ----
template <class G, int MODE> __device__ __forceinline__ void init_acc(f32x16 (&acc)[G::MI][2], const IgemmArgs& a, char* smem, int wave, int lane, int colw) {
    float* bsc = (float*)smem + wave * 64;              // this wave's 64 bias values (the A tiles are not in use yet)
    const int lh = lane >> 5;
    float bv = 0.f;
    if (MODE != 1 && a.bias) {
        int co0 = colw;
        if (MODE == 0) { const int tp = colw / a.Cout; co0 = colw - tp * a.Cout; }
        bv = a.bias[co0 + lane];
    }
    bsc[lane] = bv;
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 b4 = *(const f32x4*)(bsc + j * 32 + 8 * g + 4 * lh);
#pragma unroll
            for (int i = 0; i < G::MI; ++i) { acc[i][j][4 * g] = b4[0]; acc[i][j][4 * g + 1] = b4[1]; acc[i][j][4 * g + 2] = b4[2]; acc[i][j][4 * g + 3] = b4[3]; }
        }
    __syncthreads();                                    // (the bias scratch aliases the first activation tile)
}

// ---- epilogue: bf16, per-wave LDS transpose (ds_write_b64: four channels of a pixel), 16-byte stores of 64 contiguous channels; the
// tensors beside the stored pieces (join: the other contribution and the ReLU reference; BNS: y) and the statistics rows ----
template <class G, int MODE, bool BNS, bool JOIN>
__device__ __forceinline__ void epilogue(const IgemmArgs& a, f32x16 (&acc)[G::MI][2], char* smem, int tid, int wave, int mtile, int n0, int x0r, int W, float invW) {
    constexpr bool DG = MODE == 1, PLAIN = MODE == 2, LIN = DG || PLAIN;         // LIN: the output is pixel-linear (no scatter)
    constexpr int EPITCH = G::EPITCH, MI = G::MI, BN = G::BN, WN = G::WN, WM = G::WM;
    const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5, wm = wave / WN, wn = wave % WN, m0 = mtile * G::BM;
    char* ep = smem + wave * (32 * EPITCH);
    const int colw = n0 + wn * 64;               // first of this wave's 64 columns
    int tap = 0, co0 = colw;
    if (!LIN) { tap = colw / a.Cout; co0 = colw - tap * a.Cout; }
    float st1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, st2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // PLAIN: statistics of the lane's 8 channels (lane & 7)
    // stores: 32-bit offsets behind the wave's own base through a buffer resource (soffset 0: see conv_first.hip on why no
    // register soffset rides on a 128-bit store) -- forward: base = pixel 4 m0 - 2 W + tap offset, channel co0; a piece of row d sits
    // (4 d - 2 x + 2 W) * Cout + 8 ch behind it; gradient / plain: base = pixel m0, column colw.  Rows past M fall behind the tensor.
    const long tapoff = (long)(tap >> 1) * 2 * W + (tap & 1);
    const long o_total = LIN ? (long)a.M * a.Cout : (long)a.M * 4 * a.Cout;
    const long o_base = LIN ? (long)m0 * a.Cout + colw : ((long)4 * m0 - 2 * W + tapoff) * a.Cout + co0;
    const long o_left = (o_total - o_base) * 2;
    const __amdgpu_buffer_rsrc_t ors = buffer_behind((elt_t*)a.out0 + o_base, o_left);
    // this lane's pieces of a sub-tile: pixel rows r0 + 8 t (t = 0..3), channel group ch -- x advances by 8 per piece
    const int r0 = lane >> 3, ch = lane & 7;
    // BNS (round 4): da written here is the gradient at a BatchNorm + ReLU layer's output (the conv2 under this ConvTranspose); its
    // backward sums sum(da mask), sum(da mask y) are formed from the stored pieces and the 16 bytes of y beside each, as one
    // statistics row per 128-pixel tile (the tile lies inside one pass: the plan checks) -- conv_halo_bf16.hip, same idea
    float bsc[8], bsh[8];
    __amdgpu_buffer_rsrc_t yrs = ors;
    if constexpr (BNS) {
        if (JOIN && !a.bnsc) {          // a BatchNorm that no ReLU follows (bn3): every position counts
#pragma unroll
            for (int q = 0; q < 8; ++q) { bsc[q] = 0.f; bsh[q] = 1.f; }
        } else {
            const long go = a.bn_gN > 0 ? (long)(m0 / (a.bn_gN * a.Hb * a.Wb)) * a.bn_gstride : 0;
            const float* ps = a.bnsc + go + colw + ch * 8;
            const float* pb = a.bnsh + go + colw + ch * 8;
            const f32x4 s0 = *(const f32x4*)ps, s1_ = *(const f32x4*)(ps + 4), b0 = *(const f32x4*)pb, b1 = *(const f32x4*)(pb + 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) { bsc[q] = s0[q]; bsc[4 + q] = s1_[q]; bsh[q] = b0[q]; bsh[4 + q] = b1[q]; }
        }
        yrs = buffer_behind((elt_t*)a.bny + o_base, o_left);
    }
    // JOIN: the other contribution and the ReLU reference beside every stored piece (same layout as the output; a null tensor
    // reads through a zero-length resource: zeros, and "no reference" means no mask)
    __amdgpu_buffer_rsrc_t jars = ors, jrrs = ors;
    if constexpr (JOIN) {
        jars = buffer_behind(a.join_add ? (elt_t*)a.join_add + o_base : (elt_t*)a.out0, a.join_add ? o_left : 0);
        jrrs = buffer_behind(a.join_ref ? (elt_t*)a.join_ref + o_base : (elt_t*)a.out0, a.join_ref ? o_left : 0);
    }
    const bool j_mask = JOIN && a.join_ref != nullptr;
    __syncthreads();                              // every wave is done with the activation tiles the scratch aliases
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int d0 = wm * 32 * MI + 32 * i + r0;
        // The side loads do not depend on the product: all of a sub-tile's loads (up to twelve 16-byte pieces per lane) are issued
        // HERE, in front of the LDS transposition, instead of one piece at a time between the stores -- hipcc kept each load behind the
        // store before it (it cannot tell the resources apart) and every piece waited out a memory round trip of its own (16 per wave
        // and tile).  (Issued one sub-tile further ahead -- 24 pieces in flight, 256 registers -- measured the same.)
        u32x4 pb[4], pr[4], py[4];
        if constexpr (JOIN || BNS) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int d = d0 + 8 * t;
                const int vo = (m0 + d < a.M) ? (d * a.Cout + ch * 8) * 2 : OOBV;
                if constexpr (JOIN) {
                    pb[t] = __builtin_amdgcn_raw_buffer_load_b128(jars, vo, 0, 0);
                    pr[t] = __builtin_amdgcn_raw_buffer_load_b128(jrrs, vo, 0, 0);
                }
                if constexpr (BNS) py[t] = __builtin_amdgcn_raw_buffer_load_b128(yrs, vo, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 h4;
#pragma unroll
                for (int q = 0; q < 4; ++q) h4[q] = (elt_t)acc[i][j][4 * g + q];
                *(bf16x4*)(ep + l31 * EPITCH + (j * 32 + 8 * g + 4 * lh) * 2) = h4;
            }
        wave_lds_sync();
        int x = LIN ? 0 : fastmod(x0r + d0, W, invW);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = r0 + 8 * t;
            bf16x8 v8 = *(const bf16x8*)(ep + row * EPITCH + ch * 16);
            const int d = d0 + 8 * t;
            const bool ok = m0 + d < a.M;
            const int vo = LIN ? (d * a.Cout + ch * 8) * 2 : ((4 * d - 2 * x + 2 * W) * a.Cout + ch * 8) * 2;
            if constexpr (JOIN) {       // (the unfused pair rounds the product to the storage type, adds in f32 and rounds again: so does this)
                const bf16x8 b8 = __builtin_bit_cast(bf16x8, pb[t]);
                const bf16x8 r8 = __builtin_bit_cast(bf16x8, pr[t]);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float g = (float)v8[q] + (float)b8[q];
                    v8[q] = (elt_t)((!j_mask || (float)r8[q] > 0.f) ? g : 0.f);
                }
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v8), ors, ok ? vo : OOBV, 0, 0);
            if constexpr (BNS) {
                const bf16x8 y8 = __builtin_bit_cast(bf16x8, py[t]);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float yf = (float)y8[q];
                    const float dz = (ok && yf * bsc[q] + bsh[q] > 0.f) ? (float)v8[q] : 0.f;
                    st1[q] += dz; st2[q] += dz * yf;
                }
            }
            if constexpr (PLAIN && !BNS) {          // statistics see the stored values; rows past M are not counted
                if (a.stat) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) { const float f = ok ? (float)v8[q] : 0.f; st1[q] += f; st2[q] += f * f; }
                }
            }
            if (!LIN) {                             // the next piece is 8 pixels on: x advances without a division from W = 8 up
                if (W >= 8) { x += 8; x = x >= W ? x - W : x; }
                else x = fastmod(x0r + d + 8, W, invW);
            }
        }
        wave_lds_sync();
    }
    if constexpr (PLAIN || BNS) {
        if (a.stat) {       // fixed order: the lanes that hold the same channels (lane & 7), then the WM waves that share these columns
            __syncthreads();
            float* red = (float*)smem;            // [WM][2][BN]
#pragma unroll
            for (int q = 0; q < 8; ++q) {
#pragma unroll
                for (int o = 8; o < 64; o <<= 1) { st1[q] += __shfl_xor(st1[q], o); st2[q] += __shfl_xor(st2[q], o); }
                if (lane < 8) {
                    red[(wm * 2 + 0) * BN + wn * 64 + lane * 8 + q] = st1[q];
                    red[(wm * 2 + 1) * BN + wn * 64 + lane * 8 + q] = st2[q];
                }
            }
            __syncthreads();
            for (int t = tid; t < 2 * BN; t += 256) {
                const int q = t / BN, cc = t % BN;
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < WM; ++w) v += red[(w * 2 + q) * BN + cc];
                a.stat[((long)mtile * 2 + q) * a.Cout + n0 + cc] = v;
            }
        }
    }
}

// MODE 0: forward (a.src[0] = activation source, a.Cin = Cin, a.Cout = Cout, out0 = u, bias)
// MODE 1: dgrad   (a.src[0] = du [N,2H,2W,Cout] contiguous, a.Cin = Cout, a.Cout = Cin, out0 = da)
// MODE 2: a plain 1x1 convolution (round 2: the bottleneck GEMMs of DeepLabV2-ResNet, reference networks/backbone/resnet.py:
//         12-13,66,70): [M x Cin] x [Cin x Cout] with the forward's loader (producer's BatchNorm + ReLU on load), the
//         dgrad's plain epilogue, optional bias, and BatchNorm-statistics partials (one row per 128-pixel tile) of the
//         rounded outputs
// BREG: weights through registers (WeightsReg) -- no weight tile in LDS, no LDS-DMA beside the compiler-visible activation loads
// (which made hipcc drain vmcnt(0) at every chunk) -- and the waves share only the activation tile: one barrier per 64-channel chunk.
// JOIN (round 6, MODE 2 only): the 1x1 GEMM is the input gradient of a bottleneck's conv1 (DeepLabV2-ResNet backward, reference
// networks/backbone/resnet.py:87-105 under autograd) and its epilogue performs the residual join that followed it as a pass of its
// own: stored = (product + join_add) * (join_ref > 0) -- the gradient of the previous block's pre-ReLU sum -- and, with BNS, the two
// BatchNorm-backward sums of that block's bn3 (sum(g), sum(g y3): a.bnsc = 0, a.bnsh = 1 make the mask all ones) from the stored
// pieces.  7 tensor passes over the widest maps of the network become 4.
template <int BN, int BK, int MODE, bool BREG, bool BNS = false, bool JOIN = false>
__global__ __launch_bounds__(256, 2) void convT_bf16_kernel(const IgemmArgs a, const int mt_total, const int nt_total) {
    typedef ConvTGeom<BN, BK, MODE, BREG, BNS, JOIN> G;
    constexpr bool DG = MODE == 1;
    constexpr int MI = G::MI, AIT = G::AIT, ABYTES = G::ABYTES, BCH = G::BCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem, *Bs = smem + 2 * ABYTES;
    const int bid = xcd_linear(blockIdx.x, mt_total * nt_total);
    const int mtile = bid / nt_total, ntile = bid % nt_total;
    const int n0 = ntile * BN;
    const int m0 = mtile * G::BM;               // (M < 2^29: the plan checks)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: LDS-DMA bases and role tests stay scalar
    const int wm = wave / G::WN, wn = wave % G::WN, l31 = lane & 31, lh = lane >> 5;
    const int W = a.Wb, nchunk = (DG ? 4 * a.Cin : a.Cin) / BK;
    const int x0r = m0 % W;                     // x of the tile's first pixel
    const float invW = 1.f / (float)W;
    // ---- prologue: item addresses, the accumulators from the bias, chunk 0 staged ----
    ActStage<G, DG> A;
    A.init(a, tid, m0, x0r, W, invW);
    const elt_t* bcol = (const elt_t*)a.W + weight_col<MODE>(a, n0 + (tid % BN));
    const long brow = (long)a.Cout * 8;
    WeightsReg<G, MODE> Br;
    if constexpr (BREG) Br.init(a, n0 + wn * 64, l31, lh);
    f32x16 acc[MI][2];
    init_acc<G, MODE>(acc, a, smem, wave, lane, n0 + wn * 64);
    if constexpr (BREG) Br.load(0, 0); else dma_weights<G>(bcol, brow, 0, Bs, tid, wave);
    A.load(a, 0, W);
    A.write(As, tid);
    if constexpr (BREG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- loop over the K chunks: the next chunk is fetched under this chunk's MFMAs ----
    int buf = 0, prow0 = wm * 32 * MI + l31;     // prow0: this lane's A row in sub-tile 0
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const bool more = c + 1 < nchunk;
        const char* Acur = As + buf * ABYTES;
        if constexpr (BREG) {
#pragma unroll
            for (int stg = 0; stg < 2; ++stg) {
                bf16x8 bcur[2][2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) { bcur[ks][0] = Br.bnx[ks][0]; bcur[ks][1] = Br.bnx[ks][1]; }
                // top: the next stage's weights (stage 1 of this chunk, or stage 0 of the next one); behind them, in stage 0, the next
                // chunk's activation items -- so that the wait for THIS stage's weights never covers a load from HBM
                if (stg == 0) { Br.load(c, 1); if (more) A.load(a, c + 1, W); }
                else if (more) Br.load(c + 1, 0);
                __builtin_amdgcn_sched_barrier(0);
                // this stage's fragments were issued one stage ago; younger than them: stage 0: the 4 loads just issued + the AIT
                // activation loads; stage 1: the activation loads issued in stage 0 + the 4 loads just issued
                if (more) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 + AIT) : "memory");
                else if (stg == 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(bcur[ks][0]), "+v"(bcur[ks][1]));      // (no MFMA above the wait)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) mfma_step<G>(acc, Acur, prow0, 2 * (2 * stg + ks) + lh, bcur[ks][0], bcur[ks][1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            if (more) { dma_weights<G>(bcol, brow, c + 1, Bs + (buf ^ 1) * (BCH * 16), tid, wave); A.load(a, c + 1, W); }
            const char* Bp = Bs + buf * (BCH * 16) + (lh * BN + wn * 64 + l31) * 16;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks)
                mfma_step<G>(acc, Acur, prow0, 2 * ks + lh, *(const bf16x8*)(Bp + (2 * ks * BN) * 16), *(const bf16x8*)(Bp + (2 * ks * BN + 32) * 16));
        }
        if (more) A.write(As + (buf ^ 1) * ABYTES, tid);
        __syncthreads();
        buf ^= 1;
    }

    epilogue<G, MODE, BNS, JOIN>(a, acc, smem, tid, wave, mtile, n0, x0r, W, invW);
}

}  // namespace

// the launch of the build convT_plan chose (igemm_launch asks the plan)
int convT_launch_bf16(const IgemmArgs& a, const ConvTPlan& p, hipStream_t st) {
    USTRUN_CHECK(p.kind != CONVT_NONE && p.lds > 0, "convT: the plan names no build");
    if (p.join) {
        USTRUN_CHECK((a.bnsc == nullptr) == (a.bnsh == nullptr), "conv1x1_join: scale / shift come together");
        USTRUN_CHECK(!a.bny || a.stat, "conv1x1_join: BatchNorm-backward sums need their statistics rows");
    }
    if (p.kind == CONVT_DGRAD && a.bny) USTRUN_CHECK(a.stat && a.bnsc && a.bnsh && p.bns, "convT_dgrad: BatchNorm-backward sums on an unsupported shape");
    set_last_variant(p.variant);
    switch (p.key) {
#define CONVT_LAUNCH_CASE(BN, BK, MODE, BREG, BNS, JOIN) \
    case convT_key(BN, BK, MODE, BREG, BNS, JOIN): hipLaunchKernelGGL((convT_bf16_kernel<BN, BK, MODE, BREG, BNS, JOIN>), dim3(p.grid), dim3(256), p.lds, st, a, p.mt, p.nt); break;
        CONVT_BUILDS(CONVT_LAUNCH_CASE)
#undef CONVT_LAUNCH_CASE
    }
    USTRUN_LAUNCH_CHECK("convT_bf16");
    return 0;
}

}  // namespace ustrun
