/* ustrun.h -- C ABI of libustrun.so: the MI355X (gfx950) implementation of UST-RUN's
 * 2D U-Net training hot path.
 *
 * The reference has no FFI: its boundary for this path is the torch.nn.Module API of
 * networks/unet_model.py + utils/losses.py and the inline step in train.py.  Each entry point
 * below names the reference code it replaces (file:line under the reference tree).
 *
 * Conventions
 *   - every function returns 0 on success, nonzero on error; ustrun_last_error() gives the
 *     message (thread-local).  No exceptions cross the ABI, nothing is allocated or freed here,
 *     no pointer is retained after return, nothing synchronises the device: all work is
 *     enqueued on `stream` (a hipStream_t; NULL = default stream).
 *   - all pointers are DEVICE pointers unless named host_*.
 *   - activations inside the network are NHWC ("pixel-major": channels of one pixel are
 *     contiguous); the network input and the logits are NCHW as in the reference.
 *   - dtype selects the storage type of activations, activation gradients and packed weights:
 *     USTRUN_F32 (exact f32 MFMA, the parity path), USTRUN_BF16 (bf16 tensors in HBM, bf16 MFMA,
 *     f32 accumulate / BatchNorm statistics / losses / optimizer) or USTRUN_F16 (the same kernels
 *     built for IEEE half: the reference's own mixed-precision type, torch.cuda.amp autocast +
 *     GradScaler, train.py:30,54,551-552,842-845; activation GRADIENTS in half need the caller's loss
 *     scale: ustrun_seg_loss_bwd's gscale carries it in, ustrun_sgd_ema_scaled takes it out and skips
 *     the update when the scaled gradient is not finite).  `void*` activation arguments follow
 *     dtype; the network input, logits, parameters and gradients of parameters are always f32.
 *     USTRUN_F32X3: every tensor, loader and epilogue of USTRUN_F32, with the products of the 3x3 convolutions (and the
 *     ConvTranspose pair) on the BF16 matrix cores over three-term operand splits x = x0 + x1 + x2, six MFMAs per product
 *     (csrc/x3.hip): f32-level results (the north_star tolerance: 1e-4 on logits, arg-max bit-exact outside 1e-4 margins) at a
 *     multiple of the f32 matrix rate.  Its packed weights are the f32 pack followed by the three bf16 planes: 2.5x the floats.
 */
#ifndef USTRUN_H
#define USTRUN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USTRUN_VERSION 100
enum { USTRUN_F32 = 0, USTRUN_BF16 = 1, USTRUN_F16 = 2, USTRUN_F32X3 = 3 };
enum { USTRUN_LOSS_SOFTMAX = 0, USTRUN_LOSS_SIGMOID = 1 };

typedef void* ustrun_stream_t;

int ustrun_version(void);
const char* ustrun_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Activation source of an implicit-GEMM loader.  The loader evaluates, per element,
 *     a = relu?( x*scale[c] + shift[c] )   then, if pool, max over the 2x2 window,
 * and zero outside the stored extent (conv zero padding, F.pad of the up path).  This is how
 * BatchNorm+ReLU (unet_parts.py:17-18), MaxPool2d(2) (:34), F.pad (:62-63) and torch.cat (:67)
 * are folded into the consumer's loads instead of being materialised.
 * ---------------------------------------------------------------------------------------- */
typedef struct ustrun_src {
    const void*  ptr;        /* stored tensor                                              */
    const float* scale;      /* per-channel affine, NULL = identity                        */
    const float* shift;
    int32_t C, H, W;         /* stored channels / extent                                   */
    int64_t sN, sH, sW, sC;  /* element strides (NHWC: sC = 1; NCHW input: sW = 1)         */
    int32_t relu;            /* max(0, .) after the affine                                 */
    int32_t pool;            /* logical pixel (y,x) = max of stored (2y..2y+1, 2x..2x+1)   */
    int32_t off_y, off_x;    /* logical (y,x) reads stored (y-off_y, x-off_x)              */
    int32_t f32;             /* 1: this tensor is f32 even when dtype is USTRUN_BF16 (the    */
                             /*    network input); otherwise its element type follows dtype  */
    int32_t gN;              /* > 0: the batch is several independent forward passes laid end to end, gN images */
    int64_t gstride;         /*      each, with their own BatchNorm statistics: image n uses scale/shift +      */
                             /*      (n / gN) * gstride; statistics rows of a forward never mix two passes       */
} ustrun_src_t;

/* ---- weight packing (done once per optimizer step) ---------------------------------------
 * conv3x3: torch [Cout][Cin][3][3] -> fwd [9][Cin][Cout] and dgrad [9][Cout][Cin]
 * convT2x2: torch [Cin][Cout][2][2] -> fwd [4][Cin][Cout] and dgrad [4][Cout][Cin]
 * (USTRUN_F32X3: each of the two buffers holds 2.5 x that many floats -- the f32 pack, then its bf16 planes)  */
int ustrun_pack_conv3x3(const float* w, int Cout, int Cin, void* w_fwd, void* w_dgrad, int dtype, ustrun_stream_t s);
int ustrun_pack_convT2x2(const float* w, int Cin, int Cout, void* w_fwd, void* w_dgrad, int dtype, ustrun_stream_t s);

/* ---- conv3x3 (pad 1, no bias) forward: replaces nn.Conv2d at unet_parts.py:16,19 ----------
 * y[N,H,W,Cout] (raw, pre-BN) = conv(loader(srcs)), plus per-channel partial sums of y and
 * y*y per M-tile for the train-mode BatchNorm that follows: stat[mtile][2][Cout] (NULL = skip).
 * ustrun_conv_mtiles gives the number of M-tiles the launch will use.                        */
int ustrun_conv_mtiles(int N, int H, int W, int Cout);
int ustrun_conv3x3_fwd(const ustrun_src_t* srcs, int nsrc, const void* w_fwd, int N, int H, int W,
                       int Cout, void* y, float* stat, int dtype, ustrun_stream_t s);
/* Same launch, but reports in *stat_rows how many rows of stat it wrote (<= ustrun_conv_mtiles) instead of
 * zero-filling the rest: pass that count to ustrun_bn_finalize and no memset is enqueued.            */
int ustrun_conv3x3_fwd_rows(const ustrun_src_t* srcs, int nsrc, const void* w_fwd, int N, int H, int W,
                            int Cout, void* y, float* stat, int* stat_rows, int dtype, ustrun_stream_t s);

/* ---- train-mode BatchNorm statistics: replaces nn.BatchNorm2d at unet_parts.py:17,20 -------
 * Reduces stat[mtiles][2][C] (fixed order, f64) to batch mean / biased variance, writes
 * scale = gamma*rstd, shift = beta - mean*scale (consumed by the next loader), mean, rstd
 * (kept for backward), and updates running_mean/var (unbiased var, momentum) and
 * num_batches_tracked when update_running != 0.  eval mode: ustrun_bn_eval_affine.           */
int ustrun_bn_finalize(float* stat /* scratch: may be overwritten */, int mtiles, int C, int64_t count, const float* gamma,
                       const float* beta, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, float momentum, float eps, int update_running,
                       float* scale, float* shift, float* mean, float* rstd, ustrun_stream_t s);
int ustrun_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, float* scale, float* shift,
                          ustrun_stream_t s);
/* eval mode with the constants the backward through frozen statistics reads: aff[4][C] = {scale, shift, running_mean, rstd},
 * rstd = 1 / sqrt(running_var + eps), scale / shift bit-identical to ustrun_bn_eval_affine (nn.BatchNorm2d in eval mode,
 * unet_parts.py:17,20 under model.eval())                                                                              */
int ustrun_bn_eval_consts(int C, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, float* aff, ustrun_stream_t s);
/* materialise a = relu(y*scale+shift) as NHWC or NCHW f32 (block-level API and feature=True) */
int ustrun_bn_relu_apply(const void* y, const float* scale, const float* shift, int64_t npix, int C,
                         int HW, float* out, int out_nchw, int dtype, ustrun_stream_t s);
/* materialise the Down block's pooled input: out[N,H/2,W/2,C] = MaxPool2d(2)(relu(src*scale+shift)) in the storage
 * dtype (replaces nn.MaxPool2d at unet_parts.py:34 together with the producer's BatchNorm+ReLU); src is a plain
 * contiguous NHWC activation, its pass groups are honoured                                                     */
/* a[N,H,W,C] = relu(src*scale+shift) in the 16-bit storage dtype (src: plain contiguous NHWC with its BatchNorm constants, pass
 * groups honoured): the input of a DoubleConv's second convolution (unet_parts.py:16-21) written out once, for the layers where
 * that costs less than applying BatchNorm + ReLU per staged item in the convolution AND its weight gradient                */
int ustrun_act16(const ustrun_src_t* src, int N, void* out, int dtype, ustrun_stream_t s);
int ustrun_pool_act(const ustrun_src_t* src, int N, void* out, int dtype, ustrun_stream_t s);
/* the same pass, also writing the un-pooled activation act[N,H,W,C] = relu(src*scale+shift) in the storage dtype (act may be
 * NULL: then exactly ustrun_pool_act): the encoder output that unet_model.py:33-36 hands to the decoder as the skip operand of
 * torch.cat (unet_parts.py:66) -- the concat convolution and its weight gradient then read a plain tensor instead of applying
 * BatchNorm + ReLU per staged item; 16-bit storage and even H, W only                                                     */
int ustrun_pool_act2(const ustrun_src_t* src, int N, void* out, void* act, int dtype, ustrun_stream_t s);
/* plain MaxPool2d(2) backward on NHWC tensors (stand-alone Down block): dx[N,H,W,C] from dp[N,H/2,W/2,C] and the
 * pooled input x; first maximum of the window wins (torch's rule)                                              */
int ustrun_maxpool_bwd(const void* dp, const void* x, int N, int H, int W, int C, void* dx, int dtype,
                       ustrun_stream_t s);

/* ---- ConvTranspose2d(k=2,s=2,bias): replaces unet_parts.py:53 ------------------------------
 * u[N,2H,2W,Cout] = convT(loader(src)) + bias.                                              */
int ustrun_convT2x2_fwd(const ustrun_src_t* src, const void* w_fwd, const float* bias, int N, int H,
                        int W, int Cout, void* u, int dtype, ustrun_stream_t s);

/* ---- input gradient of the first convolution (Conv2d(C, base, 3, padding=1, bias=False), unet_parts.py:16) ----
 * dx[N,Cin,H,W] NCHW f32 (overwritten) from dy[N,H,W,Cout] in the storage dtype and the f32 PARAMETER w[Cout,Cin,3,3].
 * Cin 1..4, Cout a multiple of 8 up to 64, any H, W >= 1.  Products of the stored values, f32 accumulation in a fixed
 * order (bit-identical repeats); USTRUN_F32X3 runs the f32 build.                                                     */
int ustrun_conv_first_dgrad(const void* dy, const float* w, int N, int H, int W, int Cout, int Cin, float* dx,
                            int dtype, ustrun_stream_t s);

/* ---- input gradient of the ResNet stem (Conv2d(3, 64, 7, stride=2, padding=3, bias=False), resnet.py:124,160) ----
 * dx[N,Cin,H,W] NCHW f32 (overwritten) from dy[N,Ho,Wo,Cout] in the storage dtype, Ho = (H-1)/2+1, Wo = (W-1)/2+1, and
 * the f32 PARAMETER w[Cout,Cin,7,7] (no pack).  Cin 3, Cout a multiple of 8 up to 64, any H, W >= 1.  Products of the
 * stored values, f32 accumulation in a fixed order (bit-identical repeats); USTRUN_F32X3 runs the f32 build.           */
int ustrun_conv_stem_dgrad(const void* dy, const float* w, int N, int H, int W, int Cout, int Cin, float* dx,
                           int dtype, ustrun_stream_t s);

/* ---- 1x1 head with bias: replaces OutConv, unet_parts.py:71-76 -----------------------------
 * logits NCHW f32 [N,K,H,W] from y[N,H,W,C] through the loader affine (scale/shift/relu).    */
int ustrun_head_fwd(const void* y, const float* scale, const float* shift, int64_t npix, int HW,
                    int C, int K, const float* w, const float* bias, float* logits, int dtype,
                    ustrun_stream_t s);
/* backward: da[N,H,W,C] (grad wrt the activated input), dw[K][C], db[K] (accumulate != 0 adds) */
int ustrun_head_bwd(const float* dlogits, const void* y, const float* scale, const float* shift,
                    int64_t npix, int HW, int C, int K, const float* w, void* da, float* dw, float* db,
                    int accumulate, float* partials, int64_t partials_bytes, int dtype, ustrun_stream_t s);

/* ---- BatchNorm+ReLU (+MaxPool) backward: autograd of unet_parts.py:17-18,34 ------------------
 * Inputs: da (grad wrt the activated output, may be NULL), dp (grad wrt the 2x2-pooled
 * activated output, may be NULL; routed to the window arg-max recomputed from y), y and the
 * forward scale/shift/mean/rstd.  A dp with H < 2 or W < 2 (a pooled map without elements) is
 * refused by every pass, as ustrun_bn_bwd_frozen refuses it.  Pass 1 (reduce) produces dgamma/dbeta and the coefficient
 * table coef[3][C]; pass 2 (apply) writes dy = coef0*dz + coef1*y + coef2, dz = da_total*(a>0). */
int64_t ustrun_bn_bwd_partials_bytes(int64_t npix, int C);
int ustrun_bn_bwd_reduce(const void* da, const void* dp, const void* y, const float* scale,
                         const float* shift, const float* mean, const float* rstd, const float* gamma,
                         int N, int H, int W, int C, float* dgamma, float* dbeta, int accumulate,
                         float* coef, float* partials, int64_t partials_bytes, int dtype, ustrun_stream_t s);
int ustrun_bn_bwd_apply(const void* da, const void* dp, const void* y, const float* scale,
                        const float* shift, const float* coef, int N, int H, int W, int C, void* dy,
                        int dtype, ustrun_stream_t s);
/* The same pass (plain, 16-bit storage, C / 8 a power of two <= 256) for the layer under the classification head when the head's
 * input gradient was not stored: da[p][c] = sum_k dlogits[k][p] head_w[k][c] is formed again per pixel, rounded to the storage type as
 * ustrun_head_bwd stores it, and applied.  dlogits [passes][N][K][H][W] f32, head_w [K][C]; y / dy hold `passes` passes of N images,
 * scale / shift `aff_stride` floats apart per pass, coef [passes][3][C].  Bit-identical to ustrun_head_bwd + ustrun_bn_bwd_apply.    */
int ustrun_bn_bwd_apply_head(const float* dlogits, const float* head_w, const void* y, const float* scale, const float* shift,
                             const float* coef, int N, int H, int W, int C, int K, void* dy, int dtype, int passes,
                             int64_t aff_stride, ustrun_stream_t s);

/* ---- BatchNorm+ReLU (+MaxPool) backward through FROZEN statistics: autograd of unet_parts.py:17-18,34 under model.eval(),
 * where nn.BatchNorm2d normalises with its running buffers (networks/unet_model.py:25-39 is an ordinary autograd module in eval
 * mode too).  With scale = gamma rstd, rstd = 1 / sqrt(running_var + eps), shift = beta - running_mean scale:
 *   g = (da [+ dp routed to the window's first arg-max]) [y scale + shift > 0],  dy = scale g,
 *   dbeta = sum g,  dgamma = rstd sum g (y - running_mean)   (mean = running_mean).
 * dy does not depend on the sums, so ONE pass reads da, dp and y once each, writes dy (dy == da, in place, is allowed) and
 * leaves per-block rows {sum g, sum g y} in `partials` (ustrun_bn_bwd_partials_bytes); a finalize adds the rows in a fixed order
 * in f64.  No atomics: a repeated call is bit-identical.  accumulate != 0 adds to dgamma / dbeta.  dgamma == dbeta == NULL
 * (frozen parameters): a pure apply pass -- no rows, no finalize, mean / rstd / partials unused and untouched.  No running
 * buffer and no num_batches_tracked is written.  da may be NULL when dp is given; dp != NULL selects the 2x2 pooled windows
 * (odd H / W included).  C a multiple of 4; USTRUN_F32X3 stores f32.                                                      */
int ustrun_bn_bwd_frozen(const void* da, const void* dp, const void* y, const float* scale, const float* shift,
                         const float* mean, const float* rstd, int N, int H, int W, int C, void* dy, float* dgamma,
                         float* dbeta, int accumulate, float* partials, int64_t partials_bytes, int dtype, ustrun_stream_t s);
/* the per-pass form: da / y / dy hold `passes` passes of N images each (dp: of N pooled images), pass g takes its constants at
 * scale / shift / mean / rstd + g * aff_stride floats; dgamma / dbeta receive the passes' contributions one after the other, as
 * `passes` calls of ustrun_bn_bwd_frozen with accumulate would add them                                                   */
int ustrun_bn_bwd_frozen_passes(const void* da, const void* dp, const void* y, const float* scale, const float* shift,
                                const float* mean, const float* rstd, int N, int H, int W, int C, void* dy, float* dgamma,
                                float* dbeta, int accumulate, float* partials, int64_t partials_bytes, int dtype, int passes,
                                int64_t aff_stride, ustrun_stream_t s);

/* ---- conv3x3 input gradient (autograd of unet_parts.py:16,19) ------------------------------
 * da = conv3x3(dy, flipped/transposed w).  Channels [0,C0) go to da0[N,H,W,C0]; channels
 * [C0,Cin) go to da1[N,H1,W1,Cin-C0] at pixel (y-o1y, x-o1x) (the cat/pad split of the up path). */
int ustrun_conv3x3_dgrad(const void* dy, const void* w_dgrad, int N, int H, int W, int Cout, int Cin,
                         void* da0, int C0, void* da1, int H1, int W1, int o1y, int o1x, int dtype,
                         ustrun_stream_t s);
/* the same input gradient (single destination) which ALSO forms the BatchNorm-backward sums of the layer whose da it writes
 * (unet_parts.py:17-21 backward: the BatchNorm2d + ReLU between the two convolutions of a DoubleConv): y = that layer's
 * pre-BatchNorm output [N,H,W,Cin] (the layout of da), scale / shift = its forward constants (gN images per pass, gstride floats
 * between the passes' constants; gN = 0: one pass); stat receives *stat_rows rows of [2][Cin] = {sum(da mask), sum(da mask y)},
 * mask = y scale + shift > 0, over the da values as stored -- what ustrun_bn_bwd_reduce would form from a second read of both
 * tensors; ustrun_bn_bwd_finalize_stat turns the rows into dgamma / dbeta / coefficients.  *stat_rows = 0 and NO launch when
 * the shape is not one the fused epilogue covers (16-bit storage, >= 128 input channels, the 256-pixel tiles): the caller then
 * runs ustrun_conv3x3_dgrad and ustrun_bn_bwd_reduce.  stat: ustrun_conv_mtiles(N, H, W, Cin) rows. */
int ustrun_conv3x3_dgrad_bnsum(const void* dy, const void* w_dgrad, int N, int H, int W, int Cout, int Cin, void* da,
                               const void* y, const float* scale, const float* shift, int gN, int64_t gstride,
                               float* stat, int* stat_rows, int dtype, ustrun_stream_t s);
/* rows of ustrun_conv3x3_dgrad_bnsum (rows_per_pass x passes rows of [2][C], pass after pass) -> dgamma, dbeta (the passes'
 * contributions added in order; accumulate != 0 adds to what is there) and coef[pass][3][C] for ustrun_bn_bwd_apply; the table
 * is reduced in place (it is scratch afterwards)                                                                          */
int ustrun_bn_bwd_finalize_stat(float* stat, int rows_per_pass, int passes, int C, int64_t count, const float* gamma,
                                const float* mean, const float* rstd, int64_t aff_stride, float* dgamma, float* dbeta,
                                int accumulate, float* coef, ustrun_stream_t s);
/* ---- conv3x3 weight gradient: dw[Cout][Cin][3][3] (torch layout, f32) ---------------------- */
int64_t ustrun_wgrad_partials_bytes(int nseg, int Cin, int Cout, int64_t npix);
/* The first convolution's weight gradient (NCHW f32 source of C <= 3 channels -> 64, 16-bit storage, the streaming kernel's
 * shapes; anything else is an error) with the layer's BatchNorm-backward apply pass on load: dY = ustrun_bn_bwd_apply(da, y) is formed
 * piece by piece in the kernel's loader and never stored.  Image n takes the constants of pass n / gN (gN = 0: one pass): scale /
 * shift + pass * aff_stride floats, coef + pass * 3 * 64.  partials as for ustrun_conv3x3_wgrad (ustrun_wgrad_partials_bytes(9, C, 64,
 * N H W)).  Bit-identical to ustrun_bn_bwd_apply + ustrun_conv3x3_wgrad.                                                          */
int ustrun_conv_first_wgrad_bn(const ustrun_src_t* src, const void* da, const void* y, const float* scale, const float* shift,
                               const float* coef, int gN, int64_t aff_stride, int N, int H, int W, int Cout, float* dw,
                               int accumulate, float* partials, int64_t partials_bytes, int dtype, ustrun_stream_t s);
int ustrun_conv3x3_wgrad(const ustrun_src_t* srcs, int nsrc, const void* dy, int N, int H, int W,
                         int Cout, float* dw, int accumulate, float* partials, int64_t partials_bytes,
                         int dtype, ustrun_stream_t s);
/* ---- ConvTranspose2d backward --------------------------------------------------------------- */
int ustrun_convT2x2_dgrad(const void* du, const void* w_dgrad, int N, int H, int W, int Cout, int Cin,
                          void* da, int dtype, ustrun_stream_t s);
/* the same, also forming the BatchNorm-backward sums of the layer whose da it writes -- the conv2 under this ConvTranspose
 * (unet_parts.py:56-68 backward into unet_parts.py:17-21): arguments and rows as ustrun_conv3x3_dgrad_bnsum, one row per 128
 * pixels; *stat_rows = 0 and no launch on a shape the fused epilogue does not cover                                       */
int ustrun_convT2x2_dgrad_bnsum(const void* du, const void* w_dgrad, int N, int H, int W, int Cout, int Cin, void* da,
                                const void* y, const float* scale, const float* shift, int gN, int64_t gstride,
                                float* stat, int* stat_rows, int dtype, ustrun_stream_t s);
int ustrun_convT2x2_wgrad(const ustrun_src_t* src, const void* du, int N, int H, int W, int Cout,
                          float* dw, float* db, int accumulate, float* partials, int64_t partials_bytes,
                          int dtype, ustrun_stream_t s);

/* ---- bilinear Up block: nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True), unet_parts.py:48-50 ----
 * x[N,H,W,C] -> y[N,2H,2W,C] (NHWC f32, C % 4 == 0); _bwd is its exact adjoint (dy -> dx), fixed summation order. */
int ustrun_upsample2x_fwd(const float* x, int N, int H, int W, int C, float* y, ustrun_stream_t s);
int ustrun_upsample2x_bwd(const float* dy, int N, int H, int W, int C, float* dx, ustrun_stream_t s);
/* the same two passes in a plan's storage dtype (the fused U-Net with bilinear = 1): the forward reads a plain contiguous NHWC
 * source through its BatchNorm constants + ReLU (pass groups honoured) and stores the interpolated activation; the backward is the
 * adjoint over dy [N,2H,2W,C] -> dx [N,H,W,C]                                                                                   */
int ustrun_upsample2x_act(const ustrun_src_t* src, int N, void* out, int dtype, ustrun_stream_t s);
int ustrun_upsample2x_bwd_t(const void* dy, int N, int H, int W, int C, void* dx, int dtype, ustrun_stream_t s);

/* ---- pseudo-labels: replaces train.py:648-667 (teacher) and :669-674 (student) ---------------
 * softmax: conf,label = max(softmax(logits,1),1); mask = conf > th   (label int64, mask f32)
 * sigmoid: label = (p >= .5); mask = (p >= th) + (p <= 1-th)          (both f32 [N,K,H,W])   */
int ustrun_pseudo_label(const float* logits, int N, int K, int HW, float threshold, int mode,
                        void* label, float* mask, ustrun_stream_t s);

/* ---- ensemble/CutMix target algebra: replaces train.py:677-697 -------------------------------
 * box[N,HW] in {0,1}; cut_label/cut_mask are already gathered by `choice`.                    */
int ustrun_mix_targets(int mode, int N, int K, int HW, const float* box, const void* pl,
                       const float* mask, const void* pl_w_ul, const float* mask_w_ul,
                       const void* pl_w_lu, const float* mask_w_lu, const void* cut_label,
                       const float* cut_mask, void* pl_w, float* mask_w, void* pl_ul, float* mask_ul,
                       void* pl_lu, float* mask_lu, ustrun_stream_t s);
/* CutMix rectangles -> {0,1} maps on the device: box[n,y,x] = (y0<=y<y1 && x0<=x<x1).  Replaces the host-built
 * maps of train.py:222-251 (cutmix_box, all_cover_box) that the reference uploads with .cuda(): only the N x 4 corner
 * ints {y0,y1,x0,x1} (HOST pointer) travel, inside the launch's argument block.                 */
#define USTRUN_MAX_RECTS 64
int ustrun_rect_masks(const int32_t* rects_host, int N, int H, int W, float* box, ustrun_stream_t s);
/* Stream-ordered upload of a few host bytes (indices, ratios) through the launch's argument block; replaces the
 * small torch.tensor(...).cuda() uploads of train.py:612-636,749-782.                          */
#define USTRUN_UPLOAD_MAX 2048
int ustrun_upload_small(void* dst, const void* src_host, int nbytes, ustrun_stream_t s);
/* CutMix image compositing out = a*(1-box) + b*box on NCHW images: train.py:644-646,688,691   */
int ustrun_box_mix(const float* a, const float* b, const float* box, int N, int C, int HW,
                   float* out, ustrun_stream_t s);
/* One launch that ASSEMBLES a batch from rows that live anywhere on the device: out row r (row_bytes bytes each, a multiple of
 * 16; every pointer 16-byte aligned) = a byte copy of rows[r].a when rows[r].b is NULL, else the CutMix composite of f32 rows
 * a*(1-box) + b*box with box[HW] broadcast over the row's channels (the arithmetic of ustrun_box_mix).  The row table is a HOST
 * array (device ADDRESSES computed by the caller: base + index * stride) and travels in the launch's argument block.  Replaces
 * the reference's fancy indexing / torch.cat / clone chains around its forward calls: cut_img[choice], cut_label[choice],
 * cut_mask[choice] (train.py:627,690-697), the three teacher inputs (:643-647), the student's inputs (:689-702,734), the
 * memory bank's torch.cat (:764-780) -- without materialising the concatenations or the index tensors.              */
typedef struct ustrun_asm_row { const void* a; const void* b; const float* box; } ustrun_asm_row_t;
#define USTRUN_ASM_MAX 128
int ustrun_assemble(const ustrun_asm_row_t* rows_host, int nrows, int64_t row_bytes, int HW, void* out, ustrun_stream_t s);
/* Label decoding of the loop head, one pass: train.py:590-608 / train_mnms.py:549-556.  y: the loader's f32 label tensor.
 * kind 0 (fundus):   y [N,HW]   -> out f32 [N,2,HW] = {y == 0, y <= 128}
 * kind 1 (prostate): y [N,HW]   -> out i64 [N,HW]   = (y == 0)
 * kind 2 (BUSI):     y [N,HW]   -> out i64 [N,HW]   = (y == 255)
 * kind 3 (MNMS):     y [N,HW,3] -> out i64 [N,HW]   = 3 if y[..,2]==255 else 2 if y[..,1]==255 else 1 if y[..,0]==255 else 0 */
int ustrun_decode_labels(const float* y, int kind, int N, int HW, void* out, ustrun_stream_t s);
/* Bounding rectangle of the union of up to four planes' non-zero pixels (train.py:722-730 + obtain_all_cover_box :242-251: the
 * low-quality sample's region = its pseudo-label planes united with the picked labelled sample's mask planes): plane k is
 * f32 or i64 (is_i64 bit k) of H*W elements; partial[USTRUN_BBOX_BLOCKS][4] int32 = per-block {min y, max y, min x, max x}
 * ({H, -1, W, -1} for a block that saw none) -- 1 KB that the host copies and folds: the 256 KB region map never exists.  */
#define USTRUN_BBOX_BLOCKS 64
int ustrun_region_bbox(const void* const* planes_host, int nplanes, int is_i64_bits, int H, int W, int32_t* partial,
                       ustrun_stream_t s);

/* ---- FFT low-frequency amplitude mix: replaces train.py:158-207,628-636 (numpy on the host) --------
 * src/trg/out are normalised NCHW images (k/127.5-1); per image n the (2b+1)^2 window of src's
 * fft-shifted amplitude is blended towards trg's with ratio ratios[n] (device array), phase kept;
 * out = clip(result,0,255)/127.5-1.  b = floor(min(H,W)*L).                                       */
int64_t ustrun_freq_mix_work_bytes(int n, int C, int b);
int ustrun_freq_mix(const float* src, const float* trg, const float* ratios, int n, int C, int H, int W,
                    int b, float* out, void* work, int64_t work_bytes, ustrun_stream_t s);

/* ---- loss term ce + dice: replaces train.py:816-817,829-836 with utils/losses.py:236-268 -----
 * softmax mode: target int64 [N,HW], mask f32 [N,HW] or NULL;  CE(reduction none)*mask, mean over
 *   all pixels (Q5) + per-class masked Dice with the class-0 mask all ones (Q4).
 * sigmoid mode: target/mask f32 [N,K,HW];  BCE-with-logits*mask mean + ONE global masked Dice.
 * fwd writes out[0]=ce, out[1]=dice, out[2..] = the reduced sums the backward needs
 * (USTRUN_LOSS_NSUMS(K) floats in all).  bwd writes
 *   dlogits = gscale * (ce_weight*g[0] * dce/dlogits + dice_weight*g[1] * ddice/dlogits),
 * g = gscale_dev (two device floats: upstream grads of ce and dice) or {1,1} when NULL.          */
#define USTRUN_LOSS_NSUMS(K) (4 + 3 * (K))
int64_t ustrun_loss_partials_bytes(int N, int K, int HW);
int ustrun_seg_loss_fwd(const float* logits, const void* target, const float* mask, int N, int K,
                        int HW, int mode, float* out, float* partials, int64_t partials_bytes,
                        ustrun_stream_t s);
int ustrun_seg_loss_bwd(const float* logits, const void* target, const float* mask, int N, int K,
                        int HW, int mode, const float* sums, const float* gscale_dev, float gscale,
                        float ce_weight, float dice_weight, float* dlogits, ustrun_stream_t s);

/* ---- DiceLossWithMask.forward in every mode combination of utils/losses.py:236-268 (the two the step uses run fused with
 * their CE / BCE terms in ustrun_seg_loss_*; this pair serves the rest of the signature: class weights, sigmoid per class,
 * softmax + multi, raw inputs).  act: 0 none, 1 softmax over classes, 2 sigmoid.  multi = 0: per-class Dice on the one-hot of a
 * class-index target [N,HW] (int64 or f32: target_is_i64), mask f32 [N,HW] or NULL encoded as the reference does (class 0:
 * all ones, class k >= 1: mask == 1 -- Q4), mean over classes of weight[k] * dice_k (weight_host: K host floats or NULL = 1).
 * multi = 1: ONE Dice over all of [N,K,HW]; target / mask f32 [N,K,HW], or [N,HW] broadcast over the classes when
 * target_per_pixel / mask_per_pixel is set.  fwd: out[0] = loss, out[1..3K] = the sums the backward needs (1 + 3K floats);
 * partials as ustrun_loss_partials_bytes.  bwd: dlogits = gscale * gscale_dev[0] * dloss/dlogits.                     */
int ustrun_dice_fwd(const float* logits, const void* target, int target_is_i64, int target_per_pixel, const float* mask,
                    int mask_per_pixel, int N, int K, int HW, int act, int multi, const float* weight_host, float* out,
                    float* partials, int64_t partials_bytes, ustrun_stream_t s);
int ustrun_dice_bwd(const float* logits, const void* target, int target_is_i64, int target_per_pixel, const float* mask,
                    int mask_per_pixel, int N, int K, int HW, int act, int multi, const float* weight_host, const float* sums,
                    const float* gscale_dev, float gscale, float* dlogits, ustrun_stream_t s);

/* ... the same pair with the Dice smoothing term as an argument (ustrun_dice_* hard-wire DiceLossWithMask's 1e-10): DiceLoss of
 * utils/losses.py:156-192 is the per-class form with smooth = 1e-5, no mask.                                            */
int ustrun_dice_smooth_fwd(const float* logits, const void* target, int target_is_i64, int target_per_pixel, const float* mask,
                           int mask_per_pixel, int N, int K, int HW, int act, int multi, const float* weight_host, float smooth,
                           float* out, float* partials, int64_t partials_bytes, ustrun_stream_t s);
int ustrun_dice_smooth_bwd(const float* logits, const void* target, int target_is_i64, int target_per_pixel, const float* mask,
                           int mask_per_pixel, int N, int K, int HW, int act, int multi, const float* weight_host, float smooth,
                           const float* sums, const float* gscale_dev, float gscale, float* dlogits, ustrun_stream_t s);

/* ---- the semi-supervised loss toolkit of utils/losses.py (csrc/consistency.hip) ------------------------------------------
 * Operands are f32 NCHW [N,K,HW], K = 1..8; softmax / sigmoid run across the K planes of a pixel.  A lane takes four consecutive
 * pixels with 16-byte accesses when HW % 4 == 0 and every pointer is 16-byte aligned, one pixel otherwise (same arithmetic).
 * Scalar results are device floats; reductions are block partial rows (partials: ustrun_loss_partials_bytes) added in a fixed
 * order in double by one block, no floating-point atomics: a repeated call is bit-identical.  Every backward takes the upstream
 * gradient as a DEVICE pointer (gout_dev: one float for a scalar result, the map for a map result) and recomputes the
 * probabilities from its inputs.
 *
 * Pair consistency between two logit tensors a, b (act: USTRUN_LOSS_SOFTMAX / USTRUN_LOSS_SIGMOID; pa, pb the probabilities):
 *   USTRUN_CONS_MSE_MAP   out[N,K,HW] = (pa - pb)^2                                        softmax_mse_loss, losses.py:65-82
 *   USTRUN_CONS_KL_MEAN   out[0] = mean over N*K*HW of pb (log pb - log pa), both logs from the log-softmax / log-sigmoid of the
 *                         logits (a term is 0 where pb is 0)                                softmax_kl_loss, losses.py:85-104
 *   USTRUN_CONS_SOFT_DICE out[0] = mean_k 1 - (2 sum pa_k pb_k + 1e-5) / (sum pa_k + sum pb_k + 1e-5), the sums NOT squared
 *                         (dice_loss1)                                                      softmax_dice_loss, losses.py:39-56
 * Scalar kinds: out holds USTRUN_CONS_NOUT floats (out[0] the loss, behind it the per-class sums the backward reads as `sums`).
 * bwd writes da and / or db (NULL skips a side), each through its own softmax / sigmoid Jacobian.                       */
enum { USTRUN_CONS_MSE_MAP = 0, USTRUN_CONS_KL_MEAN = 1, USTRUN_CONS_SOFT_DICE = 2 };
#define USTRUN_CONS_NOUT 25
int ustrun_consistency_fwd(const float* a, const float* b, int N, int K, int HW, int act, int kind, float* out, float* partials,
                           int64_t partials_bytes, ustrun_stream_t s);
int ustrun_consistency_bwd(const float* a, const float* b, int N, int K, int HW, int act, int kind, const float* sums,
                           const float* gout_dev, float* da, float* db, ustrun_stream_t s);

/* Entropy of a probability map p [N,K,HW]: e = -factor sum_k p_k log(p_k + 1e-6) per pixel (factor 1: entropy_minmization /
 * entropy_map, losses.py:271-281; factor 1/ln C: entropy_loss / entropy_loss_map, :30-36,59-62).  mean = 0: out is the map
 * [N,1,HW], gout_dev a map of that shape; mean = 1: out[0] is the mean over N*HW.
 * bwd: dp_k = -(log(p_k + 1e-6) + p_k / (p_k + 1e-6)) * factor * upstream.                                             */
int ustrun_entropy_fwd(const float* p, int N, int K, int HW, float factor, int mean, float* out, float* partials,
                       int64_t partials_bytes, ustrun_stream_t s);
int ustrun_entropy_bwd(const float* p, int N, int K, int HW, float factor, int mean, const float* gout_dev, float* dp,
                       ustrun_stream_t s);

/* FocalLoss.forward (losses.py:130-153): logits [N,K,HW], target int64 [N,HW]; per pixel -(1 - pt)^gamma alpha_t log pt with pt
 * the softmax probability of the target class, alpha_host = K host floats or NULL (no alpha); out[0] = the mean (mean = 1) or
 * the sum over N*HW.  A target outside [0,K) contributes nothing.
 * The reference DETACHES pt inside the modulating factor (losses.py:141: Variable(logpt.data.exp())), so bwd writes
 *   dlogits_k = (1 - pt)^gamma alpha_t (p_k - [k = t]) * upstream (/ N*HW for the mean)
 * with no derivative of (1 - pt)^gamma.  That is the reference's gradient, kept on purpose.                             */
int ustrun_focal_fwd(const float* logits, const int64_t* target, int N, int K, int HW, float gamma, const float* alpha_host,
                     int mean, float* out, float* partials, int64_t partials_bytes, ustrun_stream_t s);
int ustrun_focal_bwd(const float* logits, const int64_t* target, int N, int K, int HW, float gamma, const float* alpha_host,
                     int mean, const float* gout_dev, float* dlogits, ustrun_stream_t s);

/* Six sums over two flat f32 arrays of n elements in one pass, and the three scalar losses built on them:
 *   out[0..5] = sum ab, sum a^2, sum b^2, sum a, sum b, sum (a-b)^2
 *   out[6] = 1 - (2 sum ab + 1e-5) / (sum a^2 + sum b^2 + 1e-5)     dice_loss, losses.py:8-16        (USTRUN_PAIR_DICE_SQ)
 *   out[7] = 1 - (2 sum ab + 1e-5) / (sum a + sum b + 1e-5)         dice_loss1, losses.py:19-27      (USTRUN_PAIR_DICE)
 *   out[8] = sum (a-b)^2 / n                                        symmetric_mse_loss, :107-116     (USTRUN_PAIR_MSE)
 * (USTRUN_PAIR_NOUT floats).  bwd: the gradient of loss `kind` times gout_dev[0] into da and / or db (NULL skips a side).  */
enum { USTRUN_PAIR_DICE_SQ = 0, USTRUN_PAIR_DICE = 1, USTRUN_PAIR_MSE = 2 };
#define USTRUN_PAIR_NOUT 9
int ustrun_pair_sums(const float* a, const float* b, int64_t n, float* out, float* partials, int64_t partials_bytes,
                     ustrun_stream_t s);
int ustrun_pair_sums_bwd(const float* a, const float* b, int64_t n, int kind, const float* sums, const float* gout_dev,
                         float* da, float* db, ustrun_stream_t s);

/* compute_kl_loss (losses.py:284-295) on a, b viewed as [rows, C] with the softmax over the C contiguous values of a row, any C:
 * out[0] = (mean pb (log pb - log pa) + mean pa (log pa - log pb)) / 2, the means over rows*C.  One lane per row: not a hot path. */
int ustrun_row_kl_fwd(const float* a, const float* b, int64_t rows, int C, float* out, float* partials, int64_t partials_bytes,
                      ustrun_stream_t s);
int ustrun_row_kl_bwd(const float* a, const float* b, int64_t rows, int C, const float* gout_dev, float* da, float* db,
                      ustrun_stream_t s);

/* ---- label-map losses and metrics (csrc/labelmap.hip) -----------------------------------------------------------------------
 * Class-weighted cross-entropy of f32 logits [N,K,HW], K = 1..USTRUN_CE_MAP_KMAX, against an int64 label map [N,HW]: replaces
 * cross_entropy2d of utils/metrics.py:93-111 and of dataloaders/utils.py:128-144.  weight_dev: K device floats or NULL (ones).
 * A pixel is ignored if has_ignore and t == ignore_index, or if ignore_negative and t < 0; a target that is not ignored and lies
 * outside [0,K) contributes nothing and is counted.  One pass over the planes with an online log-sum-exp; four pixels per lane
 * with 16-byte accesses when HW % 4 == 0 and every pointer is 16-byte aligned, one pixel otherwise (same arithmetic).
 *   out[0] = scale * S (/ out[2] if by_weight) (/ out[3] if by_count),  out[1] = S = sum w[t] (lse - x_t),  out[2] = sum w[t],
 *   out[3] = valid pixels,  out[4] = out-of-range targets;  lse[N,HW] = the log-sum-exp of every pixel (NULL skips it).
 * No valid pixel: nan with either divisor, 0 without.  partials as ustrun_loss_partials_bytes; a repeated call is bit-identical.
 * bwd: dlogits[n,k,hw] = gout_dev[0] * coef * w[t] * (exp(x_k - lse) - [k == t]) on valid pixels and exactly 0 elsewhere, coef
 * from scale, the two flags and fwd_out (the forward's out, read on the device); lse is the forward's map.               */
#define USTRUN_CE_MAP_NOUT 5
#define USTRUN_CE_MAP_KMAX 256
int ustrun_ce_map_fwd(const float* logits, const int64_t* target, const float* weight_dev, int N, int K, int HW, int has_ignore,
                      int64_t ignore_index, int ignore_negative, float scale, int by_weight, int by_count, float* out, float* lse,
                      float* partials, int64_t partials_bytes, ustrun_stream_t s);
int ustrun_ce_map_bwd(const float* logits, const int64_t* target, const float* weight_dev, const float* lse, int N, int K, int HW,
                      int has_ignore, int64_t ignore_index, int ignore_negative, float scale, int by_weight, int by_count,
                      const float* fwd_out, const float* gout_dev, float* dlogits, ustrun_stream_t s);

/* Confusion matrices of two label maps [N,HW] (int64 or f32 class indices, as ustrun_dice_counts takes them), K = 1..
 * USTRUN_CONFUSION_KMAX, HW < 2^31: counts[n][g][p] (int32, row = gt, column = pred); skipped[n] = pixels whose gt equals
 * ignore_index (has_ignore) or where either label is outside [0,K) (an f32 label that is no integer counts as outside).  Both
 * outputs are zeroed by the call; integer atomics only, so the result does not depend on scheduling.  The counts carry get_iou
 * and get_dice of dataloaders/utils.py:150-188 and cal_dice of utils/metrics.py:13-24 with no other pass over the maps.  */
#define USTRUN_CONFUSION_KMAX 32
int ustrun_confusion(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N, int K, int64_t HW, int has_ignore,
                     int64_t ignore_index, int32_t* counts, int32_t* skipped, ustrun_stream_t s);

/* Four sums per class plane of x, t (f32 [N,K,HW], K = 1..8) over N and HW, s = x (act USTRUN_LOSS_SOFTMAX: no activation) or
 * sigmoid(x) (USTRUN_LOSS_SIGMOID); where has_ignore and t == ignore_value both operands count as 0 (utils/metrics.py:41-44):
 *   out[k] = {sum s t, sum s, sum t, sum (1 + t) bce_with_logits(x, t)}   (the last only with the sigmoid, else 0)
 * They carry dice, DiceLoss, Balanced_DiceLoss and WatershedCrossEntropy of utils/metrics.py:36-47,72-91,242-266.
 * bwd: dx = (coef[k][0] t + coef[k][1]) ds/dx + coef[k][2] (1 + t)(s - t), 0 where t is ignored; coef_dev = K x 3 device floats. */
int ustrun_plane_sums_fwd(const float* x, const float* t, int N, int K, int HW, int act, int has_ignore, float ignore_value, float* out,
                          float* partials, int64_t partials_bytes, ustrun_stream_t s);
int ustrun_plane_sums_bwd(const float* x, const float* t, int N, int K, int HW, int act, int has_ignore, float ignore_value,
                          const float* coef_dev, float* dx, ustrun_stream_t s);

/* Colour decoding of label maps [N,HW] (int64 or f32), decode_segmap of dataloaders/utils.py:86-120: out f32 [N,3,HW] =
 * palette[l][c] / 255 with palette_dev K x 3 device bytes, K = 1..USTRUN_COLORIZE_KMAX; a label outside [0,K) writes l / 255 in
 * all three channels, the value the reference's copies leave there (:105-115).                                          */
#define USTRUN_COLORIZE_KMAX 256
int ustrun_colorize(const void* labels, int labels_is_i64, int N, int HW, const uint8_t* palette_dev, int K, float* out,
                    ustrun_stream_t s);

/* ---- per-sample binary overlap counts for the numpy Dice of utils/metrics.py:114-146 ---------
 * counts[n][c] = {|pred|, |gt|, |pred & gt|} with pred/gt binarised as (x == cls[c]) or (x != 0). */
int ustrun_dice_counts(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N,
                       int K, int HW, int by_class, int32_t* counts, ustrun_stream_t s);

/* ---- per-sample surface-distance records for the medpy metrics of the reference's test(): replaces binary.hd95 / binary.asd
 * of train.py:306-325 (train_mnms.py twin, test.py:117-136) up to the host's final square roots and divisions.
 * pred / gt as ustrun_dice_counts takes them: f32 {0,1} planes [N,K,H,W] (by_class = 0) or class maps [N,H,W], int64 or f32,
 * whose part c is (x == c + 1) (by_class = 1).  border(A) = A & ~erode(A) with the 4-neighbour cross and background outside
 * the image; d2 = exact squared Euclidean distance from a border pixel of one mask to the nearest border pixel of the other.
 * out[n][c] = one USTRUN_SURFACE_RECORD_BYTES record:
 *   int32 {|border(P)|, |border(G)|, d2[k], d2[min(k+1, n-1)]} -- the order statistics of the union multiset of both directions,
 *          n = |border(P)| + |border(G)|, k = floor(0.95 (n-1)) in f64 (numpy.percentile(.., 95), linear) --,
 *   f64   sum of sqrt(d2) over border(P) (binary.asd = that / |border(P)|), a fixed-order sum: equal bits on every run.
 * A plane with an empty prediction or an empty ground truth has no distances: both counts are reported, the rest is 0, and the
 * host applies the reference's rules (train.py:313-315).  H, W in 1..1024, else an error.  work: 16-byte aligned,
 * ustrun_surface_metrics_work_bytes (-1 + error for sizes out of range); out: 8-byte aligned.                               */
#define USTRUN_SURFACE_RECORD_BYTES 24
int64_t ustrun_surface_metrics_work_bytes(int N, int K, int H, int W);
int ustrun_surface_metrics(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N, int K, int by_class,
                           int H, int W, void* work, int64_t work_bytes, void* out, ustrun_stream_t s);

/* ---- post-processing of a binary prediction, per (sample, part) plane: the reference's dataloaders/utils.py:193-204
 * (post_processing), which fills the holes of the plane and deletes every connected component smaller than a fifth of the
 * foreground.  pred as ustrun_surface_metrics reads it: f32 planes [N,K,H,W] binarised as (x != 0) (by_class = 0), or a class
 * map [N,H,W], int64 or f32, whose part c is (x == c + 1) (by_class = 1); out: f32 {0,1} planes [N,K,H,W] (after filling,
 * parts may overlap, so the result is never a class map).  For ONE plane P, background outside the image:
 *   1 fill_holes != 0: a background pixel is a hole when no 4-connected (cross) path through background leads from it to the
 *     image border (scipy.ndimage.binary_fill_holes, default structure); F = P | holes.  Otherwise F = P.
 *   2 the components of F with 8-connectivity (skimage.measure.label's default for a plane); total = |F|, counted after filling.
 *   3 component c is removed when share_den * |c| < share_num * total, in 64-bit integers.  The reference's rule
 *     |c| / total < 0.2 in f64 is share 1 / 5 exactly for planes of at most 2^20 pixels: five equal components all stay, five
 *     equal ones plus one pixel more all go (the empty plane, as the reference returns it); total = 0 gives the empty plane.
 *     share_num = 0 removes nothing.
 * fill_holes = 0 with share_num = 0 only decodes pred to planes (the ground truth's way into the same form).
 * H, W in 1..1024 and N * K <= 65535, share_num >= 0, share_den > 0, else an error before any launch
 * (ustrun_post_process_work_bytes: -1 + error).  work: 16-byte aligned, owned by the caller; everything is asynchronous on s,
 * nothing is allocated, nothing waits for the device or reads from it; the components are a unique partition found with
 * integer atomics only: equal bits on every run.                                                                          */
int64_t ustrun_post_process_work_bytes(int N, int K, int H, int W);
int ustrun_post_process(const void* pred, int pred_is_i64, int N, int K, int by_class, int H, int W,
                        int fill_holes, int share_num, int share_den,
                        void* work, int64_t work_bytes, float* out, ustrun_stream_t s);

/* ---- signed distance maps of label planes: the reference's utils/util.py:208-239 (compute_sdf, two
 * scipy.ndimage.distance_transform_edt calls per image on the host) and the transform utils/metrics.py:52-70
 * (distance_transform) means to be, on the device for all N * K planes of a batch (csrc/distmap.hip).
 *
 * ustrun_signed_dist2: mask as ustrun_surface_metrics reads pred: f32 planes [N,K,H,W] binarised as (x != 0) (by_class = 0), or
 * a class map [N,H,W], int64 or f32, whose plane c is (x == c + 1) (by_class = 1).  s2[N*K][H][W], one int32 per pixel, is the
 * SIGNED SQUARED Euclidean distance, exact in integers:
 *   + d2 to the nearest foreground pixel at a background pixel,   - d2 to the nearest background pixel at a foreground pixel,
 * over the pixels of the image only -- nothing outside the image is of either kind (scipy's convention, util.py:226-227; NOT the
 * background-outside convention of ustrun_surface_metrics).  In a plane without the opposite kind (empty or full) every pixel
 * gets + USTRUN_DIST_NONE resp. - USTRUN_DIST_NONE.  flags[N*K]: 0 = empty plane, 1 = mixed, 2 = full.
 * H, W in 1..1024 (d2 <= 2 * 1023^2 < 2^21) and N * K <= 32767, else an error before any launch.  work: 16-byte aligned,
 * ustrun_signed_dist2_work_bytes (-1 + error for sizes out of range), owned by the caller.  Planes are independent, no block
 * waits for another, no atomics: equal bits on every run.
 *
 * ustrun_sdf_from_dist2: the normalisation of util.py:231-234 per plane, from s2 and flags as written above.  With
 *   pos = d2 of a foreground pixel (0 on background), neg = d2 of a background pixel (0 on foreground),
 *   maxpos / maxneg = their integer maxima over the plane,
 *   sdf = sqrt(neg) / sqrt(maxneg) - sqrt(pos) / sqrt(maxpos)      (f32 out; each pixel in f64, rounded once)
 * -- the reference's (x - min) / (max - min) with both minima 0, which they are on every mixed plane (posdis is 0 on the
 * background, negdis on the foreground, and both kinds exist).  The inner boundary of util.py:228,234
 * (find_boundaries(posmask, mode="inner"): a foreground pixel with a background 4-neighbour inside the image, i.e. s2 == -1)
 * is written as exactly 0.0f.  Planes of flag 0 are all zeros (util.py:224 skips them); planes of flag 2 are all zeros too --
 * the reference divides 0 / 0 there -- and the flag is how the caller learns of it.  The deepest pixels of a mixed plane are
 * exactly -1 and +1.  work: 16-byte aligned, ustrun_sdf_from_dist2_work_bytes (the two maxima per plane, found with integer
 * atomicMax: exact and order-free).
 * Both entries: asynchronous on s, nothing is allocated, nothing waits for the device; null pointers, sizes out of range and a
 * short work buffer are refused before any launch.                                                                          */
#define USTRUN_DIST_NONE 0x7fffffff
int64_t ustrun_signed_dist2_work_bytes(int N, int K, int H, int W);
int ustrun_signed_dist2(const void* mask, int mask_is_i64, int N, int K, int by_class, int H, int W,
                        void* work, int64_t work_bytes, int32_t* s2, int32_t* flags, ustrun_stream_t s);
int64_t ustrun_sdf_from_dist2_work_bytes(int N, int K, int H, int W);
int ustrun_sdf_from_dist2(const int32_t* s2, const int32_t* flags, int N, int K, int H, int W,
                          void* work, int64_t work_bytes, float* sdf, ustrun_stream_t s);

/* ---- volumes [D][H][W]: the 3-D twins of the three entries above (csrc/edt3d.hip).  compute_sdf is documented for
 * shape = (batch_size, x, y, z) (utils/util.py:208-217), and the medpy functions of the reference's test() (binary.hd95 / asd,
 * train.py:306-325) are n-dimensional and take `voxelspacing`.  The metric has three integer axis weights (wz, wy, wx), each in
 * 1..255:
 *   d2(p, q) = wz^2 dz^2 + wy^2 dy^2 + wx^2 dx^2        (int32, exact; unit weights: scipy's default)
 * -- millimetre spacing is mapped onto weights by the host (utils.metrics.spacing_weights), the device never leaves integers.
 * Every entry refuses, before any launch and before any pointer is used: D, H or W outside 1..1024, D * H * W > 2^27,
 * N * K > 32767, a weight outside 1..255, and wz^2 (D-1)^2 + wy^2 (H-1)^2 + wx^2 (W-1)^2 > 2^31 - 2 (the largest d2 of the volume
 * must stay below USTRUN_DIST_NONE); then null pointers, a short work buffer (the *_work_bytes queries: -1 + error for sizes out
 * of range) and misaligned pointers (work 16-byte, out 8-byte, the rest to their element).  Asynchronous on s, nothing is
 * allocated, nothing waits for the device; integer atomics and fixed-order f64 sums only: equal bits on every run.
 *
 * ustrun_signed_dist2_3d: mask as ustrun_signed_dist2 reads it, with D * H * W voxels where that has H * W pixels.
 * s2[N*K][D][H][W], int32: + d2 to the nearest foreground voxel at a background voxel, - d2 to the nearest background voxel at a
 * foreground voxel, over the voxels of the volume only (scipy's convention).  flags[N*K]: 0 = empty, 1 = mixed, 2 = full VOLUME;
 * a volume without the opposite kind holds + USTRUN_DIST_NONE resp. - USTRUN_DIST_NONE, whatever its single slices hold.
 *
 * ustrun_sdf_from_dist2_3d: the normalisation of util.py:231-234 per volume (the maxima are taken over the whole volume), as
 * ustrun_sdf_from_dist2 per plane; defined for unit weights, where the inner boundary (find_boundaries(mode="inner") in 3-D: a
 * foreground voxel with a background 6-neighbour inside the volume) is s2 == -1 and is written as exactly 0.0f.
 *
 * ustrun_surface_metrics_3d: pred / gt as ustrun_surface_metrics takes them.  border(A) = A & ~erode(A) with the 6-neighbour
 * cross and background outside the volume (medpy: generate_binary_structure(3, 1), binary_erosion defaults); every border voxel
 * of one mask gets d2 to the nearest border voxel of the other.  out[n][c] = one USTRUN_SURFACE3D_RECORD_BYTES record:
 *   int32 |border(P)|, |border(G)|
 *   int32 d2[k], d2[min(k+1, n-1)]   the order statistics of the union multiset, n = |border(P)| + |border(G)|,
 *                                    k = floor(0.95 (n-1)) in f64
 *   int32 max d2 over border(P), max d2 over border(G)
 *   f64   sum of sqrt(d2) over border(P);   f64 sum of sqrt(d2) over border(G)     (fixed-order sums)
 * When either border is empty both counts are reported and the rest is 0.                                                   */
#define USTRUN_SURFACE3D_RECORD_BYTES 40
int64_t ustrun_signed_dist2_3d_work_bytes(int N, int K, int D, int H, int W);
int ustrun_signed_dist2_3d(const void* mask, int mask_is_i64, int N, int K, int by_class, int D, int H, int W,
                           int wz, int wy, int wx, void* work, int64_t work_bytes, int32_t* s2, int32_t* flags,
                           ustrun_stream_t s);
int64_t ustrun_sdf_from_dist2_3d_work_bytes(int N, int K, int D, int H, int W);
int ustrun_sdf_from_dist2_3d(const int32_t* s2, const int32_t* flags, int N, int K, int D, int H, int W,
                             void* work, int64_t work_bytes, float* sdf, ustrun_stream_t s);
int64_t ustrun_surface_metrics_3d_work_bytes(int N, int K, int D, int H, int W);
int ustrun_surface_metrics_3d(const void* pred, const void* gt, int pred_is_i64, int gt_is_i64, int N, int K, int by_class,
                              int D, int H, int W, int wz, int wy, int wx, void* work, int64_t work_bytes, void* out,
                              ustrun_stream_t s);

/* ---- post-processing of a binary prediction as a VOLUME [D][H][W] (csrc/components3d.hip): the 3-D twin of
 * ustrun_post_process.  The reference's dataloaders/utils.py:193-204 (post_processing) is written n-dimensionally --
 * scipy.ndimage.binary_fill_holes, skimage.measure.label and np.sum take a volume as readily as a plane -- and on the stacked
 * slices of a case it means something else than slice by slice: a ring repeated in every slice is a tube open at both ends and
 * stays open, a stray blob is weighed against the whole case.  pred as ustrun_post_process reads it, with D * H * W voxels where
 * that has H * W pixels: f32 [N,K,D,H,W] binarised as (x != 0) (by_class = 0), or a class map [N,D,H,W], int64 or f32, whose
 * part c is (x == c + 1) (by_class = 1); out: f32 {0,1} [N,K,D,H,W], never a class map.  For ONE volume P, background outside:
 *   1 fill_holes != 0: a background voxel is a hole when no path of 6-neighbour (face) steps through background leads from it to
 *     a face of the volume (binary_fill_holes, default structure generate_binary_structure(3, 1)); F = P | holes.  Every voxel
 *     of slices 0 and D - 1 touches the outside: a volume with D <= 2 gains nothing, a tube along any axis gains nothing; six
 *     voxels that touch only by edges (an octahedron) do enclose their centre.  Otherwise F = P.
 *   2 the components of F with 26-connectivity (skimage.measure.label's default for a 3-D array, connectivity = ndim): two voxels
 *     touching by a corner are one component; total = |F|, counted after filling.
 *   3 component c is removed when share_den * |c| < share_num * total, in 64-bit integers.  The reference's |c| / total < 0.2 in
 *     f64 is share 1 / 5 exactly for total <= 2^27 (a ratio below 1/5 is at least 1 / (5 total) below it, and an exact fifth
 *     rounds to the literal 0.2).  share_num = 0 removes nothing; total = 0 gives the empty volume.
 *   4 largest != 0 (not in the reference; the rule most 3-D pipelines apply): only the largest component of F stays, among equal
 *     sizes the one whose smallest voxel index (z * H + y) * W + x is smallest.  Applied after rule 3 and independent of it: a
 *     volume emptied by the share stays empty.  Chosen in integers, no floating point.
 * fill_holes = 0, share_num = 0, largest = 0 only decodes pred (the ground truth's way into the same form).
 * Refused before any launch and before any pointer is used: D, H or W outside 1..1024, D * H * W > 2^27, N * K > 32767,
 * share_num < 0, share_den <= 0; then null pointers, a short work buffer (ustrun_post_process_3d_work_bytes: -1 + error for sizes
 * out of range) and misaligned pointers (work 16-byte, out and pred to their element).  work is owned by the caller; everything
 * is asynchronous on s, nothing is allocated, nothing waits for the device or reads from it; integer atomics only: equal bits
 * on every run.                                                                                                           */
int64_t ustrun_post_process_3d_work_bytes(int N, int K, int D, int H, int W);
int ustrun_post_process_3d(const void* pred, int pred_is_i64, int N, int K, int by_class, int D, int H, int W,
                           int fill_holes, int share_num, int share_den, int largest,
                           void* work, int64_t work_bytes, float* out, ustrun_stream_t s);

/* ---- chamfer distances and binary morphology of label planes and volumes (csrc/morph.hip): the reference's GetBoundary
 * (dataloaders/custom_transforms.py:630-647: ndimage.binary_dilation / binary_erosion with iterations = width per part, the
 * pixels where the two differ, the parts ORed; built inside Normalize_tf, :659), scipy.ndimage.binary_opening / binary_closing,
 * and scipy.ndimage.distance_transform_cdt, on the device.  All are thresholds or plain values of the exact integer distance to a
 * set under metric 0 = city-block (L1; scipy's default structure generate_binary_structure(rank, 1), the cross; cdt's 'taxicab')
 * or metric 1 = chessboard (L-inf; generate_binary_structure(rank, rank), 8 / 26 neighbours; cdt's 'chessboard'):
 *   binary_dilation(A, iterations = w, border_value = b) = d(p, A) <= w,   the outside of the box part of A when b = 1
 *   binary_erosion(A, iterations = w, border_value = b)  = d(p, ~A) > w,   the outside of the box part of ~A unless b = 1
 * A voxel at index i of an axis of extent n is min(i + 1, n - i) from the outside along that axis.
 * mask as ustrun_signed_dist2 reads it: f32 [N,K,D,H,W] binarised as (x != 0) (by_class = 0), or a class map [N,D,H,W], int64 or
 * f32, whose part c is (x == c + 1) (by_class = 1).  rank 2: planes, D must be 1 and the slice axis is no axis (no border, no
 * distance); rank 3: volumes, and D = 1 is a real one-slice volume, every voxel of which is 1 from the outside along z.
 * Every entry refuses, before any launch and before any pointer is used: a rank other than 2 or 3, rank 2 with D != 1, D, H or W
 * outside 1..1024, D * H * W > 2^27, N * K > 32767, a metric, outside, op or border_value code not listed here, width outside
 * 1..4095; then null pointers, a short work buffer (the *_work_bytes queries: -1 + error) and misaligned pointers (work 16-byte,
 * the rest to their element).  Asynchronous on s, nothing is allocated, nothing waits for the device; integers only, the only
 * atomics are the integer flag words: equal bits on every run.
 *
 * ustrun_chamfer_dist: sd[N*K][D][H][W], int32: + d to the nearest foreground voxel at a background voxel, - d to the nearest
 * background voxel at a foreground voxel.  outside: 0 = nothing outside the box is of either kind (distance_transform_cdt's
 * convention), 1 = the outside is background, 2 = the outside is foreground.  flags[N*K]: 0 = empty, 1 = mixed, 2 = full (the
 * box's own content, whatever `outside` says).  Where no voxel of the opposite kind exists and `outside` does not supply it, sd
 * holds + USTRUN_DIST_NONE resp. - USTRUN_DIST_NONE.
 *
 * ustrun_morph: op 0 = dilation, 1 = erosion, 2 = opening (erosion, then dilation), 3 = closing (dilation, then erosion), 4 = band
 * = dilation & ~erosion, GetBoundary's map of one part (custom_transforms.py:636-643).  width = scipy's iterations, 1..4095 (no
 * distance in a legal box exceeds 3069: every larger count gives the same answer; iterating "until nothing changes", scipy's
 * iterations < 1, is not built).  border_value 0 or 1 with scipy's meaning, handed to BOTH halves of an opening or closing as
 * scipy does -- at the default 0 a closing therefore erodes from the box's faces.  reduce_parts != 0 ORs the K parts of an image:
 * out is u8 {0,1} [N][D][H][W] (custom_transforms.py:646), otherwise [N*K][D][H][W].                                        */
int64_t ustrun_chamfer_dist_work_bytes(int N, int K, int rank, int D, int H, int W);
int ustrun_chamfer_dist(const void* mask, int mask_is_i64, int N, int K, int by_class, int rank, int D, int H, int W,
                        int metric, int outside, void* work, int64_t work_bytes, int32_t* sd, int32_t* flags,
                        ustrun_stream_t s);
int64_t ustrun_morph_work_bytes(int N, int K, int rank, int D, int H, int W, int op);
int ustrun_morph(const void* mask, int mask_is_i64, int N, int K, int by_class, int rank, int D, int H, int W,
                 int metric, int op, int width, int border_value, int reduce_parts,
                 void* work, int64_t work_bytes, uint8_t* out, ustrun_stream_t s);

/* ---- SGD(momentum, weight decay) + EMA teacher over flat buffers: train.py:512,848,87-93 ------
 * g += wd*p; v = first ? g : mu*v + g; p -= lr*v; t = alpha*t + (1-alpha)*p                    */
/* ---- dynamic loss scale of the IEEE-half path: torch.cuda.amp.GradScaler as train.py:552,842-845 uses it, on the device.
 * amp_state = 8 floats {scale, scale, growth_tracker, found_inf, steps skipped so far, steps seen so far, 0, 0} (initialise
 * to {65536, 65536, 0, 0, 0, 0, 0, 0}); its address is what
 * ustrun_seg_loss_bwd / ustrun_dice_bwd take as gscale_dev, which scales the backward.  Per step, after the gradient
 * all-reduce: ustrun_amp_check (found_inf = 1 if any element of g is not finite) -> ustrun_sgd_ema_scaled (gradient x
 * grad_scale / scale; found_inf: parameters and momentum untouched = GradScaler.step skipping optimizer.step, the EMA line
 * still runs) -> ustrun_amp_update (scale x backoff after a skipped step, x growth after growth_interval clean ones --
 * GradScaler defaults 2, 0.5, 2000 --, found_inf cleared).  Nothing here waits for the host.                           */
int ustrun_amp_check(const float* g, int64_t n, float* amp_state, ustrun_stream_t s);
int ustrun_sgd_ema_scaled(float* p, const float* g, float* v, float* t, int64_t n, float lr, float mu, float wd,
                          int first, float alpha, float grad_scale, const float* amp_state, ustrun_stream_t s);
int ustrun_amp_update(float* amp_state, float growth_factor, float backoff_factor, int growth_interval, ustrun_stream_t s);
int ustrun_sgd_ema(float* p, const float* g, float* v, float* t, int64_t n, float lr, float mu,
                   float wd, int first, float alpha, float grad_scale, ustrun_stream_t s);

/* ---- whole-network plan: replaces UNet.forward / autograd backward, unet_model.py:25-39 -------
 * The plan is a host-side description (shapes + parameter pointers); the caller owns all device
 * memory: params, packed-weight arena, forward workspace (kept for backward) and scratch.      */
typedef struct ustrun_unet_desc {
    int32_t N, C, H, W, K;       /* batch, input channels, extent, classes                    */
    int32_t base;                /* 64 in the reference (unet_model.py:13)                    */
    int32_t dtype;               /* storage dtype of activations                              */
    int32_t train;               /* batch statistics (1) or running statistics (0)            */
    int32_t update_running;      /* update BN running buffers (train mode)                    */
    int32_t groups;              /* > 1: N = groups * n images of `groups` independent forward passes batched into one
                                  * call; BatchNorm statistics (and running-buffer updates, in order) are per pass  */
    int32_t tail;                /* > 0: N = groups * n + tail: `tail` (< n) more images follow as one further, shorter forward
                                  * pass (its own BatchNorm statistics, its running-buffer update after the others') whose
                                  * logits nobody reads: the head skips it and ustrun_unet_backward covers the first
                                  * groups * n images only (train.py:740: the low-quality sample's forward, Q2)      */
    int32_t lead;                /* > 0: the first `lead` (< groups) passes carry no gradient: the forward treats them as any other pass
                                  * (statistics, running-buffer updates in order, logits), ustrun_unet_backward starts behind them --
                                  * dlogits keeps the forward's layout (N - tail images; the leading passes' rows are ignored).
                                  * train.py:668: the student's forward on the weak view, whose arg-max alone is used (Q3), runs as
                                  * the first pass of the call that carries the four gradient passes of :699-702          */
    float   momentum, eps;
    /* parameters/buffers, torch layouts, in state_dict order:                 */
    const float* conv_w[18];     /* inc.0, inc.3, down1..4 (.0,.3), up1..4.conv (.0,.3)        */
    const float* bn_w[18];  const float* bn_b[18];
    float* bn_rm[18];       float* bn_rv[18];   int64_t* bn_nbt[18];
    const float* up_w[4];   const float* up_b[4];
    const float* head_w;    const float* head_b;
    void* packed;                /* packed-weight arena, ustrun_unet_packed_bytes()           */
    int32_t bilinear;            /* 1: the reference's UNet(bilinear=True) (unet_model.py:17-22, unet_parts.py:48-51): Up upsamples its
                                  * input 2x (bilinear, align_corners=True) instead of a ConvTranspose2d -- no up_w / up_b, down4 and the
                                  * decoder on the halved channel plan (DoubleConv(in, out, in // 2)), 56 parameter tensors           */
} ustrun_unet_desc_t;

int64_t ustrun_unet_packed_bytes(const ustrun_unet_desc_t* d);
int64_t ustrun_unet_fwd_workspace_bytes(const ustrun_unet_desc_t* d);
int64_t ustrun_unet_bwd_scratch_bytes(const ustrun_unet_desc_t* d);
int ustrun_unet_pack(const ustrun_unet_desc_t* d, ustrun_stream_t s);
/* x NCHW f32 [N,C,H,W] -> logits NCHW f32 [N,K,H,W]; feat (optional) NCHW f32 [N,base,H,W]  */
int ustrun_unet_forward(const ustrun_unet_desc_t* d, const float* x, float* logits, float* feat,
                        void* workspace, ustrun_stream_t s);
/* grads[] follow the parameter order of the reference's model.parameters() (64 tensors for
 * bilinear=False, 56 for bilinear=True): accumulate != 0 adds into them.                     */
int ustrun_unet_backward(const ustrun_unet_desc_t* d, const float* x, const float* dlogits,
                         void* workspace, void* scratch, float* const* grads, int accumulate,
                         ustrun_stream_t s);
/* the same in pieces sharing one scratch: part 1 = head + decoder (afterwards the gradients of up1..up4 and outc,
 * the contiguous tail of the parameter order, are final: their all-reduce can start), part 2 = encoder -- or part 3 =
 * down4 (parameters 24..29 final afterwards) followed by part 4 = down3..inc; part 0 = all */
int ustrun_unet_backward_part(const ustrun_unet_desc_t* d, const float* x, const float* dlogits,
                              void* workspace, void* scratch, float* const* grads, int accumulate, int part,
                              ustrun_stream_t s);
/* ... with the two gradients that make both outputs of UNet.forward(x, feature=True) ordinary autograd tensors and the
 * input a differentiable one (unet_model.py:25-39: `return logits, x_last64`; nothing there detaches x):
 *   dfeat (optional) NCHW f32, the forward's feat layout: the gradient of the feature output.  It is added to the head's
 *     input gradient in front of the last BatchNorm's backward; consumed by the part that runs the head (0 or 1).  The
 *     leading passes' rows are ignored, as dlogits' are.  dlogits may be NULL when dfeat is given: it stands for zeros
 *     (the head's weight and bias gradients are then zero).
 *   dx (optional) NCHW f32 [N,C,H,W], overwritten: the gradient of the network input, ustrun_conv_first_dgrad of inc's
 *     first convolution (unet_parts.py:16); written by the part that reaches layer 0 (0, 2 or 4).  Rows of leading
 *     passes and of the tail pass are zero.  Needs C <= 4 and base a multiple of 8 up to 64.
 * With dfeat == dx == NULL this IS ustrun_unet_backward_part, launch for launch.                                          */
/* d->train == 0: the backward through frozen BatchNorm (the forward must have run with the same eval descriptor; UNet under
 * model.eval(), unet_model.py:25-39 with nn.BatchNorm2d on its running buffers): every layer's BatchNorm backward is the one-pass
 * ustrun_bn_bwd_frozen, no running buffer moves; parts, dfeat, dx, groups / lead / tail and bilinear work as in train mode.
 * grads == NULL (either mode): the input gradient alone -- needs dx, or a part that ends before layer 0 (1 or 3); no weight
 * gradient, no head parameter gradient and no dgamma / dbeta is launched (eval mode: no sum and no finalize either; train mode
 * keeps the sums its coefficients need).  dx is bit-identical to the call with gradients.                                  */
int ustrun_unet_backward_io(const ustrun_unet_desc_t* d, const float* x, const float* dlogits, const float* dfeat,
                            void* workspace, void* scratch, float* const* grads, int accumulate, int part, float* dx,
                            ustrun_stream_t s);

/* ---- DeepLabV2-ResNet operators (reference networks/deeplabv2.py:10-33, networks/backbone/resnet.py:55-176; SURVEY.md 8f
 * row 4), forward and backward.  Activations NHWC in the compute dtype like the U-Net's.                                   */
/* torch conv weight [Cout][Cin][kh*kw] -> the forward pack of `taps` slices (bf16 [tap][Cin/8][Cout][8], f32 [tap][Cin][Cout]);
 * w_fwd holds ustrun_pack_conv_elems() elements of the compute dtype                                                      */
int ustrun_pack_conv(const float* w, int Cout, int Cin, int taps, void* w_fwd, int dtype, ustrun_stream_t s);
int64_t ustrun_pack_conv_elems(int Cout, int Cin, int taps);
/* the same count for a given compute dtype: ustrun_pack_conv_elems() for USTRUN_F32 / BF16 / F16; USTRUN_F32X3 packs the f32
 * slices and then, when Cin % 8 == 0, their three bf16 planes [tap][plane][Cin/8][Cout][8] behind them (what the three-term implicit
 * GEMM reads) -- 2.5 x the floats.  A buffer handed to ustrun_pack_conv with USTRUN_F32X3 must be sized with this entry.       */
int64_t ustrun_pack_conv_elems_dtype(int Cout, int Cin, int taps, int dtype);
/* k x k convolution (k = 1, 3, 5, 7), stride 1 or 2, dilation d, padding d * (k / 2) (nn.Conv2d of resnet.py:8-15,124 and
 * deeplabv2.py:15-17) of the concatenated sources -> y [N, Ho, Wo, Cout] (compute dtype, or f32 when y_f32); bias optional;
 * stat (optional): BatchNorm-statistics partial rows [rows][2][Cout] -- the buffer must hold ustrun_conv_mtiles(N, Ho, Wo,
 * Cout) rows (which kernel serves the launch decides how many are written), *stat_rows receives the count written       */
int ustrun_conv2d_fwd(const ustrun_src_t* srcs, int nsrc, const void* w_fwd, const float* bias, int N, int Ho, int Wo, int Cout,
                      int k, int stride, int dilation, void* y, int y_f32, float* stat, int* stat_rows, int dtype, ustrun_stream_t s);
/* a k x k convolution over FEW input channels (the 7x7 / stride-2 stem, resnet.py:124) as `nrows` row segments of a source the
 * caller has zero-padded and describes window-wise: src->C = the k * Cin contiguous NHWC elements of one kernel row rounded up
 * to a multiple of 8, src->sW = Cin (pixel stride in elements), src->sH / sN = the padded tensor's strides, src->H / W = the
 * rows / window starts available; output pixel (y, x), segment s reads the window at (stride*y + s, stride*x); weights packed
 * by ustrun_pack_conv as [Cout][src->C]["taps" = nrows]                                                                    */
int ustrun_conv_rowwin_fwd(const ustrun_src_t* src, const void* w_fwd, int N, int Ho, int Wo, int Cout, int nrows, int stride, void* y,
                           float* stat, int* stat_rows, int dtype, ustrun_stream_t s);
/* MaxPool2d(3, stride 2, padding 1) of relu(y * scale + shift) (resnet.py:127): [N,H,W,C] -> [N,(H+1)/2,(W+1)/2,C]       */
int ustrun_maxpool3x3s2(const void* y, const float* scale, const float* shift, int N, int H, int W, int C, void* out, int dtype,
                        ustrun_stream_t s);
/* the bottleneck's join (resnet.py:97-103): out = relu(y * scale + shift + identity), identity = idn * iscale + ishift
 * (the downsample branch's BatchNorm) or idn itself when iscale is NULL                                                   */
int ustrun_bn_add_relu(const void* y, const float* scale, const float* shift, const void* idn, const float* iscale,
                       const float* ishift, int64_t npix, int C, void* out, int dtype, ustrun_stream_t s);
/* the classifier's dilated 3x3 branches (deeplabv2.py:15-17,26-28) evaluated as ONE 1x1 GEMM z [N,h,w,nrates*9*K] (column
 * (r*9+tap)*K+k = sum_c x[c] w_r[k][c][tap], from ustrun_conv2d_fwd with k = 1) followed by this shifted add:
 * out[N,h,w,K] = bias_sum[k] + sum_{r,tap} z[p + rates[r]*(tap/3-1, tap%3-1)][(r*9+tap)*K+k], zero outside the image;
 * rates: host array of nrates (<= 4) ints                                                                                  */
int ustrun_aspp_gather(const float* z, int N, int h, int w, int K, int nrates, const int* host_rates, const float* bias_sum,
                       float* out, ustrun_stream_t s);
/* sum of up to four f32 NHWC maps [N,h,w,K] (the classifier's dilated branches, deeplabv2.py:26-28), resized bilinearly with
 * align_corners=True to NCHW f32 [N,K,H,W] (deeplabv2.py:30)                                                               */
int ustrun_sum_resize_bilinear(const float* const* maps, int nmaps, int N, int h, int w, int K, int H, int W, float* out,
                               ustrun_stream_t s);

/* the same row windows written out as GEMM rows: out [N*Ho*Wo][k_padded] in the compute dtype, column s * src->C + j = element j of
 * the window of kernel row s, columns >= nrows * src->C zero (k_padded % 8 == 0).  With it the stem is ONE 1x1 convolution over
 * k_padded "channels" (ustrun_conv2d_fwd / ustrun_conv2d_wgrad with k = 1) on the fast GEMM kernels                             */
int ustrun_rowwin_patches(const ustrun_src_t* src, int N, int Ho, int Wo, int nrows, int stride, int k_padded, void* out, int dtype,
                          ustrun_stream_t s);

/* ---- DeepLabV2-ResNet backward (autograd of the modules above).  Input gradients of the stride-1 convolutions are
 * ustrun_conv2d_fwd launches over dy with the flipped / transposed weights (packed by ustrun_pack_conv from
 * w.flip(2,3).transpose(0,1)); BatchNorm backward is ustrun_bn_bwd_reduce / _apply (a BatchNorm that is NOT followed by a ReLU
 * -- bn3, the projection shortcut's -- passes scale = 0, shift = 1 so that the kernels' ReLU mask is all ones).                */
/* weight gradient of ustrun_conv2d_fwd's convolution (k = 1 or 3): dw[Cout][Cin][k][k] (torch layout, f32); partials: scratch
 * of ustrun_wgrad_partials_bytes(k*k, Cin, Cout, N*Ho*Wo) bytes                                                              */
int ustrun_conv2d_wgrad(const ustrun_src_t* srcs, int nsrc, const void* dy, int N, int Ho, int Wo, int Cout, int k, int stride,
                        int dilation, float* dw, int accumulate, float* partials, int64_t partials_bytes, int dtype, ustrun_stream_t s);
/* weight gradient of ustrun_conv_rowwin_fwd: dw[Cout][src->C][nrows] (the layout its weights were packed from)               */
int ustrun_conv_rowwin_wgrad(const ustrun_src_t* src, const void* dy, int N, int Ho, int Wo, int Cout, int nrows, int stride, float* dw,
                             int accumulate, float* partials, int64_t partials_bytes, int dtype, ustrun_stream_t s);
/* the input gradient of a 1x1, stride-1 convolution with what follows it in a bottleneck's backward (resnet.py:87-105 under
 * autograd), in one launch: g[N,H,W,Cin] = (dy (*) w_dgrad + add) * (ref > 0) -- what ustrun_conv2d_fwd over dy followed by
 * ustrun_relu_bwd_add computes, rounding included (add / ref may be NULL as there: conv1's input gradient and the residual join)
 * -- and, with y != NULL, the BatchNorm-backward sums of the layer whose OUTPUT gradient g is, as *stat_rows rows of [2][Cin] =
 * {sum(g mask), sum(g mask y)} for ustrun_bn_bwd_finalize_stat (stat: ustrun_conv_mtiles(N, H, W, Cin) rows): mask = y scale +
 * shift > 0 (a BatchNorm + ReLU layer: conv3's input gradient feeding bn2), or all ones with scale = shift = NULL (a BatchNorm no
 * ReLU follows: the previous block's bn3, resnet.py:96, behind the join).  *fused = 0 and NO launch when the shape is not covered
 * (16-bit storage, Cin % 128 == 0, Cout % 64 == 0): the caller then runs the separate calls.                                   */
int ustrun_conv1x1_dgrad_join(const void* dy, const void* w_dgrad, int N, int H, int W, int Cout, int Cin, const void* add,
                              const void* ref, void* g, const void* y, const float* scale, const float* shift, float* stat,
                              int* stat_rows, int* fused, int dtype, ustrun_stream_t s);
/* space-to-batch for a dilated 3x3 convolution's weight gradient: out[(n r + a) r + b][i][j][c] = act(src[n][i r + a][j r + b][c]),
 * every residue class (a, b) of the r x r pixel lattice as an image of its own, all padded with ZEROS to ceil(H / r) x ceil(W / r)
 * (out: N r r images); act = relu(x scale + shift) when the source carries constants, else a copy (src: plain contiguous NHWC,
 * 16-bit storage, C % 8 == 0).  With BOTH operands laid out this way ustrun_conv2d_wgrad(k = 3, dilation = 1) over N r r images
 * returns the weight gradient of the dilation-r convolution (networks/backbone/resnet.py:92-93 with replace_stride_with_dilation)
 * on the all-taps kernel.                                                                                                        */
int ustrun_space_to_batch(const ustrun_src_t* src, int N, int r, void* out, int dtype, ustrun_stream_t s);
/* the input gradient of a (dilated) 3x3, stride-1 convolution as ustrun_conv2d_fwd forms it (a convolution of dy with the pack of
 * w.flip(2,3).transpose(0,1)) that also forms the BatchNorm-backward sums of the BatchNorm + ReLU layer whose output gradient da
 * is -- conv2's input gradient feeding bn1 (resnet.py:89-93 under autograd): rows and mask as ustrun_conv3x3_dgrad_bnsum.
 * *stat_rows = 0 and NO launch when the fused epilogue does not cover the shape (16-bit storage, Cin % 128 == 0, dilation 1 / 2 / 4). */
int ustrun_conv2d_dgrad_bnsum(const void* dy, const void* w_flipped, int N, int H, int W, int Cout, int Cin, int dilation, void* da,
                              const void* y, const float* scale, const float* shift, float* stat, int* stat_rows, int dtype,
                              ustrun_stream_t s);
/* gradient of the bottleneck's join with respect to its pre-ReLU sum: g = (a + b) * (ref > 0) over n elements (n % 4 == 0);
 * b = NULL: one contribution, ref = NULL: no ReLU (the max-pool output feeding layer1)                                       */
int ustrun_relu_bwd_add(const void* a, const void* b, const void* ref, int64_t n, void* g, int dtype, ustrun_stream_t s);
/* MaxPool2d(3, 2, 1) backward: dp [N,(H+1)/2,(W+1)/2,C] -> da [N,H,W,C] (gradient of the ACTIVATED tensor relu(y*scale+shift),
 * whose ReLU the following ustrun_bn_bwd_* applies); the first maximum of a window wins (torch's rule); gather, fixed order   */
int ustrun_maxpool3x3s2_bwd(const void* dp, const void* y, const float* scale, const float* shift, int N, int H, int W, int C, void* da,
                            int dtype, ustrun_stream_t s);
/* adjoint of ustrun_sum_resize_bilinear for one map: dout NCHW f32 [N,K,H,W] -> dlow NHWC f32 [N,h,w,K]                      */
int ustrun_sum_resize_bilinear_bwd(const float* dout, int N, int h, int w, int K, int H, int W, float* dlow, ustrun_stream_t s);
/* adjoint of ustrun_aspp_gather: dz [N,h,w,zc_padded] in the compute dtype (columns >= nrates*9*K are zero)                  */
int ustrun_aspp_scatter(const float* dlow, int N, int h, int w, int K, int nrates, const int* host_rates, int zc_padded, void* dz,
                        int dtype, ustrun_stream_t s);
/* out[c] (+)= sum over rows of x[row][c] (f32, f64 accumulation, fixed order): the classifier biases' gradient              */
int ustrun_colsum(const float* x, int64_t rows, int C, float* out, int accumulate, ustrun_stream_t s);

/* test aid: tile configuration of the last halo-tiled bf16 3x3 convolution launched by this process, as
 * TH<<24 | TW<<16 | BN<<8 | MI<<4 | NT<<2 | POOL<<1 | XF (0 before any) -- lets a parity test assert that its shape
 * reached the production tile it was written for                                                   */
int ustrun_debug_last_conv_variant(void);
/* the 1x1 / ConvTranspose GEMM kernel (convT_bf16.hip) reports 0x43540000 | (BN / 32) << 8 | (BK / 32) << 4 | MODE there
 * (MODE 0 ConvTranspose forward, 1 its input gradient, 2 a 1x1 convolution).
 * Same for the last weight-gradient launch: the one-tap-per-block kernel (wgrad_tap_bf16.hip) reports
 * 0x54000000 | (TM / 64) << 20 | (TN / 64) << 16 | loader << 12 | ksplit (loader 2 = pixel-linear 1x1, 1 = one shifted tap,
 * 0 = k x k taps); the all-taps halo kernel 0x48000000 | build << 20 | ksplit (build 0 = round-2 kernel, 1 = buffer-addressed
 * transfers, 2 = two wave groups in opposite phases); dtype USTRUN_F32X3's one-tap-per-block kernel (wgrad_tap_x3.hip)
 * 0x58000000 | (TM / 64) << 20 | (TN / 64) << 16 | slab layout << 12 | ksplit (layout 1 = one tap, slabs [Cout][Cin]; 0 = 3 x 3 taps,
 * slabs [tap][Cin][Cout]); 0 before any / for the generic kernels.
 * ustrun_debug_last_conv_variant of the ConvTranspose / 1x1 GEMM kernel: 0x43540000 | (weights through registers ? 0x1000 : 0) |
 * (BN / 32) << 8 | (BK / 32) << 4 | mode (0 forward, 1 input gradient, 2 plain 1x1)                              */
int ustrun_debug_last_wgrad_variant(void);
/* the last BatchNorm-backward launch (ustrun_bn_bwd_reduce / _apply / _frozen and the whole-network backward):
 * 0x424E0000 | pass << 8 (0 reduce, 1 apply, 2 frozen) | element bytes << 4 | even-sized pooled windows << 2 | pooled << 1 |
 * eight channels (16 bytes) per lane; 0 before any                                                              */
int ustrun_debug_last_bn_variant(void);
/* the routes the calling thread's last ustrun_unet_backward / _part / _io call took at the two full-resolution layers:
 * bit 0: layer 17 (under the head) -- the head stored no input gradient, the BatchNorm-backward apply pass formed it from dlogits;
 * bit 1: layer 0 -- no apply pass, the first convolution's weight gradient formed dY from da and y on load.
 * A call that does not cover the layer (parts) leaves its bit clear.                                                            */
int ustrun_debug_last_backward_route(void);
/* test aid, host only (no launch, no device access): the number of BatchNorm-statistics rows the kernel that would serve a
 * k x k convolution of a dense NHWC source [N, Cin] -> [N, Ho, Wo, Cout] writes.  tests/test_host_logic.py sweeps shapes
 * with it: the count must never exceed ustrun_conv_mtiles(N, Ho, Wo, Cout), which is what callers allocate           */
int ustrun_debug_conv_stat_rows(int N, int Ho, int Wo, int Cin, int Cout, int k, int stride, int dilation, int pooled, int dtype);
/* test / tuning aid: process-wide kernel-selection flags, returns the previous value.  bit 0: run the 64 -> 64 channel
 * full-resolution convolutions on the halo-tiled kernel instead of the weight-stationary row-streaming one (A/B timing
 * inside one process); bit 1: the four-wave build of the streaming kernel for every launch, bit 2: the eight-wave build for every
 * launch; bit 4 (16): no consumer / producer build (then eight waves for plain sources without statistics, four waves otherwise),
 * bit 5 (32): the consumer / producer build for every launch -- it is the default since round 3.
 * bit 3 (8): halo-tiled kernel with weight tiles in LDS (round 2) instead of weights through registers;
 * bit 6 (64): all-taps weight gradient with per-item pointers (round 2) instead of buffer-addressed transfers;
 * bit 7 (128): that kernel with extra LDS so that one block fits a CU (occupancy experiment);
 * bit 8 (256): no two-group weight-gradient kernel; bit 9 (512): ConvTranspose / 1x1 GEMM with weight tiles in LDS (round 2).
 * bits 10-11: force the halo kernel's tile in the 128-column case (1: 8 x 32 px, 2: 16 x 16, 3: 8 x 16; 0: chosen by padding).
 * bit 12 (4096): BatchNorm backward (plain, bf16) on the 4-channel-per-lane kernels instead of the 8-channel ones.
 * The last-variant code of the streaming kernel is 0x57530000 | (eight waves ? 0x100 : consumer / producer ? 0x200 : 0) | XF, and on the
 *   consumer / producer build | 0x400 with the BatchNorm-backward sums and | 0x800 on the flat plan (equal row steps per block).
 * The halo-tiled kernel runs plain sources (the input gradients) on its 256-pixel x 128-channel tiles on v_mfma_f32_16x16x32
 *   (ustrun_debug_last_conv_variant then carries bit 7, 0x80); bit 15 (32768): on every tile; bit 21 (2097152): on none.
 * bit 14 (16384): first convolution (C <= 4 -> 64) on the tile-per-block kernel of rounds 1-3 instead of the streaming one.
 * bits 16-20: layer + 1 at which ustrun_unet_backward stops early (tests/diag_grad.py; 0: runs through).
 * bit 22 (4194304): ustrun_unet_forward finalizes each layer's BatchNorm statistics in ONE launch (last-ticket pattern) instead of
 *   two; bit-identical results, measured no faster (profiles/r04_ab_bn_fused_finalize.log), off by default.
 * bit 23 (8388608): ustrun_unet_backward runs the BatchNorm-backward reduce pass of the layer under the head (rounds 1-3)
 *   instead of taking its two sums from the head kernel's partial rows.
 * bit 24 (16777216), ENVIRONMENT ONLY (USTRUN_DEBUG_FLAGS at load; ustrun_debug_flags does not change it): the decoder reads
 *   its skip operands through BatchNorm + ReLU on load (rounds 1-3) instead of the activation tensors ustrun_pool_act2
 *   materialises -- the switch shapes the workspace that ustrun_unet_forward and _backward share, so it must not differ
 *   between the threads that call them.
 * bit 25 (33554432): ustrun_unet_backward never asks an input gradient for the BatchNorm-backward sums of the layer it feeds
 *   (ustrun_conv3x3_dgrad_bnsum): every BatchNorm backward runs its reduce pass, as in rounds 1-3.
 * bit 26 (67108864), ENVIRONMENT ONLY like bit 24: the second convolution of every DoubleConv reads its operand through
 *   BatchNorm + ReLU on load (rounds 1-3) instead of the activation ustrun_act16 writes out on the levels from 256 channels.
 * bit 27 (134217728): ustrun_head_fwd on its generic 16-bit kernel instead of the 64-channel one.
 * bit 13 (8192): 64-output-channel 3x3 layers on >= 32-wide maps on the 16 x 32-pixel tile (one block per CU; A/B runs).
 * A caller that runs a forward and its backward on different threads sets the same value on both (the Python host does:
 * ustrun/engine.py hands the forward's flags to autograd's backward thread).
 * The value is PER CALLING THREAD (as are the last-variant codes and the stamp buffer below): a thread that sets it changes
 * kernel selection for the launches it issues itself and for nobody else, so the library keeps no process-wide mutable
 * state.  Every thread starts from the value the environment variable USTRUN_DEBUG_FLAGS had when the library was loaded
 * (read once at load, never on a launch path).                                                                    */
int ustrun_debug_flags(int flags);
/* a second word of the same kind (the first is full), same rules: per calling thread, returns the previous value, starts from the
 * environment variable USTRUN_DEBUG_FLAGS2 as read at load.
 * bit 0 (1): the halo-tiled 3x3 kernel never runs on its linear tiles (round 5: maps with 18 / 24 / 36 / 72-pixel rows; DESIGN.md
 *   10.9) -- the rectangular tile of the padding rule instead (A/B runs, and the tests that pin those tiles).
 * bit 1 (2): dtype USTRUN_F32X3 launches its halo-tiled convolution and its weight gradient once per pass of a batched call, as
 *   before they took the pass's constants per image (A/B runs).
 * bit 2 (4): the 64 -> 64 streaming kernel keeps its uniform strip split (round 6: the flat plan gives every block the same number
 *   of row steps at any image count) -- A/B runs.
 * bit 3 (8): ustrun_conv1x1_dgrad_join never fuses (*fused = 0) -- A/B runs and the tests of the unfused path.
 * bit 4 (16): ustrun_unet_backward stores the head's input gradient and runs layer 17's BatchNorm-backward apply pass over it, and
 *   runs layer 0's apply pass in front of the first convolution's weight gradient, as before those two round trips were dropped
 *   (ustrun_debug_last_backward_route reads 0) -- A/B runs and the equality tests.  The workspace is the same either way.
 *   bit 5 (32): layer 17's round trip alone, bit 6 (64): layer 0's alone -- each half timed with the other in place.
 * bit 7 (128): ustrun_post_process_3d unites every neighbour pair between adjacent slices, leaving none out as redundant -- A/B
 *   runs and the test that the result does not depend on the pruning.                                                       */
int ustrun_debug_flags2(int flags);
/* Operator-level declaration (per calling thread; returns the previous value): while `allow` is nonzero, the convolution entry
 * points accept a batch whose LAST pass is shorter than ustrun_src_t::gN (N % gN != 0 -- the caller then owns a constants table of
 * ceil(N / gN) entries and splits the statistics rows accordingly).  Otherwise N % gN != 0 is an error ("inconsistent pass
 * groups"): a mis-sized batch is not a tail.  ustrun_unet_forward / _backward set it themselves from ustrun_unet_desc_t::tail.   */
int ustrun_short_last_pass(int allow);
/* development aid: while a device buffer is set here (per calling thread), the 64 -> 64 streaming kernel and the two-group
 * all-taps weight gradient run their phase-stamping diagnostic builds and write per-wave cycle sums there as
 * [workgroup][8 waves][8] u64 = 64 u64 per workgroup (tools/ab_ws64.py --diag, tools/diag_wgrad.py).  n_u64 = the buffer's
 * length: a launch whose grid needs more (grid x 64) fails with an error instead of writing past the end.  NULL restores
 * the product kernels                                                                                              */
int ustrun_debug_buffer(void* device_u64, int64_t n_u64);
/* measurement aid (tools/clock_probe.py, bench.py): `blocks` workgroups each write 4 u64 {s_memtime (shader-clock ticks),
 * s_memrealtime (100 MHz ticks), XCC id, HW_ID} to device_u64[blocks][4].  Two probes on one stream around a series of
 * launches give the shader clock the chip held meanwhile: d(memtime) / d(memrealtime) x 100 MHz, per XCD.          */
int ustrun_debug_clock_probe(void* device_u64, int blocks, ustrun_stream_t s);

/* ---- optional launch profiler (bench.py): HIP events recorded on the launch stream around every
 * implicit-GEMM (kind 0) / weight-gradient (kind 1) launch while enabled; collect synchronises on
 * the recorded events, returns the sums and resets that kind.                                   */
int ustrun_profile_enable(int on);
int ustrun_profile_collect(int kind, double* host_ms, double* host_flops, double* host_bytes,
                           int64_t* host_launches);
/* only != 0: time only the launches issued on stream s (a launch on a side stream overlaps the profiled stream's
 * kernels, its event pair would measure contention); only == 0: every stream (the default)      */
int ustrun_profile_stream(ustrun_stream_t s, int only);
/* one record per timed launch, in launch order, WITHOUT resetting (call before ustrun_profile_collect).  tag: the
 * whole-network calls label their launches -- 3x3 conv i (0..17, network order) forward = i, ConvTranspose j (0..3)
 * forward = 20 + j, the input gradients of the same layers + 100, the weight gradients + 200; -1 for operator-level
 * calls.  n = images in the launch.  flops / bytes = the launch's ALGORITHMIC cost (every stored input, output and
 * weight element touched once at its stored size).  Returns the number of records written, -1 on error.        */
typedef struct ustrun_prof_rec {
    int32_t kind, tag, n, pad;
    double  ms, flops, bytes;
} ustrun_prof_rec_t;
int64_t ustrun_profile_records(ustrun_prof_rec_t* host_out, int64_t max_records);

/* ------------------------------------------------------------------------------------------
 * Data augmentation of resident image pools (csrc/augment.hip).  The reference runs
 * these per sample in PIL / scipy on loader workers (dataloaders/dataloader.py:95-107,
 * dataloaders/custom_transforms.py); here a batch is a set of uint8 HWC buffers on the device
 * and every stage reads uint8 and writes uint8 where the reference quantises.
 *   images [B][H][W][C] (C = 1 or 3), labels [B][H][W][Cl] (Cl = 1 or 3), H, W <= 1024.
 *   `params` is the batch's int32 parameter block: sample b reads params + b * stride; a float
 *   or double parameter is stored as its bit pattern (doubles: low word first).  Word 0 of every
 *   stage's row is its gate: 0 = the sample is copied.  The host draws the rows
 *   (ustrun/datasets.py: AugmentSampler), the only host-to-device copy of a step.
 * ---------------------------------------------------------------------------------------- */
/* batch buffers out of the pools: img_out[b] = images[idx[b]], lab_out[b] = labels[idx[b]] (the DataLoader's
 * index sampling + default collate, train.py:490-491).  An index outside [0, n_pool) copies nothing.           */
int ustrun_aug_gather(const uint8_t* images, const uint8_t* labels, const int32_t* idx, int64_t n_pool, int32_t B,
                      int64_t img_bytes, int64_t lab_bytes, uint8_t* img_out, uint8_t* lab_out, ustrun_stream_t stream);
/* RandomScaleCrop (custom_transforms.py:529-550) + RandomCrop (:311-344): PIL resize((w, h), BILINEAR) of the image
 * (fixed-point two-tap triangle, horizontal then vertical pass, uint8 after each), resize(NEAREST) of the label, the
 * border of RandomCrop's padded branch (image 0, label `fill`), then the P x P window at (x1, y1).  Only the window
 * is sampled.  Row: {gate, w, h, pad, x1, y1, fill, 0}; gate 0 -> w = Ws, h = Hs (pad and the window still apply).
 * fill packs one byte per label channel, channel c = (fill >> 8c) & 255: PIL's reading of an integer colour.      */
int ustrun_aug_scale_crop(const uint8_t* img, const uint8_t* lab, const int32_t* params, int32_t stride, int32_t B,
                          int32_t Hs, int32_t Ws, int32_t C, int32_t Cl, int32_t P, uint8_t* img_out, uint8_t* lab_out,
                          ustrun_stream_t stream);
/* RandomScaleRotate (custom_transforms.py:507-526) with RandomHorizontalFlip (:387-397) folded into the output
 * address: PIL rotate(deg, BILINEAR) about the centre for the image (double arithmetic, truncation, 0 outside),
 * rotate(deg, NEAREST, fillcolor) for the label (PIL's 16.16 fixed-point walk).  Row: {gate, flip, fill, 0,
 * fixed a0..a5 (6 words), the affine matrix a..f as doubles (12 words)}: the host forms the matrix as PIL does.     */
int ustrun_aug_rotate(const uint8_t* img, const uint8_t* lab, const int32_t* params, int32_t stride, int32_t B,
                      int32_t H, int32_t W, int32_t C, int32_t Cl, uint8_t* img_out, uint8_t* lab_out,
                      ustrun_stream_t stream);
/* The displacement fields of elastic_transform (custom_transforms.py:207-225): two uniform(-1, 1) fields per gated
 * sample, each smoothed by a separable Gaussian (sigma = 0.08 H, radius int(4 sigma + 0.5), zeros outside; axis 0
 * first) and scaled by 2 H.  noise == NULL: the fields come from a counter-based hash of (seed, sample, field,
 * pixel) -- the reference draws them from an unseeded RandomState; noise != NULL (tests): [B][2][H][W] floats.
 * field, work: [B][2][H][W] floats each.  Row: {gate}.  H != W is an error (the reference's index convention is
 * only consistent for square patches).                                                                           */
int ustrun_aug_elastic_field(const float* noise, int64_t seed, const int32_t* params, int32_t stride, int32_t B,
                             int32_t H, int32_t W, float* field, float* work, ustrun_stream_t stream);
/* the generator's [B][2][H][W] values on their own (tests): what ustrun_aug_elastic_field smooths when noise == NULL */
int ustrun_aug_elastic_noise(int64_t seed, int32_t B, int32_t H, int32_t W, float* noise, ustrun_stream_t stream);
/* elastic_transform's resampling (custom_transforms.py:227-255): out[i][j] = in(i + field[b][0][i][j],
 * j + field[b][1][i][j]); image: scipy map_coordinates(order=1) of a uint8 array, constant 0 outside, rounded to
 * nearest (the result takes the input's dtype); label: order=0, mode='nearest'.  Row: {gate}.  H != W is an error. */
int ustrun_aug_elastic_warp(const uint8_t* img, const uint8_t* lab, const float* field, const int32_t* params,
                            int32_t stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Cl, uint8_t* img_out,
                            uint8_t* lab_out, ustrun_stream_t stream);
/* bytes of `work` ustrun_aug_strong needs */
int64_t ustrun_aug_strong_work_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
/* The strong view (train.py:453-457): ImageEnhance.Brightness (blend with black), ImageEnhance.Contrast (blend with
 * the grey int(mean(L) + 0.5) of the brightened image; one block per image, integer sum), GaussianBlur
 * (custom_transforms.py:78-118: / 255, reflection pad r, 2r + 1 taps down then across, * 255, truncated).
 * Row: {gate, brightness, contrast, sigma} (floats as bits); gate bit 0 = brightness and contrast, bit 1 = blur (the
 * reference applies all three: 3).  r < min(H, W), r <= 63.                                                        */
int ustrun_aug_strong(const uint8_t* img, const int32_t* params, int32_t stride, int32_t B, int32_t H, int32_t W,
                      int32_t C, int32_t r, uint8_t* img_out, void* work, int64_t work_bytes, ustrun_stream_t stream);
/* Normalize_tf + ToTensor (custom_transforms.py:650-684, :728-753): xw, xs [B][C][H][W] f32 = x / 127.5 - 1 of the
 * weak and the strong image (strong, xs may be NULL), y [B][H][W][Cl] f32 = the label's byte values.              */
int ustrun_aug_finish(const uint8_t* weak, const uint8_t* strong, const uint8_t* lab, int32_t B, int32_t H, int32_t W,
                      int32_t C, int32_t Cl, float* xw, float* xs, float* y, ustrun_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation overlays of `test.py --save_img` (csrc/render.hip).  The reference
 * draws them per image on the host in numpy / cv2 (utils/util.py:299-390, called at test.py:110-113);
 * here a batch is rendered on the device and three bytes per pixel reach the host.
 *   img [N][C][H][W] f32 (C = 1 or 3; one channel is repeated to three), out [N][H][W][3] uint8 RGB.
 *   pred / gt, by `kind`: 0 = f32 planes [N][P][H][W]; 1 = int64 labels [N][H][W], part i = label i + 1.
 *   H, W <= 8192, N <= 65535.
 * ---------------------------------------------------------------------------------------- */
/* range[n] = {min, max} of image n over all its channels (img.min() / img.max() of util.py:357,378-380).       */
int ustrun_render_range(const float* img, int32_t N, int32_t C, int32_t H, int32_t W, float* range,
                        ustrun_stream_t stream);
/* draw_mask_and_save (util.py:367-390): v = (img + 1) * 127.5 where the image's min < -0.5, else img * 255 where
 * its max < 1.5, else img (f32, each step rounded); a pixel of part i (kind 0: value == 1) takes colour_i =
 * {red, green, blue, yellow, magenta}[i] and factor 0.5, the lowest i winning; out = trunc((v + colour) * factor)
 * in double, clamped to 0..255 (the reference's cast is undefined outside that range).  P <= 5.                   */
int ustrun_render_mask(const float* img, const float* range, const void* pred, int32_t pred_kind, int32_t N, int32_t C,
                       int32_t P, int32_t H, int32_t W, uint8_t* out, ustrun_stream_t stream);
/* draw_contour_and_save (util.py:299-365): v = (img - min) / (max - min) * 255 (f32, each step rounded; 0 where
 * max == min, the reference has NaN there); for i = 0..P-1 the contour of pred part i in {green, blue, yellow,
 * magenta}[i], then that of gt part i in red, the last one drawn winning.  A contour pixel is a background pixel
 * (kind 0: value > 0 is foreground) with a foreground pixel among its 8 neighbours inside the image (cv2.dilate,
 * 3 x 3, minus the map).  out = v rounded half to even and clamped to 0..255 (cv2's saturating cast).  P <= 4.   */
int ustrun_render_contour(const float* img, const float* range, const void* pred, const void* gt, int32_t kind,
                          int32_t N, int32_t C, int32_t P, int32_t H, int32_t W, uint8_t* out, ustrun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* USTRUN_H */
