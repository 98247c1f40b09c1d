/*
 * acgan_hip.h — C ABI of libacgan_hip.so: the MI355X (gfx950) kernels behind the
 * Augmented CycleGAN training step of adrianalbert/domain-transfer-GAN.
 *
 * The reference has NO native layer: its hot path reaches the
 * device through torch.nn modules.  Each entry point below therefore cites the
 * reference call site(s) whose arithmetic it replaces (paths relative to
 * /root/reference/augmented_cyclegan/).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - plain C: pointers + ints, no torch types.  All pointers are DEVICE pointers
 *    owned by the caller; the library never allocates device memory, never
 *    synchronises, and only enqueues on `stream` (a hipStream_t passed as void*).
 *  - return 0 on success, a negative acg_status otherwise; acg_last_error()
 *    returns a thread-local message for the last failure on this thread.
 *  - activations are fp32 NHWC with the channel count padded to a multiple of 16
 *    ("C16"); padded channels hold zeros.  IMAGE tensors — up to 4 real channels: the
 *    networks' inputs and outputs (networks.py:159-160, 187-188, 321, 365, 445), their
 *    gradients, the PatchGAN maps — may be stored with 4 channels ("C4", 16 bytes per pixel)
 *    where they are the thin side of a thin layer: see acg_conv_desc.  Weights are passed in
 *    the packed forms produced by acg_pack_conv_weight().
 */
#ifndef ACGAN_HIP_H
#define ACGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACG_VERSION 118

typedef enum {
    ACG_OK = 0,
    ACG_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    ACG_ERR_WORKSPACE = -2, /* workspace too small */
    ACG_ERR_LAUNCH = -3,    /* hip launch error */
    ACG_ERR_COMM = -4       /* RCCL unavailable or an RCCL call failed */
} acg_status;

/* ACG_ACT_SIGMOID (--no_lsgan discriminator heads, networks.py:293,340,384,421): a convolution applies it to the REAL output
 * channels only (acg_conv_desc.Cor, required) and stores exactly 0 in the padded ones (sigmoid(0) = 0.5 would break the
 * zero-padding invariant); only acg_conv2d_fwd, acg_act_bwd and the dense layers take it. */
typedef enum {
    ACG_ACT_NONE = 0, ACG_ACT_RELU = 1, ACG_ACT_LRELU = 2 /* slope 0.2 */, ACG_ACT_TANH = 3, ACG_ACT_SIGMOID = 4
} acg_act;
typedef enum { ACG_PAD_ZERO = 0, ACG_PAD_REFLECT = 1 } acg_pad_mode;
typedef enum { ACG_IMPL_MFMA = 0, ACG_IMPL_DIRECT = 1 } acg_conv_impl;
typedef enum { ACG_PREC_F32 = 0, ACG_PREC_BF16 = 1, ACG_PREC_BF16X3 = 2 } acg_precision;

/* Geometry of one nn.Conv2d (or of the Conv2d whose adjoint an nn.ConvTranspose2d is).
 * Ci / Co are the STORED channel counts of the NHWC tensors: multiples of 16, or 4 for an image tensor (Cir resp. Cor <= 4)
 * on the thin side of a layer with K > 1 whose other side is wider — the layers whose kernels gather / write 4 channels per
 * pixel anyway.  Packed weights do not depend on it (acg_pack_conv_weight takes widths padded to 16). */
typedef struct {
    int N, Hi, Wi, Ci;
    int Ho, Wo, Co;
    int K, stride, pad, pad_mode;
    int Cir, Cor; /* REAL (unpadded) channel counts, 0 = unknown.  Cir <= 4 / Cor <= 4 select the thin-channel
                   * K-flattening (8 taps x 4 channels per 32-deep stage) in the fp32 kernels. */
} acg_conv_desc;

int acg_version(void);
const char *acg_last_error(void);
/* Name, template arguments included, of the convolution kernel the calling thread dispatched last (e.g.
 * "igemm_conv_x3_ws<REFLECT=1,STATS=1,ROWP=1>").  Diagnostic: the reference delegates algorithm choice to
 * torch.nn.Conv2d / cuDNN (networks.py:158-189) and cannot say what ran; bench.py labels its roofline with this. */
const char *acg_last_kernel(void);
/* Measurement hooks (bench.py; the reference has no counterpart — its timing is train.py:243's wall clock per image).
 * acg_debug_mid_event: `event` (a hipEvent_t) is recorded by the NEXT weight-gradient entry point of the calling thread
 * between its main kernel and its split-K reduction launch, then forgotten: the two are timed apart.
 * acg_probe_mfma_rate: enqueues a register-only v_mfma_f32_16x16x32_bf16 loop (`iters` x 16 MFMAs per wave, 8 waves per
 * CU, random operands, no LDS / memory traffic) and returns the FLOPs it executes in *flops_out; timed by the caller it
 * gives the matrix rate the device sustains in its present clock / power state (scratch: >= 512 floats per CU, never written). */
int acg_debug_mid_event(void *event);
int acg_probe_mfma_rate(float *scratch, size_t scratch_floats, int iters, double *flops_out, void *stream);
/* selects the convolution implementation for subsequent calls on this process
 * (MFMA implicit GEMM = product path; DIRECT = naive one-thread-per-output kernels kept
 * as an on-device cross-check).  Both are HIP kernels; there is no CPU path. */
int acg_set_conv_impl(int impl);
/* arithmetic of the MFMA convolution kernels (tensors stay fp32 in HBM in every mode):
 *  ACG_PREC_BF16X3 (default) each fp32 operand is split into bf16 hi + lo on its way into LDS and every product is
 *                  formed as lo*hi + hi*lo + hi*hi by three v_mfma_f32_32x32x16_bf16 with fp32 accumulation: operands
 *                  keep 16 mantissa bits (~4e-6 rms error per convolution), inside the 1e-3 parity bar, at bf16 rate;
 *  ACG_PREC_F32    exact fp32 FMA chain on v_mfma_f32_32x32x2_f32 — the strict mode;
 *  ACG_PREC_BF16   operands rounded to bf16, fp32 accumulate — throughput mode, NOT a parity path.
 * Packed weights must be re-packed (acg_pack_conv_weight) after a switch. */
int acg_set_conv_precision(int prec);

/* ---- data path (dataloader.py:17-35): raw[N,H,W,Craw] -> first C channels, NaN -> 0, per-sample / per-channel min-max
 *      scaling to [-1, 1] (constant planes -> 0), written NCHW.  Once per data set, on the device. ---- */
int acg_minmax_scale_nhwc_to_nchw(const float *raw, float *out_nchw, int N, int H, int W, int Craw, int C, void *stream);

/* ---- layout at the API edge (reference tensors are NCHW: dataloader.py:26, model.py:404) ---- */
int acg_nchw_to_nhwc16(const float *src, float *dst, int N, int C, int H, int W, int Cp, void *stream);
int acg_nhwc16_to_nchw(const float *src, float *dst, int N, int C, int H, int W, int Cp, void *stream);
/* torch.cat((a, b), 1) on C16 tensors — model.py:410, 472 */
int acg_concat_channels(const float *a, int Ca, int Cap, const float *b, int Cb, int Cbp, float *dst, int Cdp,
                        size_t npix, void *stream);
/* adjoint of the above: splits d(dst) into d(a), d(b) (either may be NULL) */
int acg_split_channels(const float *gdst, int Cdp, float *ga, int Ca, int Cap, float *gb, int Cb, int Cbp,
                       size_t npix, void *stream);

/* ---- weights: OIHW (torch layout, real channel counts Or x Ir) -> packed, zero padded ----
 * wf: [K*K][Ci/8][CoP][8]  (B operand of forward / ConvTranspose-backward GEMMs)
 * wb: [K*K][Co/8][CiP][8]  (B operand of data-gradient / ConvTranspose-forward GEMMs)
 * CoP = acg_ncols_pad(Co), CiP = acg_ncols_pad(Ci); Ci / Co here are widths padded to 16.  Either output may be NULL.
 * Size the buffers with acg_packed_w{f,b}_elems: some layers carry a second packed form behind the first. */
int acg_ncols_pad(int c);
size_t acg_packed_wf_elems(int K, int Ci, int Co);
size_t acg_packed_wb_elems(int K, int Ci, int Co);
int acg_pack_conv_weight(const float *w_oihw, int Or, int Ir, int K, int Ci, int Co, float *wf, float *wb, void *stream);
/* The regular (non-thin) layers of a whole network in ONE launch — the packed copies are refreshed once per optimiser step
 * (model.py:447-452, 510-515 `optimizer.step()` changes every weight), and one launch per layer was 68 five-microsecond
 * kernels per training step.  bf16 / bf16x3 arithmetic; a layer qualifies where acg_pack_conv_weights_multi_supported
 * (thin layers and the exact-fp32 mode keep acg_pack_conv_weight).  Same bytes as acg_pack_conv_weight writes. */
typedef struct {
    const float *w;      /* OIHW, real Or x Ir */
    float *wf, *wb;      /* acg_packed_w{f,b}_elems floats each */
    int Or, Ir, K, Ci, Co;
} acg_pack_item;
int acg_pack_conv_weights_multi_supported(int Or, int Ir, int K);
int acg_pack_conv_weights_multi(const acg_pack_item *items, int n, void *stream);
int acg_pad_vector(const float *src, int n, float *dst, int np, void *stream); /* bias -> C16 */

/* ---- nn.Conv2d forward (+bias, + fused activation) — networks.py:159-188, 211-243, 321-338,
 *      365-382, 445-471; modules.py:162,180,211,227 (reflection pad folded into the loader). */
int acg_conv2d_fwd(const acg_conv_desc *d, const float *x, const float *wf, const float *bias, float *y, int act,
                   void *stream);
/* acg_conv2d_fwd with act = NONE that also writes, from its epilogue, the per-tile partial statistics of y that the
 * InstanceNorm / CondInstanceNorm behind the convolution needs (modules.py:24-31, 46-55): stats[n][tile][{mean,M2}][Co]
 * over tiles of 128 consecutive output pixels, to be merged by acg_norm_stats_from_partials(rows_per_chunk = 128).
 * Supported (query first) for the bf16x3 128-column tile: Co >= 128, Ci % 32 == 0, Ho*Wo % 128 == 0. */
int acg_conv2d_fwd_stats_supported(const acg_conv_desc *d);
/* 1: every entry acg_conv2d_fwd_stats writes for d is the (mean, M2) of its own 128-pixel tile; 0: entries may be joint
 * statistics of several tiles whose grouping follows the batch (the row pipeline), so an image's merged statistics are not
 * bit-identical across batch sizes.  model.py:606-733's translations run group by group and must not depend on the grouping. */
int acg_conv2d_fwd_stats_per_tile(const acg_conv_desc *d);
int acg_conv2d_fwd_stats(const acg_conv_desc *d, const float *x, const float *wf, const float *bias, float *y,
                         float *stats, void *stream);
/* data gradient of the above (autograd of nn.Conv2d / ReflectionPad2d): dy -> dx.
 * Reflect padding needs a workspace for the padded gradient image. */
size_t acg_conv2d_bwd_data_workspace_bytes(const acg_conv_desc *d);
int acg_conv2d_bwd_data(const acg_conv_desc *d, const float *dy, const float *wb, float *dx, void *workspace,
                        size_t ws_bytes, void *stream);
/* dx = data gradient + addend (same shape as dx), fused into the convolution epilogue: the gradient arriving over a
 * ResnetBlock's skip connection (modules.py:185-188, 232-235) joins the gradient of the block's first convolution without
 * a separate element-wise pass.  Supported (query first) where the reflect data gradient takes its frame path. */
int acg_conv2d_bwd_data_add_supported(const acg_conv_desc *d);
int acg_conv2d_bwd_data_add(const acg_conv_desc *d, const float *dy, const float *wb, const float *addend,
                            const unsigned *addend_sign_mask, float *dx, void *ws, size_t ws_bytes, void *stream);
/* addend_sign_mask (may be NULL): acg_norm_apply's sign bitmask of the block output; only elements whose bit is set are
 * added, i.e. the skip gradient dy * (y > 0) is formed here from dy itself and never written to memory. */
/* dx = data gradient * (x > 0), x = this convolution's own INPUT when that input is the ReLU output of the layer in front
 * (ResnetBlock: pad-conv-ReLU-pad-conv, modules.py:211-227): dx is then the gradient w.r.t. that layer's PRE-activation and
 * its separate activation-backward pass is skipped (torch runs threshold_backward there).  Same support query as _add. */
int acg_conv2d_bwd_data_relu(const acg_conv_desc *d, const float *dy, const float *wb, const float *x, float *dx,
                             void *ws, size_t ws_bytes, void *stream);
/* ---- Pre-split ("S16") activation storage for the MFMA-bound 3x3 layers (the ResnetBlock / CINResnetBlock convolutions,
 * modules.py:139-235, in the bf16x3 arithmetic).  An S16 tensor has the shape and byte size of its fp32 NHWC twin; per pixel
 * and 8-channel group it holds 16 bytes of bf16 hi (RNE of x) followed by 16 bytes of bf16 lo (RNE of x - hi): the operand
 * form the convolutions split every fp32 value into inside their loaders otherwise.  Written once by the producer of an
 * activation (norm apply, convolution epilogue), it lets both operands of the convolution travel global -> LDS by LDS-DMA.
 * acg_conv2d_s16_supported: forward, data gradient and weight gradient of this layer all take S16 operands. */
int acg_s16_encode(const float *x, void *y_s16, size_t n, void *stream);   /* n elements, n % 8 == 0 */
int acg_s16_decode(const void *x_s16, float *y, size_t n, void *stream);   /* y = hi + lo */
int acg_conv2d_s16_supported(const acg_conv_desc *d);
/* x S16; y fp32, or S16 when out_s16 != 0; stats (may be NULL): the per-tile statistics of acg_conv2d_fwd_stats (fp32 y,
 * act NONE only) */
int acg_conv2d_fwd_s16(const acg_conv_desc *d, const void *x_s16, const float *wf, const float *bias, void *y, int act,
                       float *stats, int out_s16, void *stream);
/* dy S16.  out_s16 == 0: dx fp32, optional addend (+ sign bitmask) as acg_conv2d_bwd_data_add.  out_s16 != 0: dx S16,
 * optional relu_src_s16 as acg_conv2d_bwd_data_relu (the convolution's own S16 input; only its sign is read). */
int acg_conv2d_bwd_data_s16(const acg_conv_desc *d, const void *dy_s16, const float *wb, void *dx, void *ws, size_t ws_bytes,
                            const float *addend, const unsigned *addend_sign_mask, const void *relu_src_s16, int out_s16,
                            void *stream);
/* ... that also produces the first pass of the backward of the (Cond)InstanceNorm whose OUTPUT gradient dx is
 * (modules.py:83-97, 121-131: y = act(norm(x) * gamma + beta [+ res]); fp32 dx only): per 128-pixel tile of dx the sums
 * part[((n * (Hi*Wi/128) + tile) * 2 + {0, 1}) * Ci + c] = (sum gy, sum gy * xhat), gy = dx * act'(y), xhat = (x - mean) *
 * rstd — what acg_norm_bwd computes in a pass of its own over dx and x; hand them to acg_norm_bwd_partials.  The activation
 * mask comes from sign_mask (the bitmask acg_norm_apply stored) or, when that is NULL, is recomputed from x with gamma /
 * beta (gstride 0 or Ci); act NONE or RELU. */
typedef struct acg_norm_sums {
    const float *x, *mean, *rstd;     /* the norm's input (N,Hi,Wi,Ci) and its statistics [N*Ci] */
    const float *gamma, *beta;        /* read only when act != NONE and sign_mask == NULL */
    int gstride;
    const unsigned *sign_mask;
    int act;
    float *part;
} acg_norm_sums;
int acg_conv2d_bwd_data_s16_sums_supported(const acg_conv_desc *d);
int acg_conv2d_bwd_data_s16_sums(const acg_conv_desc *d, const void *dy_s16, const float *wb, float *dx, void *ws,
                                 size_t ws_bytes, const float *addend, const unsigned *addend_sign_mask,
                                 const acg_norm_sums *ns, void *stream);
/* ... and on fp32 operands: the persistent row pipeline (zero-padded 3x3 stride 1, Co == 32, Ci == 64, Wi % 128 == 0), and
 * from round 6 the generic row-patch tile (3x3 stride 1, Ci == 32, Co == 64, Wi % 128 == 0), the four-phase tile of the stride-2
 * 3x3 layer (Ci == 64, Wo % 128 == 0) and the thin-row kernel of the 7x7 head (Ci == 32, a C4 image on the output side, Hi % 8 == 0, Wi % 16 == 0).  ns->sign_mask must be NULL (the activation
 * mask is recomputed from ns->x); part[N][Hi * Wi / 128][2][Ci], every entry written. */
int acg_conv2d_bwd_data_sums_supported(const acg_conv_desc *d);
int acg_conv2d_bwd_data_sums(const acg_conv_desc *d, const float *dy, const float *wb, float *dx, void *ws, size_t ws_bytes,
                             const acg_norm_sums *ns, void *stream);
/* conv + ReLU with S16 output that also stores (y > 0) as a sign bitmask (layout of acg_norm_apply's: bit e % 32 of word e / 32
 * for float index e; Co % 32 == 0), and the S16-output data gradient of the convolution BEHIND it masked by that bitmask
 * instead of by the sign of its S16 input (where acg_conv2d_bwd_data_s16_sums_supported(d)): the pad-conv-ReLU-pad-conv chain
 * of modules.py:211-227 without reading the activation a second time */
int acg_conv2d_fwd_s16_mask(const acg_conv_desc *d, const void *x_s16, const float *wf, const float *bias, void *y_s16,
                            unsigned *sign_mask, void *stream);
int acg_conv2d_bwd_data_s16_mask(const acg_conv_desc *d, const void *dy_s16, const float *wb, void *dx_s16, void *ws,
                                 size_t ws_bytes, const unsigned *relu_sign_mask, void *stream);
/* x and dy S16; dw / db as acg_conv2d_bwd_weight */
int acg_conv2d_bwd_weight_s16(const acg_conv_desc *d, const void *x_s16, const void *dy_s16, float *dw, float *db, int Or,
                              int Ir, void *ws, size_t ws_bytes, int accumulate, void *stream);
/* weight (+bias) gradient: x, dy -> dw in torch OIHW layout (Or x Ir real channels), db[Or] (may be NULL).
 * Deterministic split-K over pixels with a second-stage reduction (no atomics).  accumulate != 0: the result is ADDED to
 * dw / db — pass the parameter's .grad (what autograd's AccumulateGrad does after loss.backward(), model.py:445, 509,
 * with one extra element-wise kernel per parameter); 0: dw / db are overwritten. */
size_t acg_conv2d_bwd_weight_workspace_bytes(const acg_conv_desc *d);
int acg_conv2d_bwd_weight(const acg_conv_desc *d, const float *x, const float *dy, float *dw_oihw, float *db,
                          int Or, int Ir, void *workspace, size_t ws_bytes, int accumulate, void *stream);

/* ---- nn.ConvTranspose2d(k3,s2,p1,op1) — networks.py:178-179, 231-234.  `d` describes the
 *      Conv2d it is the adjoint of (Hi,Wi,Ci = the LARGE side = ConvTranspose output). ---- */
int acg_conv_transpose2d_fwd(const acg_conv_desc *d, const float *x, const float *wb, const float *bias, float *y,
                             int act, void *stream);
/* ... that also emits the per-tile statistics of acg_conv2d_fwd_stats for an InstanceNorm behind the transposed convolution
 * (networks.py:178-181, 231-236): stats [N][Hi*Wi/128][2][Ci], Hi x Wi x Ci = the transposed convolution's OUTPUT. */
int acg_conv_transpose2d_fwd_stats_supported(const acg_conv_desc *d);
int acg_conv_transpose2d_fwd_stats(const acg_conv_desc *d, const float *x, const float *wb, const float *bias, float *y,
                                   float *stats, void *stream);
int acg_conv_transpose2d_bwd_data(const acg_conv_desc *d, const float *dy, const float *wf, float *dx, void *stream);
int acg_conv_transpose2d_bwd_weight(const acg_conv_desc *d, const float *x, const float *dy, float *dw_oihw,
                                    float *db, int Or, int Ir, void *workspace, size_t ws_bytes, int accumulate,
                                    void *stream);

/* ---- normalisation: InstanceNorm (modules.py:64-97, biased var), CondInstanceNorm
 *      (modules.py:104-132, UNBIASED var, per-sample affine), BatchNorm2d/1d train mode
 *      (networks.py:407-415, 450-466).  Tensor viewed as [G groups][P pixels][C]:
 *      IN/CIN: G=N, P=H*W;  BN: G=1, P=N*H*W. ---- */
size_t acg_norm_workspace_bytes(int G, size_t P, int C);
/* mean[G*C], rstd[G*C]; unbiased!=0 selects var*P/(P-1).  If run_mean/run_var are non-NULL
 * (BatchNorm) they are updated with momentum (running_var takes the unbiased variance). */
int acg_norm_stats(const float *x, int G, size_t P, int C, float eps, int unbiased, float *mean, float *rstd,
                   float *run_mean, float *run_var, float momentum, void *workspace, size_t ws_bytes, void *stream);
/* the same statistics from per-chunk (mean, M2) partials a producer already holds (acg_conv2d_fwd_stats), merged with
 * Chan's formula; x is not read.  part[((g*nchunks + chunk)*2 + {0,1})*C + c], nchunks = ceil(P / rows_per_chunk). */
int acg_norm_stats_from_partials(const float *part, int G, size_t P, int C, int rows_per_chunk, float eps, int unbiased,
                                 float *mean, float *rstd, void *stream);
/* BatchNorm eval mode: mean/rstd (length Cp) from the running buffers (length C) */
int acg_bn_eval_stats(const float *run_mean, const float *run_var, int C, int Cp, float eps, float *mean, float *rstd,
                      void *stream);
/* y = act((x-mean)*rstd*gamma + beta [+ res]); gamma/beta indexed [g*gstride + c]: gstride 0 (shared), C, or any row stride
 * >= C that is a multiple of 4 (a column block of a wider [G][gstride] matrix).
 * Every norm entry point rejects (-1 and acg_last_error, nothing is launched) C % 4 != 0, C > 1024 (one workgroup row of
 * 256 float4), G > 65535 and G, P or C of 0.  On top of that:
 *   acg_norm_stats / acg_norm_stats_from_partials: unbiased != 0 with P < 2; acg_norm_stats: running statistics with G != 1.
 *   acg_norm_apply: a gstride below C or not a multiple of 4; ACG_ACT_SIGMOID; fmt != 0 with anything but ReLU or with
 *     C % 8 != 0; fmt 1 / 3 without res; sign_mask without res, with an activation other than ReLU / LeakyReLU, or with
 *     P*C/4 % 8 != 0 (just outside: P = 63, C = 16).  fmt 2 takes an fp32 res (and a sign_mask) like fmt 0.
 *   acg_norm_bwd / acg_norm_bwd_partials: tanh / sigmoid (no norm of the networks is followed by one); dx_s16 with dres,
 *     with an activation other than ReLU, with C % 8 != 0 or with y given and no sign_mask; accumulate with gstride != 0;
 *     nparam outside 0..C; a gstride below C or not a multiple of 4; an activation with neither y, sign_mask nor beta;
 *     sign_mask with P*C/4 % 8 != 0; acg_norm_bwd_partials without partials.  unbiased == 1 with P < 2 is NOT checked
 *     here (the statistics call before it refuses it).
 *   acg_norm_bwd_sums / acg_norm_bwd_apply (the SyncBN halves): an activation without y; acg_norm_bwd_sums a short
 *     workspace (-2).  They do NOT reject tanh (it is dispatched: 1 - y^2), take ACG_ACT_SIGMOID for no activation,
 *     and do not check Ptot. */
int acg_norm_apply(const float *x, const float *mean, const float *rstd, const float *gamma, const float *beta,
                   int gstride, const float *res, float *y, unsigned *sign_mask, int G, size_t P, int C, int act, int fmt,
                   void *stream);
/* fmt: 0 = fp32 tensors; bit 1 set: y is written pre-split (S16, see acg_s16_encode), bit 0 set: res is read pre-split
 * (fmt 2 or 3; ReLU, C % 8 == 0): the producer of a residual-block activation writes the operand form of the next
 * convolution once, instead of every convolution loader splitting it again.  fmt 1 (res pre-split, y fp32) is the output
 * norm of the LAST block of a trunk: the layer behind it reads fp32, so no acg_s16_decode pass is needed. */
/* sign_mask (may be NULL; needs res, ReLU/LeakyReLU, P*C/4 % 8 == 0): ceil(G*P*C/32) words, bit e%32 of word e/32 =
 * (y[e] > 0).  acg_norm_bwd takes it in place of y: the backward of ReLU(x + IN(conv(..))) (modules.py:185-188, 232-235)
 * needs only the sign of y, and reads 1/32 of a tensor instead of the tensor, twice. */
/* backward: dy (w.r.t. y), y, x -> dx, dres (if has_res; = dy*act'(y)), dgamma/dbeta.
 * gstride == 0 (InstanceNorm / BatchNorm): dgamma/dbeta hold the first `nparam` (real, unpadded) channels, summed over the
 * groups; accumulate != 0 ADDS them to the destination (pass the parameter's .grad: no separate accumulation kernel).
 * gstride == C (CondInstanceNorm): dgamma/dbeta are [G*C] (gradients of the per-sample scale / shift), nparam and accumulate
 * are ignored (must be 0).  y may be NULL when no residual was added: the activation mask is then recomputed from x with
 * gamma/beta (one tensor stream less per pass).  unbiased as in acg_norm_stats; unbiased == 2 means the statistics were
 * constants (BatchNorm eval mode): dx = gamma*rstd*dy*act'. */
int acg_norm_bwd(const float *dy, const float *y, const unsigned *sign_mask, const float *x, const float *mean,
                 const float *rstd,
                 const float *gamma, const float *beta, int gstride, float *dx, float *dres, float *dgamma, float *dbeta,
                 int nparam, int accumulate, int G, size_t P, int C, int act, int unbiased, int dx_s16, void *workspace,
                 size_t ws_bytes, void *stream);
/* dx_s16 != 0: dx is written pre-split (S16) for the convolution gradients that consume it (ReLU, no dres, C % 8 == 0) */
/* the same with the first pass already done: part[((g * nchunks + chunk) * 2 + {0, 1}) * C + c] partial sums over any
 * partition of the P rows into nchunks chunks (acg_conv2d_bwd_data_s16_sums: 128-pixel tiles) */
int acg_norm_bwd_partials(const float *dy, const float *y, const unsigned *sign_mask, const float *x, const float *mean,
                          const float *rstd, const float *gamma, const float *beta, int gstride, float *dx, float *dres,
                          float *dgamma, float *dbeta, int nparam, int accumulate, int G, size_t P, int C, int act,
                          int unbiased, int dx_s16, const float *part, int nchunks, void *workspace, size_t ws_bytes,
                          void *stream);

/* the two halves of acg_norm_bwd, for SyncBN: local sums[(g*2+{0,1})*C+c] = (sum gy, sum gy*xhat), then — after the
 * caller has all-reduced them — the apply pass with the GLOBAL pixel count Ptot. */
int acg_norm_bwd_sums(const float *dy, const float *y, const float *x, const float *mean, const float *rstd, float *sums,
                      int G, size_t P, int C, int act, void *workspace, size_t ws_bytes, void *stream);
int acg_norm_bwd_apply(const float *dy, const float *y, const float *x, const float *mean, const float *rstd,
                       const float *gamma, int gstride, const float *sums, float *dx, float *dres, int G, size_t P,
                       size_t Ptot, int C, int act, int unbiased, void *stream);

/* out = x where the sign-bitmask bit (acg_norm_apply layout) is set, else 0 — the materialised form of a masked skip
 * gradient, for the paths that cannot fuse it (n % 4 == 0) */
int acg_mask_apply(const float *x, const unsigned *sign_mask, float *out, size_t n, void *stream);
/* nn.Dropout(p), training mode (replaces modules.py:167-168, 214-215 `nn.Dropout(0.5)` behind the first ReLU of a residual
 * block): out = keep ? x * scale : 0, scale = 1 / (1 - p); the Bernoulli(1 - p) draw is GIVEN, one bit per element in the
 * sign-bitmask layout (bit e % 32 of word e / 32), so forward and backward (the same call on the gradient) share it and a
 * test can inject it.  n % 4 == 0. */
int acg_dropout_apply(const float *x, const unsigned *keep_bits, float scale, float *out, size_t n, void *stream);

/* ---- elementwise ---- */
int acg_act_bwd(const float *dy, const float *y, float *dx, size_t n, int act, void *stream); /* dx = dy*act'(y) */

/* ---- small dense layers: nn.Linear (networks.py:406-418), the 1x1 convs on the (N,nl,1,1) latent
 *      inside CondInstanceNorm (modules.py:111-118).  y[N][Op] = act(x[N][I] W[O][I]^T + b); columns
 *      O..Op-1 are written as zeros. ---- */
int acg_linear_fwd(const float *x, const float *w, const float *b, float *y, int N, int I, int ldx, int O, int Op,
                   int act, void *stream);
/* g = dy*act'(y) is applied inside; dx may be NULL; dw[O][I], db[O] are overwritten */
int acg_linear_bwd(const float *dy, const float *y, const float *x, const float *w, float *dx, float *dw, float *db,
                   int N, int I, int ldx, int O, int Op, int act, void *stream);
/* dst[s][i] (+)= src[off[s] + i] for i < len[s], every segment in ONE launch: hands the slices of a concatenated gradient
 * (the scale / shift layers of all CondInstanceNorms of a generator run as one dense layer, networks.py:98-132) to the
 * layers' own gradient tensors.  accumulate != 0 adds (the parameter's .grad), 0 overwrites. */
#define ACG_MAX_SEGMENTS 96
typedef struct acg_segments {
    void *dst[ACG_MAX_SEGMENTS];
    int off[ACG_MAX_SEGMENTS], len[ACG_MAX_SEGMENTS];
    int n;
} acg_segments;
int acg_segments_accumulate(const float *src, const acg_segments *segs, int accumulate, void *stream);

/* ---- DiscriminatorLatent (networks.py:396-433) fused: Linear(I->H) BatchNorm1d LeakyReLU(0.2), two more H->H stages, then
 *      Linear(H->1), BatchNorm in train mode (batch statistics; running buffers updated when non-NULL).  One launch per
 *      direction; the batch must fit one workgroup's LDS (acg_latent_mlp_supported), else use acg_linear_* + acg_norm_*.
 *      w[l] are torch nn.Linear weights [out][in]; z is [N][ldz] with I valid columns; out is [N][4] (column 0 = the
 *      prediction).  a_save [3][N][H] and stats_save [3][2][H] carry the pre-norm activations and (mean, rstd) to the
 *      backward pass.  Gradient pointers may be NULL; accumulate != 0 adds to them (parameter .grad). ---- */
typedef struct {
    const float *w[4], *b[4], *gamma[3], *beta[3];
    float *run_mean[3], *run_var[3];
    int head_act;   /* ACG_ACT_NONE, or ACG_ACT_SIGMOID (use_sigmoid, networks.py:421): out = sigmoid(Linear(H->1)) */
} acg_latent_mlp_params;
typedef struct {
    float *dw[4], *db[4], *dgamma[3], *dbeta[3];
} acg_latent_mlp_grads;
int acg_latent_mlp_supported(int N, int I, int H);
int acg_latent_mlp_fwd(const acg_latent_mlp_params *params, const float *z, int ldz, int N, int I, int H, float eps,
                       float momentum, float *a_save, float *stats_save, float *out, void *stream);
/* out: the forward's output, read when head_act is ACG_ACT_SIGMOID (dout * out * (1 - out)); may be NULL otherwise */
int acg_latent_mlp_bwd(const acg_latent_mlp_params *params, const acg_latent_mlp_grads *grads, const float *z, int ldz, int N,
                       int I, int H, const float *a_save, const float *stats_save, const float *out, const float *dout, float *dz,
                       int accumulate, void *stream);

/* ---- spatial mean over H*W of a C16 map -> [N][Cp] (LatentEncoder extension for S != 64,
 *      identity at the reference's 1x1 map — networks.py:482) ---- */
int acg_spatial_mean_fwd(const float *x, float *y, int N, size_t P, int Cp, void *stream);
int acg_spatial_mean_bwd(const float *dy, float *dx, int N, size_t P, int Cp, void *stream);

/* ---- losses: results are written to device scalars (no host sync) ----
 * tensors are C16; only channels < C count.  out[0] = mean((p-target)^2)  (model.py:65-70) */
size_t acg_reduce_workspace_bytes(size_t n);
int acg_mse_const_fwd(const float *p, size_t npix, int C, int Cp, float target, float *out, void *workspace,
                      size_t ws_bytes, void *stream);
int acg_mse_const_bwd(const float *p, size_t npix, int C, int Cp, float target, const float *gout, float *dp,
                      void *stream);
/* out[0] = F.binary_cross_entropy(p, full(target)) = mean(-(t max(log p, -100) + (1 - t) max(log(1 - p), -100))), p a
 * probability (sigmoid head), target 0 or 1 as a FLOAT (the reference's Long target, model.py:59-63, is rejected by torch).
 * Same partial-sum tree as acg_mse_const_fwd: deterministic, no atomics.  Backward (torch's formula):
 * dp = gout (p - t) / max(p (1 - p), 1e-12) / (npix C); padded channels get 0. */
int acg_bce_const_fwd(const float *p, size_t npix, int C, int Cp, float target, float *out, void *workspace,
                      size_t ws_bytes, void *stream);
int acg_bce_const_bwd(const float *p, size_t npix, int C, int Cp, float target, const float *gout, float *dp,
                      void *stream);
/* out[0] = mean(|a-b|) (F.l1_loss, model.py:391,468,486,494) */
int acg_l1_fwd(const float *a, const float *b, size_t npix, int C, int Cp, float *out, void *workspace,
               size_t ws_bytes, void *stream);
int acg_l1_bwd(const float *a, const float *b, size_t npix, int C, int Cp, const float *gout, float *da, float *db,
               void *stream);
/* out[0] = mean(x) over valid channels (P_t_A ... monitors, model.py:522-523) */
int acg_mean_fwd(const float *x, size_t npix, int C, int Cp, float *out, void *workspace, size_t ws_bytes,
                 void *stream);

/* ---- the variational bound of the offline evaluator (evaluate.py:93-122 — also run by train.py every epoch —,
 *      test.py:137-175 train_logvar / the MVGauss baseline, test.py:111-121 eval_bpp_MVGauss_B) ----
 * x, mu: (N, npix, Cp) NHWC image tensors (C4 for the networks' images), C channels valid, Cp a multiple of 4, 16-byte
 * aligned; logvar: ONE (npix, Cp) plane broadcast over the batch.
 * acg_pixel_nll_fwd: out[n] = -sum over pixels and valid channels of log p(x | mu, logvar) — ACG_NLL_LAPLACE
 * 0.5 lv + |x - mu| / exp(0.5 lv) + log 2 (log_prob_laplace, model.py:24-28), ACG_NLL_GAUSSIAN
 * 0.5 lv + (x - mu)^2 / (2 exp(lv)) + 0.5 log 2 pi (log_prob_gaussian, model.py:31-34).  Per-block partials in the workspace
 * (acg_pixel_nll_workspace_bytes), folded in a fixed order: deterministic, no atomics.
 * acg_pixel_nll_bwd: gradients of sum_n g[n] out[n] (g: N device floats).  dmu (N, npix, Cp) per element, one launch as wide
 * as the tensor; dlogvar (npix, Cp) summed over the batch by one thread per pixel walking n in order, a launch of its own only
 * when asked for.  Either may be NULL; padded channels get exactly 0;
 * the Laplace gradient takes sign(0) = 0 (torch's abs backward). */
typedef enum { ACG_NLL_LAPLACE = 0, ACG_NLL_GAUSSIAN = 1 } acg_nll_kind;
size_t acg_pixel_nll_workspace_bytes(int N, size_t npix);
int acg_pixel_nll_fwd(int kind, const float *x, const float *mu, const float *logvar, int N, size_t npix, int C, int Cp,
                      float *out, void *workspace, size_t ws_bytes, void *stream);
int acg_pixel_nll_bwd(int kind, const float *x, const float *mu, const float *logvar, int N, size_t npix, int C, int Cp,
                      const float *g, float *dmu, float *dlogvar, void *stream);
/* One iterate's latent tail of the bound (evaluate.py:93-122), one workgroup, on (N, L) row-major tensors:
 *  1-2. kld[n] of the current (mu, logvar) (kld_std_guss, model.py:45-53); trace_row[0..2] = mean over n of
 *       nll[n] + kld[n] + npx log 127.5, mean kld, and that bound / (npx log 2) (bits per pixel).  nll: acg_pixel_nll_fwd's out.
 *  3. the gradients of that mean bound w.r.t. mu and logvar: dz is d mean_n(nll[n]) / dz for z = clamp(eps exp(0.5 logvar) + mu,
 *     -4, 4) (gauss_reparametrize, model.py:15-22; eps: the draw z was made with), passed where -4 <= pre-clamp <= 4 inclusive
 *     (torch's clamp backward), plus the KLD's term / N.
 *  4. torch.optim.RMSprop (no momentum, not centred) on mu and logvar in place; sq_mu / sq_logvar: its square averages, held by
 *     the caller (zeros before the first step).
 *  5. z_next = clamp(eps_next exp(0.5 logvar) + mu, -4, 4) from the updated parameters (eps_next and z_next both NULL: none).
 * dz NULL: steps 1-4 are skipped (the first iterate's code from the initial parameters).  trace_row may be NULL. */
int acg_latent_bound_step(int N, int L, int npx, float *mu, float *logvar, float *sq_mu, float *sq_logvar, const float *eps,
                          const float *dz, const float *nll, float lr, float alpha, float rms_eps, float *trace_row,
                          const float *eps_next, float *z_next, void *stream);

/* ---- ensemble statistics of M translations per input (model.translate_ensemble, test.py --metric ensemble) ----
 * x: members (N*M, npix, Cp) NHWC fp32, member m of input n at row n*M + m; y: the paired target (N, npix, Cp) or NULL.
 * Cp is the stored width (4 for C4 images, else a multiple of 16), C <= Cp valid channels; padded channels are ignored.
 * q: nq quantile levels in HOST memory (read before the launch, passed by value), sorted inside [0, 1].  1 <= M <= 64,
 * 1 <= nq <= 8.  Per cell (input, pixel, channel), members sorted x_(1..M):
 *   mean, stdev (unbiased, 0 when M = 1): (N, C, npix) NCHW;  quant: numpy's linear rule, (N, nq, C, npix);
 *   crps_map: E1 - E2/2 with E1 = mean |x_i - y|, E2 = mean over pairs |x_i - x_j| (sorted form), (N, C, npix), needs y;
 *   sums (N, 6): per input over its C*npix cells sum E1, sum E2, sum (mean - y)^2, sum stdev^2, count of cells with the lowest
 *     quantile <= y <= the highest, the cell count; needs y;
 *   rank_hist (N, M + 1): cells per rank #{x_i < y} + floor(#{x_i = y} / 2); needs y.
 * Every output may be NULL.  The float sums fold per-block partials of the workspace (acg_ensemble_workspace_bytes; needed
 * only with y) in a fixed order: deterministic, no float atomics. */
size_t acg_ensemble_workspace_bytes(int N, size_t npix);
int acg_ensemble_stats(const float *x, const float *y, int N, int M, size_t npix, int C, int Cp, const float *q, int nq,
                       float *mean, float *stdev, float *quant, float *crps_map, float *sums, unsigned *rank_hist,
                       void *workspace, size_t ws_bytes, void *stream);

/* ---- radially averaged power spectra (model.translate_spectrum, test.py --metric spectrum; no reference call site: the
 *      reference has no spectral code, tests/spectrum_ref.py states the definition) ----
 * x: rows x C real fields of S x S fp32 pixels; pixel (h, w) of channel c of row r is x[r row_stride + c chan_stride +
 * (h S + w) pix_stride] (strides in floats): NHWC with Cp stored channels is (S S Cp, Cp, 1) - padded channels are never
 * read into a result - and planar NCHW is (C S S, 1, S S).  S: a power of two, 16 .. 1024; anything else is refused before a
 * launch.  Per field F = fft2(x) (unnormalised, no taper, no mean removal), P = |F|^2 / S^2; with signed integer wavenumbers
 * (fx, fy) and s = fx^2 + fy^2 the cell's bin is 0 for s = 0, else the largest b with b (b - 1) < s (sqrt(s) rounded to
 * nearest); psd (rows, C, S/2 + 1): the mean of P over the cells of bins 0 .. S/2, the corners beyond are dropped.
 * fp32 transform, ring sums in double in a fixed order: deterministic, no float atomics, the same bits for every layout.
 * S <= 128 needs no workspace (one workgroup per field, nothing but psd is written); above, the workspace
 * (acg_radial_spectrum_workspace_bytes, 16-byte aligned) holds the half spectrum between the row and the column pass. */
size_t acg_radial_spectrum_workspace_bytes(int rows, int C, int S);
int acg_radial_spectrum(const float *x, int rows, int C, int S, long long row_stride, int pix_stride, long long chan_stride,
                        float *psd, void *workspace, size_t ws_bytes, void *stream);
/* The data gradient of the above (ops.RadialSpectrum, ops.spectral_loss): g (rows, C, S/2 + 1) is the cotangent of psd,
 * gx = d sum_b g[b] psd[b] / dx = 2 Re ifft2(w F) per field, w[ky, kx] = g[bin] / count[bin] by the same integer ring rule
 * (0 in the dropped corners), ifft2 normalised by 1 / S^2.  x, its strides, S and the refusals are the forward's; gx has the
 * layout of x and must not alias it.  Cp: the channels stored per pixel of gx, channels C .. Cp - 1 are written as 0 (NHWC:
 * Cp = pix_stride; planar: Cp = C).  The inverse transform is the forward's Stockham stages on conj(w F), all inside the
 * packed half spectrum; the ring cell counts come from the integer rule (a launch of their own into the head of the
 * workspace).  Deterministic, no float atomics, the same bits for every layout.  S <= 128: one workgroup per field; above:
 * the forward's row pass, a column pass per tile and an inverse row pass through the half spectrum in the workspace
 * (acg_radial_spectrum_bwd_workspace_bytes, never 0, 16-byte aligned). */
size_t acg_radial_spectrum_bwd_workspace_bytes(int rows, int C, int S);
int acg_radial_spectrum_bwd(const float *x, const float *g, int rows, int C, int Cp, int S, long long row_stride,
                            int pix_stride, long long chan_stride, float *gx, void *workspace, size_t ws_bytes, void *stream);
/* Paired cross-spectra (ops.cross_spectrum, model.translate_coherence, test.py --metric coherence; tests/cross_spectrum_ref.py
 * states the definition): row r of x pairs with row r / x_per_y of y, channel by channel (x_per_y ensemble members share one
 * truth; rows % x_per_y must be 0).  With X = fft2(x), Y = fft2(y) as above, out (rows, C, 3, S/2 + 1) holds the ring means of
 * Pxx = |X|^2 / S^2, Pyy = |Y|^2 / S^2 and the co-spectrum Cxy = Re(X conj Y) / S^2, in that order, by the ring rule of
 * acg_radial_spectrum.  The quadrature part Im(X conj Y) sums to 0 over every ring of two real fields and is no output.  Each
 * operand has its own strides (their meaning, S and the refusals are acg_radial_spectrum's); padded channels are never read
 * into a result.  Each field is transformed as acg_radial_spectrum transforms it (the two never share a complex transform:
 * a faint field keeps its own accuracy beside a strong one); the products are formed per cell.  fp32 transform, ring sums in double
 * in a fixed order: deterministic, no float atomics, the same bits for every layout.  S <= 64 needs no workspace (one
 * workgroup per pair); above, the workspace (acg_cross_spectrum_workspace_bytes, 16-byte aligned) holds both half spectra of
 * every pair between the row and the column pass. */
size_t acg_cross_spectrum_workspace_bytes(int rows, int C, int S);
int acg_cross_spectrum(const float *x, const float *y, int rows, int x_per_y, int C, int S, long long x_row_stride,
                       int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                       long long y_chan_stride, float *out, void *workspace, size_t ws_bytes, void *stream);
/* Whole-field spectra (ops.field_spectrum, ops.field_cross_spectrum, model.translate_field_spectrum, test.py --metric
 * field_spectrum; tests/field_spectrum_ref.py states the definition): the two above for fields of any H x W with both extents
 * in 16 .. 1024.  Pixel (h, w) sits at (h W + w) pix_stride; the strides, x_per_y and the outputs' order mean what they mean
 * above.  F = fft2(x), P = |F|^2 / (H W); with L = min(H, W) and signed wavenumbers (fy, fx) the cell's bin is 0 for
 * fy = fx = 0, else the largest b with b (b - 1) H^2 W^2 < L^2 (fy^2 W^2 + fx^2 H^2): the radius L sqrt((fy/H)^2 + (fx/W)^2)
 * rounded to nearest, in int64.  nb = L/2 + 1 bins, psd (rows, C, nb), out (rows, C, 3, nb); the cells beyond are dropped.
 * H = W = S a power of two is forwarded to acg_radial_spectrum / acg_cross_spectrum: their bits, their workspace.  Otherwise
 * four launches on the stream: the chirps and transformed filters of the axes that are no power of two into the head of the
 * workspace (nothing is cached between calls), a row pass (two real rows per complex transform -> half spectra of W/2 + 1
 * columns), a column pass (-> weighted products per cell) and the ring sums.  A length that is no power of two is Bluestein's
 * chirp-z on radix-2 Stockham stages of the power of two M >= 2 N - 1 (M <= 2048), the chirp's arguments reduced mod 2 N in
 * integers; the axes choose independently.  fp32 transform, ring sums in double in a fixed order: deterministic, no float
 * atomics, the same bits for every layout, and Pxx of a pair has the bits of acg_field_spectrum(x).  acg_last_kernel names the
 * path and each axis' M.  Refused before any launch with ACG_ERR_INVALID: an extent outside 16 .. 1024, C < 1, rows < 1, a
 * stride < 1, rows % x_per_y != 0, a null tensor, a workspace off the 16-byte grid; a short workspace: ACG_ERR_WORKSPACE. */
size_t acg_field_spectrum_workspace_bytes(int rows, int C, int H, int W);
int acg_field_spectrum(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                       float *psd, void *workspace, size_t ws_bytes, void *stream);
size_t acg_field_cross_spectrum_workspace_bytes(int rows, int C, int H, int W);
int acg_field_cross_spectrum(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                             int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                             long long y_chan_stride, float *out, void *workspace, size_t ws_bytes, void *stream);

/* ---- neighbourhood fractions skill scores (ops.fss, model.translate_fss, test.py --metric fss; no reference call site: the
 *      reference has no verification code, tests/fss_ref.py states the definition; Roberts & Lean 2008) ----
 * x: rows x C fields of H x W fp32 cells, y: rows / x_per_y x C paired truths; row r of x pairs with row r / x_per_y of y
 * (x_per_y ensemble members share one truth).  The strides (in floats) mean what they mean in acg_cross_spectrum: NHWC with
 * Cp stored channels is (H W Cp, Cp, 1) - padded channels never reach a result - and planar NCHW is (C H W, 1, H W); each
 * operand has its own.  thr: (C, T) thresholds on the device; windows: nw odd widths in HOST memory, read before the launch.
 * Per field, channel c, threshold t and window n: the events are b = [x >= thr[c][t]] (NaN is no event), the count plane is
 * c(i, j) = the events in the cells |i' - i| <= n/2, |j' - j| <= n/2 inside the domain (cells outside count 0; the fraction
 * c / n^2 is never formed); with cf of x and co of its truth
 *   out     (rows, C, T, nw, 3) int64: sum cf^2, sum co^2, sum cf co over the H W cells;
 *   ens_out (rows / x_per_y, C, T, nw, 3) int64: sum E^2, sum co^2, sum E co with E = the sum of cf over the x_per_y members
 *           of a truth (the window count of the exceedance-count plane).  With x_per_y = 1 it is allowed and equals out.
 * Either may be NULL, not both; both are fully written.  FSS = 2 sum cf co / (sum cf^2 + sum co^2), after the triples of a
 * set of pairs are summed (ops.fss_summary).  All arithmetic on counts is integer, products and sums in 64 bits: exact, no
 * atomics, the same bits for every layout and launch order.  Nothing is read back; capturable in a HIP graph.
 * Limits: 1 <= H, W <= 1024 (need not be equal), 1 <= T <= 8, 1 <= nw <= 8, 1 <= x_per_y <= 64; a window n >= 2 max(H, W) - 1
 * is the whole domain.  Refused before a launch (-1, acg_last_error starts with "acg_fss"): an even or non-positive window,
 * rows % x_per_y != 0, a stride < 1, both outputs NULL, a misaligned workspace (16 bytes), and "overflow": a window whose
 * largest possible sum (v min(n, H) min(n, W))^2 H W reaches 2^63, v = x_per_y with ens_out, else 1 (1024^2 with the whole
 * domain and v = 1 is exactly 2^60 and accepted).  A workspace below acg_fss_workspace_bytes returns -2.
 * The workspace holds event planes, per plane one bit per cell in rows of WW = ceil(W / 64) 64-bit words and WW + 1 16-bit row
 * prefixes: 16-byte rounded 8 P H WW + 2 P H (WW + 1) bytes for the P = rows C T planes of x, then the same for the planes of
 * y, then, with want_ens and x_per_y > 1, for bit_width(x_per_y) slices per plane of y (the bits of the exceedance count); it
 * does not depend on nw.  Kernels: fss_events (one wave per image row), then one workgroup per (row, c, t) walking all
 * windows with its two planes in LDS when they fit 64 KiB - 512 (fss_box<lds>, up to 321^2 and beyond), else from the
 * workspace (fss_box<global>); ens_out adds fss_slices and the same walk over the slices, one workgroup per (truth row, c, t)
 * (fss_ens<lds>: 16 members at 256^2 fit; fss_ens<global> above). */
size_t acg_fss_workspace_bytes(int rows, int x_per_y, int C, int H, int W, int T, int nw, int want_ens);
int acg_fss(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride, int x_pix_stride,
            long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride, const float *thr, int T,
            const int *windows, int nw, long long *out, long long *ens_out, void *workspace, size_t ws_bytes, void *stream);

/* ---- intensity-scale triples of the same events (ops.fss_scales, model.translate_fss(scales=True), test.py --metric fss
 *      --fss_scales 1; tests/fss_scales_ref.py states the definition; Casati et al. 2004, Casati 2010) ----
 * x, y, the strides, x_per_y, thr and the events are acg_fss's.  With L = ceil(log2(max(H, W))) and nl = L + 1, level
 * l = 0 .. L cuts the plane into blocks of 2^l x 2^l cells anchored at cell (0, 0); the blocks at the right and bottom edge
 * are cut by the domain (the same as zero-padding the event planes to 2^L x 2^L).  With bf, bo the events of x and of its
 * truth in a block
 *   out     (rows, C, T, nl, 3) int64: sum bf^2, sum bo^2, sum bf bo over the blocks of level l;
 *   ens_out (rows / x_per_y, C, T, nl, 3) int64: sum E^2, sum bo^2, sum E bo, E the events of a truth's x_per_y members in
 *           the block.  With x_per_y = 1 it equals out.
 * Either may be NULL, not both; both are fully written.  Level 0 is (n_f, n_o, hits), bit for bit acg_fss's window-1 triple;
 * level L is (n_f^2, n_o^2, n_f n_o).  The largest value is (64 * 2^20)^2 = 2^52: nothing is refused for its size.  The Haar
 * component energies, the skill against a random forecast and the energy bias follow on the host from the summed triples
 * (ops.fss_scale_summary).  Integer after the comparison, no atomics, the same bits in every layout and launch order; nothing
 * is read back; capturable in a HIP graph.  Limits: 1 <= H, W <= 1024, 1 <= T <= 8, 1 <= x_per_y <= 64.  Refused before a
 * launch (-1, acg_last_error starts with "acg_fss_scales"), in this order: rows or C < 1, a stride < 1, x_per_y outside
 * 1..64 or not dividing rows, both outputs NULL, H or W outside 1..1024, T outside 1..8, a misaligned workspace (16 bytes); a
 * workspace below acg_fss_scales_workspace_bytes returns -2.  The workspace is acg_fss's (it never depended on the windows):
 * the planes of x, of y and, with want_ens and x_per_y > 1, the slices; nothing it held before the call, nor its padded bits,
 * reach a result.  Kernels: fss_events and fss_slices as in acg_fss, then fss_scales, one workgroup of four waves per
 * (row, c, t): a wave per 64 x 64 tile, levels 0..6 by popcounts and lane exchanges, levels 7..10 from the tiles' totals. */
size_t acg_fss_scales_workspace_bytes(int rows, int x_per_y, int C, int H, int W, int T, int want_ens);
int acg_fss_scales(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                   int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                   const float *thr, int T, long long *out, long long *ens_out, void *workspace, size_t ws_bytes, void *stream);

/* ---- Minkowski functionals of excursion sets (ops.minkowski, model.translate_minkowski, test.py --metric minkowski; no
 *      reference call site: the reference has no verification code, tests/minkowski_ref.py states the definition) ----
 * x: rows x C fields of H x W fp32 cells; the strides (in floats) mean what they mean in acg_fss: NHWC with Cp stored channels
 * is (H W Cp, Cp, 1) - padded channels never reach a result - and planar NCHW is (C H W, 1, H W).  thr: (C, T) thresholds on
 * the device, per channel finite and non-decreasing (repeats allowed): the caller's contract, the kernel cannot refuse them
 * (with others it still ends and reads and writes only inside its operands).
 * Per field and channel c the level of a pixel is L = #{t : thr[c][t] <= x} in 0 .. T: x == thr is an event and NaN has level
 * 0, as in acg_fss; +inf has level T, -inf level 0.  The excursion set at threshold t is {L >= t + 1}; the sets are nested.
 * The field stands in a ring of level-0 cells (outside the domain there is no event, so an event pixel on the border
 * contributes its border edges to the perimeter).  Five multisets of levels: F, the H W pixels; Emax / Emin, the max / min of
 * the two pixels on either side of each of the H (W + 1) + (H + 1) W unit edges; Vmax / Vmin, the max / min of the four pixels
 * around each of the (H + 1) (W + 1) vertices.  With n_X[t] = #{elements of X with level >= t + 1}:
 *   out (rows, C, T, 5) int64: (nF, nE1, nE2, nV1, nV4) = (n_F, n_Emax, n_Emin, n_Vmax, n_Vmin)[t], fully written.
 * They are linear over fields: sum them over a set of fields, then (ops.minkowski_summary) area = nF, perimeter = nE1 - nE2
 * (edges with exactly one side in the set), euler8 = nV1 - nE1 + nF (pixels as closed squares: 8-connected components minus
 * their holes), euler4 = nF - nE2 + nV4 (4-connected components minus their holes).  One pass over the field serves all T
 * thresholds.  Integer after the comparison: exact, the same bits for every layout and launch order.  Nothing is read back;
 * capturable in a HIP graph.
 * Limits: 1 <= H, W <= 1024 (need not be equal), 1 <= T <= 255 (levels fit a byte).  Refused before a launch (-1,
 * acg_last_error starts with "acg_minkowski"): a null x, thr or out, an extent or T out of range, rows < 1, C < 1, rows C
 * ceil((H + 1) / 8) or rows C T above 2^31 - 1, a stride < 1, a misaligned workspace (16 bytes).  A workspace below
 * acg_minkowski_workspace_bytes returns -2; the size query is 0 for a refused size.
 * The workspace holds (rows, C, bands, 5, T) 32-bit bins, bands = ceil((H + 1) / 8), rounded up to 16 bytes.  Kernels:
 * mink_hist, one workgroup per (row, band of 8 lattice rows) for NHWC with four stored channels (mink_hist<c4>: a pixel's
 * channels from one 16-byte load) and per (row, channel, band) otherwise (mink_hist<strided>): levels by bisection into an
 * LDS byte tile, histograms in LDS by integer adds aggregated over runs of equal levels, bins stored plainly; then
 * mink_finish, one workgroup per (row, channel): the bands summed, the suffix sums, the int64 stores.  No global atomics;
 * neither the workspace's nor out's earlier contents matter. */
size_t acg_minkowski_workspace_bytes(int rows, int C, int H, int W, int T);
int acg_minkowski(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                  const float *thr, int T, long long *out, void *workspace, size_t ws_bytes, void *stream);

/* ---- Connected components of excursion sets (ops.components, model.translate_minkowski(components=), test.py --metric
 *      minkowski --mink_components; no reference call site, tests/components_ref.py states the definition) ----
 * x, its strides and thr (C, T): as in acg_minkowski.  A plane is one (row, channel c, threshold t); its set is
 * [x >= thr[c][t]]: x == thr is inside, NaN outside, cells beyond the field outside (acg_minkowski's conventions; for
 * non-decreasing thresholds the sets are the same).  conn = 4: cells sharing an edge are connected; conn = 8: cells sharing an
 * edge or a corner.  Per plane, with the components of the set:
 *   out (rows, C, T, 25) int64, fully written: [0] n, the number of components; [1] area, the cells in the set (acg_minkowski's
 *   nF); [2] sum_sq, the sum over the components of area^2 (at most 2^40); [3] n_border, the components with a cell in the first
 *   or last row or column; [4 + b], b = 0 .. 20, the components with 2^b <= area < 2^(b + 1).
 *   labels (rows, C, T, H, W) int32, or NULL: 0 outside the set, inside 1 + the row-major index of the first cell of the cell's
 *   component: canonical, so comparable for equality.
 * All are linear over fields: sum them, then ops.components_summary (holes = n - euler of acg_minkowski's counts).  Exact
 * integers, the same bits on every call, in every layout and whatever the workspace held.  Launches only: nothing is read back,
 * no host synchronisation, capturable in a HIP graph.
 * Limits: 1 <= H, W <= 1024, 1 <= T <= 255, conn in {4, 8}.  Refused before a launch (-1, acg_last_error starts with
 * "acg_components"): a null x, thr or out, an extent, T or conn out of range, rows < 1, C < 1, rows C T above 2^31 - 1, labels
 * given with rows C T H W above 2^31 - 1, a stride < 1, a misaligned workspace (16 bytes).  A workspace below ONE plane returns -2.
 * The workspace holds whole planes of 8 H W bytes rounded up to 16 (int32 parents, uint32 areas); the call runs in passes of as
 * many planes as ws_bytes holds.  acg_components_workspace_bytes: the bytes of all rows C T planes, capped at the whole planes
 * that fit 256 MiB, never below one plane; 0 for a refused size.
 * Kernels, per pass: comp_label, one workgroup per (row [, channel], 32 x 64 tile) - NHWC with four stored channels: a
 * pixel's channels from one 16-byte load (comp_label<c4>), otherwise comp_label<strided> - keeps its cells in registers and, for
 * every plane of its row that the pass holds, builds the tile's union-find forest in LDS, flattens it, reduces area and border
 * flag per tile root in LDS and stores parents (global indices) and areas; comp_merge, a thread per cell of a tile's first row
 * and column, joins trees across the seams (and tile corners) with agent-scope atomic loads, min and compare-and-swap only;
 * comp_root points every tile root at its root and adds its area and flag there (integer atomics); comp_stats writes the labels
 * and adds each root's bins, reduced per workgroup in LDS, to the plane's out (integer atomics; comp_label zeroed it).  A
 * parent index is always below its child's, a union hooks the larger root under the smaller by compare-and-swap: every chase
 * descends, a failed swap means another lane hooked that root, nothing waits.  Fields of one tile skip comp_merge and comp_root. */
size_t acg_components_workspace_bytes(int rows, int C, int H, int W, int T);
int acg_components(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                   const float *thr, int T, int conn, long long *out, int *labels, void *workspace, size_t ws_bytes, void *stream);

/* ---- SAL: structure, amplitude and location of the objects of a field (Wernli et al. 2008; ops.sal, ops.sal_scores,
 *      model.translate_sal, test.py --metric fss --fss_sal 1; no reference call site, tests/sal_ref.py states the definition) ----
 * x, its strides, thr (C, T), conn, the planes and their sets: as in acg_components.  The mass of a cell is the fixed-point
 * integer q = clamp(rint((x - floor) 2^20), 0, 2^24), in fp32 with every operation rounded on its own (subtract, multiply,
 * round to nearest even); a NaN cell has q = 0, -inf 0, +inf 2^24.  floor: the lower end of the data range, so that mass is
 * "amount above the floor".  Every sum of masses is an exact integer below 2^54 and independent of its order.
 *   field (rows, C, 3) int64, fully written: Q, QY, QX = the sums of q, q h and q w over ALL H W cells (h the row, w the column).
 *   obj (rows, C, T, 4) int64, fully written: [0] n, the components of the plane's set; [1] area, the cells in the set (both as
 *   acg_components gives them); [2] Robj, the mass in the set; [3] Rmax, the largest mass of a component (0 without one).
 *   shape (rows, C, T, 2) double, fully written: with R_n, Y_n, X_n the sums of q, q h, q w and P_n the maximum of q over the
 *   cells of component n, every integer converted to double first and every operation rounded on its own, over the
 *   components with R_n > 0: [0] SV = sum R_n (R_n / P_n), the mass-weighted scaled volume; [1] SR = sum R_n
 *   sqrt((Y_n / R_n - QY / Q)^2 + (X_n / R_n - QX / Q)^2), the mass-weighted distance of the objects from the field's centre of
 *   mass.  0.0 where no component has mass.  The terms are summed per thread of a fixed partition in index order of the
 *   components' first cells, then by a fixed tree: within (n + 8) 2^-52 of any other order, relatively.
 * ops.sal_scores turns two such triples into S, A, L1, L2, L on the host.  The same bits on every call, in every layout, for
 * every workspace size and whatever the workspace held: integer atomics only, no floating-point atomics.  Launches only:
 * nothing is read back, no host synchronisation, capturable in a HIP graph.
 * Limits: 1 <= H, W <= 1024, 1 <= T <= 255, conn in {4, 8}, floor finite.  Refused before a launch (-1, acg_last_error starts
 * with "acg_sal"): a null x, thr, field, obj or shape, an extent, T or conn out of range, a floor that is not finite, rows < 1,
 * C < 1, rows C T above 2^31 - 1, a stride < 1, a misaligned workspace (16 bytes).  A workspace below ONE plane returns -2.
 * The workspace holds whole planes of 32 H W bytes (int32 parents, uint32 peaks, three uint64 sums), each rounded up to 16;
 * the call runs in passes of as many planes as ws_bytes holds.  acg_sal_workspace_bytes: the bytes of all rows C T planes,
 * capped at the whole planes that fit 256 MiB, never below one plane; 0 for a refused size.
 * Kernels: once per call sal_zero and sal_field, one workgroup per chunk of 8192 cells of a field row (NHWC with four stored
 * channels, sal_field<c4>) or of a (row, channel) (sal_field<strided>), which adds its sums to field (64-bit integer atomics);
 * then per pass sal_label, comp_label's walk that reduces the three sums and the peak per
 * tile root in LDS (64 KiB per workgroup); comp_merge; sal_root, which adds every tile root's sums and peak to its root's
 * (64-bit add, 32-bit max, agent scope); sal_finish, one workgroup per plane.  Fields of one tile skip comp_merge and sal_root. */
size_t acg_sal_workspace_bytes(int rows, int C, int H, int W, int T);
int acg_sal(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
            const float *thr, int T, int conn, float floor, long long *field, long long *obj, double *shape, void *workspace,
            size_t ws_bytes, void *stream);

/* ---- the marginal loss (ops.field_sort, ops.marginal_loss, --lambda_marg_A / --lambda_marg_B; no reference call site: the
 *      reference has no distributional loss, tests/marginal_ref.py states the definition) ----
 * acg_field_sort: a stable sort of each of the rows x C fields of H x W fp32 pixels of x, with its permutation.  The strides
 * (in floats) mean what they mean in acg_radial_spectrum: NHWC with Cp stored channels is (H W Cp, Cp, 1) - padded channels are
 * never read - and planar NCHW is (C H W, 1, H W).  Pixel p = h W + w comes before pixel q iff x[p] < x[q] as floats, or
 * x[p] == x[q] and p < q: -0.0 and +0.0 tie, ties break by pixel index (numpy.argsort(kind="stable") of x + 0.0).  sorted
 * (rows, C, P), P = H W: the values in that order, the bits of x (a -0.0 leaves as +0.0); rank (rows, C, P) int32, or NULL:
 * rank[r][c][p] is the position of pixel p.  Both are planar whatever the layout of x, and the same bits for every layout.
 * NaN is outside the contract; the kernels still end and write only inside sorted and rank.  Any H, W >= 1 with H W <= 2^20.
 * A bitonic network on the words (key << 32) | p, fields padded to Ppad = the next power of two: up to Ppad = 8192 one
 * launch and no workspace (one workgroup per 8192 words: a field, or several small ones); above, the words live in the
 * workspace (acg_field_sort_workspace_bytes = 8 rows C Ppad, 16-byte aligned) and a sort takes 1 + sum over s = 1 .. log2(Ppad
 * / 8192) of (ceil(s / 2) + 1) launches: the chunk sorts, then per merge stage s its s strides >= 8192 two per launch and one
 * launch that finishes the stage in LDS (3 at Ppad = 2^14, 8 at 2^16, 24 at 2^20; acg_last_kernel names the path and the
 * count).  Refused before a launch (-1, acg_last_error starts with the
 * entry's name): a null x or sorted, rows < 1, C < 1, H W outside 1 .. 2^20, a stride < 1, outputs that alias x or each other,
 * a misaligned workspace; a workspace below acg_field_sort_workspace_bytes returns -2.  The size query is 0 for a refused
 * size. */
size_t acg_field_sort_workspace_bytes(int rows, int C, int H, int W);
int acg_field_sort(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                   float *sorted, int *rank, void *workspace, size_t ws_bytes, void *stream);
/* The loss on two sorted batches sx (rows_x, C, P) and sy (rows_y, C, P) (the rows need not pair): d (C, P) = the mean of sx
 * over its rows - the mean of sy over its rows (the difference of the two batches' mean quantile functions, their Wasserstein
 * barycentres), loss[0] = the mean of d^2 over C P: the squared 2-Wasserstein distance of the barycentres, averaged over the
 * channels.  The row sums run in row order in fp32 and d is fp32; its squares are summed in double over fixed slices into the workspace
 * (acg_marginal_loss_workspace_bytes, 16-byte aligned, never 0 for a valid size) and from there by one workgroup: the same
 * bits on every call.  Two launches.  Refused before a launch: a null pointer, rows_x, rows_y or C < 1, P outside 1 .. 2^20,
 * d or loss aliasing an input (-1); a short workspace (-2). */
size_t acg_marginal_loss_workspace_bytes(int C, long long P);
int acg_marginal_loss_fwd(const float *sx, int rows_x, const float *sy, int rows_y, int C, long long P, float *d, float *loss,
                          void *workspace, size_t ws_bytes, void *stream);
/* Its data gradient: gx[r][c][p] = gscale[0] (2 / (C P rows)) d[c][rank[r][c][p]] in the layout the strides describe (those
 * of the x that acg_field_sort ranked); gscale is the upstream gradient, one float on the device, so nothing is read back
 * and the launch can be captured.  A gather, one thread per pixel: no atomics, deterministic.  Cp: the channels stored per
 * pixel of gx, channels C .. Cp - 1 are written as 0 (NHWC: Cp = pix_stride; planar: Cp = C); the C4 image layout leaves as
 * one 16-byte store per pixel.  One launch.  Refused before a launch (-1): a null pointer, rows < 1, C < 1, C > Cp, H W
 * outside 1 .. 2^20, a stride < 1, gx aliasing an input. */
int acg_marginal_loss_bwd(const float *d, const int *rank, const float *gscale, int rows, int C, int Cp, int H, int W,
                          long long row_stride, int pix_stride, long long chan_stride, float *gx, void *stream);
/* The evaluator on sorted fields (ops.sorted_scores, ops.marginal_scores, test.py --metric marginal; tests/marginal_eval_ref.py
 * states the definition).  sx (rows, C, P) and sy (rows / x_per_y, C, P), or NULL: fp32, every field ascending and planar, as
 * acg_field_sort writes them; row r of sx pairs with row r / x_per_y of sy (x_per_y ensemble members share one truth).  Per
 * (row, channel):
 *   w     (rows, C, 2) double, exactly when sy is given (else NULL): w1 = mean_k |sx[k] - sy[k]| and w2sq = mean_k (sx[k] -
 *         sy[k])^2, the differences taken and summed in double: the 1-Wasserstein and the squared 2-Wasserstein distance of the
 *         two fields' value distributions (equal sample sizes);
 *   q     (rows, C, L) fp32, exactly when L > 0: the order-statistic quantile with linear interpolation (numpy.quantile,
 *         method="linear") at levels[l]: pos = level (P - 1), lo = floor(pos), hi = min(lo + 1, P - 1), q = sx[lo] + (pos - lo)
 *         (sx[hi] - sx[lo]) in double, not contracted, rounded once to fp32.  levels: L doubles in HOST memory, each in
 *         [0, 1], read before the launch; 0 <= L <= 16;
 *   below (rows, C, E) int32, exactly when E > 0: #{k : sx[k] < edges[c][e]}, exact, by bisection in the sorted field; P -
 *         below is the count of acg_fss's events [x >= thr].  edges: (C, E) fp32 on the device in any order; 0 <= E <= 256.
 * Every output element is written.  NaN in a field is outside the contract; the kernel still ends and reads and writes only
 * inside its operands.  One launch (marginal_scores), one workgroup of 1024 threads per field: sx and sy are read once; a
 * thread sums groups of four pixels in a fixed order, then a shuffle tree per wave and the waves in order: no atomics, the same
 * bits on every call and for every alignment.  Nothing is read back; capturable in a HIP graph.  Refused before a launch (-1,
 * acg_last_error starts with "acg_marginal_scores"): a null sx, rows < 1, C < 1, P outside 1 .. 2^20, L or E outside their
 * ranges, nothing to compute (no sy, L = 0, E = 0), w given without sy or missing with it, q (or levels) and below (or edges)
 * likewise against L and E, rows % x_per_y != 0, a level outside [0, 1] or NaN, an output aliasing an input or another output. */
int acg_marginal_scores(const float *sx, const float *sy, int rows, int x_per_y, int C, long long P, const double *levels, int L,
                        const float *edges, int E, double *w, float *q, int *below, void *stream);

/* ---- structural similarity (ops.ssim, ops.ssim_loss, --lambda_ssim_A / --lambda_ssim_B, test.py --metric ssim; no reference
 *      call site: the reference compares pixels by L1 alone, tests/ssim_ref.py states the definition; Wang et al. 2004) ----
 * x: rows x C fields of H x W fp32 pixels, y: rows / x_per_y x C paired fields; row r of x pairs with row r / x_per_y of y
 * (x_per_y ensemble members share one truth).  The strides (in floats) mean what they mean in acg_cross_spectrum: NHWC with
 * Cp stored channels is (H W Cp, Cp, 1) - padded channels never reach a result - and planar NCHW is (C H W, 1, H W); each
 * operand has its own.  w: the separable 11 x 11 Gaussian, sigma = 1.5, each axis normalised to sum 1.  For every window
 * position p of the (H - 10) x (W - 10) 'valid' region (the window covers pixels p .. p + 10 on both axes):
 *   mu_x = sum w x, mu_y = sum w y, s_x = sum w x^2 - mu_x^2, s_y = sum w y^2 - mu_y^2, s_xy = sum w x y - mu_x mu_y,
 *   A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = s_x + s_y + C2,
 *   C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range (2 for fields in [-1, 1]),
 *   S(p) = A1 A2 / (B1 B2), cs(p) = A2 / B2 (the contrast-structure factor); no clamping of the variances.
 * out (rows, C, 2): the mean of S and the mean of cs over the valid region.  11 <= H, W <= 1024.
 * dmaps (or NULL): 3 planes of (rows, C, H - 10, W - 10), fully written: a = dS/d mu_x (total: 2 mu_y A2 / (B1 B2) -
 * 2 mu_x S / B1 - c mu_y - 2 b mu_x), b = dS/dE[x^2] = -S / B2, c = dS/dE[xy] = 2 A1 / (B1 B2): what acg_ssim_bwd reads.
 * fp32 per window position, the moments taken about a per-tile pivot (x at the tile's first pixel; variances are
 * shift-invariant, the means get it back), the sums over positions in double: per tile of 32 x 16 positions into the
 * workspace (acg_ssim_workspace_bytes = 16 rows C tiles, 16-byte aligned), then one wave per (row, channel) in a fixed order.
 * Two launches, no atomics, nothing read back; the same bits on every run and for every layout.  Refused before a launch
 * (-1, acg_last_error starts with "acg_ssim"): a null x, y or out, rows < 1, C < 1, an extent outside 11 .. 1024, a stride
 * < 1, rows % x_per_y != 0, data_range <= 0 or not finite, aliasing outputs, a misaligned workspace; a short workspace: -2.
 * The size query is 0 for a refused size. */
size_t acg_ssim_workspace_bytes(int rows, int C, int H, int W);
int acg_ssim(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride, int x_pix_stride,
             long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride, float data_range,
             float *out, float *dmaps, void *workspace, size_t ws_bytes, void *stream);
/* The data gradient of loss = 1 - mean over rows and channels of the mean S, rows of x and y pairing one to one:
 * gx(q) = -g[0] / (rows C (H - 10) (W - 10)) ((w * a)(q) + 2 x(q) (w * b)(q) + y(q) (w * c)(q)), * the full correlation of
 * a map (zero outside the valid region) with the window, the result H x W.  g: the upstream gradient, one float on the
 * device.  gx is written in x's layout; Cp: the channels stored per pixel of gx, channels C .. Cp - 1 are written as 0
 * (NHWC: Cp = pix_stride; planar: Cp = C).  One workgroup per tile of 32 x 16 pixels, a gather: no atomics, deterministic,
 * the same bits for every layout.  One launch.  Refused before a launch (-1): a null pointer, rows < 1, C < 1, C > Cp, an
 * extent outside 11 .. 1024, a stride < 1, gx aliasing an input. */
int acg_ssim_bwd(const float *dmaps, const float *x, const float *y, const float *g, int rows, int C, int Cp, int H, int W,
                 long long x_row_stride, int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                 long long y_chan_stride, float *gx, void *stream);

/* ---- the CRPS training loss (ops.crps_loss, train.py --lambda_crps_B; no reference call site: the reference's paired step
 *      penalises one translation per input by L1, tests/crps_ref.py states the definition; Ferro 2014, Lang et al. 2024) ----
 * x: rows = N M fields of C channels of H x W fp32 pixels, member m of input n at row n M + m (acg_ensemble_stats's order),
 * M = x_per_y; y: the N truths, row n.  Each operand has its own three strides (in floats), meaning what they mean in
 * acg_fss.  1 <= H, W <= 1024, 1 <= M <= 16, any C >= 1.  Per cell (n, c, pixel) with members x_1 .. x_M and truth y:
 *   e1 = (1/M) sum_i |x_i - y|,  e2 = sum_{i<j} |x_i - x_j|,  s = e1 - w e2,
 *   w = alpha / (M (M - 1)) + (1 - alpha) / M^2 (0 for M = 1): alpha = 1 the fair CRPS, alpha = 0 the ensemble CRPS e1 - e2 / M^2.
 * acg_crps_fwd writes out (N, C, 2) in DOUBLE: per input and channel the sums over the pixels of e1 and of e2; the loss is
 * (sum out[.., 0] - w sum out[.., 1]) / (N C H W), the caller's to form.  Differences and sums in double (float -> double is
 * exact); a workgroup of 256 threads owns 1024 consecutive pixels, thread t the pixels t, t + 256, t + 512, t + 768 of them,
 * added in that order, the threads by a fixed tree into the workspace (acg_crps_workspace_bytes = 16 N C ceil(H W / 1024),
 * 16-byte aligned), one wave per (n, c) folds them in a fixed order.  A thread holds the M values of a cell in registers and
 * walks the M (M - 1) / 2 pairs there.  A C4 pixel's channels come from one 16-byte load per member, everything else value by
 * value (a planar row is read 256 bytes per wave and load as it is); the order of every sum is the same: the same bits on
 * every call and in every layout.  Two launches, no atomics, out fully written whatever it and the workspace held, nothing
 * read back, capturable in a HIP graph.  acg_last_kernel(): "crps_fwd<x, y> + crps_fold", x and y each c4 or strided.  Refused before a launch (-1, acg_last_error starts with
 * "acg_crps_fwd"), in this order: a null x, y or out; an extent outside 1 .. 1024; rows < 1 or C < 1; too many fields for a
 * grid; a stride < 1; x_per_y outside 1 .. 16 or not dividing rows; out aliasing an input; a misaligned workspace; a short
 * workspace: -2.  The size query is 0 for a refused size. */
size_t acg_crps_workspace_bytes(int rows, int x_per_y, int C, int H, int W);
int acg_crps_fwd(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride, int x_pix_stride,
                 long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride, double *out,
                 void *workspace, size_t ws_bytes, void *stream);
/* The data gradient of that loss in x.  The signs are recomputed from x and y (sign(0) = 0, what torch.abs propagates; no maps
 * are kept between the passes): per member i of a cell the integers sy = sign(x_i - y), sp = sum_{j != i} sign(x_i - x_j), and
 *   dx_i = (float)(g[0] (coef_y sy - coef_pair sp)),  coef_y = 1 / (M N C H W),  coef_pair = w / (N C H W),
 * the two coefficients formed by the caller in double, the combine in double without contraction, rounded once.  g: the
 * upstream gradient, one float on the device.  dx is written in x's layout; Cp: the channels stored per pixel of dx,
 * channels C .. Cp - 1 are written as 0 (NHWC: Cp = pix_stride; planar: the stored planes).  y gets no gradient.  One launch,
 * no workspace, nothing read back, capturable.  acg_last_kernel(): "crps_bwd<x, y>".  Refused before a launch (-1), in this
 * order: a null pointer; an extent outside 1 .. 1024; rows < 1, C < 1 or C > Cp; too many fields; a stride < 1; x_per_y
 * outside 1 .. 16 or not dividing rows; a coefficient that is not finite; dx aliasing an input. */
int acg_crps_bwd(const float *x, const float *y, const float *g, int rows, int x_per_y, int C, int Cp, int H, int W,
                 long long x_row_stride, int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                 long long y_chan_stride, double coef_y, double coef_pair, float *dx, void *stream);

/* ---- the fractions-skill-score training loss (ops.fss_loss, train.py --lambda_fss_A / --lambda_fss_B; no reference call site,
 *      tests/fss_loss_ref.py states the definition; Roberts & Lean 2008, Ebert-Uphoff et al. 2021) ----
 * x: rows forecasts of C channels of H x W fp32 pixels, y: the paired truths, row for row.  Each operand has its own three
 * strides (in floats), meaning what they mean in acg_fss.  thr: (C, T) fp32 on the device; windows: nw odd widths in host
 * memory, read during the call.  1 <= H, W <= 1024 (need not be equal), 1 <= T <= 8, 1 <= nw <= 8, odd 1 <= n <= 65, any C >= 1.
 *   soft events  p = 1 / (1 + exp(-(x - thr[c][t]) inv_tau)), q the same of y: fp32 in exactly this form, so they saturate to
 *                exactly 0 and 1 (exp overflows to inf, underflows to 0).  NaN is not masked: it reaches the sums.
 *   window sums  cf(i, j) = sum of p over the cells |i' - i| <= n/2, |j' - j| <= n/2 inside the domain (cells outside count 0,
 *                / n^2 is never formed), co of q: fp32, n terms along the row, then n row sums down the column, each in
 *                ascending order.  Window sums of 0/1 planes are exact integers.
 *   per (row, c, t, window)  num = sum over cells (cf - co)^2, den = sum over cells (cf^2 + co^2), differences, squares and sums
 *                in double.  With saturated events they equal ff + oo - 2 fo and ff + oo of acg_fss's triples exactly.
 * acg_fss_loss_fwd writes out (rows, C, T, nw, 2) in DOUBLE, (num, den); the pooled ratio R = sum_rows num / sum_rows den
 * (0 where the denominator is 0) and loss = mean of R over C, T, nw are the caller's to form.  A workgroup of 256 threads owns
 * a tile of 32 x 32 cells of one (row, c, t) and walks the windows: the (32 + 2 (n/2))^2 events around the tile go to LDS (dynamic,
 * sized by the call's largest window: 21 KiB at n = 17, 60 KiB at n = 65), are summed along rows and then down columns; thread k adds its cells k, k + 256, k + 512, k + 768 of the tile in
 * that order, the threads by a fixed tree, one partial pair per tile into the workspace, one wave per (row, c, t, window) folds
 * the tiles in a fixed order.  Every layout is read value by value through its strides: the same bits on every call and in
 * every layout.  Two launches, no atomics, out fully written whatever it and the workspace held, nothing read back,
 * capturable in a HIP graph.  acg_last_kernel(): "fss_loss_fwd + fss_loss_fold".  acg_fss_loss_workspace_bytes serves both
 * passes: the larger of 16 rows C T nw ceil(H/32) ceil(W/32) and 4 rows C T nw H W bytes, 16-byte aligned; 0 for a refused size.
 * Refused before a launch (-1, acg_last_error starts with "acg_fss_loss_fwd"), in this order: a null x, y, thr, windows or
 * out; an extent outside 1 .. 1024; rows < 1 or C < 1; T or nw outside 1 .. 8; a window that is even, not positive or above
 * 65; a stride < 1; inv_tau not finite or not positive; too many fields for a grid; out aliasing an input; a short
 * workspace: -2; a misaligned workspace. */
size_t acg_fss_loss_workspace_bytes(int rows, int C, int H, int W, int T, int nw);
int acg_fss_loss_fwd(const float *x, const float *y, int rows, int C, int H, int W, long long x_row_stride, int x_pix_stride,
                     long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride, const float *thr,
                     int T, const int *windows, int nw, float inv_tau, double *out, void *workspace, size_t ws_bytes, void *stream);
/* The data gradient of that loss in x.  coef: (C, T, nw, 2) DOUBLE on the device, the caller's a = 2 (1 - R) / Den and
 * b = 2 / Den, already multiplied by the upstream gradient and by 1 / (C T nw) and 0 where Den == 0: no host synchronisation.
 * B_n, the window sum, is symmetric:
 *   dx(q) = sum_t p_t (1 - p_t) inv_tau sum_w B_n( a cf - b co )(q),
 * the inner plane living on the domain's cells only (cells outside contribute 0 to the second sum; not a padded convolution
 * of a padded convolution).  p and q are recomputed, no maps are kept between the passes.  a cf - b co = B_n u with the one
 * plane u = (float)(a p - b q), combined in double and rounded once: "fss_loss_g" window-sums u with the forward's code and
 * writes one fp32 plane per (row, c, t, window) into the workspace, "fss_loss_dx" (a workgroup per 32 x 32 tile of (row, c))
 * window-sums those planes, adds the windows and then the thresholds in ascending order in fp32; p (1 - p) is exactly 0 where
 * p is saturated.  A gather: no atomics, deterministic, the same bits in every layout.  dx is written in x's layout; Cp: the
 * channels stored per pixel of dx, channels C .. Cp - 1 are written as 0 (NHWC: Cp = pix_stride; planar: the stored planes).
 * y gets no gradient.  Two launches, nothing read back, capturable.  acg_last_kernel(): "fss_loss_g + fss_loss_dx".  Refused
 * before a launch (-1) as the forward and in its order, with a null coef or dx among the null pointers, then C > Cp, dx
 * aliasing an input, a short workspace (-2), a misaligned workspace. */
int acg_fss_loss_bwd(const float *x, const float *y, int rows, int C, int Cp, int H, int W, long long x_row_stride, int x_pix_stride,
                     long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride, const float *thr,
                     int T, const int *windows, int nw, float inv_tau, const double *coef, float *dx, void *workspace,
                     size_t ws_bytes, void *stream);

/* ---- optimiser: torch.nn.utils.clip_grad_norm + torch.optim.Adam.step (model.py:447-452, 510-515)
 *      on one flat fp32 buffer per network. ---- */
int acg_sumsq(const float *g, size_t n, float *out, void *workspace, size_t ws_bytes, void *stream);
/* coef = min(1, max_norm/(sqrt(*sumsq)+1e-6)) read on device; p,m,v updated in place; g is NOT modified
 * unless scale_grads != 0 (then g *= coef, matching the reference's in-place clip). */
int acg_adam_step(float *p, float *g, float *m, float *v, size_t n, const float *sumsq, float max_norm, float lr,
                  float beta1, float beta2, float eps, int step, int scale_grads, void *stream);

/* The same for every network of an optimiser phase in three launches (multi-tensor clip + Adam: model.py:447-452 clips and
 * steps D_A, D_B (and D_z_B); model.py:510-515 G_A_B, G_B_A (and E_B)).  Per group: *sumsq = sum(g^2), then
 * coef = min(1, max_norm/(sqrt(*sumsq)+1e-6)), g *= coef, Adam on (p, m, v).  Bit-identical to acg_sumsq + acg_adam_step
 * (scale_grads = 1) per group.  The group array is host memory, read during the call.  step_dev (device, may be NULL): when
 * given, the step number of the bias corrections is *step_dev + 1, read by the kernel — for a launch recorded into a HIP
 * graph, whose arguments are fixed at capture (`step` is then ignored). */
#define ACG_ADAM_MAX_GROUPS 8
typedef struct {
    float *p, *g, *m, *v; /* device: parameters, gradients, first and second moments of one network, n floats each */
    size_t n;
    float *sumsq;         /* device: receives the network's gradient sum of squares (1 float) */
} acg_adam_group;
size_t acg_clip_adam_multi_workspace_bytes(int ngroups);
int acg_clip_adam_multi(const acg_adam_group *groups, int ngroups, float max_norm, float lr, float beta1, float beta2, float eps,
                        int step, const int *step_dev, void *workspace, size_t ws_bytes, void *stream);

/* ---- averaged weights (new, no reference counterpart; --ema_decay): an exponential moving average of the parameters of
 *      one or more networks, kept behind their optimiser step.  One launch for all groups.  Per element
 *      e += (1 - d_t) (p - e), d_t = min(decay, (1 + t) / (10 + t)), t the 1-based number of the optimiser step just taken:
 *      t = step, or, with step_dev (device, may be NULL), *step_dev + 1 read by the kernel, the convention of
 *      acg_clip_adam_multi for a launch recorded into a HIP graph (`step` is then ignored).  d_t is formed inside the kernel
 *      from the integer t in both cases, so an eager and a replayed launch at the same t give the same bits.  p is read
 *      only; any n, 128-bit accesses where p and e of a group are both 16-byte aligned; no workspace.  The group array is
 *      host memory, read during the call.  Refused before a launch (-1): decay outside (0, 1), ngroups outside
 *      1..ACG_EMA_MAX_GROUPS, a null pointer, n == 0, step < 1 without step_dev.
 *      acg_swap_multi exchanges p[i] and e[i] in place on the same table (the averaged weights become the live ones and
 *      back; twice is the identity). ---- */
#define ACG_EMA_MAX_GROUPS 8
typedef struct {
    float *p, *e; /* device: the live parameters of one network and their average, n floats each */
    size_t n;
} acg_ema_group;
int acg_ema_multi(const acg_ema_group *groups, int ngroups, float decay, int step, const int *step_dev, void *stream);
int acg_swap_multi(const acg_ema_group *groups, int ngroups, void *stream);

/* ---- windows of native-resolution fields (new, no reference counterpart: the reference resizes every field to one grid,
 *      dataloader.py:17-35; ops.window_gather / ops.window_blend, model.translate_field, train.py --native_res) ----
 * acg_window_gather cuts T windows of S x S out of fields (N, C, H, W) NCHW and writes them (T, S, S, Cp) NHWC, Cp the stored
 *   width (4 for C4 images, else a multiple of 16), channels C..Cp-1 zero: the layout change of acg_nchw_to_nhwc16 fused into
 *   the cut, an exact copy.  table: T rows of 4 ints in DEVICE memory, 16-byte aligned: src (the field), oy, ox (the window's
 *   origin), flip (bit 0 mirrors x, bit 1 mirrors y: window pixel (i, j) is field pixel (oy + i', ox + j'), i' = S-1-i resp.
 *   j' = S-1-j where mirrored).  PRECONDITION for direct callers: every row has 0 <= src < N, 0 <= oy <= H-S,
 *   0 <= ox <= W-S and 0 <= flip <= 3.  The scalars are checked here; the rows live on the device and are NOT: the kernel
 *   does not clamp (a clamp would hide a wrong table), a row outside these ranges reads outside `fields`.
 * acg_window_blend is the inverse for a separable window grid: tiles (rows*ny*nx, S, S, Cp) NHWC, tile (ky, kx) of canvas row r
 *   at index (r*ny + ky)*nx + kx with its origin at (oy[ky], ox[kx]), blended into canvas (rows, C, H, W) NCHW.  Tile pixel
 *   (i, j) weighs w(i) w(j), w(i) = min(i+1, S-i, R) / R; a canvas pixel is sum(w v) / sum(w) over the tiles that cover it, in
 *   the fixed order ky, kx ascending with one lane per canvas pixel (no atomics: a repeat gives the same bits); a pixel under
 *   exactly ONE tile takes that tile's bits, no multiply and no divide.  The record is host memory, passed to the kernel by
 *   value.  Refused before a launch (-1): counts outside 1..ACG_WINDOW_MAX, origins not strictly ascending, a first origin
 *   other than 0, a last one other than H-S (W-S), a gap between neighbours above S, R outside 1..S, S above 4096. ---- */
#define ACG_WINDOW_MAX 64
typedef struct {
    int H, W, S, R; /* canvas extents, window edge, ramp length of the weight */
    int ny, nx;     /* windows along y and x */
    int oy[ACG_WINDOW_MAX], ox[ACG_WINDOW_MAX];
} acg_window_plan;
int acg_window_gather(const float *fields, const int *table, float *out, int N, int C, int H, int W, int T, int S, int Cp,
                      void *stream);
int acg_window_blend(const float *tiles, const acg_window_plan *plan, float *canvas, int rows, int C, int Cp, void *stream);

/* ---- gradient exchange of the data-parallel step (replaces nn.parallel.data_parallel, networks.py:193-197 etc.): one
 *      process per GPU; rank 0 makes an id and ships its ACG_COMM_ID_BYTES to the other ranks by any side channel; every
 *      rank then joins with its current HIP device.  acg_comm_allreduce_mean averages a flat fp32 buffer (a network's
 *      gradients, model.py:447-449 / 510-512 clip AFTER it) in place across the ranks, enqueued on `stream` (ncclAvg over
 *      xGMI).  RCCL is bound at run time; the rest of the library does not need it. ---- */
#define ACG_COMM_ID_BYTES 128
int acg_comm_unique_id(void *id);
int acg_comm_init(void **comm, const void *id, int nranks, int rank);
int acg_comm_allreduce_mean(void *comm, float *buf, size_t n, void *stream);
int acg_comm_destroy(void *comm);

#ifdef __cplusplus
}
#endif
#endif /* ACGAN_HIP_H */
