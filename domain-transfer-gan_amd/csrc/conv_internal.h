// Internal geometry shared by the convolution kernels (not part of the C ABI).
#pragma once
#include "common.h"

#define ACG_KC 16 // K-channels per implicit-GEMM stage

struct Taps {
    int n;
    short dy[64];
    short dx[64];
    short w[64];
    // (dy & 0xff) | (dx & 0xff) << 8 | w << 16 per tap: ONE dword the kernels fetch with a scalar load per stage
    // (16-bit array elements go through vector memory and leave the weight-slab offset in a VGPR).  Filled by
    // acg_taps_pack() in the launchers.
    int pk[64];
    // row-patch stages of the generic bf16 tile (conv_bf16.hip, filled by its launcher): runs of up to 3 consecutive taps
    // with one dy and dx values within a span of 3.  gpk[16 ph + i] = first tap (relative to the phase's first) | taps << 8 |
    // (smallest dx & 0xff) << 16; ngrp = the group counts of the (up to four) phases, one byte each
    int gpk[64];
    int ngrp;
};

static inline Taps acg_taps_pack(const Taps &t)
{
    Taps r = t;
    for (int i = 0; i < 64; ++i)
        r.pk[i] = i < t.n ? ((t.dy[i] & 0xff) | ((t.dx[i] & 0xff) << 8) | ((int)t.w[i] << 16)) : 0;
    return r;
}

struct Geom {
    int Hin, Win, Cin;    // gathered tensor (K-channels = Cin, multiple of 16)
    int Hout, Wout, Cout; // written tensor; columns >= Cout are masked
    int GH, GW;           // grid of output positions per image covered by this launch
    int os, oy0, ox0;     // output pixel = (gy*os + oy0, gx*os + ox0)
    int is;               // gathered pixel = (gy*is + dy[t], gx*is + dx[t])
    int reflect;          // 1: mirror out-of-range coordinates (ReflectionPad2d), 0: zeros
    int act;
    int ncols_pad;        // packed-weight column count (multiple of the N tile)
    long long w_elems;    // element count of the packed weight array (bf16 modes: where the lo part starts)
    // Data gradient of a reflection-padded convolution, computed on the padded grid (Hout x Wout = fold_H+2p x fold_W+2p).
    // fold_p > 0 (wave-specialised kernel only): padded-grid pixels whose input pixel receives no mirrored contribution
    // are stored straight into out2 (N, fold_H, fold_W, Cout); only the frame (pad ring + the rows/columns it mirrors
    // onto) goes to `out`, and reflect_fold_frame_kernel sums that 3 % of the pixels afterwards.
    int fold_p = 0, fold_H = 0, fold_W = 0;
    float *out2 = nullptr;
    const float *addend = nullptr; // fold_p > 0 only: tensor of out2's shape added to the result (residual-path gradient)
    // optional sign bitmask of the addend (norm.hip layout: bit e%32 of word e/32 for float index e): only elements whose
    // bit is set are added — the skip gradient dy * (y > 0) of ReLU(x + IN(..)) without materialising it
    const unsigned *addend_mask = nullptr;
    // fold_p > 0 only: tensor of out2's shape whose SIGN masks the result (value > 0 ? keep : 0) before the addend — the
    // convolution's own input when that input is the ReLU output of the layer in front: dx is then already the gradient
    // w.r.t. that layer's pre-activation and its separate activation-backward pass (3 tensor streams) disappears
    const float *relu_src = nullptr;
    // pre-split ("S16") storage, conv_x3_pre.hip: per pixel and 8-channel group 16 bytes of bf16 hi then 16 bytes of bf16 lo
    // (x = hi + lo + O(2^-17 |x|); the same 4 bytes per element as fp32).  out_s16: the written tensor (out2 on the frame
    // path) takes that form; relu_s16: relu_src is stored that way (its sign = the sign of the hi halves).
    int out_s16 = 0, relu_s16 = 0;
    // out_s16 only.  mask_out: the launch also stores (output > 0) as one bit per element (norm.hip layout: bit e % 32 of word
    // e / 32 for float index e) — all a later data gradient needs of a conv + ReLU output; relu_mask: such a bitmask takes the
    // place of relu_src (1/32 of the bytes)
    unsigned *mask_out = nullptr;
    const unsigned *relu_mask = nullptr;
    // unpad (pre-split kernel only): data gradient of a ReflectionPad2d(1) 3x3 convolution computed on the UN-padded grid,
    // every tile one grid row.  The adjoint of the mirror folds pad row -1 onto row 1 and pad row H onto row H-2: for the
    // tiles of those two rows the kernel row that reads the mirrored dy row takes the packed slabs 9 + kw = w[0][kw] +
    // w[2][kw] instead of its own (acg_packed_wb_elems), and the column part of the fold — two pixels per grid row — is
    // a separate small GEMM (dgrad_colfix_kernel) whose result colfix[(image row * 2 + {left, right}) * Cout + c] is
    // added to pixels 1 and W-2 before the side inputs.  No padded scratch tensor, no fold pass.
    int unpad = 0;
    const float *colfix = nullptr;
    // unpad only (acg_norm_sums): the tile's share of the backward sums of the norm whose output gradient this launch writes
    const float *ns_x = nullptr, *ns_mean = nullptr, *ns_rstd = nullptr, *ns_gamma = nullptr, *ns_beta = nullptr;
    const unsigned *ns_mask = nullptr;
    float *ns_part = nullptr;
    int ns_gstride = 0, ns_act = 0;
    // per-tile statistics for an InstanceNorm behind the convolution (acg_conv2d_fwd_stats): (mean, M2) of every output
    // channel over the 128 output pixels of a tile, written to stats[((img * stats_cpi + stats_chunk0 + tile) * 2 + {0,1}) *
    // Cout + c], tile = the tile's index within its image in THIS launch (stats_cpi = chunks per image over all launches
    // that fill the tensor: the four sub-pixel phases of a ConvTranspose2d each add their own chunks)
    float *stats = nullptr;
    int stats_cpi = 0, stats_chunk0 = 0;
    // nphase == 4 (generic bf16 tile only): the four sub-pixel phases of a stride-2 data gradient / ConvTranspose2d forward
    // in ONE launch.  Phase ph = 2 py + px writes output pixels (2 gy + py, 2 gx + px) from the taps pk[16 ph .. 16 ph +
    // ph_ntaps[ph]); all phases share GH x GW (even output sizes).  Workgroup w handles phase w % 4 of tile w / 4, so the four
    // phases of a tile — which gather the same rows of the input — run side by side on one XCD and share its L2.
    int nphase = 0;
    int ph_ntaps = 0;     // tap counts of the four phases, one byte each (an array here would be indexed at run time in the
                          // kernel and drag the by-value argument structs into scratch memory: 2-3x slower, measured)
    int thin;             // 1: K flattened over (tap, 4 channels): stage s = taps 8s..8s+7, channels 0..3 of each
    int bk8;              // 8-float k-chunks per packed weight slab (Cin/8; thin: 4*ceil(ntaps/8), single slab)
    long long Mtot;       // N*GH*GW
};

int acg_igemm_launch(const float *in, const float *wp, const float *bias, float *out, const Geom &g, const Taps &t,
                     hipStream_t st);

// weight-gradient implicit GEMM: dw_part[split][tap][CiP][CoP] partial sums over pixel ranges
struct WGeom {
    int Hin, Win, Cin;    // gathered (conv-input side) tensor
    int Hg, Wg, Cg;       // gradient (conv-output side) tensor, one row per GEMM-K pixel
    int is;               // gathered pixel = (gy*is + dy[t], gx*is + dx[t]) for gradient pixel (gy, gx)
    int reflect;
    int CiP, CoP;         // padded dims of the partial buffer
    int nsplit;
    long long Mtot;       // N*Hg*Wg
    long long m_per_split;
    int thin;             // 1: gathered operand columns = (tap, 4 channels) flattened, 8 taps per 32-column tile
    int bias_from;        // 0: none, 1: column sums of the gradient-side operand, 2: of the gathered-side operand
    float *bias_part;     // [nsplit][CoP or CiP] partial column sums (written by the tap-0 / tile-0 blocks)
};
int acg_wgrad_launch(const float *x, const float *dy, float *part, const WGeom &g, const Taps &t, hipStream_t st);
void acg_wgrad_tiles(int Ci, int Co, int *bci, int *bco, int ntaps);
int acg_wgrad_taps_per_wg(int Ci, int Co, int ntaps, int thin);
// conv_wgrad_k4.hip: kernel-row weight gradient of the zero-padded 4x4 layers (D_B) and the stride-2 3x3 pair of the generators
bool acg_wgrad_krowg_shape_ok(int K, int stride, int pad, int reflect, int Wi, int Wo, int Cx, int Cg);
bool acg_wgrad_krowg_ok(const WGeom &g, const Taps &t);
int acg_wgrad_krowg_launch(const float *x, const float *dy, float *part, const WGeom &g, const Taps &t, hipStream_t st);

extern int g_acg_precision;
extern int g_acg_conv_impl;

// ---- what packing (conv_pack.hip) and dispatch (conv_api.hip) must agree on, stated once ------------------------------------
// packed weights are bf16 (hi, and for BF16X3 also lo right behind it) whenever the bf16 matrix pipe is used
static inline bool use_bf16() { return g_acg_precision != ACG_PREC_F32 && g_acg_conv_impl == ACG_IMPL_MFMA; }
static inline bool bf16x3_mfma() { return g_acg_precision == ACG_PREC_BF16X3 && g_acg_conv_impl == ACG_IMPL_MFMA; }
// thin-channel K-flattening (fp32 MFMA kernels): the gathered tensor has <= 4 real channels and K > 1
// (thin layers keep the fp32-tile thin kernels — loader, LDS tiles, packed weights — in every mode: they beat the padded bf16
// path; outside the strict fp32 mode their products run as bf16x3, conv_igemm.hip / conv_wgrad.hip X3)
static inline bool thin_ok(int creal, int K) { return creal >= 1 && creal <= 4 && K > 1 && g_acg_conv_impl == ACG_IMPL_MFMA; }
// a layer is treated as thin on exactly one side (3->3 convolutions do not occur on this path and stay regular)
static inline bool thin_in(const acg_conv_desc *d) { return thin_ok(d->Cir, d->K) && !thin_ok(d->Cor, d->K); }
static inline bool thin_out(const acg_conv_desc *d) { return thin_ok(d->Cor, d->K) && !thin_ok(d->Cir, d->K); }
// The VALU thin-output kernel (conv_aux.hip) beats the padded 32-column MFMA tile only against the fp32 matrix pipe (1.7 vs
// 2.9 ms on the 7x7 32->3 head); on the bf16 pipe the MFMA tile wins 2x (0.87 ms in bf16x3).  It pays off up to 64 gathered
// channels (>= 4 pixels per wave) and needs C/4 lanes per pixel to divide a wave: 16, 32 or 64 stored channels
static inline bool thin_valu_c(int C) { return !use_bf16() && (C == 16 || C == 32 || C == 64); }
// Packed weights are laid out on channel counts padded to 16 whatever the stored width of the activation tensors: an image
// tensor (<= 4 real channels) may be stored with 4 channels ("C4", acg_conv_desc), its layer's weights are packed as before.
__host__ __device__ static inline int c16(int c) { return (c + 15) / 16 * 16; }
// K == 3: three more wb slabs behind the nine taps, 9 + kw = w[0][kw] + w[2][kw] (bf16 packings only): what the kernel row that
// reads a mirrored row uses in the un-padded data gradient of a reflection-padded layer (Geom.unpad)
__host__ __device__ static inline int wb_slabs(int K) { return K * K + (K == 3 ? 3 : 0); }
// One packed operand gathers Ck channels and has Cn columns (wf: Ck = Ci, Cn = Co; wb: Ck = Co, Cn = Ci).  Its regular form
// [slab][Ck/8][ncols_pad(Cn)][8] floats always has room; a second form may sit right behind it (the "tail"):
//   N-packed   — thin-OUTPUT operands with 32 gathered channels (7x7 32 -> nc head, data gradient of the nc -> 32 stem;
//                conv_patch.hip conv_patchn_x3): K rows x (K + 3) window columns of 1 KB hi + 1 KB lo, where the 16 MFMA
//                columns are (4 horizontally adjacent output pixels) x (4 channels);
//   row-packed — thin-INPUT operands with 32 columns (7x7 nc -> 32 stem forward, data gradient of the 32 -> nc head;
//                conv_patch.hip conv_thinrow_x3): per kernel row one 32-deep K step = 8 window columns (the eighth zero)
//                x 4 channels, [row][k-group 4][32 columns][8] bf16 hi + lo = 4 KB per row.
enum { ACG_TAIL_NONE = 0, ACG_TAIL_NPACK, ACG_TAIL_TROW };
static inline int pack_tail(int K, int Ck, int Cn)
{
    if (K <= 1 || K > 7) return ACG_TAIL_NONE;
    return c16(Cn) == 16 && c16(Ck) == 32 ? ACG_TAIL_NPACK : (c16(Ck) == 16 && c16(Cn) == 32 ? ACG_TAIL_TROW : ACG_TAIL_NONE);
}
static inline size_t pack_tail_elems(int tail, int K)   // floats
{
    return tail == ACG_TAIL_NPACK ? (size_t)K * (K + 3) * 512 : (tail == ACG_TAIL_TROW ? (size_t)K * 1024 : 0);
}
// element count of the regular form = float offset of the tail (Geom.w_elems)
static inline size_t wf_regular_elems(int K, int Ci, int Co) { return (size_t)K * K * (c16(Ci) / 8) * acg_ncols_pad(c16(Co)) * 8; }
static inline size_t wb_regular_elems(int K, int Ci, int Co) { return (size_t)wb_slabs(K) * (c16(Co) / 8) * acg_ncols_pad(c16(Ci)) * 8; }
int acg_igemm_x3_ws_launch(const float *in, const void *wp, const float *bias, float *out, const Geom &g, const Taps &t,
                           long long n_w_elems, hipStream_t st, float *stats = nullptr);
bool acg_igemm_uses_ws(const Geom &g);
// conv_x3_pre.hip: the same tile on a pre-split (S16) gathered tensor, both operands by LDS-DMA
bool acg_igemm_x3_pre_ok(const Geom &g, const Taps &t);
int acg_igemm_x3_pre_launch(const void *in, const void *wp, const float *bias, float *out, const Geom &g, const Taps &t,
                            long long n_w_elems, hipStream_t st, float *stats = nullptr);
bool acg_conv_patch16_ok(const Geom &g, const Taps &t);
int acg_conv_patch16_launch(const float *in, const void *wp, const float *bias, float *out, const Geom &g, const Taps &t,
                            long long n_w_elems, hipStream_t st);
// conv_rows.hip: persistent row pipeline for the full-resolution 3x3 stride-1 32 -> 64 channel layers
bool acg_conv_rows_ok(const Geom &g, const Taps &t);
int acg_conv_rows_launch(const float *in, const void *wp, const float *bias, float *out, const Geom &g, const Taps &t,
                         long long n_w_elems, hipStream_t st);
bool acg_conv_patchn_ok(const Geom &g, const Taps &t);   // ... with C4 output and N-packed weights (conv_patchn_x3)
int acg_conv_patchn_launch(const float *in, const void *wn, const float *bias, float *out, const Geom &g, const Taps &t, hipStream_t st);
bool acg_conv_thinrow_ok(const Geom &g, const Taps &t);  // C4 gathered tensor -> 32 channels, one K step per kernel row (conv_thinrow_x3)
int acg_conv_thinrow_launch(const float *in, const void *wr, const float *bias, float *out, const Geom &g, const Taps &t, hipStream_t st);
// conv_ph4.hip: stride-2 data gradient / ConvTranspose2d forward with the four sub-pixel phases in one tile (64 columns)
bool acg_igemm_ph4_ok(const Geom &g);
bool acg_ph4_plan(const Taps &t, const int nt[4], Taps *out);
int acg_igemm_ph4_launch(const float *in, const void *wp, const float *bias, float *out, const Geom &g, const Taps &plan,
                         long long n_w_elems, hipStream_t st);
int acg_igemm_bf16_launch(const float *in, const void *wp, const float *bias, float *out, const Geom &g, const Taps &t,
                          int bn, long long n_w_elems, hipStream_t st);
int acg_wgrad_bf16_launch(const float *x, const float *dy, float *part, const WGeom &g, const Taps &t, int bci, int bco,
                          hipStream_t st);
// conv_wgrad_tr.hip: one kernel row per workgroup (stride-1 3x3, 128-multiple channels, bf16x3).  The *_shape_ok predicates
// take the convolution's shape (x side Hi x Wi x Cx, gradient side Ho x Wo x Cg): the split plan (wgrad_plan, conv_api.hip)
// asks them, the WGeom-level *_ok predicates build on them
bool acg_wgrad_krow_shape_ok(int K, int stride, int pad, int Hi, int Wi, int Ho, int Wo, int Cx, int Cg);
bool acg_wgrad_krow_ok(const WGeom &g, const Taps &t);
int acg_wgrad_krow_launch(const float *x, const float *dy, float *part, const WGeom &g, hipStream_t st);
int acg_wgrad_krow_s16_launch(const void *x, const void *dy, float *part, const WGeom &g, hipStream_t st); // pre-split operands
bool acg_wgrad_krow_s_shape_ok(int K, int stride, int pad, int Hi, int Wi, int Ho, int Wo, int Cx, int Cg);
bool acg_wgrad_krow_s_ok(const WGeom &g, const Taps &t);   // its 32 <-> 64 channel, 128-pixel-run variant
// conv_wgrad_thin.hip: the 7x7 image layers (C4 tensor on one side, 32 channels on the other), persistent over 8 x 16 tiles
bool acg_wgrad_thin_patch_shape_ok(int K, int stride, int Hthin, int Wthin, int Hwide, int Wwide, int Cthin, int Cwide);
bool acg_wgrad_thin_patch_ok(const WGeom &g, const Taps &t, int *K, int *flip);
int acg_wgrad_thin_patch_tiles(const WGeom &g);
int acg_wgrad_thin_patch_launch(const float *thin, const float *wide, float *part, const WGeom &g, const Taps &t, hipStream_t st);
int acg_wgrad_krow_s_launch(const float *x, const float *dy, float *part, const WGeom &g, hipStream_t st);

// conv_aux.hip: the support kernels of the entry points in conv_api.hip
int acg_thin_out_launch(const float *in, const float *wn, const float *bias, float *out, const Geom &g, const Taps &t, hipStream_t st);
int acg_dgrad_colfix_launch(const acg_conv_desc *d, const void *dy, const float *wb, long long w_lo_elems, float *colfix, hipStream_t st);
int acg_reflect_fold_launch(const acg_conv_desc *d, const float *dxp, float *dx, hipStream_t st);
int acg_reflect_fold_frame_launch(const acg_conv_desc *d, const float *dxp, float *dx, const float *addend, const float *relu_src,
                                  const unsigned *addend_mask, int out_s16, int relu_s16, hipStream_t st);
size_t acg_colsum_ws_bytes(long long M, int C);
int acg_colsum_launch(const float *dy, long long M, int C, int Cr, float *db, float *ws, hipStream_t st, int accumulate);
int acg_wgrad_reduce_launch(const float *part, int nsplit, int KK, int CiP, int CoP, int Or, int Ir, float *dw, int thin,
                            int accumulate, const float *bias_part, int Cp, int Cr, float *db, int bias_slots, hipStream_t st);
// conv_direct.hip: the naive cross-check kernels (ACG_IMPL_DIRECT)
int acg_direct_fwd_launch(const acg_conv_desc *d, const float *x, const float *wf, const float *bias, float *y, int act, hipStream_t st);
int acg_direct_dgrad_launch(const acg_conv_desc *d, const float *dy, const float *wb, const float *bias, float *dx, int act, hipStream_t st);
int acg_direct_wgrad_launch(const acg_conv_desc *d, const float *x, const float *dy, float *dw, int Or, int Ir, int accumulate, hipStream_t st);

#ifdef __HIPCC__
// bf16x3 operand split of 8 fp32 values: hi = RNE bf16(x), lo = RNE bf16(x - hi), each returned as 8 packed bf16
// (x = hi + lo + O(2^-17 |x|)).  Written pairwise so every conversion is one v_cvt_pk_bf16_f32 and the residuals one
// v_pk_add_f32: 20 VALU instructions per 8 values (a whole-vector __builtin_convertvector on gathered scalars
// compiles to one conversion per element).
typedef unsigned acg_u32x4 __attribute__((ext_vector_type(4)));
// byte offset of a buffer load, or 0xFFFFFFFF (range-checked by the buffer resource -> zeros) for a masked lane.
// Bit arithmetic on purpose: with `ok ? off : ~0u` LLVM sinks the load into both arms of a branch and separates the two
// copies with s_waitcnt vmcnt(0) (same destination registers), so every load of a stage pays a full memory latency —
// measured on the weight-gradient loaders: 0.89 -> 0.72 ms.
__device__ __forceinline__ unsigned acg_masked_off(unsigned off, bool ok)
{
    const unsigned keep = 0u - (unsigned)ok;
    return (off & keep) | ~keep;
}
__device__ __forceinline__ void acg_split8(const float (&v)[8], acg_u32x4 &hi, acg_u32x4 &lo)
{
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){v[2 * q], v[2 * q + 1]}, bf16x2_t));
        const float ha = __builtin_bit_cast(float, h << 16), hb = __builtin_bit_cast(float, h & 0xffff0000u);
        hi[q] = h;
        lo[q] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){v[2 * q] - ha, v[2 * q + 1] - hb}, bf16x2_t));
    }
}
__device__ __forceinline__ acg_u32x4 acg_round8(const float (&v)[8]) // bf16 mode: the hi part only
{
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    acg_u32x4 r;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        r[q] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){v[2 * q], v[2 * q + 1]}, bf16x2_t));
    return r;
}
#endif
