// Packed weight forms: which form each operand of a layer takes (operand_form), the buffer sizes that follow from it, one
// packer kernel per form, and the entry points that refresh the packed copies (one layer, or every regular layer of a network).
#include "conv_internal.h"

// w[o][i][tap] of the OIHW tensor (KK taps per channel pair), or 0 outside the real Or x Ir block
__device__ __forceinline__ float oihw(const float *__restrict__ w, int Or, int Ir, int KK, int o, int i, int tap)
{
    return (o < Or && i < Ir) ? w[((long long)o * Ir + i) * KK + tap] : 0.f;
}

// ---- regular forms: OIHW (real Or x Ir) -> wf [tap][Ci/8][CoP][8], wb [tap][Co/8][CiP][8] --------------------------------------
__global__ void pack_weight_kernel(const float *__restrict__ w, int Or, int Ir, int K, int Ci, int Co, int CoP, int CiP, float *__restrict__ wf, float *__restrict__ wb)
{
    const int KK = K * K;
    const long long nf = (long long)KK * (Ci / 8) * CoP * 8;
    const long long nb = (long long)KK * (Co / 8) * CiP * 8;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nf + nb; i += (long long)gridDim.x * blockDim.x) {
        const bool fwd = i < nf;
        float *const out = fwd ? wf : wb;
        if (out == nullptr) continue;
        const int Ck = fwd ? Ci : Co, ColP = fwd ? CoP : CiP;   // gathered channels, columns
        long long r = fwd ? i : i - nf;
        const int c8 = (int)(r % 8); r /= 8;
        const int col = (int)(r % ColP); r /= ColP;
        const int k = (int)(r % (Ck / 8)) * 8 + c8; r /= (Ck / 8);
        out[fwd ? i : i - nf] = fwd ? oihw(w, Or, Ir, KK, col, k, (int)r) : oihw(w, Or, Ir, KK, k, col, (int)r);
    }
}

// bf16 packing: wf16 [tap][Ci/16][CoP][16], wb16 [tap][Co/16][CiP][16] (same element counts, half the bytes)
// split != 0: also write lo = bf16(w - float(hi)) at [n_elems ...) of each buffer (the buffers are sized in floats)
// i0 / stride: the calling thread's first element and step over the layer's nf + nb elements
__device__ __forceinline__ void pack_bf16_body(const float *__restrict__ w, int Or, int Ir, int K, int Ci, int Co, int CoP, int CiP,
                                               __bf16 *__restrict__ wf, __bf16 *__restrict__ wb, int split, long long i0, long long stride)
{
    const int KK = K * K;
    const long long nf = (long long)KK * (Ci / 16) * CoP * 16;
    const long long nb = (long long)wb_slabs(K) * (Co / 16) * CiP * 16;
    for (long long i = i0; i < nf + nb; i += stride) {
        if (i < nf) {
            if (wf == nullptr) continue;
            long long r = i;
            const int c16 = (int)(r % 16); r /= 16;
            const int co = (int)(r % CoP); r /= CoP;
            const int cb = (int)(r % (Ci / 16)); r /= (Ci / 16);
            const int tap = (int)r;
            const int ci = cb * 16 + c16;
            const float v = oihw(w, Or, Ir, KK, co, ci, tap);
            const __bf16 hi = (__bf16)v;
            wf[i] = hi;
            if (split) wf[nf + i] = (__bf16)(v - (float)hi);
        } else {
            if (wb == nullptr) continue;
            long long r = i - nf;
            const int c16 = (int)(r % 16); r /= 16;
            const int ci = (int)(r % CiP); r /= CiP;
            const int cb = (int)(r % (Co / 16)); r /= (Co / 16);
            const int tap = (int)r;
            const int co = cb * 16 + c16;
            float v = 0.f;
            if (co < Or && ci < Ir) {
                const float *wv = w + ((long long)co * Ir + ci) * KK;
                v = tap < KK ? wv[tap] : wv[tap - KK] + wv[6 + tap - KK]; // slab 9 + kw: kernel rows 0 and 2 together
            }
            const __bf16 hi = (__bf16)v;
            wb[i - nf] = hi;
            if (split) wb[nb + i - nf] = (__bf16)(v - (float)hi);
        }
    }
}
__global__ void pack_weight_bf16_kernel(const float *__restrict__ w, int Or, int Ir, int K, int Ci, int Co, int CoP,
                                        int CiP, __bf16 *__restrict__ wf, __bf16 *__restrict__ wb, int split)
{
    pack_bf16_body(w, Or, Ir, K, Ci, Co, CoP, CiP, wf, wb, split, blockIdx.x * (long long)blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}
// every regular (non-thin) layer of a network in ONE launch (acg_pack_conv_weights_multi): the packed copies are refreshed once
// per optimiser step, and one launch per layer was 68 five-microsecond kernels per training step
#define PACK_MAX_ITEMS 48
struct PackTable {
    acg_pack_item it[PACK_MAX_ITEMS];
    int first[PACK_MAX_ITEMS + 1];   // first workgroup of item i
    short cop[PACK_MAX_ITEMS], cip[PACK_MAX_ITEMS];   // acg_ncols_pad of the item's Co / Ci
    int n, split;
};
__global__ __launch_bounds__(256) void pack_weight_bf16_multi_kernel(PackTable T)
{
    int k = 0;
    while (k + 1 < T.n && (int)blockIdx.x >= T.first[k + 1]) ++k;   // (uniform)
    const acg_pack_item q = T.it[k];
    const int nblk = T.first[k + 1] - T.first[k];
    pack_bf16_body(q.w, q.Or, q.Ir, q.K, q.Ci, q.Co, T.cop[k], T.cip[k], (__bf16 *)q.wf, (__bf16 *)q.wb, T.split,
                   ((long long)blockIdx.x - T.first[k]) * 256 + threadIdx.x, (long long)nblk * 256);
}

// ---- thin forms.  mode 0 packs wf (gathered channel = input channel, column = output channel), mode 1 packs wb (gathered
// channel = output channel, column = input channel): (gathered, column) -> (o, i) of the OIHW tensor
__device__ __forceinline__ float oihw_gc(const float *__restrict__ w, int Or, int Ir, int KK, int mode, int g, int col, int tap)
{
    return mode == 0 ? oihw(w, Or, Ir, KK, col, g, tap) : oihw(w, Or, Ir, KK, g, col, tap);
}

// thin-K packing: rows are k = tap*4 + c (c < 4 gathered channels), grouped in 8-chunks: out[kc][col][8]
__global__ void pack_weight_thin_kernel(const float *__restrict__ w, int Or, int Ir, int KK, int ColP, int mode,
                                        float *__restrict__ out)
{
    const int nkc = 4 * ((KK + 7) / 8);
    const long long total = (long long)nkc * ColP * 8;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int c8 = (int)(r % 8); r /= 8;
        const int col = (int)(r % ColP); r /= ColP;
        const int kflat = (int)r * 8 + c8;
        const int tap = kflat >> 2, c = kflat & 3;
        out[i] = tap < KK ? oihw_gc(w, Or, Ir, KK, mode, c, col, tap) : 0.f;
    }
}

// thin-N packing (the VALU thin-output kernel): out[(tap*Kc + k)*4 + n], n < 4 columns, k over the Kc gathered channels
__global__ void pack_weight_thinN_kernel(const float *__restrict__ w, int Or, int Ir, int KK, int Kc, int mode,
                                         float *__restrict__ out)
{
    const long long total = (long long)KK * Kc * 4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i & 3);
        const int k = (int)((i >> 2) % Kc);
        const int tap = (int)((i >> 2) / Kc);
        out[i] = oihw_gc(w, Or, Ir, KK, mode, k, n, tap);
    }
}

// Row-packed thin-K weights: out[hi | lo][ry][kg (4)][col (32)][8]: k = 8 kg + j = window column kw = 2 kg + (j >> 2), gathered
// channel ch = j & 3.  mode 0 (forward of a thin-input layer): tap (ry, kw); mode 1 (data gradient of a thin-output layer):
// the flipped kernel, tap (K-1-ry, K-1-kw).  Zero for kw >= K (the eighth column of a 7-wide row).
__global__ void pack_weight_trow_kernel(const float *__restrict__ w, int Or, int Ir, int K, int mode, __bf16 *__restrict__ out)
{
    const int total = K * 1024;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i & 7, col = (i >> 3) & 31, kg = (i >> 8) & 3, ry = i >> 10;
        const int kw = 2 * kg + (j >> 2), ch = j & 3;
        const int tap = mode == 0 ? ry * K + kw : (K - 1 - ry) * K + (K - 1 - kw);
        const float v = kw < K ? oihw_gc(w, Or, Ir, K * K, mode, ch, col, tap) : 0.f;
        const __bf16 hi = (__bf16)v;
        out[i] = hi;
        out[total + i] = (__bf16)(v - (float)hi);
    }
}

// N-packed weights: out[hi | lo][(ry * (K + 3) + u)][kg (4)][col (16)][8]: k = 8 kg + j is the gathered channel, col = 4 dxo + c
// the output pixel offset dxo and column channel c, window column kw = u - dxo.  mode 0 (forward of a thin-output layer): tap
// (ry, kw); mode 1 (data gradient of a thin-input layer): the window walks the flipped kernel, tap (K-1-ry, K-1-kw).  Zero
// where kw falls outside the kernel.
__global__ void pack_weight_npack_kernel(const float *__restrict__ w, int Or, int Ir, int K, int mode, __bf16 *__restrict__ out)
{
    const int KU = K + 3, total = K * KU * 512;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i & 7, col = (i >> 3) & 15, kg = (i >> 7) & 3, slab = i >> 9;
        const int ry = slab / KU, u = slab - ry * KU, dxo = col >> 2, c = col & 3, k = kg * 8 + j, kw = u - dxo;
        const int tap = mode == 0 ? ry * K + kw : (K - 1 - ry) * K + (K - 1 - kw);
        const float v = kw >= 0 && kw < K ? oihw_gc(w, Or, Ir, K * K, mode, k, c, tap) : 0.f;
        const __bf16 hi = (__bf16)v;
        out[i] = hi;
        out[total + i] = (__bf16)(v - (float)hi);
    }
}

// ---- which form an operand takes, in the current precision and implementation ------------------------------------------------
// A thin layer (<= 4 real channels on exactly one side) packs each operand in the layout its kernel wants; all fit in the
// regular-size region:
//   Cin <= 4 : wf = thin-K (flattened taps, MFMA fwd)   wb = thin-N (VALU data gradient into the image)
//   Cout <= 4: wf = thin-N (VALU forward)               wb = thin-K (MFMA data gradient gathers thin dy)
// where the VALU kernel does not take the layer (thin_valu_c) the thin-N side stays regular.  A regular operand follows the
// precision mode.  The tails are written in the bf16x3 arithmetic only: the N-packed one behind the operand whose COLUMNS
// are the thin side, the row-packed one behind the operand that GATHERS the thin side.
enum { FORM_F32, FORM_BF16, FORM_THIN_K, FORM_THIN_N };
struct OperandForm {
    int main, tail;      // FORM_*, ACG_TAIL_* (the tail the buffer has room for)
    bool tail_live;      // ... and whether the current mode writes it
    size_t tail_off;     // floats: the regular region's size
    size_t elems;        // floats: the whole buffer
};
static OperandForm operand_form(int mode, int Or, int Ir, int K, int Ci, int Co)   // mode 0: wf, 1: wb
{
    const int Ck = mode ? Co : Ci, Cn = mode ? Ci : Co, gathered_real = mode ? Or : Ir, column_real = mode ? Ir : Or;
    const bool thin_g = thin_ok(gathered_real, K) && !thin_ok(column_real, K), thin_c = thin_ok(column_real, K) && !thin_ok(gathered_real, K);
    OperandForm f;
    f.main = thin_g ? FORM_THIN_K : (thin_c && thin_valu_c(Ck) ? FORM_THIN_N : (use_bf16() ? FORM_BF16 : FORM_F32));
    f.tail = pack_tail(K, Ck, Cn);
    f.tail_live = bf16x3_mfma() && ((f.tail == ACG_TAIL_NPACK && thin_c) || (f.tail == ACG_TAIL_TROW && thin_g));
    f.tail_off = mode ? wb_regular_elems(K, Ci, Co) : wf_regular_elems(K, Ci, Co);
    f.elems = f.tail_off + pack_tail_elems(f.tail, K);
    return f;
}
// the buffer sizes depend on the padded shape alone (real counts = padded counts: no thin side)
extern "C" size_t acg_packed_wf_elems(int K, int Ci, int Co) { return operand_form(0, Co, Ci, K, Ci, Co).elems; }
extern "C" size_t acg_packed_wb_elems(int K, int Ci, int Co) { return operand_form(1, Co, Ci, K, Ci, Co).elems; }

// the regular form of either or both operands (a null one is skipped)
static void pack_regular(const float *w, int Or, int Ir, int K, int Ci, int Co, float *wf, float *wb, int blocks, hipStream_t st)
{
    if (use_bf16())
        hipLaunchKernelGGL(pack_weight_bf16_kernel, dim3(blocks), dim3(256), 0, st, w, Or, Ir, K, Ci, Co, acg_ncols_pad(Co),
                           acg_ncols_pad(Ci), (__bf16 *)wf, (__bf16 *)wb, (int)(g_acg_precision == ACG_PREC_BF16X3));
    else
        hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks), dim3(256), 0, st, w, Or, Ir, K, Ci, Co, acg_ncols_pad(Co),
                           acg_ncols_pad(Ci), wf, wb);
}

// a thin layer's operands: `thin` gathers the thin side (thin-K, row-packed tail), `wide` has it as columns
struct PackOperand { float *out; int mode; OperandForm f; };   // out may be null: skipped
static void pack_thin_layer(const float *w, int Or, int Ir, int K, int Ci, int Co, const PackOperand &thin, const PackOperand &wide, int blocks, hipStream_t st)
{
    auto main_form = [&](const PackOperand &p) {
        const int Ck = p.mode ? Co : Ci, Cn = p.mode ? Ci : Co;
        if (p.out == nullptr) return;
        if (p.f.main == FORM_THIN_K)
            hipLaunchKernelGGL(pack_weight_thin_kernel, dim3(64), dim3(256), 0, st, w, Or, Ir, K * K, acg_ncols_pad(Cn), p.mode, p.out);
        else if (p.f.main == FORM_THIN_N)
            hipLaunchKernelGGL(pack_weight_thinN_kernel, dim3(64), dim3(256), 0, st, w, Or, Ir, K * K, Ck, p.mode, p.out);
        else   // the wide operand where its kernel is the regular MFMA one
            pack_regular(w, Or, Ir, K, Ci, Co, p.mode ? nullptr : p.out, p.mode ? p.out : nullptr, blocks, st);
    };
    main_form(thin.mode == 0 ? thin : wide);   // wf, then wb
    main_form(thin.mode == 0 ? wide : thin);
    if (wide.out && wide.f.tail_live)
        hipLaunchKernelGGL(pack_weight_npack_kernel, dim3(64), dim3(256), 0, st, w, Or, Ir, K, wide.mode, (__bf16 *)(wide.out + wide.f.tail_off));
    if (thin.out && thin.f.tail_live)
        hipLaunchKernelGGL(pack_weight_trow_kernel, dim3(28), dim3(256), 0, st, w, Or, Ir, K, thin.mode, (__bf16 *)(thin.out + thin.f.tail_off));
}

extern "C" int acg_pack_conv_weight(const float *w, int Or, int Ir, int K, int Ci, int Co, float *wf, float *wb, void *stream)
{
    ACG_REQUIRE(Ci % 16 == 0 && Co % 16 == 0 && Or <= Co && Ir <= Ci && K >= 1 && K <= 7,
                "acg_pack_conv_weight: bad dims Or=%d Ir=%d K=%d Ci=%d Co=%d", Or, Ir, K, Ci, Co);
    const PackOperand f = {wf, 0, operand_form(0, Or, Ir, K, Ci, Co)}, b = {wb, 1, operand_form(1, Or, Ir, K, Ci, Co)};
    const long long n = (long long)f.f.elems + (long long)b.f.elems;
    const int blocks = acg_cdiv(n, 256) > 2048 ? 2048 : acg_cdiv(n, 256);
    if (f.f.main == FORM_THIN_K || b.f.main == FORM_THIN_K) {
        if (f.f.main == FORM_THIN_K) pack_thin_layer(w, Or, Ir, K, Ci, Co, f, b, blocks, (hipStream_t)stream);
        else pack_thin_layer(w, Or, Ir, K, Ci, Co, b, f, blocks, (hipStream_t)stream);
        ACG_CHECK_LAUNCH("pack_weight_thin_kernel");
        return ACG_OK;
    }
    pack_regular(w, Or, Ir, K, Ci, Co, wf, wb, blocks, (hipStream_t)stream);
    ACG_CHECK_LAUNCH("pack_weight_kernel");
    return ACG_OK;
}

// the same for the regular layers of a whole network at once (bf16 / bf16x3 arithmetic; thin layers keep acg_pack_conv_weight)
extern "C" int acg_pack_conv_weights_multi_supported(int Or, int Ir, int K)
{
    return use_bf16() && thin_ok(Ir, K) == thin_ok(Or, K) ? 1 : 0;
}
extern "C" int acg_pack_conv_weights_multi(const acg_pack_item *items, int n, void *stream)
{
    ACG_REQUIRE(items != nullptr && n >= 1 && use_bf16(), "acg_pack_conv_weights_multi: bf16 / bf16x3 arithmetic only (see acg_pack_conv_weights_multi_supported)");
    for (int base = 0; base < n; base += PACK_MAX_ITEMS) {
        PackTable T;
        T.n = n - base < PACK_MAX_ITEMS ? n - base : PACK_MAX_ITEMS;
        T.split = (int)(g_acg_precision == ACG_PREC_BF16X3);
        T.first[0] = 0;
        for (int i = 0; i < T.n; ++i) {
            const acg_pack_item &q = items[base + i];
            ACG_REQUIRE(q.w != nullptr && q.wf != nullptr && q.wb != nullptr && q.Ci % 16 == 0 && q.Co % 16 == 0 && q.Or <= q.Co && q.Ir <= q.Ci && q.K >= 1 && q.K <= 7 &&
                        acg_pack_conv_weights_multi_supported(q.Or, q.Ir, q.K),
                        "acg_pack_conv_weights_multi: item %d: bad dims or a thin layer (Or=%d Ir=%d K=%d Ci=%d Co=%d)", base + i, q.Or, q.Ir, q.K, q.Ci, q.Co);
            T.it[i] = q;
            T.cop[i] = (short)acg_ncols_pad(q.Co); T.cip[i] = (short)acg_ncols_pad(q.Ci);
            const long long ne = (long long)acg_packed_wf_elems(q.K, q.Ci, q.Co) + (long long)acg_packed_wb_elems(q.K, q.Ci, q.Co);
            const int nb = acg_cdiv(ne, 256 * 8) > 256 ? 256 : acg_cdiv(ne, 256 * 8);   // ~8 elements per thread
            T.first[i + 1] = T.first[i] + (nb < 1 ? 1 : nb);
        }
        hipLaunchKernelGGL(pack_weight_bf16_multi_kernel, dim3(T.first[T.n]), dim3(256), 0, (hipStream_t)stream, T);
        ACG_CHECK_LAUNCH("pack_weight_bf16_multi_kernel");
    }
    return ACG_OK;
}

__global__ void pad_vector_kernel(const float *__restrict__ s, int n, float *__restrict__ d, int np)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) d[i] = i < n ? s[i] : 0.f;
}
extern "C" int acg_pad_vector(const float *src, int n, float *dst, int np, void *stream)
{
    hipLaunchKernelGGL(pad_vector_kernel, dim3(acg_cdiv(np, 256)), dim3(256), 0, (hipStream_t)stream, src, n, dst, np);
    ACG_CHECK_LAUNCH("pad_vector_kernel");
    return ACG_OK;
}
