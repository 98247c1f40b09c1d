// Convolution entry points of the C ABI: descriptor checks, geometry -> tap lists, the dispatch to the kernel families and
// the split-K plan of the weight gradient.  Host code only: the packed weight forms live in conv_pack.hip, the support
// kernels (thin-output convolution, reflection-pad folds, column sums, split-K reduction) in conv_aux.hip, the naive
// cross-check kernels in conv_direct.hip; what they share with the dispatch is stated once in conv_internal.h.
#include "conv_internal.h"

int g_acg_conv_impl = ACG_IMPL_MFMA;
int g_acg_precision = ACG_PREC_BF16X3;
extern "C" int acg_set_conv_precision(int prec)
{
    ACG_REQUIRE(prec == ACG_PREC_F32 || prec == ACG_PREC_BF16 || prec == ACG_PREC_BF16X3, "acg_set_conv_precision: unknown precision %d", prec);
    g_acg_precision = prec;
    return ACG_OK;
}
extern "C" int acg_set_conv_impl(int impl)
{
    ACG_REQUIRE(impl == ACG_IMPL_MFMA || impl == ACG_IMPL_DIRECT, "acg_set_conv_impl: unknown impl %d", impl);
    g_acg_conv_impl = impl;
    return ACG_OK;
}
// the layers the VALU thin-output kernel takes (conv_aux.hip; their thin-N packing: conv_pack.hip)
static bool thin_out_valu_fwd(const acg_conv_desc *d) { return thin_out(d) && thin_valu_c(d->Ci); }
static bool thin_in_valu_dgrad(const acg_conv_desc *d) { return thin_in(d) && thin_valu_c(d->Co); }

// ---- descriptor checks + tap-list builders ----------------------------------------------------------------------------------
static int check_desc(const acg_conv_desc *d, const char *who)
{
    ACG_REQUIRE(d != nullptr, "%s: null descriptor", who);
    ACG_REQUIRE(d->N > 0 && d->Hi > 0 && d->Wi > 0 && d->Ho > 0 && d->Wo > 0, "%s: empty tensor", who);
    // stored channel counts: multiples of 16, or 4 for a tensor of <= 4 real channels on the thin side of a thin layer (K > 1,
    // the other side wider: what thin_in / thin_out select) — every other kernel gathers 16-channel chunks
    ACG_REQUIRE(d->Ci > 0 && d->Co > 0 && (d->Ci % 16 == 0 || d->Ci == 4) && (d->Co % 16 == 0 || d->Co == 4),
                "%s: channels must be padded to 16, or to 4 for image tensors (Ci=%d Co=%d)", who, d->Ci, d->Co);
    ACG_REQUIRE(d->Ci != 4 || (d->Cir >= 1 && d->Cir <= 4 && d->K > 1 && !(d->Cor >= 1 && d->Cor <= 4)),
                "%s: a 4-channel input needs a thin-input layer (Cir=%d Cor=%d K=%d)", who, d->Cir, d->Cor, d->K);
    ACG_REQUIRE(d->Co != 4 || (d->Cor >= 1 && d->Cor <= 4 && d->K > 1 && !(d->Cir >= 1 && d->Cir <= 4)),
                "%s: a 4-channel output needs a thin-output layer (Cir=%d Cor=%d K=%d)", who, d->Cir, d->Cor, d->K);
    ACG_REQUIRE(d->K >= 1 && d->K <= 7 && (d->stride == 1 || d->stride == 2), "%s: K=%d stride=%d unsupported", who,
                d->K, d->stride);
    ACG_REQUIRE(d->pad >= 0 && d->pad < d->K, "%s: pad=%d", who, d->pad);
    ACG_REQUIRE(d->Ho == (d->Hi + 2 * d->pad - d->K) / d->stride + 1 && d->Wo == (d->Wi + 2 * d->pad - d->K) / d->stride + 1,
                "%s: output size %dx%d inconsistent with input %dx%d K=%d s=%d p=%d", who, d->Ho, d->Wo, d->Hi, d->Wi,
                d->K, d->stride, d->pad);
    if (d->pad_mode == ACG_PAD_REFLECT)
        ACG_REQUIRE(d->stride == 1 && d->pad < d->Hi && d->pad < d->Wi, "%s: reflect pad needs stride 1 and pad < size", who);
    return ACG_OK;
}

#define ACG_CHECK_DESC(d, who) do { if (int rc__ = check_desc(d, who)) return rc__; } while (0)
// refusal of a workspace that is missing or shorter than `need` (who: the name the message carries)
static int ws_check(const char *who, const void *ws, size_t ws_bytes, size_t need)
{
    if (ws != nullptr && ws_bytes >= need) return ACG_OK;
    acg_set_error("%s: workspace %zu < %zu", who, ws_bytes, need);
    return ACG_ERR_WORKSPACE;
}

// the K x K tap list in kernel order: tap (kh, kw) gathers pixel (base + step kh, base + step kw) relative to the grid position
static void square_taps(Taps *t, int K, int base, int step)
{
    t->n = 0;
    for (int kh = 0; kh < K; ++kh)
        for (int kw = 0; kw < K; ++kw) {
            t->dy[t->n] = (short)(base + step * kh); t->dx[t->n] = (short)(base + step * kw); t->w[t->n] = (short)(kh * K + kw);
            t->n++;
        }
}

static void fwd_geom(const acg_conv_desc *d, Geom *g, Taps *t, int act)
{
    g->Hin = d->Hi; g->Win = d->Wi; g->Cin = d->Ci;
    g->Hout = d->Ho; g->Wout = d->Wo; g->Cout = d->Co;
    g->GH = d->Ho; g->GW = d->Wo; g->os = 1; g->oy0 = 0; g->ox0 = 0; g->is = d->stride;
    g->reflect = d->pad_mode == ACG_PAD_REFLECT; g->ncols_pad = acg_ncols_pad(d->Co);
    g->act = act == ACG_ACT_SIGMOID ? acg_act_sigmoid_ch(d->Cor > 0 ? d->Cor : d->Co) : act;
    g->Mtot = (long long)d->N * d->Ho * d->Wo;
    g->thin = thin_in(d) ? 1 : 0;
    g->w_elems = (long long)wf_regular_elems(d->K, d->Ci, d->Co);
    square_taps(t, d->K, -d->pad, 1);
}

// data gradient (and ConvTranspose forward): gathers from the conv-OUTPUT side tensor `src`
// (N,Ho,Wo,Co) with packed wb, writes the conv-INPUT side tensor `dst` (N,Hi,Wi,Ci).
// (DgradSide.addend / relu_src: only the frame path and the un-padded grid below implement them)
static void dgrad_geom(const acg_conv_desc *d, int act, Geom *g)   // the fields both strides share
{
    g->Hin = d->Ho; g->Win = d->Wo; g->Cin = d->Co;
    g->Cout = d->Ci; g->reflect = 0; g->act = act; g->ncols_pad = acg_ncols_pad(d->Ci); g->is = 1;
    g->thin = (d->stride == 1 && thin_out(d)) ? 1 : 0;
    g->w_elems = (long long)wb_regular_elems(d->K, d->Ci, d->Co);
}

// Stride 1: the grid is the padded one (Hi+2p x Wi+2p, folded afterwards) for a reflect-padded layer, else the Hi x Wi input.
// unpad: the un-padded grid of the pre-split reflect data gradient (Geom.unpad).  Zero padding: dy row = iy + p - kh; reflect
// (padded grid): dy row = py - kh.  t may be null (the dispatch queries that need only the Geom).
static void dgrad_s1_geom(const acg_conv_desc *d, int act, bool unpad, Geom *g, Taps *t)
{
    dgrad_geom(d, act, g);
    const int e = d->pad_mode == ACG_PAD_REFLECT && !unpad ? d->pad : 0;
    g->Hout = d->Hi + 2 * e; g->Wout = d->Wi + 2 * e; g->GH = g->Hout; g->GW = g->Wout;
    g->os = 1; g->oy0 = 0; g->ox0 = 0;
    g->Mtot = (long long)d->N * g->GH * g->GW;
    if (t != nullptr) square_taps(t, d->K, d->pad - e, -1);
}

static bool dgrad_frame_ok(const acg_conv_desc *d, const Geom &g)
{
    const int p = d->pad;
    return d->stride == 1 && d->pad_mode == ACG_PAD_REFLECT && p > 0 && !thin_in_valu_dgrad(d) && acg_igemm_uses_ws(g) &&
           d->Hi > 4 * p + 1 && d->Wi > 4 * p + 1;
}

// the un-padded grid of the pre-split reflect data gradient (Geom.unpad): 3x3, pad 1, rows that are whole 128-pixel tiles
static bool dgrad_unpad_ok(const acg_conv_desc *d)
{
    return d->stride == 1 && d->pad_mode == ACG_PAD_REFLECT && d->K == 3 && d->pad == 1 && d->Wi % 128 == 0 &&
           d->Hi % 32 == 0 && d->Hi >= 64 && d->Co % 128 == 0;
}

// a sign bitmask over a tensor of dx's shape (one bit per element, acg_norm_apply's layout) as the kernels index it
static bool sign_mask_fits(const acg_conv_desc *d) { return ((long long)d->Hi * d->Wi * (d->Ci / 4)) % 8 == 0; }

// the fused side inputs of a data gradient (the acg_conv2d_bwd_data* entry points, the ConvTranspose2d forwards): all optional
struct DgradSide {
    const float *addend = nullptr, *relu_src = nullptr;   // dst = (gradient + addend) masked by relu_src > 0; both of dst's shape
    const unsigned *addend_mask = nullptr, *relu_mask = nullptr;   // sign bitmask gating the addend / standing in for relu_src
    int in_s16 = 0, out_s16 = 0, relu_s16 = 0;            // src / dst / relu_src are pre-split
    float *stats = nullptr;                               // per-tile (mean, M2) of dst (ConvTranspose2d forward)
    const acg_norm_sums *ns = nullptr;                    // the norm in front: its backward sums leave with the tiles
};

// what the pre-split kernel can combine: a pre-split ReLU source only with pre-split output, an addend only with fp32 output
static bool presplit_combo_ok(const Geom &g, const Taps &t, const DgradSide &s)
{
    return acg_igemm_x3_pre_ok(g, t) && (s.relu_s16 == 0 || s.out_s16) && (s.out_s16 == 0 || s.addend == nullptr) &&
           (s.relu_src == nullptr || s.relu_s16 == s.out_s16);
}

// *ns -> g's ns_* fields.  Returns whether it is well-formed for rows of C channels (a sums buffer; per-sample scale / shift
// rows at least C wide in whole float4s): what the un-padded pre-split path asks; the fp32-operand paths have their own conditions
static bool geom_norm_sums(Geom *g, const acg_norm_sums *ns, int C)
{
    g->ns_x = ns->x; g->ns_mean = ns->mean; g->ns_rstd = ns->rstd; g->ns_gamma = ns->gamma; g->ns_beta = ns->beta;
    g->ns_gstride = ns->gstride; g->ns_mask = ns->sign_mask; g->ns_act = ns->act; g->ns_part = ns->part;
    return ns->part != nullptr && (ns->gstride == 0 || (ns->gstride >= C && ns->gstride % 4 == 0));
}

static int dgrad_igemm(const acg_conv_desc *d, const float *src, const float *wb, const float *bias, float *dst, int act,
                       void *ws, size_t ws_bytes, hipStream_t st, const DgradSide &s)
{
    const acg_norm_sums *const ns = s.ns;
    ACG_REQUIRE(act != ACG_ACT_SIGMOID, "dgrad / ConvTranspose2d: no sigmoid epilogue");
    Geom g; Taps t;
    const int p = d->pad, K = d->K;
    if (d->stride == 1) {
        const bool refl = d->pad_mode == ACG_PAD_REFLECT && p > 0;   // compute on the padded grid, then fold
        dgrad_s1_geom(d, act, false, &g, &t);
        float *out = dst;
        if (refl) {
            const size_t need = (size_t)d->N * (d->Hi + 2 * p) * (d->Wi + 2 * p) * d->Ci * sizeof(float);
            if (int rc = ws_check("acg_conv2d_bwd_data", ws, ws_bytes, need)) return rc;
            ACG_REQUIRE(bias == nullptr && act == ACG_ACT_NONE, "dgrad: reflect with epilogue unsupported");
            out = (float *)ws;
        }
        // Pre-split operands, 3x3, pad 1, rows that are whole tiles: the un-padded grid (Geom.unpad) — 3 % fewer tiles than the
        // padded grid, one row segment per tile, and the fold pass over the frame goes away
        if (refl && s.in_s16 && dgrad_unpad_ok(d) && dgrad_frame_ok(d, g)) {
            dgrad_s1_geom(d, act, true, &g, &t);
            ACG_REQUIRE(presplit_combo_ok(g, t, s) && d->Co % 128 == 0,
                        "dgrad: unsupported pre-split combination (query acg_conv2d_s16_supported)");
            if (int rc = acg_dgrad_colfix_launch(d, src, wb, g.w_elems, (float *)ws, st)) return rc;
            g.unpad = 1; g.colfix = (const float *)ws; g.out2 = dst; g.addend = s.addend; g.relu_src = s.relu_src; g.addend_mask = s.addend_mask;
            g.out_s16 = s.out_s16; g.relu_s16 = s.relu_s16; g.relu_mask = s.relu_mask;
            if (ns != nullptr) ACG_REQUIRE(geom_norm_sums(&g, ns, d->Ci), "dgrad: bad acg_norm_sums");
            return acg_igemm_x3_pre_launch(src, wb, bias, dst, g, t, g.w_elems, st);
        }
        ACG_REQUIRE((ns == nullptr || (!refl && !s.in_s16 && !s.out_s16 && s.addend == nullptr && s.relu_src == nullptr)) && s.relu_mask == nullptr,
                    "dgrad: norm sums / a sign bitmask as the ReLU source need the un-padded pre-split path or the row pipeline (query acg_conv2d_bwd_data_s16_sums_supported / acg_conv2d_bwd_data_sums_supported)");
        // the wave-specialised kernel stores the pixels nothing is mirrored onto straight into dst: only the frame is folded
        const bool frame = refl && dgrad_frame_ok(d, g);
        ACG_REQUIRE((s.addend == nullptr && s.relu_src == nullptr) || frame,
                    "dgrad: the fused addend / ReLU mask need the frame path (query acg_conv2d_bwd_data_add_supported)");
        if (frame) { g.fold_p = p; g.fold_H = d->Hi; g.fold_W = d->Wi; g.out2 = dst; g.addend = s.addend; g.relu_src = s.relu_src; g.addend_mask = s.addend_mask; }
        int rc;
        if (s.in_s16 || s.out_s16 || s.relu_s16) { // pre-split operands: the frame path of the pre-split kernel only
            ACG_REQUIRE(s.in_s16 && frame && presplit_combo_ok(g, t, s),
                        "dgrad: unsupported pre-split combination (query acg_conv2d_s16_supported)");
            g.out_s16 = s.out_s16; g.relu_s16 = s.relu_s16;
            rc = acg_igemm_x3_pre_launch(src, wb, bias, out, g, t, g.w_elems, st);
        } else {
            if (ns != nullptr) {   // fp32 operands: only the persistent row pipeline (conv_rows.hip) emits the norm-backward sums
                geom_norm_sums(&g, ns, d->Ci);
                // (which kernel takes them is checked where the launch is dispatched: conv_bf16.hip / conv_igemm.hip refuse a
                // geometry that would land on a kernel without the sums epilogue)
                ACG_REQUIRE(ns->part != nullptr && !thin_in_valu_dgrad(d) && !frame && acg_conv2d_bwd_data_sums_supported(d),
                            "dgrad: norm sums on fp32 operands: unsupported geometry (query acg_conv2d_bwd_data_sums_supported)");
            }
            rc = thin_in_valu_dgrad(d) ? acg_thin_out_launch(src, wb, bias, out, g, t, st) : acg_igemm_launch(src, wb, bias, out, g, t, st);
        }
        if (rc != ACG_OK) return rc;
        if (frame)
            return acg_reflect_fold_frame_launch(d, (const float *)ws, dst, s.addend, s.relu_src, s.addend_mask, s.out_s16, s.relu_s16, st);
        return refl ? acg_reflect_fold_launch(d, (const float *)ws, dst, st) : ACG_OK;
    }
    ACG_REQUIRE(!thin_out(d), "dgrad: stride 2 with <= 4 output channels is not supported by the thin packing");
    // stride 2: four sub-pixel phases, each a dense small-tap convolution (no zero insertion)
    ACG_REQUIRE(d->pad_mode == ACG_PAD_ZERO, "dgrad: stride 2 needs zero padding");
    ACG_REQUIRE(s.addend == nullptr && s.relu_src == nullptr && s.relu_mask == nullptr && !s.in_s16 && !s.out_s16, "dgrad: stride 2 takes no fused side inputs");
    ACG_REQUIRE(ns == nullptr || acg_conv2d_bwd_data_sums_supported(d), "dgrad: norm sums on this stride-2 geometry (query acg_conv2d_bwd_data_sums_supported)");
    dgrad_geom(d, act, &g);
    g.Hout = d->Hi; g.Wout = d->Wi; g.os = 2;
    auto phase_taps = [&](int py, int px, Taps &tt, int base) {
        int n = 0;
        for (int kh = 0; kh < K; ++kh) {
            if ((py + p - kh) & 1) continue;
            for (int kw = 0; kw < K; ++kw) {
                if ((px + p - kw) & 1) continue;
                tt.dy[base + n] = (short)((py + p - kh) / 2); tt.dx[base + n] = (short)((px + p - kw) / 2);
                tt.w[base + n] = (short)(kh * K + kw);
                n++;
            }
        }
        return n;
    };
    // One launch for the four phases where the generic bf16 tile runs them anyway: even output sizes (equal phase grids of
    // whole 128-pixel tiles), at most 16 taps per phase.  The phases of a tile read the same rows of `src`: side by side on
    // one XCD they fetch them from HBM once (four launches: 2.0x the algorithmic traffic, profiles/r02_a_layer_traffic).
    g.GH = d->Hi / 2; g.GW = d->Wi / 2; g.oy0 = 0; g.ox0 = 0;
    g.Mtot = (long long)d->N * g.GH * g.GW;
    if (d->Hi % 2 == 0 && d->Wi % 2 == 0 && g.Mtot % 128 == 0 && (K + 1) / 2 * ((K + 1) / 2) <= 16 &&
        g_acg_precision != ACG_PREC_F32 && g_acg_conv_impl == ACG_IMPL_MFMA && !g.thin && !thin_in_valu_dgrad(d) && !thin_out(d) &&
        !acg_igemm_uses_ws(g)) {
        t.n = 64;
        for (int i = 0; i < 64; ++i) { t.dy[i] = 0; t.dx[i] = 0; t.w[i] = 0; }
        g.nphase = 4;
        g.ph_ntaps = 0;
        int ntp[4];
        for (int ph = 0; ph < 4; ++ph) {
            const int nt = phase_taps(ph >> 1, ph & 1, t, 16 * ph);
            ACG_REQUIRE(nt > 0, "dgrad: empty phase (K=%d p=%d)", K, p);
            g.ph_ntaps |= nt << (8 * ph);
            ntp[ph] = nt;
        }
        if (s.stats != nullptr) {
            const int per = (int)(((long long)g.GH * g.GW) / 128);
            g.stats = s.stats; g.stats_cpi = 4 * per; g.stats_chunk0 = 0;
        }
        // 64 output channels in the bf16x3 arithmetic: all four phases in one tile, the input rows fetched once (conv_ph4.hip)
        Geom g4 = g;
        g4.nphase = 0; g4.ph_ntaps = 0;
        Taps plan;
        if (ns != nullptr) {   // the first backward pass of the norm in front of the stride-2 convolution rides on the four-phase tile
            geom_norm_sums(&g4, ns, d->Ci);
            ACG_REQUIRE(ns->part != nullptr && s.stats == nullptr && acg_igemm_ph4_ok(g4) && acg_ph4_plan(t, ntp, &plan),
                        "dgrad: norm sums on a stride-2 data gradient need the four-phase tile (query acg_conv2d_bwd_data_sums_supported)");
            return acg_igemm_ph4_launch(src, wb, bias, dst, g4, plan, g.w_elems, st);
        }
        if (acg_igemm_ph4_ok(g4) && acg_ph4_plan(t, ntp, &plan)) return acg_igemm_ph4_launch(src, wb, bias, dst, g4, plan, g.w_elems, st);
        return acg_igemm_launch(src, wb, bias, dst, g, t, st);
    }

    ACG_REQUIRE(ns == nullptr, "dgrad: norm sums on a stride-2 data gradient need the four-phase tile (query acg_conv2d_bwd_data_sums_supported)");
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            g.oy0 = py; g.ox0 = px;
            g.GH = (d->Hi - py + 1) / 2; g.GW = (d->Wi - px + 1) / 2;
            g.Mtot = (long long)d->N * g.GH * g.GW;
            t.n = phase_taps(py, px, t, 0);
            ACG_REQUIRE(t.n > 0, "dgrad: empty phase (K=%d p=%d)", K, p);
            if (s.stats != nullptr) { // each phase owns a quarter of every image's 128-pixel chunks
                const int per = (int)(((long long)g.GH * g.GW) / 128);
                g.stats = s.stats; g.stats_cpi = 4 * per; g.stats_chunk0 = (py * 2 + px) * per;
            }
            int rc = thin_in_valu_dgrad(d) ? acg_thin_out_launch(src, wb, bias, dst, g, t, st) : acg_igemm_launch(src, wb, bias, dst, g, t, st);
            if (rc != ACG_OK) return rc;
        }
    return ACG_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------
extern "C" int acg_conv2d_fwd(const acg_conv_desc *d, const float *x, const float *wf, const float *bias, float *y,
                              int act, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_fwd");
    ACG_REQUIRE(act >= ACG_ACT_NONE && act <= ACG_ACT_SIGMOID, "acg_conv2d_fwd: unknown activation %d", act);
    // the sigmoid stores 0 in the padded channels: it needs the real count (the head convolutions of the discriminators)
    ACG_REQUIRE(act != ACG_ACT_SIGMOID || (d->Cor >= 1 && d->Cor <= d->Co), "acg_conv2d_fwd: sigmoid needs Cor (real Co) in 1..Co");
    hipStream_t st = (hipStream_t)stream;
    if (g_acg_conv_impl == ACG_IMPL_DIRECT) return acg_direct_fwd_launch(d, x, wf, bias, y, act, st);
    Geom g; Taps t;
    fwd_geom(d, &g, &t, act);
    if (thin_out_valu_fwd(d)) return acg_thin_out_launch(x, wf, bias, y, g, t, st);
    return acg_igemm_launch(x, wf, bias, y, g, t, st);
}

// Forward convolution that ALSO emits per-128-pixel-tile (mean, M2) of its output for the InstanceNorm behind it
// (modules.py:24-31 computes those statistics from the conv output in a separate pass).  Only the wave-specialised
// bf16x3 kernel implements it: 128-column tiles, Cin % 32 == 0, Ho*Wo % 128 == 0.  stats: [N][Ho*Wo/128][2][Co].
extern "C" int acg_conv2d_fwd_stats_supported(const acg_conv_desc *d)
{
    if (d == nullptr || g_acg_precision == ACG_PREC_F32 || g_acg_conv_impl != ACG_IMPL_MFMA) return 0;
    // the C4 image -> 32 channel stem (conv_thinrow_x3): statistics over its 8 x 16 pixel tiles
    if (thin_in(d) && d->Ci == 4 && d->Co == 32 && d->stride == 1 && d->K <= 7 && g_acg_precision == ACG_PREC_BF16X3 && d->Ho % 8 == 0 &&
        d->Wo % 16 == 0)
        return 1;
    if (thin_in(d) || thin_out(d) || d->Co < 32 || d->Ci % 16 != 0) return 0;    // MFMA tiles of the bf16 kernels only
    return ((long long)d->Ho * d->Wo) % 128 == 0 ? 1 : 0;
}

// Are the statistics acg_conv2d_fwd_stats emits for d those of each 128-pixel tile on its own (1), or may entries be the joint
// statistics of several tiles (0)?  The row pipeline (conv_rows.hip) writes the joint (mean, M2) of the rows a workgroup owns,
// and that count follows the batch: the merged mean / rstd of an image then depend, in their last bits, on how many images
// share the launch.  A caller that needs a pass to be bit-identical across batch sizes (the ensemble groups of the evaluator)
// asks here and leaves the statistics to the norm's own pass (acg_norm_stats: fixed chunks per image) where the answer is 0.
extern "C" int acg_conv2d_fwd_stats_per_tile(const acg_conv_desc *d)
{
    if (!acg_conv2d_fwd_stats_supported(d)) return 0;
    if (thin_in(d)) return 1;   // the thin-row stem: one entry per 8 x 16 tile
    Geom g; Taps t;
    static float probe;   // (only compared with nullptr)
    fwd_geom(d, &g, &t, ACG_ACT_NONE);
    g.stats = &probe; g.stats_chunk0 = 0; g.stats_cpi = (int)(((long long)d->Ho * d->Wo) / 128);
    return !acg_igemm_uses_ws(g) && acg_conv_rows_ok(g, t) ? 0 : 1;   // (the dispatch order of acg_igemm_bf16_launch)
}

extern "C" int acg_conv2d_fwd_stats(const acg_conv_desc *d, const float *x, const float *wf, const float *bias, float *y,
                                    float *stats, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_fwd_stats");
    ACG_REQUIRE(acg_conv2d_fwd_stats_supported(d) && stats != nullptr, "acg_conv2d_fwd_stats: unsupported shape or mode");
    Geom g; Taps t;
    fwd_geom(d, &g, &t, ACG_ACT_NONE);
    g.stats = stats; g.stats_chunk0 = 0; g.stats_cpi = (int)(((long long)d->Ho * d->Wo) / 128);
    return acg_igemm_launch(x, wf, bias, y, g, t, (hipStream_t)stream);
}

// ConvTranspose2d forward that also emits the per-tile statistics: its four sub-pixel phase launches each cover a quarter
// of every image's pixels and write their own chunks.  stats: [N][Hi*Wi/128][2][Ci] (Hi x Wi = the transposed
// convolution's OUTPUT, Ci its output channels).
extern "C" int acg_conv_transpose2d_fwd_stats_supported(const acg_conv_desc *d)
{
    if (d == nullptr || g_acg_precision == ACG_PREC_F32 || g_acg_conv_impl != ACG_IMPL_MFMA) return 0;
    if (d->stride != 2 || thin_in(d) || thin_out(d) || d->Ci < 32 || d->Co % 16 != 0 || d->Ci >= 128) return 0;
    if (d->Hi % 2 || d->Wi % 2) return 0;
    return ((long long)(d->Hi / 2) * (d->Wi / 2)) % 128 == 0 ? 1 : 0;
}

extern "C" size_t acg_conv2d_bwd_data_workspace_bytes(const acg_conv_desc *d)
{
    if (d == nullptr || d->pad_mode != ACG_PAD_REFLECT || d->pad == 0) return 0;
    return (size_t)d->N * (d->Hi + 2 * d->pad) * (d->Wi + 2 * d->pad) * d->Ci * sizeof(float);
}

extern "C" int acg_conv2d_bwd_data(const acg_conv_desc *d, const float *dy, const float *wb, float *dx, void *ws,
                                   size_t ws_bytes, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data");
    hipStream_t st = (hipStream_t)stream;
    if (g_acg_conv_impl == ACG_IMPL_DIRECT) return acg_direct_dgrad_launch(d, dy, wb, nullptr, dx, ACG_ACT_NONE, st);
    return dgrad_igemm(d, dy, wb, nullptr, dx, ACG_ACT_NONE, ws, ws_bytes, st, DgradSide());
}

// dx = data gradient + addend (a tensor of dx's shape): the residual-path gradient of a ResnetBlock joins the gradient
// of the block's first convolution (modules.py:185-188, 232-235: out = x + conv_block(x)) inside the convolution's
// epilogue instead of in a separate element-wise pass.  Implemented by the frame path of the reflect data gradient.
extern "C" int acg_conv2d_bwd_data_add_supported(const acg_conv_desc *d)
{
    if (d == nullptr || g_acg_conv_impl != ACG_IMPL_MFMA) return 0;
    Geom g;
    dgrad_s1_geom(d, ACG_ACT_NONE, false, &g, nullptr);
    return dgrad_frame_ok(d, g) ? 1 : 0;
}

extern "C" int acg_conv2d_bwd_data_add(const acg_conv_desc *d, const float *dy, const float *wb, const float *addend,
                                       const unsigned *addend_mask, float *dx, void *ws, size_t ws_bytes, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data_add");
    ACG_REQUIRE(addend != nullptr && acg_conv2d_bwd_data_add_supported(d), "acg_conv2d_bwd_data_add: unsupported shape or mode");
    ACG_REQUIRE(addend_mask == nullptr || sign_mask_fits(d), "acg_conv2d_bwd_data_add: the sign bitmask layout needs Hi*Wi*Ci/4 %% 8 == 0");
    DgradSide s; s.addend = addend; s.addend_mask = addend_mask;
    return dgrad_igemm(d, dy, wb, nullptr, dx, ACG_ACT_NONE, ws, ws_bytes, (hipStream_t)stream, s);
}

extern "C" int acg_conv2d_bwd_data_relu(const acg_conv_desc *d, const float *dy, const float *wb, const float *x,
                                        float *dx, void *ws, size_t ws_bytes, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data_relu");
    ACG_REQUIRE(x != nullptr && acg_conv2d_bwd_data_add_supported(d), "acg_conv2d_bwd_data_relu: unsupported shape or mode");
    DgradSide s; s.relu_src = x;
    return dgrad_igemm(d, dy, wb, nullptr, dx, ACG_ACT_NONE, ws, ws_bytes, (hipStream_t)stream, s);
}

// ---- pre-split ("S16") activation storage for the MFMA-bound 3x3 layers (conv_x3_pre.hip) ---------------------------------
// An S16 tensor has the shape and byte size of its fp32 NHWC twin; per pixel and 8-channel group it holds 16 bytes of bf16
// hi followed by 16 bytes of bf16 lo (x = hi + lo up to 2^-17 |x|: exactly the operand the bf16x3 convolutions consume).
// Replaces the per-launch split of `modules.py:205-227`'s activations inside the convolution loaders.
// the kernel-row weight gradients (conv_wgrad_tr.hip) of the stride-1 3x3 layers: 128-multiple channels (the one the
// pre-split operands need), and the 32 <-> 64 channel variant
static bool wgrad_krow(const acg_conv_desc *d)
{
    return !thin_in(d) && acg_wgrad_krow_shape_ok(d->K, d->stride, d->pad, d->Hi, d->Wi, d->Ho, d->Wo, d->Ci, d->Co);
}
static bool wgrad_krow_s(const acg_conv_desc *d)
{
    return !thin_in(d) && acg_wgrad_krow_s_shape_ok(d->K, d->stride, d->pad, d->Hi, d->Wi, d->Ho, d->Wo, d->Ci, d->Co);
}

static bool s16_dgrad_geom_ok(const acg_conv_desc *d)
{
    if (d->stride != 1 || d->pad_mode != ACG_PAD_REFLECT || d->pad <= 0) return false;
    Geom g; Taps t;
    dgrad_s1_geom(d, ACG_ACT_NONE, false, &g, &t);
    return dgrad_frame_ok(d, g) && acg_igemm_x3_pre_ok(g, t);
}

extern "C" int acg_conv2d_s16_supported(const acg_conv_desc *d)
{
    if (d == nullptr || !bf16x3_mfma()) return 0;
    if (check_desc(d, "acg_conv2d_s16_supported") != ACG_OK || thin_in(d) || thin_out(d)) return 0;
    Geom g; Taps t;
    fwd_geom(d, &g, &t, 0);
    if (!acg_igemm_x3_pre_ok(g, t) || !s16_dgrad_geom_ok(d)) return 0;
    return wgrad_krow(d) ? 1 : 0;
}

extern "C" int acg_conv2d_fwd_s16(const acg_conv_desc *d, const void *x, const float *wf, const float *bias, void *y, int act,
                                  float *stats, int out_s16, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_fwd_s16");
    ACG_REQUIRE(bf16x3_mfma(), "acg_conv2d_fwd_s16: bf16x3 MFMA mode only");
    Geom g; Taps t;
    fwd_geom(d, &g, &t, stats != nullptr ? (int)ACG_ACT_NONE : act);
    ACG_REQUIRE(stats == nullptr || act == ACG_ACT_NONE, "acg_conv2d_fwd_s16: statistics with an activation");
    ACG_REQUIRE(act != ACG_ACT_SIGMOID, "acg_conv2d_fwd_s16: no sigmoid epilogue");
    g.out_s16 = out_s16;
    return acg_igemm_x3_pre_launch(x, wf, bias, (float *)y, g, t, g.w_elems, (hipStream_t)stream, stats);
}

// dy pre-split; addend (fp32, + optional sign bitmask) only with fp32 output; relu_src (pre-split) only with pre-split output
extern "C" int acg_conv2d_bwd_data_s16(const acg_conv_desc *d, const void *dy, const float *wb, void *dx, void *ws,
                                       size_t ws_bytes, const float *addend, const unsigned *addend_mask, const void *relu_src,
                                       int out_s16, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data_s16");
    ACG_REQUIRE(bf16x3_mfma() && s16_dgrad_geom_ok(d), "acg_conv2d_bwd_data_s16: unsupported shape or mode");
    ACG_REQUIRE(addend_mask == nullptr || (addend != nullptr && sign_mask_fits(d)),
                "acg_conv2d_bwd_data_s16: the sign bitmask needs an addend and Hi*Wi*Ci/4 %% 8 == 0");
    DgradSide s; s.addend = addend; s.addend_mask = addend_mask; s.relu_src = (const float *)relu_src;
    s.in_s16 = 1; s.out_s16 = out_s16; s.relu_s16 = relu_src != nullptr ? 1 : 0;
    return dgrad_igemm(d, (const float *)dy, wb, nullptr, (float *)dx, ACG_ACT_NONE, ws, ws_bytes, (hipStream_t)stream, s);
}

// conv + ReLU with pre-split output that also leaves the sign bitmask of that output, and the data gradient of the NEXT
// convolution masked by it (instead of reading the pre-split activation for its sign: 1/32 of the bytes)
extern "C" int acg_conv2d_fwd_s16_mask(const acg_conv_desc *d, const void *x, const float *wf, const float *bias, void *y,
                                       unsigned *sign_mask, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_fwd_s16_mask");
    ACG_REQUIRE(bf16x3_mfma() && sign_mask != nullptr && d->Co % 32 == 0,
                "acg_conv2d_fwd_s16_mask: bf16x3 MFMA mode, 32-multiple output channels");
    Geom g; Taps t;
    fwd_geom(d, &g, &t, ACG_ACT_RELU);
    g.out_s16 = 1; g.mask_out = sign_mask;
    return acg_igemm_x3_pre_launch(x, wf, bias, (float *)y, g, t, g.w_elems, (hipStream_t)stream, nullptr);
}

extern "C" int acg_conv2d_bwd_data_s16_mask(const acg_conv_desc *d, const void *dy, const float *wb, void *dx, void *ws,
                                            size_t ws_bytes, const unsigned *relu_sign_mask, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data_s16_mask");
    ACG_REQUIRE(relu_sign_mask != nullptr && acg_conv2d_bwd_data_s16_sums_supported(d) && d->Ci % 32 == 0,
                "acg_conv2d_bwd_data_s16_mask: unsupported shape or mode (query acg_conv2d_bwd_data_s16_sums_supported)");
    DgradSide s; s.relu_mask = relu_sign_mask; s.in_s16 = 1; s.out_s16 = 1;
    return dgrad_igemm(d, (const float *)dy, wb, nullptr, (float *)dx, ACG_ACT_NONE, ws, ws_bytes, (hipStream_t)stream, s);
}

extern "C" int acg_conv2d_bwd_data_s16_sums_supported(const acg_conv_desc *d)
{
    return acg_conv2d_s16_supported(d) && dgrad_unpad_ok(d) && d->Ci % 4 == 0 && ((long long)d->Hi * d->Wi) % 128 == 0 ? 1 : 0;
}

extern "C" int acg_conv2d_bwd_data_s16_sums(const acg_conv_desc *d, const void *dy, const float *wb, float *dx, void *ws,
                                            size_t ws_bytes, const float *addend, const unsigned *addend_mask,
                                            const acg_norm_sums *ns, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data_s16_sums");
    ACG_REQUIRE(ns != nullptr && acg_conv2d_bwd_data_s16_sums_supported(d), "acg_conv2d_bwd_data_s16_sums: unsupported shape or mode");
    ACG_REQUIRE(addend_mask == nullptr || (addend != nullptr && sign_mask_fits(d)),
                "acg_conv2d_bwd_data_s16_sums: the sign bitmask needs an addend and Hi*Wi*Ci/4 %% 8 == 0");
    ACG_REQUIRE(ns->sign_mask == nullptr || sign_mask_fits(d), "acg_conv2d_bwd_data_s16_sums: bitmask layout");
    DgradSide s; s.addend = addend; s.addend_mask = addend_mask; s.in_s16 = 1; s.ns = ns;
    return dgrad_igemm(d, (const float *)dy, wb, nullptr, dx, ACG_ACT_NONE, ws, ws_bytes, (hipStream_t)stream, s);
}

// The same on fp32 operands, where the data gradient runs on the persistent row pipeline (conv_rows_x3: zero-padded 3x3 stride 1,
// 32 output and 64 input channels of the convolution, width a multiple of 128), on the generic tile (the 32 -> 64 layer's data
// gradient) or on conv_thinrow_x3 (the head's): part[N][Hi*Wi/128][2][Ci], summed over the chunks by acg_norm_bwd_partials like the
// pre-split kernel's (where a workgroup owns several chunks its sums sit in the first, zeros in the others)
extern "C" int acg_conv2d_bwd_data_sums_supported(const acg_conv_desc *d)
{
    if (d == nullptr || !bf16x3_mfma()) return 0;
    if (check_desc(d, "acg_conv2d_bwd_data_sums_supported") != ACG_OK) return 0;
    // the four-phase tile of the stride-2 3x3 data gradient (igemm_conv_ph4<SUMS>): 64 input channels of the convolution, phase
    // grid rows that are whole 128-pixel tiles
    if (d->K == 3 && d->stride == 2 && d->pad == 1 && d->pad_mode != ACG_PAD_REFLECT && d->Ci == 64 &&
        d->Co % 32 == 0 && d->Hi == 2 * d->Ho && d->Wi == 2 * d->Wo && d->Wo % 128 == 0)
        return 1;
    // the 7x7 (K <= 7) stride-1 zero-padded layer with a C4 image on its output side (the head, networks.py:187-188):
    // conv_thinrow_x3's whole 8 x 16 tiles
    if (d->stride == 1 && d->pad_mode != ACG_PAD_REFLECT && thin_out(d) && d->Co == 4 && d->Ci == 32 && d->K >= 2 && d->K <= 7 &&
        d->Hi == d->Ho && d->Wi == d->Wo && d->Hi % 8 == 0 && d->Wi % 16 == 0 && !thin_in_valu_dgrad(d))
        return 1;
    // the zero-padded same-size 3x3 stride-1 layers whose rows are whole 128-pixel tiles: the generic tile (row-patch tiles) on the
    // data gradient of the 32 -> 64 layer (networks.py:164: 64 gathered, 32 written channels — the mirror shape the row pipeline
    // does not take), the row pipeline on that of the 64 -> 32 layer
    const bool same3x3 = d->K == 3 && d->stride == 1 && d->pad == 1 && d->pad_mode != ACG_PAD_REFLECT && d->Hi == d->Ho &&
                         d->Wi == d->Wo && d->Wi % 128 == 0;
    return same3x3 && ((d->Ci == 32 && d->Co == 64) || (d->Co == 32 && d->Ci == 64)) ? 1 : 0;
}

extern "C" int acg_conv2d_bwd_data_sums(const acg_conv_desc *d, const float *dy, const float *wb, float *dx, void *ws, size_t ws_bytes,
                                        const acg_norm_sums *ns, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv2d_bwd_data_sums");
    ACG_REQUIRE(ns != nullptr && ns->sign_mask == nullptr && acg_conv2d_bwd_data_sums_supported(d), "acg_conv2d_bwd_data_sums: unsupported shape or mode");
    DgradSide s; s.ns = ns;
    return dgrad_igemm(d, dy, wb, nullptr, dx, ACG_ACT_NONE, ws, ws_bytes, (hipStream_t)stream, s);
}

// split-K plan shared by the workspace query and the launch
// the persistent patch kernel of the 7x7 image layers (conv_wgrad_thin.hip): workgroups = partial slabs, or 0 where the layer
// does not take it
static int wgrad_thin_patch_splits(const acg_conv_desc *d)
{
    const bool stem = thin_in(d) && acg_wgrad_thin_patch_shape_ok(d->K, d->stride, d->Hi, d->Wi, d->Ho, d->Wo, d->Ci, d->Co);
    const bool head = thin_out(d) && !(d->pad_mode == ACG_PAD_REFLECT && d->pad > 0) &&
                      acg_wgrad_thin_patch_shape_ok(d->K, d->stride, d->Ho, d->Wo, d->Hi, d->Wi, d->Co, d->Ci);
    if (!stem && !head) return 0;
    const long long ntiles = (long long)d->N * ((d->Ho + 7) / 8) * ((d->Wo + 15) / 16);
    return (int)(ntiles < 768 ? ntiles : 768);
}

struct WgradPlan {
    int CiP, CoP, nsplit;
    long long m_per_split;
};
static WgradPlan wgrad_plan(const acg_conv_desc *d)
{
    WgradPlan p;
    const int Cx = d->Ci, Cg = d->Co;
    const long long Mtot = (long long)d->N * d->Ho * d->Wo;
    int bci, bco;
    acg_wgrad_tiles(Cx, Cg, &bci, &bco, thin_in(d) ? 0 : d->K * d->K);
    p.CiP = (Cx + bci - 1) / bci * bci;
    p.CoP = (Cg + bco - 1) / bco * bco;
    if (thin_in(d)) { // gathered columns = (tap, 4 channels): 32 per 8 taps, ONE tap-block
        bci = bco = 32;
        p.CiP = 32 * ((d->K * d->K + 7) / 8);
        p.CoP = (Cg + 31) / 32 * 32;
    }
    const int KP = 256; // multiple of every kernel variant's pixels-per-stage (fp32: 32/128, bf16: 64/256)
    const int nt = acg_wgrad_taps_per_wg(Cx, Cg, d->K * d->K, thin_in(d) ? 1 : 0);   // taps per workgroup (bf16 kernels)
    const long long base = (thin_in(d) ? 1LL : (long long)d->K * d->K / nt) * (p.CiP / bci) * (p.CoP / bco);
    // workgroups per launch: a whole number of residency waves.  The bf16 128x128 kernel holds 2 workgroups per CU:
    // 512 = exactly one wave (vs 1536: -6..-10 %, and a third of the partial-sum traffic); 768 = 1.5 waves is the worst
    // choice (+15 %).  The smaller tiles hold 3-4 per CU and keep more, shorter workgroups.
    long long target = (g_acg_precision != ACG_PREC_F32 && g_acg_conv_impl == ACG_IMPL_MFMA && ((bci == 128 && bco == 128) || nt == 3) && !thin_in(d)) ? 512 : 1024;
    long long nblk = base;
    int gran = KP;
    // kernel-row weight gradient: three taps per workgroup, one 512-thread workgroup per CU -> one residency wave of 256
    if (wgrad_krow(d)) {
        nblk = 3LL * (p.CiP / 128) * (p.CoP / 128);
        target = 256;
        gran = 32; // its stage is a 32-pixel run: splits this fine fill 255 of the 256 CUs at batch 32 (256-pixel splits: 246)
    } else if (wgrad_krow_s(d)) {
        nblk = 3; // the 32 <-> 64 channel variant: 256 threads, two workgroups per CU
        target = 512;
        gran = 128;
    }
    if (!thin_in(d) && acg_wgrad_krowg_shape_ok(d->K, d->stride, d->pad, d->pad_mode == ACG_PAD_REFLECT, d->Wi, d->Wo, Cx, Cg)) {
        nblk = (long long)d->K * (p.CiP / (Cx == 64 ? 64 : 128)) * (p.CoP / 128);   // wgrad_x3_krowg (conv_wgrad_k4.hip): a kernel row per
        target = 256;                                                             // workgroup, one workgroup per CU, whole output rows
        gran = d->Wo;                                                             // per split
    }
    if (thin_in(d) && wgrad_thin_patch_splits(d) > 0) {   // one slab per persistent workgroup
        p.nsplit = wgrad_thin_patch_splits(d);
        p.m_per_split = (Mtot + p.nsplit - 1) / p.nsplit;
        return p;
    }
    long long ns = target / nblk;
    const long long cap = Mtot / (KP * 4);
    if (ns > cap) ns = cap;
    if (ns > 512) ns = 512;
    if (ns < 1) ns = 1;
    long long per = (Mtot + ns - 1) / ns;
    per = (per + gran - 1) / gran * gran;
    ns = (Mtot + per - 1) / per;
    p.nsplit = (int)ns;
    p.m_per_split = per;
    return p;
}

// wgrad_thin_out's split plan (<= 512 splits, or one slab per workgroup of the patch kernel).  slabs: what the workspace
// query reserves, at least nsplit
struct ThinOutPlan {
    int CiP, CoP, nsplit;
    long long per, slabs;
};
static ThinOutPlan wgrad_thin_out_plan(const acg_conv_desc *d)
{
    ThinOutPlan p;
    p.CiP = 32 * ((d->K * d->K + 7) / 8);
    p.CoP = (d->Ci + 31) / 32 * 32;
    const long long M = (long long)d->N * d->Hi * d->Wi;
    long long ns = 1536 / ((long long)(p.CiP / 32) * (p.CoP / 32)), cap = M / 1024;
    if (ns > cap) ns = cap;
    if (ns > 512) ns = 512;
    if (ns < 1) ns = 1;
    p.per = (M + ns - 1) / ns;
    p.per = (p.per + 255) / 256 * 256;
    p.nsplit = (int)((M + p.per - 1) / p.per);
    const int patch = wgrad_thin_patch_splits(d);
    if (patch > 0) p.nsplit = patch;
    p.slabs = (patch > ns ? patch : ns) + 1;
    return p;
}

static size_t wgrad_ws_bytes(const acg_conv_desc *d, const WgradPlan &wp)
{
    const size_t part = (size_t)wp.nsplit * d->K * d->K * wp.CiP * wp.CoP * sizeof(float);
    const int Cmax = d->Ci > d->Co ? d->Ci : d->Co;
    const long long Mbig = (long long)d->N * (d->Hi > d->Ho ? d->Hi : d->Ho) * (d->Wi > d->Wo ? d->Wi : d->Wo);
    const size_t bias_part = (size_t)wp.nsplit * 2 * (wp.CiP > wp.CoP ? wp.CiP : wp.CoP) * sizeof(float);   // x-side sums: `stride` slots per split
    size_t total = acg_round_up(part, 256) + acg_round_up(acg_colsum_ws_bytes(Mbig, Cmax) + bias_part, 256);
    if (thin_out(d) && d->stride == 1) { // wgrad_thin_out's partial buffer
        const ThinOutPlan p = wgrad_thin_out_plan(d);
        const size_t t2 = (size_t)p.slabs * p.CiP * p.CoP * sizeof(float);
        if (t2 > total) total = t2;
    }
    return total;
}

extern "C" size_t acg_conv2d_bwd_weight_workspace_bytes(const acg_conv_desc *d)
{
    if (d == nullptr) return 0;
    // covers both orientations (Conv2d and ConvTranspose2d use of the same descriptor)
    return wgrad_ws_bytes(d, wgrad_plan(d));
}

// x_side: conv-input-side tensor (N,Hi,Wi,Ci); g_side: conv-output-side tensor (N,Ho,Wo,Co)
// bias_from: 0 none; 1 db[c] = column sums of g_side (Conv2d bias, Or entries); 2 of x_side (ConvTranspose bias, Ir entries)
static int wgrad_common(const acg_conv_desc *d, const WgradPlan &wp, const float *x_side, const float *g_side, float *dw, int Or,
                        int Ir, void *ws, size_t ws_bytes, hipStream_t st, int accumulate, int bias_from, float *db,
                        bool thin_conv, bool s16)
{
    ACG_REQUIRE(Or <= d->Co && Ir <= d->Ci, "wgrad: Or=%d Ir=%d exceed padded dims", Or, Ir);
    if (g_acg_conv_impl == ACG_IMPL_DIRECT) return acg_direct_wgrad_launch(d, x_side, g_side, dw, Or, Ir, accumulate, st);
    WGeom g; Taps t; Geom gf;
    fwd_geom(d, &gf, &t, 0);
    g.Hin = d->Hi; g.Win = d->Wi; g.Cin = d->Ci; g.Hg = d->Ho; g.Wg = d->Wo; g.Cg = d->Co;
    g.is = d->stride; g.reflect = d->pad_mode == ACG_PAD_REFLECT;
    g.thin = (thin_conv && thin_in(d)) ? 1 : 0;
    g.Mtot = (long long)d->N * d->Ho * d->Wo;
    g.CiP = wp.CiP; g.CoP = wp.CoP; g.nsplit = wp.nsplit; g.m_per_split = wp.m_per_split;
    const int ntb = g.thin ? 1 : t.n;
    const size_t need = (size_t)g.nsplit * ntb * g.CiP * g.CoP * sizeof(float);
    if (int rc = ws_check("acg_conv2d_bwd_weight", ws, ws_bytes, need)) return rc;
    g.bias_from = db != nullptr ? bias_from : 0;
    g.bias_part = (float *)((char *)ws + acg_round_up(need, 256));
    int rc;
    if (s16) {
        ACG_REQUIRE(wgrad_krow(d) && g.CiP == d->Ci && g.CoP == d->Co && g.m_per_split % 32 == 0 && g.bias_from != 2,
                    "wgrad: pre-split operands need the kernel-row geometry (query acg_conv2d_s16_supported)");
        rc = acg_wgrad_krow_s16_launch(x_side, g_side, (float *)ws, g, st);
    } else {
        ACG_REQUIRE(g.bias_from != 2 || acg_wgrad_krowg_ok(g, t), "wgrad: x-side bias sums only in the kernel-row kernel");
        rc = acg_wgrad_launch(x_side, g_side, (float *)ws, g, t, st);
    }
    if (rc) return rc;
    acg_record_mid_event(st);
    const int Cp = bias_from == 1 ? g.CoP : g.CiP, Cr = g.bias_from ? (bias_from == 1 ? Or : Ir) : 0;
    return acg_wgrad_reduce_launch((const float *)ws, g.nsplit, t.n, g.CiP, g.CoP, Or, Ir, dw, g.thin, accumulate, g.bias_part, Cp, Cr, db,
                                   bias_from == 2 ? g.nsplit * g.is : g.nsplit, st);
}

// Weight gradient of a convolution with <= 4 OUTPUT channels (stride 1): mirror image of the thin-Cin case.
//   dW[co][ci][kh,kw] = sum_{iy,ix} x[iy,ix][ci] * dy[iy-kh+p, ix-kw+p][co]
// GEMM rows (gathered, thin) = (tap, co<4) from dy, columns = ci from the plain x rows, K = input pixels.
static int wgrad_thin_out(const acg_conv_desc *d, const float *x, const float *dy, float *dw, int Or, int Ir, void *ws,
                          size_t ws_bytes, hipStream_t st, int accumulate)
{
    WGeom g; Taps t;
    square_taps(&t, d->K, d->pad, -1);
    g.Hin = d->Ho; g.Win = d->Wo; g.Cin = d->Co;      // gathered side: dy
    g.Hg = d->Hi; g.Wg = d->Wi; g.Cg = d->Ci;         // plain rows: x
    g.is = 1; g.reflect = 0; g.thin = 1; g.bias_from = 0; g.bias_part = nullptr;
    g.Mtot = (long long)d->N * d->Hi * d->Wi;
    const ThinOutPlan p = wgrad_thin_out_plan(d);
    g.CiP = p.CiP; g.CoP = p.CoP; g.nsplit = p.nsplit; g.m_per_split = p.per;
    const size_t need = (size_t)g.nsplit * g.CiP * g.CoP * sizeof(float);
    if (int rc = ws_check("acg_conv2d_bwd_weight(thin out)", ws, ws_bytes, need)) return rc;
    if (int rc = acg_wgrad_launch(dy, x, (float *)ws, g, t, st)) return rc;
    acg_record_mid_event(st);
    return acg_wgrad_reduce_launch((const float *)ws, g.nsplit, t.n, g.CiP, g.CoP, Or, Ir, dw, /* thin */ 2, accumulate, nullptr, 0, 0, nullptr, 0, st);
}

// the checks every weight-gradient entry point opens with; `ok`: its further conditions under the same message
static int wgrad_open(const acg_conv_desc *d, const char *who, bool ok, const void *ws, size_t ws_bytes, WgradPlan *wp)
{
    ACG_CHECK_DESC(d, who);
    *wp = wgrad_plan(d);
    ACG_REQUIRE(ok && ws != nullptr && ws_bytes >= wgrad_ws_bytes(d, *wp), "%s: workspace too small", who);
    return ACG_OK;
}
// bias gradient by a separate column-sum pass over g[M][C] (where no weight-gradient launch carries it), in the workspace
// behind the partial slabs
static int colsum_fallback(const acg_conv_desc *d, const WgradPlan &wp, const char *who, const float *g, long long M, int C, int Cr,
                           float *db, void *ws, size_t ws_bytes, hipStream_t st, int accumulate)
{
    const size_t part = acg_round_up((size_t)wp.nsplit * d->K * d->K * wp.CiP * wp.CoP * sizeof(float), 256);
    ACG_REQUIRE((ws_bytes > part ? ws_bytes - part : 0) >= acg_colsum_ws_bytes(M, C), "%s: colsum workspace", who);
    return acg_colsum_launch(g, M, C, Cr, db, (float *)((char *)ws + part), st, accumulate);
}

extern "C" int acg_conv2d_bwd_weight(const acg_conv_desc *d, const float *x, const float *dy, float *dw, float *db,
                                     int Or, int Ir, void *ws, size_t ws_bytes, int accumulate, void *stream)
{
    WgradPlan wp;
    int rc = wgrad_open(d, "acg_conv2d_bwd_weight", true, ws, ws_bytes, &wp);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the mirrored thin formulation walks the UNPADDED input pixels: right for zero padding only (a reflected border
    // pairs x[refl(q)] with dy of pixels outside that walk); reflect-padded thin-output layers take the general path
    const bool tout = thin_out(d) && d->stride == 1 && !(d->pad_mode == ACG_PAD_REFLECT && d->pad > 0);
    const bool fused = dw != nullptr && db != nullptr && g_acg_conv_impl == ACG_IMPL_MFMA && !tout;
    if (dw != nullptr) {
        rc = tout ? wgrad_thin_out(d, x, dy, dw, Or, Ir, ws, ws_bytes, st, accumulate)
                  : wgrad_common(d, wp, x, dy, dw, Or, Ir, ws, ws_bytes, st, accumulate, 1, fused ? db : nullptr, /* thin_conv */ true, /* s16 */ false);
        if (rc) return rc;
    }
    if (db != nullptr && !fused)
        rc = colsum_fallback(d, wp, "acg_conv2d_bwd_weight", dy, (long long)d->N * d->Ho * d->Wo, d->Co, Or, db, ws, ws_bytes, st, accumulate);
    return rc;
}

// x and dy pre-split; dw / db fp32 as in acg_conv2d_bwd_weight (db = column sums of dy, produced by the same launch)
extern "C" int acg_conv2d_bwd_weight_s16(const acg_conv_desc *d, const void *x, const void *dy, float *dw, float *db, int Or,
                                         int Ir, void *ws, size_t ws_bytes, int accumulate, void *stream)
{
    WgradPlan wp;
    if (int rc = wgrad_open(d, "acg_conv2d_bwd_weight_s16", dw != nullptr, ws, ws_bytes, &wp)) return rc;
    return wgrad_common(d, wp, (const float *)x, (const float *)dy, dw, Or, Ir, ws, ws_bytes, (hipStream_t)stream, accumulate, 1, db,
                        /* thin_conv */ false, /* s16 */ true);
}

extern "C" int acg_conv_transpose2d_fwd(const acg_conv_desc *d, const float *x, const float *wb, const float *bias,
                                        float *y, int act, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv_transpose2d_fwd");
    hipStream_t st = (hipStream_t)stream;
    ACG_REQUIRE(act != ACG_ACT_SIGMOID, "acg_conv_transpose2d_fwd: no sigmoid epilogue");
    if (g_acg_conv_impl == ACG_IMPL_DIRECT) return acg_direct_dgrad_launch(d, x, wb, bias, y, act, st);
    return dgrad_igemm(d, x, wb, bias, y, act, /* ws */ nullptr, /* ws_bytes */ 0, st, DgradSide());
}

extern "C" int acg_conv_transpose2d_fwd_stats(const acg_conv_desc *d, const float *x, const float *wb, const float *bias,
                                             float *y, float *stats, void *stream)
{
    ACG_CHECK_DESC(d, "acg_conv_transpose2d_fwd_stats");
    ACG_REQUIRE(acg_conv_transpose2d_fwd_stats_supported(d) && stats != nullptr, "acg_conv_transpose2d_fwd_stats: unsupported shape or mode");
    DgradSide s; s.stats = stats;
    return dgrad_igemm(d, x, wb, bias, y, ACG_ACT_NONE, /* ws */ nullptr, /* ws_bytes */ 0, (hipStream_t)stream, s);
}

extern "C" int acg_conv_transpose2d_bwd_data(const acg_conv_desc *d, const float *dy, const float *wf, float *dx, void *stream)
{
    // adjoint of the adjoint: the plain forward convolution, no bias / activation
    return acg_conv2d_fwd(d, dy, wf, nullptr, dx, ACG_ACT_NONE, stream);
}

extern "C" int acg_conv_transpose2d_bwd_weight(const acg_conv_desc *d, const float *x, const float *dy, float *dw,
                                               float *db, int Or, int Ir, void *ws, size_t ws_bytes, int accumulate,
                                               void *stream)
{
    // underlying Conv2d: input side = ConvTranspose OUTPUT gradient dy (N,Hi,Wi,Ci), output side = x (N,Ho,Wo,Co);
    // weight (Cin_T, Cout_T, k, k) == OIHW of that Conv2d.  Bias gradient sums dy over pixels (Cout_T = Ir).
    WgradPlan wp;
    int rc = wgrad_open(d, "acg_conv_transpose2d_bwd_weight", true, ws, ws_bytes, &wp);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the bias sums the GATHERED-side operand (dy of the ConvTranspose), whose tap-0 gather visits only a strided subset of
    // its pixels: fused only in the kernel-row kernel (conv_wgrad_k4.hip), where kernel rows 1 .. stride visit every row
    // once; otherwise one separate column-sum pass
    const bool fused = dw != nullptr && db != nullptr && g_acg_conv_impl == ACG_IMPL_MFMA && d->stride <= 2 &&
                       d->Hi == d->stride * d->Ho && d->Wi == d->stride * d->Wo &&
                       acg_wgrad_krowg_shape_ok(d->K, d->stride, d->pad, d->pad_mode == ACG_PAD_REFLECT, d->Wi, d->Wo, d->Ci, d->Co);
    if (dw != nullptr) {
        rc = wgrad_common(d, wp, dy, x, dw, Or, Ir, ws, ws_bytes, st, accumulate, fused ? 2 : 0, fused ? db : nullptr, /* thin_conv */ false, /* s16 */ false);
        if (rc) return rc;
    }
    if (db != nullptr && !fused)
        rc = colsum_fallback(d, wp, "acg_conv_transpose2d_bwd_weight", dy, (long long)d->N * d->Hi * d->Wi, d->Ci, Ir, db, ws, ws_bytes, st, accumulate);
    return rc;
}
