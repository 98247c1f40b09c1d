// The marginal loss (ops.field_sort, ops.marginal_loss, --lambda_marg_A / --lambda_marg_B): a stable sort of every field with
// its permutation, the squared distance of two batch-mean quantile functions on the sorted fields and its data gradient.
// tests/marginal_ref.py states the definition.  At the end of the file, the evaluator on the same sorted fields
// (acg_marginal_scores: ops.sorted_scores, ops.marginal_scores, --metric marginal; tests/marginal_eval_ref.py).
//
// The sort is a bitonic network on 64-bit words (key << 32) | pixel: key is the order-preserving image of the float's bits
// after -0.0 -> +0.0, so the words of a field are distinct and their order is the stable order of the values.  A field is
// padded to Ppad = the next power of two with all-ones words (no pixel makes one: a pixel index is below 2^20), which sort
// last and are dropped when the words are unpacked.  Compare-exchange partners i and i ^ j of stage k sort upwards iff bit k of
// the lower word's index inside its field is clear; the last stage (k = Ppad) sorts every field upwards.
//
// One workgroup of MS_THREADS threads owns a chunk of MS_T consecutive words (of one field, or MS_T / Ppad whole fields)
// with MS_E words per thread in registers.  The eight words of a thread sit at ms_idx<SH>(t, e): index bits SH .. SH + 2
// count the registers, so the three strides 4, 2, 1 << SH are register swaps.  SH = 10 and SH = 7 serve the strides 4096 ..
// 128 (consecutive lanes read consecutive words of LDS); SH = 0 (a thread's words are neighbours) serves 4, 2, 1 as
// register swaps and 8 .. 256, its lane bits, as cross-lane exchanges without LDS.  The stages up to k = 512 never leave
// the registers.  LDS is read and written through ms_phys, a rotation of the low three index bits by bits 5 .. 7, which
// spreads the 64-byte rows of the SH = 0 layout over all banks and leaves every other layout a permutation inside its rows.
//
// Ppad <= MS_T: one launch sorts and unpacks (marginal_sort<x, unpack>).  Above, the launch chain of ms_launches(Ppad):
// marginal_sort<x, words> sorts every chunk (bit MS_T of the index turns every other chunk downwards), then per merge stage
// k = 2 MS_T .. Ppad the strides k/2 .. MS_T on the words in the workspace, two per launch with four words per thread
// (marginal_merge_global<2>) and an odd one left alone (marginal_merge_global<1>), and one marginal_sort<words, words> that
// finishes the strides below MS_T in LDS; the last of them unpacks.
#include "common.h"
#include "field.h"
#include "pair_sum.h"

typedef unsigned long long u64;

constexpr int MS_T = 8192;                                         // words of a chunk: 64 KiB of LDS, two chunks fit a CU's 160 KiB
constexpr int MS_THREADS = 1024;
constexpr int MS_E = MS_T / MS_THREADS;                            // 8 words per thread
constexpr int MS_MAX_P = 1 << 20;
constexpr u64 MS_PAD = ~0ull;
static_assert(MS_E == 8, "ms_idx and the register strides are written for eight words per thread");

static int ms_ppad(long long P)
{
    int p = 1;
    while (p < P) p <<= 1;
    return p;
}

__device__ __forceinline__ u64 ms_word(float v, unsigned pixel)
{
    unsigned b = __float_as_uint(v + 0.0f);                        // -0.0 + 0.0 = +0.0: the two zeros tie
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)b << 32) | pixel;
}

__device__ __forceinline__ float ms_value(u64 w)
{
    const unsigned b = (unsigned)(w >> 32);
    return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

__device__ __forceinline__ int ms_phys(int i) { return (i & ~7) | ((i + (i >> 5)) & 7); }

template <int SH>
__device__ __forceinline__ int ms_idx(int t, int e)
{
    return ((t >> SH) << (SH + 3)) | (e << SH) | (t & ((1 << SH) - 1));
}

template <int SH>
__device__ __forceinline__ void ms_from_lds(const u64 *lds, int t, u64 (&v)[MS_E])
{
#pragma unroll
    for (int e = 0; e < MS_E; ++e) v[e] = lds[ms_phys(ms_idx<SH>(t, e))];
}

template <int SH>
__device__ __forceinline__ void ms_to_lds(u64 *lds, int t, const u64 (&v)[MS_E])
{
#pragma unroll
    for (int e = 0; e < MS_E; ++e) lds[ms_phys(ms_idx<SH>(t, e))] = v[e];
}

// the register strides (4, 2, 1) << SH of stage k that lie in jlo .. jhi; fi0: the index of the chunk's first word inside
// its field, pmask = Ppad - 1
template <int SH>
__device__ __forceinline__ void ms_reg_strides(u64 (&v)[MS_E], int t, int jhi, int jlo, unsigned fi0, unsigned pmask, unsigned k)
{
#pragma unroll
    for (int s = 4; s >= 1; s >>= 1) {
        const int j = s << SH;
        if (j > jhi || j < jlo) continue;
#pragma unroll
        for (int e = 0; e < MS_E; ++e) {
            if (e & s) continue;
            const bool up = (((fi0 + (unsigned)ms_idx<SH>(t, e)) & pmask) & k) == 0;
            const u64 a = v[e], b = v[e | s];
            if ((a > b) == up) v[e] = b, v[e | s] = a;
        }
    }
}

// strides jhi (<= 256) .. 1 of stage k on the SH = 0 layout: the lane bits across lanes, then the register bits
__device__ __forceinline__ void ms_tail(u64 (&v)[MS_E], int t, int jhi, unsigned fi0, unsigned pmask, unsigned k)
{
    for (int j = jhi < 256 ? jhi : 256; j >= 8; j >>= 1) {
#pragma unroll
        for (int e = 0; e < MS_E; ++e) {
            const unsigned i = (unsigned)(t * MS_E + e);
            const u64 o = __shfl_xor(v[e], j >> 3);
            const bool up = (((fi0 + i) & pmask) & k) == 0;
            const bool low = (i & (unsigned)j) == 0;
            const bool keep_min = low == up;
            v[e] = (keep_min == (o < v[e])) ? o : v[e];
        }
    }
    ms_reg_strides<0>(v, t, jhi, 1, fi0, pmask, k);
}

// strides jhi (<= MS_T / 2) .. 1 of stage k; the words enter in layout IN (10: in registers, as loaded from global memory;
// else: in LDS) and leave in the registers of the SH = 0 layout.  Every thread of the workgroup calls it.
template <bool IN10>
__device__ __forceinline__ void ms_merge(u64 *lds, u64 (&v)[MS_E], int t, int jhi, unsigned fi0, unsigned pmask, unsigned k)
{
    if (jhi >= 1024) {
        if (!IN10) ms_from_lds<10>(lds, t, v);
        ms_reg_strides<10>(v, t, jhi, 1024, fi0, pmask, k);
        ms_to_lds<10>(lds, t, v);
        __syncthreads();
    } else if (IN10) {
        ms_to_lds<10>(lds, t, v);
        __syncthreads();
    }
    if (jhi >= 512) {
        ms_from_lds<7>(lds, t, v);
        ms_reg_strides<7>(v, t, 512, 128, fi0, pmask, k);
        ms_to_lds<7>(lds, t, v);
        __syncthreads();
    }
    ms_from_lds<0>(lds, t, v);
    ms_tail(v, t, jhi >= 512 ? 64 : jhi, fi0, pmask, k);
}

// FROM_X: the words are made from x and sorted from the start (stages 2 .. min(Ppad, MS_T)); else they are read from
// `words` and only stage k is finished (strides MS_T / 2 .. 1).  UNPACK: the words leave as sorted / rank; else to `words`.
// total: rows C Ppad words; a chunk beyond them (Ppad < MS_T only) is padding.
template <bool FROM_X, bool UNPACK>
__global__ __launch_bounds__(MS_THREADS) void marginal_sort_kernel(Field f, int C, u64 *__restrict__ words, long long total, int P,
                                                                   int Ppad, unsigned k, float *__restrict__ sorted,
                                                                   int *__restrict__ rank)
{
    __shared__ __attribute__((aligned(16))) u64 lds[MS_T];
    const int t = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * MS_T;
    const int lg = 31 - __clz(Ppad);                               // Ppad is a power of two
    const unsigned pmask = (unsigned)Ppad - 1u;
    const unsigned fi0 = (unsigned)(g0 & pmask);
    u64 v[MS_E];
#pragma unroll
    for (int e = 0; e < MS_E; ++e) {                               // layout 10: consecutive lanes, consecutive words
        const long long g = g0 + ms_idx<10>(t, e);
        if (FROM_X) {
            const unsigned field = (unsigned)(g >> lg);            // rows C fits 31 bits (acg_field_sort)
            const unsigned p = (unsigned)(g & pmask);
            u64 w = MS_PAD;
            if (g < total && p < (unsigned)P) {
                const unsigned r = field / (unsigned)C, c = field - r * (unsigned)C;
                w = ms_word(f.x[r * f.row + c * f.chan + (long long)p * f.pix], p);
            }
            v[e] = w;
        } else {
            v[e] = words[g];
        }
    }
    if (FROM_X) {
        ms_to_lds<10>(lds, t, v);
        __syncthreads();
        ms_from_lds<0>(lds, t, v);
        const unsigned kmax = Ppad < MS_T ? (unsigned)Ppad : (unsigned)MS_T;
        for (unsigned kk = 2; kk <= kmax && kk <= 512; kk <<= 1) ms_tail(v, t, (int)(kk >> 1), fi0, pmask, kk);
        for (unsigned kk = 1024; kk <= kmax; kk <<= 1) {
            ms_to_lds<0>(lds, t, v);
            __syncthreads();
            ms_merge<false>(lds, v, t, (int)(kk >> 1), fi0, pmask, kk);
        }
    } else {
        ms_merge<true>(lds, v, t, MS_T / 2, fi0, pmask, k);
    }
    __syncthreads();                                               // every read of LDS above is done
    ms_to_lds<0>(lds, t, v);
    __syncthreads();
    ms_from_lds<10>(lds, t, v);
#pragma unroll
    for (int e = 0; e < MS_E; ++e) {
        const long long g = g0 + ms_idx<10>(t, e);
        if (!UNPACK) {
            words[g] = v[e];
            continue;
        }
        const unsigned pixel = (unsigned)v[e];
        const unsigned pos = (unsigned)(g & pmask);
        if (g >= total || pos >= (unsigned)P || pixel >= (unsigned)P) continue;   // padding sorts behind the P pixels
        const long long plane = (g >> lg) * (long long)P;
        sorted[plane + pos] = ms_value(v[e]);
        if (rank != nullptr) rank[plane + pixel] = (int)pos;
    }
}

// NS = 1: the stride j >= MS_T of stage k on the words in the workspace, one pair per thread; NS = 2: the strides j and j / 2
// (j >= 2 MS_T), four words per thread: the pairs of j, then the pairs of j / 2 on the same four words
template <int NS>
__global__ __launch_bounds__(256) void marginal_merge_global_kernel(u64 *__restrict__ words, long long groups, unsigned j, unsigned k,
                                                                    unsigned pmask)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= groups) return;
    const long long h = NS == 2 ? j >> 1 : j;                      // the lowest stride: NS zero bits go in at its position
    const long long i = ((q & ~(h - 1)) << NS) | (q & (h - 1));
    const bool up = (((unsigned)(i & pmask)) & k) == 0;
    if (NS == 1) {
        const u64 a = words[i], b = words[i + j];
        if ((a > b) == up) words[i] = b, words[i + j] = a;
    } else {
        u64 w[4] = {words[i], words[i + h], words[i + 2 * h], words[i + 3 * h]};
#pragma unroll
        for (int s = 2; s >= 1; s >>= 1)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e & s) continue;
                const u64 a = w[e], b = w[e | s];
                if ((a > b) == up) w[e] = b, w[e | s] = a;
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) words[i + e * h] = w[e];
    }
}

// launches of a sort of fields padded to Ppad words
static int ms_launches(int Ppad)
{
    int n = 1, strides = 0;
    for (long long k = 2LL * MS_T; k <= Ppad; k <<= 1) n += (++strides + 1) / 2 + 1;   // the strides >= MS_T in pairs, the LDS finish
    return n;
}

static bool ms_shape_ok(int rows, int C, int H, int W)
{
    return rows >= 1 && C >= 1 && H >= 1 && W >= 1 && (long long)H * W <= MS_MAX_P;
}

extern "C" size_t acg_field_sort_workspace_bytes(int rows, int C, int H, int W)
{
    if (!ms_shape_ok(rows, C, H, W)) return 0;
    const int Ppad = ms_ppad((long long)H * W);
    return Ppad <= MS_T ? 0 : (size_t)rows * (size_t)C * (size_t)Ppad * sizeof(u64);
}

extern "C" int acg_field_sort(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride,
                              long long chan_stride, float *sorted, int *rank, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_field_sort";
    ACG_REQUIRE(x != nullptr && sorted != nullptr, "acg_field_sort: null tensor");
    const Field f = {x, row_stride, chan_stride, pix_stride, FIELD_SCALAR};
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(ms_shape_ok(rows, C, H, W), "acg_field_sort: fields must hold 1 .. %d pixels (H=%d, W=%d)", MS_MAX_P, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, &f, 1));
    ACG_REQUIRE((const void *)x != (const void *)sorted && (const void *)x != (const void *)rank && (void *)sorted != (void *)rank,
                "acg_field_sort: sorted and rank must not alias x or each other");
    const int P = H * W, Ppad = ms_ppad(P);
    const long long total = (long long)rows * C * Ppad;
    const long long chunks = (total + MS_T - 1) / MS_T;
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL && chunks <= 0x7fffffffLL && total / 2 / 256 <= 0x7fffffffLL, "acg_field_sort: too many fields (rows=%d, C=%d)", rows, C);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_field_sort_workspace_bytes(rows, C, H, W)));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks), block(MS_THREADS);
    if (Ppad <= MS_T) {
        hipLaunchKernelGGL((marginal_sort_kernel<true, true>), grid, block, 0, st, f, C, (u64 *)nullptr, total, P, Ppad, 0u, sorted, rank);
        acg_note_kernel("marginal_sort<x, unpack>");
    } else {
        u64 *words = (u64 *)ws;
        const unsigned pmask = (unsigned)Ppad - 1u;
        hipLaunchKernelGGL((marginal_sort_kernel<true, false>), grid, block, 0, st, f, C, words, total, P, Ppad, 0u, (float *)nullptr,
                           (int *)nullptr);
        for (long long k = 2LL * MS_T; k <= Ppad; k <<= 1) {
            long long j = k >> 1;
            for (; j >= 2 * MS_T; j >>= 2)
                hipLaunchKernelGGL(marginal_merge_global_kernel<2>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, words,
                                   total / 4, (unsigned)j, (unsigned)k, pmask);
            if (j >= MS_T)
                hipLaunchKernelGGL(marginal_merge_global_kernel<1>, dim3((unsigned)((total / 2 + 255) / 256)), dim3(256), 0, st, words,
                                   total / 2, (unsigned)j, (unsigned)k, pmask);
            if (k < Ppad)
                hipLaunchKernelGGL((marginal_sort_kernel<false, false>), grid, block, 0, st, f, C, words, total, P, Ppad, (unsigned)k,
                                   (float *)nullptr, (int *)nullptr);
            else
                hipLaunchKernelGGL((marginal_sort_kernel<false, true>), grid, block, 0, st, f, C, words, total, P, Ppad, (unsigned)k, sorted,
                                   rank);
        }
        acg_note_kernel("marginal_sort<x, words> + marginal_merge chain: %d launches", ms_launches(Ppad));
    }
    ACG_CHECK_LAUNCH("acg_field_sort");
    return ACG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The loss on the sorted fields: d[c][k] = mean_r sx[r][c][k] - mean_r sy[r][c][k], loss = mean d^2.  Both means run over
// the rows in their order in fp32, and d is fp32; its squares are summed in double by ML_BLOCKS workgroups over fixed slices,
// tree-reduced in LDS into the workspace, and by one workgroup over those partials: the same bits on every call.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int ML_THREADS = 256, ML_BLOCKS = 512;

__device__ __forceinline__ double ml_block_sum(double s, double *red)
{
    red[threadIdx.x] = s;
    __syncthreads();
    for (int n = ML_THREADS / 2; n >= 1; n >>= 1) {
        if ((int)threadIdx.x < n) red[threadIdx.x] += red[threadIdx.x + n];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(ML_THREADS) void marginal_diff_kernel(const float *__restrict__ sx, int rows_x, const float *__restrict__ sy,
                                                                   int rows_y, long long CP, float *__restrict__ d,
                                                                   double *__restrict__ part)
{
    __shared__ double red[ML_THREADS];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * ML_THREADS + threadIdx.x; i < CP; i += (long long)ML_BLOCKS * ML_THREADS) {
        float qx = 0.f, qy = 0.f;
        for (int r = 0; r < rows_x; ++r) qx += sx[r * CP + i];
        for (int r = 0; r < rows_y; ++r) qy += sy[r * CP + i];
        const float v = qx / (float)rows_x - qy / (float)rows_y;
        d[i] = v;
        s += (double)v * (double)v;
    }
    s = ml_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(ML_THREADS) void marginal_loss_kernel(const double *__restrict__ part, long long CP, float *__restrict__ loss)
{
    __shared__ double red[ML_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < ML_BLOCKS; i += ML_THREADS) s += part[i];
    s = ml_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)CP);
}

extern "C" size_t acg_marginal_loss_workspace_bytes(int C, long long P)
{
    if (C < 1 || P < 1 || P > MS_MAX_P) return 0;
    return ML_BLOCKS * sizeof(double);
}

extern "C" int acg_marginal_loss_fwd(const float *sx, int rows_x, const float *sy, int rows_y, int C, long long P, float *d,
                                     float *loss, void *ws, size_t ws_bytes, void *stream)
{
    ACG_REQUIRE(sx != nullptr && sy != nullptr && d != nullptr && loss != nullptr, "acg_marginal_loss_fwd: null tensor");
    ACG_REQUIRE(rows_x >= 1 && rows_y >= 1 && C >= 1, "acg_marginal_loss_fwd: need rows >= 1 and C >= 1 (rows_x=%d, rows_y=%d, C=%d)",
                rows_x, rows_y, C);
    ACG_REQUIRE(P >= 1 && P <= MS_MAX_P, "acg_marginal_loss_fwd: fields must hold 1 .. %d pixels (P=%lld)", MS_MAX_P, P);
    ACG_REQUIRE(d != sx && d != sy && loss != sx && loss != sy && loss != d, "acg_marginal_loss_fwd: d and loss must not alias an input");
    FIELD_CHECK(field_refuse_workspace("acg_marginal_loss_fwd", ws, ws_bytes, acg_marginal_loss_workspace_bytes(C, P)));
    hipStream_t st = (hipStream_t)stream;
    const long long CP = (long long)C * P;
    hipLaunchKernelGGL(marginal_diff_kernel, dim3(ML_BLOCKS), dim3(ML_THREADS), 0, st, sx, rows_x, sy, rows_y, CP, d, (double *)ws);
    hipLaunchKernelGGL(marginal_loss_kernel, dim3(1), dim3(ML_THREADS), 0, st, (const double *)ws, CP, loss);
    acg_note_kernel("marginal_diff + marginal_loss");
    ACG_CHECK_LAUNCH("acg_marginal_loss_fwd");
    return ACG_OK;
}

// The data gradient: gx[r][c][p] = gscale[0] (2 / (C P rows)) d[c][rank[r][c][p]], one thread per pixel.  C4: the pixel's four
// stored channels leave as one 16-byte store.  Channels C .. Cp - 1 are written as 0.
template <bool C4>
__global__ __launch_bounds__(256) void marginal_bwd_kernel(const float *__restrict__ d, const int *__restrict__ rank,
                                                           const float *__restrict__ gscale, long long pixels, int C, int Cp, int P,
                                                           long long row, int pix, long long chan, float coef, float *__restrict__ gx)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const long long r = i / P;
    const int p = (int)(i - r * P);
    const float g = gscale[0];
    float *o = gx + r * row + (long long)p * pix;
    float v4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
        int k = rank[(r * C + c) * P + p];
        k = k < 0 ? 0 : (k >= P ? P - 1 : k);                      // a rank is a position of the field: never read outside d
        const float v = (d[(long long)c * P + k] * coef) * g;
        if (C4) v4[c] = v;
        else o[c * chan] = v;
    }
    if (C4) *(float4 *)o = make_float4(v4[0], v4[1], v4[2], v4[3]);
    else
        for (int c = C; c < Cp; ++c) o[c * chan] = 0.f;
}

extern "C" int acg_marginal_loss_bwd(const float *d, const int *rank, const float *gscale, int rows, int C, int Cp, int H, int W,
                                     long long row_stride, int pix_stride, long long chan_stride, float *gx, void *stream)
{
    ACG_REQUIRE(d != nullptr && rank != nullptr && gscale != nullptr && gx != nullptr, "acg_marginal_loss_bwd: null tensor");
    ACG_REQUIRE(rows >= 1 && C >= 1 && C <= Cp,
                "acg_marginal_loss_bwd: need rows >= 1 and 1 <= C <= Cp stored channels (rows=%d, C=%d, Cp=%d)", rows, C, Cp);
    ACG_REQUIRE(ms_shape_ok(rows, C, H, W), "acg_marginal_loss_bwd: fields must hold 1 .. %d pixels (H=%d, W=%d)", MS_MAX_P, H, W);
    const Field f = {gx, row_stride, chan_stride, pix_stride, FIELD_SCALAR};   // gx, in the layout of the x it is the gradient of
    FIELD_CHECK(field_refuse_operands("acg_marginal_loss_bwd", rows, C, &f, 1));
    ACG_REQUIRE((const void *)gx != (const void *)d && (const void *)gx != (const void *)rank && (const void *)gx != (const void *)gscale,
                "acg_marginal_loss_bwd: gx must not alias an input");
    const int P = H * W;
    const long long pixels = (long long)rows * P;
    ACG_REQUIRE((pixels + 255) / 256 <= 0x7fffffffLL, "acg_marginal_loss_bwd: too many pixels (rows=%d)", rows);
    const float coef = (float)(2.0 / ((double)C * (double)P * (double)rows));
    const bool c4 = Cp == 4 && field_load_mode(f, C) == FIELD_C4;
    const dim3 grid((unsigned)((pixels + 255) / 256));
    if (c4)
        hipLaunchKernelGGL(marginal_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, d, rank, gscale, pixels, C, Cp, P,
                           row_stride, pix_stride, chan_stride, coef, gx);
    else
        hipLaunchKernelGGL(marginal_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, d, rank, gscale, pixels, C, Cp, P,
                           row_stride, pix_stride, chan_stride, coef, gx);
    acg_note_kernel(c4 ? "marginal_bwd<c4>" : "marginal_bwd<scalar>");
    ACG_CHECK_LAUNCH("acg_marginal_loss_bwd");
    return ACG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The evaluator on the sorted fields (ops.sorted_scores, ops.marginal_scores, --metric marginal; tests/marginal_eval_ref.py):
// per (row, channel) the Wasserstein distances w1 = mean |sx - sy| and w2sq = mean (sx - sy)^2 against the paired sorted truth,
// the order-statistic quantiles at L levels and the counts of values below E edges.  One workgroup per field streams sx and sy
// once.  A thread sums the groups of four neighbouring pixels t, t + MQ_THREADS, .. in that order in double, then one of the
// P % 4 last pixels; a shuffle tree per wave, the waves in order: the same bits on every call, whatever the alignment of the
// operands.  The quantile is s[lo] + frac (s[hi] - s[lo]) in double without contraction, rounded once; a count
// is a lower bound by bisection, at most 21 steps, every probe inside the field whatever the values are.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MQ_THREADS = 1024, MQ_WAVES = MQ_THREADS / 64;
constexpr int MQ_MAX_L = 16, MQ_MAX_E = 256;

struct MqLevels {
    double v[MQ_MAX_L];
};

__global__ __launch_bounds__(MQ_THREADS) void marginal_scores_kernel(FieldSrc<2> src, int P, bool paired, MqLevels levels, int L,
                                                                     const float *__restrict__ edges, int E, double *__restrict__ w,
                                                                     float *__restrict__ q, int *__restrict__ below)
{
#pragma clang fp contract(off)
    __shared__ double red[2][MQ_WAVES];
    const int t = threadIdx.x, p = blockIdx.x;
    int c;
    const float *sx = field_first(src, 0, p, c);
    if (paired) {
        const float *sy = field_first(src, 1, p, c);
        const int G = P >> 2;
        double a = 0.0, b = 0.0;
        for (int g = t; g < G; g += MQ_THREADS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double d = (double)sx[4 * g + i] - (double)sy[4 * g + i];
                a += fabs(d);
                b += d * d;
            }
        }
        if (4 * G + t < P) {
            const double d = (double)sx[4 * G + t] - (double)sy[4 * G + t];
            a += fabs(d);
            b += d * d;
        }
        // (sums of |d| and of d d are never -0.0: adding the waves from 0.0 gives the bits of starting from the first wave)
        pair_block_sum<MQ_THREADS>(a, b, red, [=](double s0, double s1) {
            w[2 * (long long)p] = s0 / (double)P;
            w[2 * (long long)p + 1] = s1 / (double)P;
        });
    }
    for (int l = t; l < L; l += MQ_THREADS) {
        const double pos = levels.v[l] * (double)(P - 1);
        int lo = (int)floor(pos);
        lo = lo < 0 ? 0 : (lo > P - 1 ? P - 1 : lo);                   // a level lies in [0, 1]: never read outside the field
        const int hi = lo + 1 < P ? lo + 1 : P - 1;
        const double frac = pos - (double)lo, slo = (double)sx[lo], shi = (double)sx[hi];
        q[(long long)p * L + l] = (float)(slo + frac * (shi - slo));
    }
    for (int e = t; e < E; e += MQ_THREADS) {
        const float edge = edges[c * E + e];
        int lo = 0, hi = P;                                            // the first position whose value is not below the edge
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (sx[mid] < edge) lo = mid + 1;
            else hi = mid;
        }
        below[(long long)p * E + e] = lo;
    }
}

extern "C" int acg_marginal_scores(const float *sx, const float *sy, int rows, int x_per_y, int C, long long P, const double *levels,
                                   int L, const float *edges, int E, double *w, float *q, int *below, void *stream)
{
    const char *fn = "acg_marginal_scores";
    ACG_REQUIRE(sx != nullptr, "acg_marginal_scores: null sx");
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(P >= 1 && P <= MS_MAX_P, "acg_marginal_scores: fields must hold 1 .. %d pixels (P=%lld)", MS_MAX_P, P);
    ACG_REQUIRE(L >= 0 && L <= MQ_MAX_L && E >= 0 && E <= MQ_MAX_E,
                "acg_marginal_scores: need 0 .. %d levels and 0 .. %d edges (L=%d, E=%d)", MQ_MAX_L, MQ_MAX_E, L, E);
    ACG_REQUIRE(sy != nullptr || L > 0 || E > 0, "acg_marginal_scores: nothing to compute (no sy, no levels, no edges)");
    ACG_REQUIRE((w != nullptr) == (sy != nullptr), "acg_marginal_scores: null or stray w: it is written exactly when sy is given");
    ACG_REQUIRE((q != nullptr) == (L > 0) && (L == 0 || levels != nullptr),
                "acg_marginal_scores: null or stray q or levels: q is written exactly when L > 0 (L=%d)", L);
    ACG_REQUIRE((below != nullptr) == (E > 0) && (E == 0 || edges != nullptr),
                "acg_marginal_scores: null or stray below or edges: below is written exactly when E > 0 (E=%d)", E);
    FieldSrc<2> src = {};
    src.f[0] = {sx, (long long)C * P, P, 1, FIELD_SCALAR};
    src.f[1] = {sy, (long long)C * P, P, 1, FIELD_SCALAR};
    src.C = C;
    FIELD_CHECK(field_refuse_operands(fn, rows, C, src.f, sy != nullptr ? 2 : 1));
    FIELD_CHECK(field_refuse_pairing(fn, rows, sy != nullptr ? x_per_y : 1, rows));
    src.x_per_y = sy != nullptr ? x_per_y : 1;
    MqLevels lv = {};
    for (int l = 0; l < L; ++l) {
        ACG_REQUIRE(levels[l] >= 0.0 && levels[l] <= 1.0, "acg_marginal_scores: level %d must lie in [0, 1] (got %g)", l, levels[l]);
        lv.v[l] = levels[l];
    }
    const void *in[3] = {sx, sy, edges}, *out[3] = {w, q, below};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            ACG_REQUIRE(out[i] == nullptr || (out[i] != in[j] && (j <= i || out[i] != out[j])),
                        "acg_marginal_scores: w, q and below must not alias an input or each other");
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL, "acg_marginal_scores: too many fields (rows=%d, C=%d)", rows, C);
    hipLaunchKernelGGL(marginal_scores_kernel, dim3((unsigned)(rows * C)), dim3(MQ_THREADS), 0, (hipStream_t)stream, src, (int)P,
                       sy != nullptr, lv, L, edges, E, w, q, below);
    acg_note_kernel("marginal_scores<%s>", sy == nullptr ? "single" : "paired");
    ACG_CHECK_LAUNCH("acg_marginal_scores");
    return ACG_OK;
}
