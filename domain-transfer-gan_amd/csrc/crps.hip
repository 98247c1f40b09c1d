// The CRPS training loss (ops.crps_loss, --lambda_crps_B; tests/crps_ref.py states the definition, include/acgan_hip.h repeats
// it).  x holds rows = N M fields, member m of input n at row n M + m (acg_ensemble_stats's order, x_per_y = M), y the N truths.
// Per cell (input, channel, pixel) with members x_1 .. x_M and truth y: e1 = (1/M) sum_i |x_i - y|, e2 = sum_{i<j} |x_i - x_j|.
//
// Forward (crps_fwd): a workgroup of 256 threads owns 1024 consecutive pixels of one input, thread t the pixels t, t + 256,
// t + 512, t + 768 of them, so that the lanes of a wave read neighbouring pixels.  A thread holds the M values of a cell in
// registers and walks the M (M - 1) / 2 pairs there; differences and sums in double (float -> double is exact).  The pixels of
// a thread are added in ascending order, the threads by a fixed shuffle tree, the four waves in order, one partial pair per
// (input, channel, workgroup) into the workspace; crps_fold (one wave per (input, channel)) adds the partials in a fixed
// order.  What a thread loads at once depends on the layout - a C4 pixel's channels of every member from one 16-byte load each
// (FIELD_C4: the thread then carries all C channels), else one value of one channel (a planar row is then read 256 bytes per
// wave and load, which needs no wider access) - but never the order of a sum: the same bits on every call and in every
// layout.  No atomics.
//
// Backward (crps_bwd): the same ownership.  The signs are recomputed from x and y (comparisons: sign(0) = 0, a NaN compares
// as 0), per member the integer sums sy = sign(x_i - y) and sp = sum_{j != i} sign(x_i - x_j) are combined in double,
// g (coef_y sy - coef_pair sp), and rounded once to float.  dx leaves in x's layout; stored channels C .. Cp - 1 leave as 0.
//
// The file is compiled without floating-point contraction: the combine is the reference's expression, term by term.
#include "common.h"
#include "field.h"
#include "pair_sum.h"
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

constexpr int CR_THREADS = 256, CR_PER_THREAD = 4, CR_BLOCK_PIXELS = CR_THREADS * CR_PER_THREAD;
constexpr int CR_MAX_HW = 1024, CR_MAX_M = 16;

// the members' and the truth's values of one cell -> the sums over the members of |x_i - y| and over the pairs of |x_i - x_j|
template <int MB>
__device__ __forceinline__ void cr_cell(const float (&x)[MB], float y, int M, double &s1, double &s2)
{
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int i = 0; i < MB; ++i)
        if (i < M) a += fabs((double)x[i] - (double)y);
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = i + 1; j < MB; ++j)
            if (j < M) b += fabs((double)x[i] - (double)x[j]);
    s1 = a, s2 = b;
}

// the gradient of every member of one cell: scale (cy sign(x_i - y) - cp sum_{j != i} sign(x_i - x_j)), rounded once
template <int MB>
__device__ __forceinline__ void cr_cell_grad(const float (&x)[MB], float y, int M, double scale, double cy, double cp, float (&d)[MB])
{
    int sp[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) sp[i] = 0;
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = i + 1; j < MB; ++j)
            if (j < M) {
                const int s = (int)(x[i] > x[j]) - (int)(x[i] < x[j]);
                sp[i] += s, sp[j] -= s;
            }
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        if (i >= M) continue;
        const int sy = (int)(x[i] > y) - (int)(x[i] < y);
        d[i] = (float)(scale * (cy * (double)sy - cp * (double)sp[i]));
    }
}

__device__ __forceinline__ void cr_unpack(float4 q, float (&v)[4]) { v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w; }

// the truth's channels beside a C4 pixel of x: one 16-byte load where y is C4 too, else gathered one by one
__device__ __forceinline__ void cr_load_y4(const Field &fy, const float *yb, int C, int p, float (&v)[4])
{
    if (fy.mode == FIELD_C4) {
        cr_unpack(*reinterpret_cast<const float4 *>(yb + (long long)p * 4), v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < C ? yb[k * fy.chan + (long long)p * fy.pix] : 0.f;
    }
}

// who a workgroup is: blockIdx.x = (input n * Cg + cg) * nblk + blk; Cg = 1 where x is FIELD_C4 (the thread carries every
// channel), else C and cg is the channel
struct CrWho {
    long long n;
    int cg, blk;
};
__device__ __forceinline__ CrWho cr_who(int Cg, int nblk)
{
    CrWho w;
    const long long q = blockIdx.x / nblk;
    w.blk = (int)(blockIdx.x - q * nblk);
    w.n = q / Cg;
    w.cg = (int)(q - w.n * Cg);
    return w;
}

// part: (N, C, nblk, 2) doubles
template <int MB>
__global__ __launch_bounds__(CR_THREADS) void crps_fwd_kernel(FieldSrc<2> s, int M, int HW, int nblk, int Cg, double *__restrict__ part)
{
    __shared__ double red[2][CR_THREADS / 64];
    const Field &fx = s.f[0], &fy = s.f[1];
    const CrWho who = cr_who(Cg, nblk);
    const int C = s.C;
    const float *xb = fx.x + who.n * M * fx.row, *yb = fy.x + who.n * fy.row;
    double acc[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    float cell[MB];
    for (int k = 0; k < CR_PER_THREAD; ++k) {
        const int p = who.blk * CR_BLOCK_PIXELS + k * CR_THREADS + threadIdx.x;
        if (p >= HW) break;
        if (fx.mode == FIELD_C4) {
            float xv[MB][4], yv[4];
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) cr_unpack(*reinterpret_cast<const float4 *>(xb + i * fx.row + (long long)p * 4), xv[i]);
            cr_load_y4(fy, yb, C, p, yv);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= C) continue;
#pragma unroll
                for (int i = 0; i < MB; ++i) cell[i] = xv[i][c];
                double s1, s2;
                cr_cell<MB>(cell, yv[c], M, s1, s2);
                acc[c][0] += s1, acc[c][1] += s2;
            }
        } else {
            const long long at = who.cg * fx.chan + (long long)p * fx.pix;
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) cell[i] = xb[i * fx.row + at];
            double s1, s2;
            cr_cell<MB>(cell, yb[who.cg * fy.chan + (long long)p * fy.pix], M, s1, s2);
            acc[0][0] += s1, acc[0][1] += s2;
        }
    }
    const int nacc = fx.mode == FIELD_C4 ? C : 1;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a >= nacc) continue;                                   // uniform over the workgroup
        const int c = fx.mode == FIELD_C4 ? a : who.cg;
        pair_block_store<CR_THREADS>(acc[a][0], acc[a][1], red, part + ((who.n * C + c) * nblk + who.blk) * 2);
    }
}

// one wave per (input, channel): its workgroups' partial pairs in a fixed order -> (sum of e1, sum of e2)
__global__ __launch_bounds__(64) void crps_fold_kernel(const double *__restrict__ part, int nblk, double M, double *__restrict__ out)
{
    pair_fold(part, nblk, [=](double s0, double s1) {
        out[(long long)blockIdx.x * 2] = s0 / M;
        out[(long long)blockIdx.x * 2 + 1] = s1;
    });
}

// dx in x's layout; the stored channels C .. Cp - 1 leave as 0
template <int MB>
__global__ __launch_bounds__(CR_THREADS) void crps_bwd_kernel(FieldSrc<2> s, const float *__restrict__ g, int M, int Cp, int HW, int nblk,
                                                              int Cg, double cy, double cp, float *__restrict__ dx)
{
    const Field &fx = s.f[0], &fy = s.f[1];
    const CrWho who = cr_who(Cg, nblk);
    const int C = s.C;
    const float *xb = fx.x + who.n * M * fx.row, *yb = fy.x + who.n * fy.row;
    float *db = dx + who.n * M * fx.row;
    const double scale = (double)g[0];
    float cell[MB], d[MB];
    for (int k = 0; k < CR_PER_THREAD; ++k) {
        const int p = who.blk * CR_BLOCK_PIXELS + k * CR_THREADS + threadIdx.x;
        if (p >= HW) break;
        if (fx.mode == FIELD_C4) {
            float xv[MB][4], yv[4], dv[MB][4];
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) cr_unpack(*reinterpret_cast<const float4 *>(xb + i * fx.row + (long long)p * 4), xv[i]);
            cr_load_y4(fy, yb, C, p, yv);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int i = 0; i < MB; ++i) cell[i] = xv[i][c];
                if (c < C) cr_cell_grad<MB>(cell, yv[c], M, scale, cy, cp, d);
#pragma unroll
                for (int i = 0; i < MB; ++i) dv[i][c] = c < C ? d[i] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) *reinterpret_cast<float4 *>(db + i * fx.row + (long long)p * 4) = make_float4(dv[i][0], dv[i][1], dv[i][2], dv[i][3]);
        } else {
            const int c = who.cg;
            const long long at = c * fx.chan + (long long)p * fx.pix;
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) cell[i] = xb[i * fx.row + at];
            cr_cell_grad<MB>(cell, yb[c * fy.chan + (long long)p * fy.pix], M, scale, cy, cp, d);
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                if (i >= M) continue;
                float *o = db + i * fx.row;
                o[at] = d[i];
                if (c == 0)                                        // the first channel's thread clears the pixel's padding
                    for (int cc = C; cc < Cp; ++cc) o[cc * fx.chan + (long long)p * fx.pix] = 0.f;
            }
        }
    }
}

static bool cr_extent_ok(int H, int W) { return H >= 1 && W >= 1 && H <= CR_MAX_HW && W <= CR_MAX_HW; }
static bool cr_shape_ok(int rows, int x_per_y, int C, int H, int W)
{
    return rows >= 1 && C >= 1 && cr_extent_ok(H, W) && x_per_y >= 1 && x_per_y <= CR_MAX_M && rows % x_per_y == 0;
}
static int cr_blocks(int H, int W) { return (H * W + CR_BLOCK_PIXELS - 1) / CR_BLOCK_PIXELS; }

// how the two operands of a launch are loaded: a C4 x (and dx, the gradient beside it) 16 bytes at a time; y likewise where x
// is, else value by value like everything else
static void cr_modes(Field (&f)[2], int C, int Cp, const void *dx)
{
    f[0].mode = field_load_mode(f[0], C, false, dx);
    if (f[0].mode == FIELD_C4 && dx != nullptr && Cp != 4) f[0].mode = FIELD_SCALAR;   // x's pixels leave as they came: 16 bytes of dx
    f[1].mode = f[0].mode == FIELD_C4 ? field_load_mode(f[1], C) : FIELD_SCALAR;
}
static const char *cr_mode_name(int mode) { return mode == FIELD_C4 ? "c4" : "strided"; }

extern "C" size_t acg_crps_workspace_bytes(int rows, int x_per_y, int C, int H, int W)
{
    if (!cr_shape_ok(rows, x_per_y, C, H, W)) return 0;
    return (size_t)(rows / x_per_y) * (size_t)C * (size_t)cr_blocks(H, W) * 2 * sizeof(double);
}

extern "C" int acg_crps_fwd(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                            int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                            double *out, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_crps_fwd";
    ACG_REQUIRE(x != nullptr && y != nullptr && out != nullptr, "%s: null tensor", fn);
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    ACG_REQUIRE(cr_extent_ok(H, W), "%s: fields must be H x W with 1 <= H, W <= %d (got %d x %d)", fn, CR_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    const int nblk = cr_blocks(H, W);
    ACG_REQUIRE((long long)rows * C * nblk <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d, H=%d, W=%d)", fn, rows, C, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, CR_MAX_M));
    ACG_REQUIRE((const void *)out != (const void *)x && (const void *)out != (const void *)y, "%s: out must not alias an input", fn);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_crps_workspace_bytes(rows, x_per_y, C, H, W)));
    cr_modes(f, C, 0, nullptr);
    hipStream_t st = (hipStream_t)stream;
    const int M = x_per_y, N = rows / M, Cg = f[0].mode == FIELD_C4 ? 1 : C;
    FieldSrc<2> src = {{f[0], f[1]}, C, M};
    const dim3 grid((unsigned)((long long)N * Cg * nblk)), block(CR_THREADS);
#define CR_FWD(MB) hipLaunchKernelGGL(crps_fwd_kernel<MB>, grid, block, 0, st, src, M, H * W, nblk, Cg, (double *)ws)
    if (M <= 2) CR_FWD(2);
    else if (M <= 4) CR_FWD(4);
    else if (M <= 8) CR_FWD(8);
    else CR_FWD(16);
#undef CR_FWD
    hipLaunchKernelGGL(crps_fold_kernel, dim3((unsigned)((long long)N * C)), dim3(64), 0, st, (const double *)ws, nblk, (double)M, out);
    acg_note_kernel("crps_fwd<%s, %s> + crps_fold", cr_mode_name(f[0].mode), cr_mode_name(f[1].mode));
    ACG_CHECK_LAUNCH("acg_crps_fwd");
    return ACG_OK;
}

extern "C" int acg_crps_bwd(const float *x, const float *y, const float *g, int rows, int x_per_y, int C, int Cp, int H, int W,
                            long long x_row_stride, int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                            long long y_chan_stride, double coef_y, double coef_pair, float *dx, void *stream)
{
    const char *fn = "acg_crps_bwd";
    ACG_REQUIRE(x != nullptr && y != nullptr && g != nullptr && dx != nullptr, "%s: null tensor", fn);
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    ACG_REQUIRE(cr_extent_ok(H, W), "%s: fields must be H x W with 1 <= H, W <= %d (got %d x %d)", fn, CR_MAX_HW, H, W);
    ACG_REQUIRE(rows >= 1 && C >= 1 && C <= Cp, "%s: need rows >= 1 and 1 <= C <= Cp stored channels (rows=%d, C=%d, Cp=%d)", fn, rows, C, Cp);
    const int nblk = cr_blocks(H, W);
    ACG_REQUIRE((long long)rows * C * nblk <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d, H=%d, W=%d)", fn, rows, C, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, CR_MAX_M));
    ACG_REQUIRE(isfinite(coef_y) && isfinite(coef_pair), "%s: the coefficients must be finite (got %g, %g)", fn, coef_y, coef_pair);
    ACG_REQUIRE((const void *)dx != (const void *)x && (const void *)dx != (const void *)y && (const void *)dx != (const void *)g,
                "%s: dx must not alias an input", fn);
    cr_modes(f, C, Cp, dx);
    hipStream_t st = (hipStream_t)stream;
    const int M = x_per_y, N = rows / M, Cg = f[0].mode == FIELD_C4 ? 1 : C;
    FieldSrc<2> src = {{f[0], f[1]}, C, M};
    const dim3 grid((unsigned)((long long)N * Cg * nblk)), block(CR_THREADS);
#define CR_BWD(MB) hipLaunchKernelGGL(crps_bwd_kernel<MB>, grid, block, 0, st, src, g, M, Cp, H * W, nblk, Cg, coef_y, coef_pair, dx)
    if (M <= 2) CR_BWD(2);
    else if (M <= 4) CR_BWD(4);
    else if (M <= 8) CR_BWD(8);
    else CR_BWD(16);
#undef CR_BWD
    acg_note_kernel("crps_bwd<%s, %s>", cr_mode_name(f[0].mode), cr_mode_name(f[1].mode));
    ACG_CHECK_LAUNCH("acg_crps_bwd");
    return ACG_OK;
}
