// The fractions-skill-score training loss (ops.fss_loss, --lambda_fss_A / --lambda_fss_B; tests/fss_loss_ref.py states the
// definition, include/acgan_hip.h repeats it).  x holds rows forecasts, y the paired truths.  Per channel c, threshold t and odd
// window n <= 65: soft events p = 1 / (1 + exp(-(x - thr[c][t]) inv_tau)) (q of y), fp32 in exactly this form, so that they
// saturate to exactly 0 and 1; window sums cf = B_n p, co = B_n q over the cells of the centred n x n window inside the domain
// (cells outside count 0, / n^2 is never formed), fp32, n terms along a row and then n terms down a column, each in ascending
// order; num = sum (cf - co)^2 and den = sum (cf^2 + co^2) over the H x W cells in double.  NaN is not masked.
//
// One window-sum routine serves every pass: a workgroup of 256 threads owns a tile of 32 x 32 cells.  fl_fill puts the
// (32 + 2r) x (32 + 2r) cells around it into LDS (r = n / 2; 0 for a cell outside the domain), fl_hsum the sums of 2r + 1
// neighbours along each of its 32 + 2r rows, fl_vsum the 2r + 1 row sums above and below a cell.  LDS is dynamic and sized by
// the largest window of the call: (32 + 2R)^2 floats for the region and two times (32 + 2R) x 32 for the row sums of p and of
// q, 21 KiB at n = 17 (seven workgroups on a CU's 160 KiB) and 60 KiB at n = 65, under the 64 KiB a workgroup gets by default.
// Plain summation: at most 65 terms a pass, window sums of 0/1 planes are exact integers.
//
// Forward (fss_loss_fwd): a workgroup per (row, c, t, tile) walks the windows; per window it fills and row-sums p, then q,
// column-sums both at its cells (thread k the cells k, k + 256, k + 512, k + 768 of the tile, row-major) and adds the two
// products in double in that order; the threads by a fixed shuffle tree, the four waves in order, one partial pair per
// (row, c, t, window, tile) into the workspace.  fss_loss_fold (one wave per (row, c, t, window)) adds the tiles in a fixed
// order.  Every layout is read value by value through its strides: the arithmetic never sees the layout, the same bits in
// every one.  No atomics.
//
// Backward: B_n is symmetric and a, b are scalars per (c, t, window), so a cf - b co = B_n u on the domain's cells with the one
// plane u = (float)(a p - b q) (the combine in double, rounded once).  fss_loss_g (a workgroup per (row, c, t, tile), walking
// the windows) recomputes p and q, window-sums u and writes g = B_n u on the domain's cells into the workspace, one fp32 plane
// per (row, c, t, window).  fss_loss_dx (a workgroup per (row, c, tile)) window-sums those planes once more - fl_fill reads 0
// outside the domain, never a padded convolution of a padded convolution - adds the windows of a threshold in ascending order,
// multiplies by p (1 - p) inv_tau (exactly 0 where p is saturated) and adds the thresholds in ascending order.  A gather: no
// atomics.  dx leaves in x's layout; the workgroups of channel 0 clear the stored channels C .. Cp - 1.
//
// The file is compiled without floating-point contraction: the expressions are the reference's, term by term.
#include "common.h"
#include "field.h"
#include "pair_sum.h"
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

constexpr int FL_THREADS = 256, FL_TILE = 32, FL_MAX_R = 32;
constexpr int FL_CELLS = FL_TILE * FL_TILE / FL_THREADS;           // cells of the tile per thread
constexpr int FL_MAX_HW = 1024, FL_MAX_T = 8, FL_MAX_NW = 8, FL_MAX_N = 2 * FL_MAX_R + 1;

struct FlWindows {
    int n, rmax, r[FL_MAX_NW];           // radii n / 2 and the largest of them, which sizes the LDS of a launch
};

struct FlWho {                           // a workgroup's field and tile: blockIdx.x = field * ntiles + tile
    long long field;
    int tile, i0, j0;
};
__device__ __forceinline__ FlWho fl_who(int ntiles, int tw)
{
    FlWho w;
    w.field = blockIdx.x / ntiles;
    w.tile = (int)(blockIdx.x - w.field * ntiles);
    const int ti = w.tile / tw;
    w.i0 = ti * FL_TILE, w.j0 = (w.tile - ti * tw) * FL_TILE;
    return w;
}

__device__ __forceinline__ float fl_event(float v, float thr, float inv_tau) { return 1.f / (1.f + expf(-(v - thr) * inv_tau)); }

// the region of halo r around the tile at (i0, j0) -> A, (FL_TILE + 2r)^2 floats row-major; val(i, j) inside the domain, 0 outside
template <class F>
__device__ __forceinline__ void fl_fill(float *A, int i0, int j0, int r, int H, int W, F val)
{
    const int RW = FL_TILE + 2 * r;
    for (int idx = threadIdx.x; idx < RW * RW; idx += FL_THREADS) {
        const int ri = idx / RW, i = i0 - r + ri, j = j0 - r + idx - ri * RW;
        A[idx] = i >= 0 && i < H && j >= 0 && j < W ? val(i, j) : 0.f;
    }
}
// B[ri][j] = A[ri][j] + .. + A[ri][j + 2r] for the FL_TILE + 2r rows of the region and the FL_TILE columns of the tile
__device__ __forceinline__ void fl_hsum(const float *A, float *B, int r)
{
    const int RW = FL_TILE + 2 * r;
    for (int idx = threadIdx.x; idx < RW * FL_TILE; idx += FL_THREADS) {
        const float *a = A + (idx / FL_TILE) * RW + idx % FL_TILE;
        float s = 0.f;
        for (int k = 0; k <= 2 * r; ++k) s += a[k];
        B[idx] = s;
    }
}
// the window sum at cell (i, j) of the tile
__device__ __forceinline__ float fl_vsum(const float *B, int i, int j, int r)
{
    float s = 0.f;
    for (int k = 0; k <= 2 * r; ++k) s += B[(i + k) * FL_TILE + j];
    return s;
}

// part: (rows, C, T, nw, ntiles, 2) doubles; blockIdx.x = ((row * C + c) * T + t) * ntiles + tile
__global__ __launch_bounds__(FL_THREADS) void fss_loss_fwd_kernel(Field fx, Field fy, int C, int H, int W, const float *__restrict__ thr,
                                                                  int T, FlWindows win, float inv_tau, int tw, int ntiles,
                                                                  double *__restrict__ part)
{
    extern __shared__ float fl_lds[];                              // fl_lds_bytes(win, 2): the region, then the row sums of p and of q
    __shared__ double red[2][FL_THREADS / 64];
    const int RW = FL_TILE + 2 * win.rmax;
    float *A = fl_lds, *B[2] = {A + RW * RW, A + RW * RW + RW * FL_TILE};
    const FlWho who = fl_who(ntiles, tw);
    const long long fc = who.field / T, f = fc / C;
    const int t = (int)(who.field - fc * T), c = (int)(fc - f * C);
    const float th = thr[c * T + t];
    const Field side[2] = {fx, fy};
    for (int w = 0; w < win.n; ++w) {
        const int r = win.r[w];
        for (int s = 0; s < 2; ++s) {
            const float *base = side[s].x + f * side[s].row + c * side[s].chan;
            const int pix = side[s].pix;
            __syncthreads();                                       // the region's and the row sums' last readers are done
            fl_fill(A, who.i0, who.j0, r, H, W, [&](int i, int j) { return fl_event(base[((long long)i * W + j) * pix], th, inv_tau); });
            __syncthreads();
            fl_hsum(A, B[s], r);
        }
        __syncthreads();
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int k = 0; k < FL_CELLS; ++k) {
            const int cell = k * FL_THREADS + threadIdx.x, i = cell / FL_TILE, j = cell % FL_TILE;
            if (who.i0 + i < H && who.j0 + j < W) {
                const double cf = (double)fl_vsum(B[0], i, j, r), co = (double)fl_vsum(B[1], i, j, r), d = cf - co;
                num += d * d;
                den += cf * cf + co * co;
            }
        }
        pair_block_store<FL_THREADS>(num, den, red, part + ((who.field * win.n + w) * ntiles + who.tile) * 2);
    }
}

// one wave per (row, c, t, window): its tiles' partial pairs in a fixed order -> (num, den)
__global__ __launch_bounds__(64) void fss_loss_fold_kernel(const double *__restrict__ part, int ntiles, double *__restrict__ out)
{
    pair_fold(part, ntiles, [=](double s0, double s1) { out[(long long)blockIdx.x * 2] = s0, out[(long long)blockIdx.x * 2 + 1] = s1; });
}

// g: (rows, C, T, nw, H, W) floats, B_n of u = a p - b q on the domain's cells; blockIdx.x as in the forward
__global__ __launch_bounds__(FL_THREADS) void fss_loss_g_kernel(Field fx, Field fy, int C, int H, int W, const float *__restrict__ thr,
                                                                int T, FlWindows win, float inv_tau, const double *__restrict__ coef,
                                                                int tw, int ntiles, float *__restrict__ g)
{
    extern __shared__ float fl_lds[];                              // fl_lds_bytes(win, 1): the region, then its row sums
    const int RW = FL_TILE + 2 * win.rmax;
    float *A = fl_lds, *B = A + RW * RW;
    const FlWho who = fl_who(ntiles, tw);
    const long long fc = who.field / T, f = fc / C;
    const int t = (int)(who.field - fc * T), c = (int)(fc - f * C);
    const float th = thr[c * T + t];
    const float *xb = fx.x + f * fx.row + c * fx.chan, *yb = fy.x + f * fy.row + c * fy.chan;
    const int xpix = fx.pix, ypix = fy.pix;
    for (int w = 0; w < win.n; ++w) {
        const int r = win.r[w];
        const double a = coef[((c * T + t) * win.n + w) * 2], b = coef[((c * T + t) * win.n + w) * 2 + 1];
        __syncthreads();
        fl_fill(A, who.i0, who.j0, r, H, W, [&](int i, int j) {
            const long long at = (long long)i * W + j;
            const float p = fl_event(xb[at * xpix], th, inv_tau), q = fl_event(yb[at * ypix], th, inv_tau);
            return (float)(a * (double)p - b * (double)q);
        });
        __syncthreads();
        fl_hsum(A, B, r);
        __syncthreads();
        float *gp = g + (who.field * win.n + w) * H * W;
#pragma unroll
        for (int k = 0; k < FL_CELLS; ++k) {
            const int cell = k * FL_THREADS + threadIdx.x, i = cell / FL_TILE, j = cell % FL_TILE;
            if (who.i0 + i < H && who.j0 + j < W) gp[(long long)(who.i0 + i) * W + who.j0 + j] = fl_vsum(B, i, j, r);
        }
    }
}

// dx in x's layout; blockIdx.x = (row * C + c) * ntiles + tile; the stored channels C .. Cp - 1 leave as 0
__global__ __launch_bounds__(FL_THREADS) void fss_loss_dx_kernel(Field fx, int C, int Cp, int H, int W, const float *__restrict__ thr, int T,
                                                                 FlWindows win, float inv_tau, const float *__restrict__ g, int tw,
                                                                 int ntiles, float *__restrict__ dx)
{
    extern __shared__ float fl_lds[];                              // fl_lds_bytes(win, 1)
    const int RW = FL_TILE + 2 * win.rmax;
    float *A = fl_lds, *B = A + RW * RW;
    const FlWho who = fl_who(ntiles, tw);
    const long long f = who.field / C;
    const int c = (int)(who.field - f * C);
    const float *xb = fx.x + f * fx.row + c * fx.chan;
    float acc[FL_CELLS];
#pragma unroll
    for (int k = 0; k < FL_CELLS; ++k) acc[k] = 0.f;
    for (int t = 0; t < T; ++t) {
        const float th = thr[c * T + t];
        float s[FL_CELLS];
#pragma unroll
        for (int k = 0; k < FL_CELLS; ++k) s[k] = 0.f;
        for (int w = 0; w < win.n; ++w) {
            const int r = win.r[w];
            const float *gp = g + ((who.field * T + t) * win.n + w) * H * W;
            __syncthreads();
            fl_fill(A, who.i0, who.j0, r, H, W, [&](int i, int j) { return gp[(long long)i * W + j]; });
            __syncthreads();
            fl_hsum(A, B, r);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < FL_CELLS; ++k) {
                const int cell = k * FL_THREADS + threadIdx.x, i = cell / FL_TILE, j = cell % FL_TILE;
                if (who.i0 + i < H && who.j0 + j < W) s[k] += fl_vsum(B, i, j, r);
            }
        }
#pragma unroll
        for (int k = 0; k < FL_CELLS; ++k) {
            const int cell = k * FL_THREADS + threadIdx.x, i = who.i0 + cell / FL_TILE, j = who.j0 + cell % FL_TILE;
            if (i < H && j < W) {
                const float p = fl_event(xb[((long long)i * W + j) * fx.pix], th, inv_tau);
                acc[k] += p * (1.f - p) * inv_tau * s[k];
            }
        }
    }
    float *db = dx + f * fx.row;
#pragma unroll
    for (int k = 0; k < FL_CELLS; ++k) {
        const int cell = k * FL_THREADS + threadIdx.x, i = who.i0 + cell / FL_TILE, j = who.j0 + cell % FL_TILE;
        if (i >= H || j >= W) continue;
        const long long at = ((long long)i * W + j) * fx.pix;
        db[c * fx.chan + at] = acc[k];
        if (c == 0)                                                // the first channel's workgroup clears the pixel's padding
            for (int cc = C; cc < Cp; ++cc) db[cc * fx.chan + at] = 0.f;
    }
}

// the dynamic LDS of a launch: the region of the call's largest window and `planes` sets of row sums; 60 KiB at n = 65, planes = 2
static size_t fl_lds_bytes(const FlWindows &win, int planes)
{
    const size_t RW = FL_TILE + 2 * win.rmax;
    return (RW * RW + planes * RW * FL_TILE) * sizeof(float);
}

static bool fl_extent_ok(int H, int W) { return H >= 1 && W >= 1 && H <= FL_MAX_HW && W <= FL_MAX_HW; }
static int fl_tiles(int H, int W) { return acg_cdiv(H, FL_TILE) * acg_cdiv(W, FL_TILE); }
static bool fl_shape_ok(int rows, int C, int H, int W, int T, int nw)
{
    return rows >= 1 && C >= 1 && fl_extent_ok(H, W) && T >= 1 && T <= FL_MAX_T && nw >= 1 && nw <= FL_MAX_NW &&
           (long long)rows * C * T * fl_tiles(H, W) <= 0x7fffffffLL;
}

// the larger of the forward's partial pairs and the backward's planes g
extern "C" size_t acg_fss_loss_workspace_bytes(int rows, int C, int H, int W, int T, int nw)
{
    if (!fl_shape_ok(rows, C, H, W, T, nw)) return 0;
    const size_t fields = (size_t)rows * C * T * nw;
    const size_t fwd = fields * fl_tiles(H, W) * 2 * sizeof(double), bwd = fields * H * W * sizeof(float);
    return acg_round_up(fwd > bwd ? fwd : bwd, 16);
}

// what both entry points refuse of the sizes, the windows and the temperature, in the order the header lists
static int fl_refuse(const char *fn, int rows, int C, int H, int W, int T, const int *windows, int nw, float inv_tau, const Field *f,
                     FlWindows &win)
{
    ACG_REQUIRE(fl_extent_ok(H, W), "%s: fields must be H x W with 1 <= H, W <= %d (got %d x %d)", fn, FL_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(T >= 1 && T <= FL_MAX_T && nw >= 1 && nw <= FL_MAX_NW, "%s: need 1 <= T <= %d thresholds and 1 <= nw <= %d windows (T=%d, nw=%d)",
                fn, FL_MAX_T, FL_MAX_NW, T, nw);
    win.n = nw, win.rmax = 0;
    for (int k = 0; k < FL_MAX_NW; ++k) win.r[k] = 0;
    for (int k = 0; k < nw; ++k) {
        const int n = windows[k];
        ACG_REQUIRE(n >= 1 && n % 2 == 1 && n <= FL_MAX_N, "%s: windows must be odd and lie in 1..%d (window %d is %d)", fn, FL_MAX_N, k, n);
        win.r[k] = n / 2;
        if (win.r[k] > win.rmax) win.rmax = win.r[k];
    }
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    ACG_REQUIRE(isfinite(inv_tau) && inv_tau > 0.f, "%s: inv_tau must be positive and finite (got %g)", fn, (double)inv_tau);
    ACG_REQUIRE((long long)rows * C * T * fl_tiles(H, W) <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d, T=%d, H=%d, W=%d)", fn, rows,
                C, T, H, W);
    return ACG_OK;
}

extern "C" int acg_fss_loss_fwd(const float *x, const float *y, int rows, int C, int H, int W, long long x_row_stride, int x_pix_stride,
                                long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                                const float *thr, int T, const int *windows, int nw, float inv_tau, double *out, void *ws,
                                size_t ws_bytes, void *stream)
{
    const char *fn = "acg_fss_loss_fwd";
    ACG_REQUIRE(x != nullptr && y != nullptr && thr != nullptr && windows != nullptr && out != nullptr, "%s: null tensor", fn);
    const Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    FlWindows win;
    FIELD_CHECK(fl_refuse(fn, rows, C, H, W, T, windows, nw, inv_tau, f, win));
    ACG_REQUIRE((const void *)out != (const void *)x && (const void *)out != (const void *)y && (const void *)out != (const void *)thr,
                "%s: out must not alias an input", fn);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_fss_loss_workspace_bytes(rows, C, H, W, T, nw)));
    hipStream_t st = (hipStream_t)stream;
    const int tw = acg_cdiv(W, FL_TILE), ntiles = fl_tiles(H, W);
    const long long fields = (long long)rows * C * T;
    hipLaunchKernelGGL(fss_loss_fwd_kernel, dim3((unsigned)(fields * ntiles)), dim3(FL_THREADS), fl_lds_bytes(win, 2), st, f[0], f[1], C, H, W, thr, T, win,
                       inv_tau, tw, ntiles, (double *)ws);
    hipLaunchKernelGGL(fss_loss_fold_kernel, dim3((unsigned)(fields * nw)), dim3(64), 0, st, (const double *)ws, ntiles, out);
    acg_note_kernel("fss_loss_fwd + fss_loss_fold");
    ACG_CHECK_LAUNCH("acg_fss_loss_fwd");
    return ACG_OK;
}

extern "C" int acg_fss_loss_bwd(const float *x, const float *y, int rows, int C, int Cp, int H, int W, long long x_row_stride,
                                int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                                long long y_chan_stride, const float *thr, int T, const int *windows, int nw, float inv_tau,
                                const double *coef, float *dx, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_fss_loss_bwd";
    ACG_REQUIRE(x != nullptr && y != nullptr && thr != nullptr && windows != nullptr && coef != nullptr && dx != nullptr, "%s: null tensor", fn);
    const Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    FlWindows win;
    FIELD_CHECK(fl_refuse(fn, rows, C, H, W, T, windows, nw, inv_tau, f, win));
    ACG_REQUIRE(C <= Cp, "%s: need C <= Cp stored channels (C=%d, Cp=%d)", fn, C, Cp);
    ACG_REQUIRE((const void *)dx != (const void *)x && (const void *)dx != (const void *)y && (const void *)dx != (const void *)thr &&
                    (const void *)dx != (const void *)coef,
                "%s: dx must not alias an input", fn);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_fss_loss_workspace_bytes(rows, C, H, W, T, nw)));
    hipStream_t st = (hipStream_t)stream;
    const int tw = acg_cdiv(W, FL_TILE), ntiles = fl_tiles(H, W);
    const long long fields = (long long)rows * C * T;
    hipLaunchKernelGGL(fss_loss_g_kernel, dim3((unsigned)(fields * ntiles)), dim3(FL_THREADS), fl_lds_bytes(win, 1), st, f[0], f[1], C, H, W, thr, T, win,
                       inv_tau, coef, tw, ntiles, (float *)ws);
    hipLaunchKernelGGL(fss_loss_dx_kernel, dim3((unsigned)((long long)rows * C * ntiles)), dim3(FL_THREADS), fl_lds_bytes(win, 1), st, f[0], C, Cp, H, W, thr,
                       T, win, inv_tau, (const float *)ws, tw, ntiles, dx);
    acg_note_kernel("fss_loss_g + fss_loss_dx");
    ACG_CHECK_LAUNCH("acg_fss_loss_bwd");
    return ACG_OK;
}
