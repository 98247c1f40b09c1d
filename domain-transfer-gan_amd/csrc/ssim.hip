// Structural similarity (ops.ssim, ops.ssim_loss, --lambda_ssim_A / --lambda_ssim_B, test.py --metric ssim; tests/ssim_ref.py
// states the definition, include/acgan_hip.h repeats it).  Wang et al. 2004 with the separable 11 x 11 Gaussian window
// (sigma 1.5, normalised) over the (H - 10) x (W - 10) 'valid' window positions; per (row, channel) the mean of S and the mean
// of the contrast-structure factor cs.
//
// Forward (ssim_fwd): one workgroup of 256 threads per output tile of SS_TW x SS_TH = 32 x 16 window positions of one row of
// x, all its channels one after the other.  The tile and its 10-pixel halo (42 x 26 pixels) of x and y sit in LDS as dense
// planes per channel; a C4 NHWC operand is staged once, every channel of a pixel from one 16-byte load, any other operand
// channel by channel.  Per channel: the horizontal 11-tap pass of the five moments x, y, x^2, y^2, xy (26 x 32 items), the
// vertical pass (two window positions per thread), S and cs, then a block reduction in double (a fixed shuffle tree, the
// four waves in order) and one partial pair per (row, channel, tile) into the workspace.  ssim_fold (one wave per (row,
// channel)) adds the partials in a fixed order: the same bits on every run and for every layout.  With dmaps the same kernel
// stores the derivatives a = dS/d mu_x (total), b = dS/dE[x^2], c = dS/dE[xy] of every window position.
// The moments are taken about a pivot, the operand x at the tile's first pixel (of either field: one pivot for both, so
// that E[xy] shifts like the variances): variances and the covariance are shift-invariant, the means get the pivot back, and
// E[x^2] - mu^2 no longer cancels on a flat field away from zero.
// Every lane group of 32 reads or writes 32 consecutive floats of one plane row in both passes (the tile is 32 wide, the
// planes are dense): no LDS bank conflicts (32 banks for 4-byte reads and all writes).  LDS: (4 + 4) x 42 x 26 floats of
// pixels, 5 x 26 x 32 of row sums, 64 bytes of reduction = 51648 bytes with both operands C4, inside the default 64 KiB.
//
// Backward (ssim_bwd): one workgroup per 32 x 16 tile of PIXELS.  gx(q) = -g / (rows C Hv Wv) ((w * a)(q) + 2 x(q) (w * b)(q) +
// y(q) (w * c)(q)), * the full correlation with the (symmetric) window: the maps over tile + 10 to the left and above, zero
// outside the valid region, go through the same two passes, then the point-wise combine.  A gather: no atomics.
//
// The file is compiled without floating-point contraction; the tap loops call fmaf themselves.  Every instantiation then
// evaluates the same expressions in the same order, whatever the layout.
#include "common.h"
#include "field.h"
#include "pair_sum.h"
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

constexpr int SS_K = 11, SS_HALO = SS_K - 1;
constexpr int SS_TW = 32, SS_TH = 16;                              // a tile of window positions (forward) / pixels (backward)
constexpr int SS_IW = SS_TW + SS_HALO, SS_IH = SS_TH + SS_HALO;    // with its halo: 42 x 26
constexpr int SS_THREADS = 256;
constexpr int SS_MIN_HW = SS_K, SS_MAX_HW = 1024;
constexpr int SS_PER_THREAD = SS_TW * SS_TH / SS_THREADS;          // 2 outputs per thread
static_assert(SS_TW == 32 && SS_TW * SS_TH % SS_THREADS == 0, "lane groups of 32 walk one tile row");

struct SsWin {
    float w[SS_K];
};

// the tile's pixels (oy + r, ox + j), r < SS_IH, j < SS_IW, of row `base` -> planes; outside H x W: 0.  C4: channels 0 .. C - 1
// into planes 0 .. C - 1 from one 16-byte load per pixel; else channel c into plane 0.
template <bool C4>
__device__ __forceinline__ void ss_stage(float *planes, const Field &f, const float *base, int c, int C, int oy, int ox, int H, int W)
{
    for (int p = threadIdx.x; p < SS_IH * SS_IW; p += SS_THREADS) {
        const int r = p / SS_IW, j = p - r * SS_IW;
        const int gy = oy + r, gx = ox + j;
        const bool in = gy >= 0 && gx >= 0 && gy < H && gx < W;
        const long long pixel = (long long)gy * W + gx;
        if (C4) {
            const float4 q = in ? *reinterpret_cast<const float4 *>(base + pixel * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < C; ++k) planes[k * (SS_IH * SS_IW) + p] = field_pick(q, k);
        } else {
            planes[p] = in ? base[c * f.chan + pixel * f.pix] : 0.f;
        }
    }
}

// blockIdx.x = row r of x * tiles + tile.  part: (rows, C, tiles, 2) doubles; dmaps (or NULL): 3 planes of (rows, C, Hv, Wv),
// `plane` floats apart.
template <bool XC4, bool YC4>
__global__ __launch_bounds__(SS_THREADS) void ssim_fwd_kernel(Field x, Field y, int C, int H, int W, int x_per_y, int ntx,
                                                              int tiles, SsWin win, float c1, float c2, double *__restrict__ part,
                                                              float *__restrict__ dmaps, long long plane)
{
    constexpr int NX = XC4 ? 4 : 1, NY = YC4 ? 4 : 1, IP = SS_IH * SS_IW;
    __shared__ float sx[NX * IP];
    __shared__ float sy[NY * IP];
    __shared__ float hb[5][SS_IH * SS_TW];
    __shared__ double red[2][SS_THREADS / 64];
    const int t = threadIdx.x;
    const long long r = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - r * tiles);
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int oy = ty * SS_TH, ox = tx * SS_TW;
    const int Hv = H - SS_HALO, Wv = W - SS_HALO;
    const float *xb = x.x + r * x.row, *yb = y.x + (r / x_per_y) * y.row;
    for (int c = 0; c < C; ++c) {
        if (!XC4 || c == 0) ss_stage<XC4>(sx, x, xb, c, C, oy, ox, H, W);
        if (!YC4 || c == 0) ss_stage<YC4>(sy, y, yb, c, C, oy, ox, H, W);
        __syncthreads();
        const float *px = sx + (XC4 ? c * IP : 0), *py = sy + (YC4 ? c * IP : 0);
        const float pv = px[0];                                    // the pivot: x at the tile's first pixel, always inside
        for (int it = t; it < SS_IH * SS_TW; it += SS_THREADS) {
            const int rr = it >> 5, j = it & 31;
            const float *qx = px + rr * SS_IW + j, *qy = py + rr * SS_IW + j;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < SS_K; ++k) {
                const float xv = qx[k] - pv, yv = qy[k] - pv, w = win.w[k];
                m0 = fmaf(w, xv, m0), m1 = fmaf(w, yv, m1);
                m2 = fmaf(w, xv * xv, m2), m3 = fmaf(w, yv * yv, m3), m4 = fmaf(w, xv * yv, m4);
            }
            hb[0][it] = m0, hb[1][it] = m1, hb[2][it] = m2, hb[3][it] = m3, hb[4][it] = m4;
        }
        __syncthreads();
        double sum_s = 0.0, sum_cs = 0.0;
#pragma unroll
        for (int e = 0; e < SS_PER_THREAD; ++e) {
            const int o = t + e * SS_THREADS, i = o >> 5, j = o & 31;
            if (oy + i >= Hv || ox + j >= Wv) continue;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SS_K; ++k)
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(win.w[k], hb[q][(i + k) * SS_TW + j], m[q]);
            const float vx = m[2] - m[0] * m[0], vy = m[3] - m[1] * m[1], cov = m[4] - m[0] * m[1];
            const float mx = m[0] + pv, my = m[1] + pv;
            const float A1 = 2.f * mx * my + c1, A2 = 2.f * cov + c2;
            const float B1 = mx * mx + my * my + c1, B2 = vx + vy + c2;
            const float B12 = B1 * B2;
            const float S = A1 * A2 / B12;
            sum_s += (double)S, sum_cs += (double)(A2 / B2);
            if (dmaps != nullptr) {
                const float dc = 2.f * A1 / B12, db = -S / B2;
                const float da = 2.f * my * A2 / B12 - 2.f * mx * S / B1 - dc * my - 2.f * db * mx;
                float *d = dmaps + ((r * C + c) * Hv + (oy + i)) * (long long)Wv + (ox + j);
                d[0] = da, d[plane] = db, d[2 * plane] = dc;
            }
        }
        pair_block_store<SS_THREADS>(sum_s, sum_cs, red, part + ((r * C + c) * tiles + tile) * 2);
    }
}

// one wave per (row, channel): its tiles' partial pairs in a fixed order -> the means over the count window positions
__global__ __launch_bounds__(64) void ssim_fold_kernel(const double *__restrict__ part, int tiles, double count, float *__restrict__ out)
{
    pair_fold(part, tiles, [=](double s0, double s1) {
        out[(long long)blockIdx.x * 2] = (float)(s0 / count);
        out[(long long)blockIdx.x * 2 + 1] = (float)(s1 / count);
    });
}

// blockIdx.x = row r * tiles + tile, a tile of SS_TW x SS_TH pixels.  gx in x's layout; channels C .. Cp - 1 leave as 0.
template <bool XC4, bool YC4>
__global__ __launch_bounds__(SS_THREADS) void ssim_bwd_kernel(const float *__restrict__ dmaps, long long plane, Field x, Field y,
                                                              const float *__restrict__ g, int C, int Cp, int H, int W, int ntx, int tiles,
                                                              SsWin win, float coef, float *__restrict__ gx)
{
    constexpr int IP = SS_IH * SS_IW;
    __shared__ float sm[3][IP];
    __shared__ float hb[3][SS_IH * SS_TW];
    const int t = threadIdx.x;
    const long long r = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - r * tiles);
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int qy0 = ty * SS_TH, qx0 = tx * SS_TW;
    const int Hv = H - SS_HALO, Wv = W - SS_HALO;
    const float scale = coef * g[0];
    const float *xb = x.x + r * x.row, *yb = y.x + r * y.row;
    float *ob = gx + r * x.row;
    long long pixel[SS_PER_THREAD];
    bool in[SS_PER_THREAD];
    float4 x4[SS_PER_THREAD], y4[SS_PER_THREAD], o4[SS_PER_THREAD];
#pragma unroll
    for (int e = 0; e < SS_PER_THREAD; ++e) {
        const int o = t + e * SS_THREADS, i = o >> 5, j = o & 31;
        in[e] = qy0 + i < H && qx0 + j < W;
        pixel[e] = (long long)(qy0 + i) * W + (qx0 + j);
        o4[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (XC4 && in[e]) x4[e] = *reinterpret_cast<const float4 *>(xb + pixel[e] * 4);
        if (YC4 && in[e]) y4[e] = *reinterpret_cast<const float4 *>(yb + pixel[e] * 4);
    }
    for (int c = 0; c < C; ++c) {
        const float *mp = dmaps + (r * C + c) * (long long)Hv * Wv;
        for (int p = t; p < IP; p += SS_THREADS) {
            const int rr = p / SS_IW, j = p - rr * SS_IW;
            const int py = qy0 - SS_HALO + rr, px = qx0 - SS_HALO + j;
            const bool ok = py >= 0 && px >= 0 && py < Hv && px < Wv;
            const long long at = (long long)py * Wv + px;
#pragma unroll
            for (int k = 0; k < 3; ++k) sm[k][p] = ok ? mp[k * plane + at] : 0.f;
        }
        __syncthreads();
        for (int it = t; it < SS_IH * SS_TW; it += SS_THREADS) {
            const int rr = it >> 5, j = it & 31;
            float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SS_K; ++k)
#pragma unroll
                for (int q = 0; q < 3; ++q) m[q] = fmaf(win.w[k], sm[q][rr * SS_IW + j + k], m[q]);
            hb[0][it] = m[0], hb[1][it] = m[1], hb[2][it] = m[2];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < SS_PER_THREAD; ++e) {
            const int o = t + e * SS_THREADS, i = o >> 5, j = o & 31;
            if (!in[e]) continue;
            float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SS_K; ++k)
#pragma unroll
                for (int q = 0; q < 3; ++q) m[q] = fmaf(win.w[k], hb[q][(i + k) * SS_TW + j], m[q]);
            const float xv = XC4 ? field_pick(x4[e], c) : xb[c * x.chan + pixel[e] * x.pix];
            const float yv = YC4 ? field_pick(y4[e], c) : yb[c * y.chan + pixel[e] * y.pix];
            const float v = scale * (m[0] + 2.f * xv * m[1] + yv * m[2]);
            if (XC4) {
                o4[e].x = c == 0 ? v : o4[e].x, o4[e].y = c == 1 ? v : o4[e].y;
                o4[e].z = c == 2 ? v : o4[e].z, o4[e].w = c == 3 ? v : o4[e].w;
            } else {
                ob[c * x.chan + pixel[e] * x.pix] = v;
            }
        }
        __syncthreads();                                           // the next channel's maps overwrite sm and hb
    }
#pragma unroll
    for (int e = 0; e < SS_PER_THREAD; ++e) {
        if (!in[e]) continue;
        if (XC4) *reinterpret_cast<float4 *>(ob + pixel[e] * 4) = o4[e];
        else
            for (int c = C; c < Cp; ++c) ob[c * x.chan + pixel[e] * x.pix] = 0.f;
    }
}

static SsWin ss_window()
{
    double w[SS_K], sum = 0.0;
    for (int k = 0; k < SS_K; ++k) sum += w[k] = exp(-(double)((k - SS_K / 2) * (k - SS_K / 2)) / (2.0 * 1.5 * 1.5));
    SsWin win;
    for (int k = 0; k < SS_K; ++k) win.w[k] = (float)(w[k] / sum);
    return win;
}

static bool ss_shape_ok(int rows, int C, int H, int W)
{
    return rows >= 1 && C >= 1 && H >= SS_MIN_HW && W >= SS_MIN_HW && H <= SS_MAX_HW && W <= SS_MAX_HW;
}
static int ss_tiles_x(int extent) { return (extent + SS_TW - 1) / SS_TW; }
static int ss_tiles_y(int extent) { return (extent + SS_TH - 1) / SS_TH; }

extern "C" size_t acg_ssim_workspace_bytes(int rows, int C, int H, int W)
{
    if (!ss_shape_ok(rows, C, H, W)) return 0;
    const size_t tiles = (size_t)ss_tiles_x(W - SS_HALO) * ss_tiles_y(H - SS_HALO);
    return (size_t)rows * (size_t)C * tiles * 2 * sizeof(double);
}

extern "C" int acg_ssim(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                        int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                        float data_range, float *out, float *dmaps, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_ssim";
    ACG_REQUIRE(x != nullptr && y != nullptr && out != nullptr, "%s: null tensor", fn);
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(ss_shape_ok(rows, C, H, W), "%s: fields must be H x W with %d <= H, W <= %d (got %d x %d)", fn, SS_MIN_HW, SS_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, rows));
    ACG_REQUIRE(data_range > 0.f && data_range <= 3.0e38f, "%s: data_range must be positive and finite (got %g)", fn, (double)data_range);
    ACG_REQUIRE((const void *)out != (const void *)x && (const void *)out != (const void *)y && (const void *)dmaps != (const void *)x &&
                    (const void *)dmaps != (const void *)y && (const void *)dmaps != (const void *)out,
                "%s: out and dmaps must not alias an input or each other", fn);
    const int Hv = H - SS_HALO, Wv = W - SS_HALO;
    const int ntx = ss_tiles_x(Wv), tiles = ntx * ss_tiles_y(Hv);
    ACG_REQUIRE((long long)rows * tiles <= 0x7fffffffLL && (long long)rows * C <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d)", fn,
                rows, C);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_ssim_workspace_bytes(rows, C, H, W)));
    hipStream_t st = (hipStream_t)stream;
    const SsWin win = ss_window();
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    const long long plane = (long long)rows * C * Hv * Wv;
    for (Field &o : f) o.mode = field_load_mode(o, C);
    const bool xc4 = f[0].mode == FIELD_C4, yc4 = f[1].mode == FIELD_C4;
    const dim3 grid((unsigned)((long long)rows * tiles)), block(SS_THREADS);
#define SS_FWD(XC, YC)                                                                                                                 \
    hipLaunchKernelGGL((ssim_fwd_kernel<XC, YC>), grid, block, 0, st, f[0], f[1], C, H, W, x_per_y, ntx, tiles, win, c1, c2, (double *)ws, \
                       dmaps, plane)
    if (xc4 && yc4) SS_FWD(true, true);
    else if (xc4) SS_FWD(true, false);
    else if (yc4) SS_FWD(false, true);
    else SS_FWD(false, false);
#undef SS_FWD
    hipLaunchKernelGGL(ssim_fold_kernel, dim3((unsigned)((long long)rows * C)), dim3(64), 0, st, (const double *)ws, tiles,
                       (double)Hv * (double)Wv, out);
    acg_note_kernel("ssim_fwd<%s, %s>%s + ssim_fold", xc4 ? "c4" : "strided", yc4 ? "c4" : "strided", dmaps ? " with maps" : "");
    ACG_CHECK_LAUNCH("acg_ssim");
    return ACG_OK;
}

extern "C" int acg_ssim_bwd(const float *dmaps, const float *x, const float *y, const float *g, int rows, int C, int Cp, int H, int W,
                            long long x_row_stride, int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                            long long y_chan_stride, float *gx, void *stream)
{
    const char *fn = "acg_ssim_bwd";
    ACG_REQUIRE(dmaps != nullptr && x != nullptr && y != nullptr && g != nullptr && gx != nullptr, "%s: null tensor", fn);
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    ACG_REQUIRE(rows >= 1 && C >= 1 && C <= Cp, "%s: need rows >= 1 and 1 <= C <= Cp stored channels (rows=%d, C=%d, Cp=%d)", fn, rows, C, Cp);
    ACG_REQUIRE(ss_shape_ok(rows, C, H, W), "%s: fields must be H x W with %d <= H, W <= %d (got %d x %d)", fn, SS_MIN_HW, SS_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    ACG_REQUIRE((const void *)gx != (const void *)dmaps && (const void *)gx != (const void *)x && (const void *)gx != (const void *)y &&
                    (const void *)gx != (const void *)g,
                "%s: gx must not alias an input", fn);
    const int Hv = H - SS_HALO, Wv = W - SS_HALO;
    const int ntx = ss_tiles_x(W), tiles = ntx * ss_tiles_y(H);
    ACG_REQUIRE((long long)rows * tiles <= 0x7fffffffLL && (long long)rows * C <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d)", fn,
                rows, C);
    hipStream_t st = (hipStream_t)stream;
    const SsWin win = ss_window();
    const float coef = (float)(-1.0 / ((double)rows * (double)C * (double)Hv * (double)Wv));
    const long long plane = (long long)rows * C * Hv * Wv;
    f[0].mode = field_load_mode(f[0], C, false, gx), f[1].mode = field_load_mode(f[1], C);
    const bool xc4 = Cp == 4 && f[0].mode == FIELD_C4, yc4 = f[1].mode == FIELD_C4;   // x's pixels leave as they came: 16 bytes of gx
    const dim3 grid((unsigned)((long long)rows * tiles)), block(SS_THREADS);
#define SS_BWD(XC, YC) \
    hipLaunchKernelGGL((ssim_bwd_kernel<XC, YC>), grid, block, 0, st, dmaps, plane, f[0], f[1], g, C, Cp, H, W, ntx, tiles, win, coef, gx)
    if (xc4 && yc4) SS_BWD(true, true);
    else if (xc4) SS_BWD(true, false);
    else if (yc4) SS_BWD(false, true);
    else SS_BWD(false, false);
#undef SS_BWD
    acg_note_kernel("ssim_bwd<%s, %s>", xc4 ? "c4" : "strided", yc4 ? "c4" : "strided");
    ACG_CHECK_LAUNCH("acg_ssim_bwd");
    return ACG_OK;
}
