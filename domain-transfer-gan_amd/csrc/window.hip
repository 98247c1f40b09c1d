// Windows of native-resolution fields (ops.window_gather / ops.window_blend, model.translate_field, train.py --native_res).
// acg_window_gather cuts T windows of S x S out of NCHW fields and writes them NHWC with Cp stored channels (the layout
// change of acg_nchw_to_nhwc16 fused into the cut); acg_window_blend puts the tiles of a separable window grid back on an NCHW
// canvas, every canvas pixel the weighted mean of the tile pixels that cover it.
// Both kernels give one workgroup a run of WIN_THREADS pixels along x of ONE row (of a window resp. of the canvas) and one
// quad of 4 stored channels, so everything but x is workgroup-uniform: the table row, the covering tile rows and their
// weights sit in scalar registers.  A lane moves one 16-byte pixel quad on the NHWC side and one float per plane on the NCHW
// side; consecutive lanes take consecutive x, so the plane accesses of a wave are one contiguous segment in either mirror
// direction.  Neither kernel clamps an index: the gather's table is the caller's precondition (ops.window_gather checks every
// row before the upload), the blend's record is checked here before the launch.
// The blend is in gather form: a lane owns its canvas pixel and walks the covering tiles (ky outer, kx inner, ascending),
// no atomics, so a repeat gives the same bits.  The weights are the integers min(i + 1, S - i, R) — the 1 / R of the stated
// weight cancels between numerator and denominator — and a pixel under exactly one tile is copied, not computed.
#include "common.h"

#define WIN_THREADS 128

struct WinRow {
    int src, oy, ox, flip;
};

__global__ __launch_bounds__(WIN_THREADS) void window_gather_kernel(const float *__restrict__ fields, const WinRow *__restrict__ table,
                                                                    float *__restrict__ out, int C, int H, int W, int S, int nq,
                                                                    int xblocks)
{
    // block -> (window t, window row i, channel quad q, run of x)
    unsigned b = blockIdx.x;
    const int xb = (int)(b % (unsigned)xblocks);
    b /= (unsigned)xblocks;
    const int q = (int)(b % (unsigned)nq);
    b /= (unsigned)nq;
    const int i = (int)(b % (unsigned)S), t = (int)(b / (unsigned)S);
    const int j = xb * WIN_THREADS + (int)threadIdx.x;
    if (j >= S) return;
    const WinRow r = table[t];
    const int y = r.oy + ((r.flip & 2) ? S - 1 - i : i);
    const int x = r.ox + ((r.flip & 1) ? S - 1 - j : j);
    const long long HW = (long long)H * W;
    const float *p = fields + ((long long)r.src * C + 4 * q) * HW + (long long)y * W + x;
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = 4 * q + c < C ? p[c * HW] : 0.f;
    *(f32x4 *)(out + ((((long long)t * S + i) * S + j) * nq + q) * 4) = v;
}

extern "C" int acg_window_gather(const float *fields, const int *table, float *out, int N, int C, int H, int W, int T, int S,
                                 int Cp, void *stream)
{
    ACG_REQUIRE(fields != nullptr && table != nullptr && out != nullptr, "acg_window_gather: null pointer");
    ACG_REQUIRE(N >= 1 && T >= 1, "acg_window_gather: need N >= 1 fields and T >= 1 windows (N=%d, T=%d)", N, T);
    ACG_REQUIRE(S >= 1 && H >= S && W >= S, "acg_window_gather: need 1 <= S <= H, W (S=%d, H=%d, W=%d)", S, H, W);
    ACG_REQUIRE((Cp == 4 || (Cp >= 16 && Cp % 16 == 0)) && C >= 1 && C <= Cp,
                "acg_window_gather: need 1 <= C <= Cp, Cp 4 or a multiple of 16 (C=%d, Cp=%d)", C, Cp);
    ACG_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 15) == 0, "acg_window_gather: out and table must be 16-byte aligned");
    const int nq = Cp / 4, xblocks = acg_cdiv(S, WIN_THREADS);
    const long long per_line = (long long)nq * xblocks;        // blocks of one window line; the product below cannot overflow
    ACG_REQUIRE((long long)T * S <= 0x7fffffffLL / per_line, "acg_window_gather: too large (T=%d, S=%d, Cp=%d)", T, S, Cp);
    const long long blocks = (long long)T * S * per_line;
    const dim3 grid((unsigned)blocks), blk(WIN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const WinRow *tab = (const WinRow *)table;
    hipLaunchKernelGGL(window_gather_kernel, grid, blk, 0, st, fields, tab, out, C, H, W, S, nq, xblocks);
    ACG_CHECK_LAUNCH("acg_window_gather");
    return ACG_OK;
}

__device__ __forceinline__ int win_weight(int i, int S, int R) { return min(min(i + 1, S - i), R); }

__global__ __launch_bounds__(WIN_THREADS) void window_blend_kernel(const float *__restrict__ tiles, acg_window_plan P,
                                                                   float *__restrict__ canvas, int C, int nq, int xblocks)
{
    // block -> (canvas row r, channel quad q, canvas line y, run of x)
    unsigned b = blockIdx.x;
    const int xb = (int)(b % (unsigned)xblocks);
    b /= (unsigned)xblocks;
    const int y = (int)(b % (unsigned)P.H);
    b /= (unsigned)P.H;
    const int q = (int)(b % (unsigned)nq), r = (int)(b / (unsigned)nq);
    const int x = xb * WIN_THREADS + (int)threadIdx.x;
    if (x >= P.W) return;
    const int S = P.S, R = P.R;
    // the covering tile rows are a contiguous range of ky (origins ascend): workgroup-uniform
    int ky0 = 0;
    while (P.oy[ky0] + S <= y) ++ky0;
    int ky1 = ky0;
    while (ky1 < P.ny && P.oy[ky1] <= y) ++ky1;
    // along x the cover differs from lane to lane: count it, and keep the first covering column and its origin
    int nkx = 0, kxf = 0, oxf = 0;
    for (int kx = P.nx - 1; kx >= 0; --kx) {
        const int o = P.ox[kx];
        const bool in = o <= x && x < o + S;
        nkx += in ? 1 : 0;
        kxf = in ? kx : kxf;
        oxf = in ? o : oxf;
    }
    const long long tile = (long long)S * S * nq * 4, line = (long long)S * nq * 4;
    const float *base = tiles + (long long)r * P.ny * P.nx * tile + 4 * q;
    f32x4 v;
    if ((ky1 - ky0) * nkx == 1) {
        // single coverage: the tile's bits
        v = *(const f32x4 *)(base + ((long long)ky0 * P.nx + kxf) * tile + (y - P.oy[ky0]) * line + (long long)(x - oxf) * nq * 4);
    } else {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float wsum = 0.f;
        for (int ky = ky0; ky < ky1; ++ky) {
            const int iy = y - P.oy[ky], wy = win_weight(iy, S, R);
            for (int kx = 0; kx < P.nx; ++kx) {
                const int jx = x - P.ox[kx];
                if (jx < 0 || jx >= S) continue;
                const float w = (float)(wy * win_weight(jx, S, R));
                const f32x4 u = *(const f32x4 *)(base + ((long long)ky * P.nx + kx) * tile + iy * line + (long long)jx * nq * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, u[c], acc[c]);
                wsum += w;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = acc[c] / wsum;
    }
    const long long HW = (long long)P.H * P.W;
    float *o = canvas + ((long long)r * C + 4 * q) * HW + (long long)y * P.W + x;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (4 * q + c < C) o[c * HW] = v[c];
}

// origins of one axis: 1..ACG_WINDOW_MAX of them, strictly ascending from 0 to extent - S, no gap wider than S
static int win_check_axis(const char *axis, int extent, int S, int n, const int *o)
{
    ACG_REQUIRE(n >= 1 && n <= ACG_WINDOW_MAX, "acg_window_blend: need 1..%d windows along %s (got %d)", ACG_WINDOW_MAX, axis, n);
    ACG_REQUIRE(extent >= S, "acg_window_blend: extent %d along %s is below the window %d", extent, axis, S);
    ACG_REQUIRE(o[0] == 0, "acg_window_blend: the first origin along %s must be 0 (got %d)", axis, o[0]);
    ACG_REQUIRE(o[n - 1] == extent - S, "acg_window_blend: the last origin along %s must be %d (got %d)", axis, extent - S, o[n - 1]);
    for (int k = 1; k < n; ++k) {
        ACG_REQUIRE(o[k] > o[k - 1], "acg_window_blend: origins along %s must ascend (%d after %d)", axis, o[k], o[k - 1]);
        ACG_REQUIRE(o[k] - o[k - 1] <= S, "acg_window_blend: origins %d and %d along %s leave a gap (window %d)", o[k - 1], o[k], axis, S);
    }
    return ACG_OK;
}

extern "C" int acg_window_blend(const float *tiles, const acg_window_plan *plan, float *canvas, int rows, int C, int Cp, void *stream)
{
    ACG_REQUIRE(tiles != nullptr && plan != nullptr && canvas != nullptr, "acg_window_blend: null pointer");
    ACG_REQUIRE(rows >= 1, "acg_window_blend: need rows >= 1 (got %d)", rows);
    ACG_REQUIRE((Cp == 4 || (Cp >= 16 && Cp % 16 == 0)) && C >= 1 && C <= Cp,
                "acg_window_blend: need 1 <= C <= Cp, Cp 4 or a multiple of 16 (C=%d, Cp=%d)", C, Cp);
    const acg_window_plan &P = *plan;
    ACG_REQUIRE(P.S >= 1 && P.S <= 4096, "acg_window_blend: need a window of 1..4096 (S=%d)", P.S);
    ACG_REQUIRE(P.R >= 1 && P.R <= P.S, "acg_window_blend: need a ramp 1 <= R <= S (R=%d, S=%d)", P.R, P.S);
    int rc = win_check_axis("y", P.H, P.S, P.ny, P.oy);
    if (rc != ACG_OK) return rc;
    rc = win_check_axis("x", P.W, P.S, P.nx, P.ox);
    if (rc != ACG_OK) return rc;
    ACG_REQUIRE(((uintptr_t)tiles & 15) == 0, "acg_window_blend: tiles must be 16-byte aligned");
    const int nq = Cp / 4, xblocks = acg_cdiv(P.W, WIN_THREADS);
    const long long per_row = (long long)nq * P.H * xblocks;   // blocks of one canvas: H, W <= 64 S <= 2^18 here, no overflow
    ACG_REQUIRE(rows <= 0x7fffffffLL / per_row, "acg_window_blend: too large (rows=%d, H=%d, W=%d, Cp=%d)", rows, P.H, P.W, Cp);
    const long long blocks = rows * per_row;
    hipLaunchKernelGGL(window_blend_kernel, dim3((unsigned)blocks), dim3(WIN_THREADS), 0, (hipStream_t)stream, tiles, P, canvas, C,
                       nq, xblocks);
    ACG_CHECK_LAUNCH("acg_window_blend");
    return ACG_OK;
}
