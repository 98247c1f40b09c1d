// Support kernels of the convolution entry points (conv_api.hip), each behind its launcher: the VALU thin-output convolution,
// the column fix of the un-padded reflect data gradient, the reflection-pad folds, the column sums (bias gradient) and the
// split-K reduction of the weight-gradient partials.
#include "conv_internal.h"

// Convolutions whose OUTPUT has <= 4 real channels (7x7 32->3 head + tanh, PatchGAN heads, data gradients into
// image tensors).  N = 4 cannot feed a 32-wide MFMA tile, so this is a VALU kernel (HBM/L1-friendly form):
// LPP = Cin/4 lanes cooperate on one output pixel — lane j owns channels 4j..4j+3, so a wave reads whole
// contiguous pixel rows (coalesced) — each lane keeps 4 partial sums, the weights [tap][ci][4] are staged once
// per block in LDS, and the LPP partials are folded with wave shuffles.  Same Geom/Taps formulation as the MFMA
// kernel; lane 0 of each pixel writes the full C16 row (pad channels = 0).
#define THIN_PIX_ITERS 32
template <int LPP>
__global__ __launch_bounds__(256) void thin_out_conv_kernel(const float *__restrict__ in, const float *__restrict__ wn,
                                                            const float *__restrict__ bias, float *__restrict__ out,
                                                            Geom g, Taps taps)
{
    extern __shared__ __attribute__((aligned(16))) float wsm[]; // [taps.n][Cin][4]
    constexpr int PPB = 256 / LPP; // pixels per block pass
    const int tid = threadIdx.x, j = tid % LPP, pl = tid / LPP;
    const int wtot = taps.n * g.Cin; // float4 entries; slab order follows the tap LIST (taps.w indexes global slabs)
    for (int i = tid; i < wtot; i += 256) {
        const int t = i / g.Cin, k = i - t * g.Cin;
        *(f32x4 *)&wsm[i * 4] = *(const f32x4 *)(wn + ((long long)taps.w[t] * g.Cin + k) * 4);
    }
    __shared__ int tdy[64], tdx[64];
    if (tid < 64) { tdy[tid] = tid < taps.n ? taps.dy[tid] : 0; tdx[tid] = tid < taps.n ? taps.dx[tid] : 0; }
    __syncthreads();
    const int GHW = g.GH * g.GW;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 bv = z;
    if (bias != nullptr) bv = *(const f32x4 *)bias;
    for (int it = 0; it < THIN_PIX_ITERS; ++it) {
        const long long m = ((long long)blockIdx.x * THIN_PIX_ITERS + it) * PPB + pl;
        const bool mok = m < g.Mtot; // uniform across the LPP lanes of a pixel
        const long long mm = mok ? m : 0;
        const int n = (int)(mm / GHW);
        const int r = (int)(mm - (long long)n * GHW);
        const int gy = r / g.GW, gx = r - gy * g.GW;
        f32x4 acc = z;
        const float *img = in + (long long)n * g.Hin * g.Win * g.Cin + 4 * j;
        for (int t0 = 0; t0 < taps.n; t0 += 4) { // 4 taps per trip: their gathers are issued together
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + u;
                const int tt = t < taps.n ? t : 0;
                int iy = gy * g.is + tdy[tt], ix = gx * g.is + tdx[tt];
                bool ok = mok && t < taps.n;
                if (g.reflect) {
                    iy = iy < 0 ? -iy : iy;
                    iy = iy >= g.Hin ? 2 * (g.Hin - 1) - iy : iy;
                    ix = ix < 0 ? -ix : ix;
                    ix = ix >= g.Win ? 2 * (g.Win - 1) - ix : ix;
                } else {
                    ok = ok && iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Win;
                }
                v[u] = z;
                if (ok) v[u] = *(const f32x4 *)(img + ((long long)iy * g.Win + ix) * g.Cin);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + u < taps.n ? t0 + u : 0; // v[u] is zero for the tail taps
                const float *wt = &wsm[((long long)t * g.Cin + 4 * j) * 4];
                acc += v[u][0] * *(const f32x4 *)(wt) + v[u][1] * *(const f32x4 *)(wt + 4) +
                       v[u][2] * *(const f32x4 *)(wt + 8) + v[u][3] * *(const f32x4 *)(wt + 12);
            }
        }
#pragma unroll
        for (int sft = LPP / 2; sft >= 1; sft >>= 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], sft, 64);
        }
        if (j == 0 && mok) {
            acc += bv;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acg_apply_act_ch(acc[k], g.act, k);
            float *o = out + (((long long)n * g.Hout + (gy * g.os + g.oy0)) * g.Wout + (gx * g.os + g.ox0)) * g.Cout;
            *(f32x4 *)o = acc;
            for (int c = 4; c < g.Cout; c += 4) *(f32x4 *)(o + c) = z;
        }
    }
}

int acg_thin_out_launch(const float *in, const float *wn, const float *bias, float *out, const Geom &g, const Taps &t,
                           hipStream_t st)
{
    if (g.Mtot <= 0 || t.n <= 0) return ACG_OK;
    const int lpp = g.Cin / 4;
    ACG_REQUIRE(lpp == 4 || lpp == 8 || lpp == 16 || lpp == 32 || lpp == 64, "thin_out_conv: Cin=%d unsupported", g.Cin);
    const size_t lds = (size_t)t.n * g.Cin * 4 * sizeof(float);
    ACG_REQUIRE(lds <= 160 * 1024, "thin_out_conv: weights (%zu B) exceed LDS", lds);
    const int ppb = (256 / lpp) * THIN_PIX_ITERS;
    dim3 grid(acg_cdiv(g.Mtot, ppb)), block(256);
#define THIN_LAUNCH(L) hipLaunchKernelGGL((thin_out_conv_kernel<L>), grid, block, lds, st, in, wn, bias, out, g, t)
    switch (lpp) {
    case 4: THIN_LAUNCH(4); break;
    case 8: THIN_LAUNCH(8); break;
    case 16: THIN_LAUNCH(16); break;
    case 32: THIN_LAUNCH(32); break;
    default: THIN_LAUNCH(64); break;
    }
#undef THIN_LAUNCH
    ACG_CHECK_LAUNCH("thin_out_conv_kernel");
    acg_note_kernel("thin_out_conv<LPP=%d>", lpp);
    return ACG_OK;
}

// Column part of the reflect adjoint for the un-padded data gradient (Geom.unpad): pad column -1 mirrors onto column 1, pad
// column W onto column W-2, i.e. dx[y][1] += sum_kh dy[y + 1 - kh][0] . w[kh][0] and dx[y][W-2] += sum_kh dy[y + 1 - kh][W-1] .
// w[kh][2] (rows outside the map are zero; rows 1 and H-2 also receive the corner terms dy[0] . w[0][.] / dy[H-1] . w[2][.]
// their own mirrored rows carry).  A (N H 2) x (3 C) x C GEMM, 0.4 % of the layer: one 32x32x16 MFMA tile per wave, both
// operands read straight into fragment layout — a pre-split pixel's 8-channel group IS an A fragment, 8 consecutive output
// channels of a packed-wb row ARE a B fragment — same bf16x3 products as the main kernel.
// grid (N * H / 32, 2, CiP / 128) x 256 threads: 32 rows of one image, one side, wave w = dx channels 32w .. 32w+31 of 128.
typedef __bf16 cf_bf16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void dgrad_colfix_kernel(const char *__restrict__ dy, const __bf16 *__restrict__ wb,
                                                           long long w_lo_elems, float *__restrict__ colfix, int H, int W,
                                                           int C, int CiP, int Cdx)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = H / 32, n = blockIdx.x / tiles, qy0 = (blockIdx.x - n * tiles) * 32, side = blockIdx.y;
    const int lr = lane & 31, kg = lane >> 5;
    const int qy = qy0 + lr, ci = blockIdx.z * 128 + wave * 32 + lr;
    const int col = side ? W - 1 : 0, kw = side ? 2 : 0;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const cf_bf16x8 zero = {};
    // kernel rows 0..2, then the corner term of the tile that holds row 1 (kh 0, dy row 0) or row H-2 (kh 2, dy row H-1).
    // A step is 128 channels = eight 16-channel chunks whose 32 fragment loads are issued together, the next step's before this
    // step's MFMAs (one wave per SIMD: registers are free, memory latency is the whole cost of this kernel).
    const int extra = qy0 == 0 ? 0 : (qy0 + 32 == H ? 2 : -1);
    const int nsteps = (3 + (extra >= 0 ? 1 : 0)) * (C / 128);
    cf_bf16x8 ah[2][8], al[2][8], bh[2][8], bl[2][8];
    auto load = [&](int s, int b) {
        const int step = s / (C / 128), c128 = s - step * (C / 128);
        const int kh = step < 3 ? step : extra;
        int ry;
        bool ok;
        if (step < 3) { ry = qy + 1 - kh; ok = (unsigned)ry < (unsigned)H; }
        else { ry = extra == 0 ? 0 : H - 1; ok = qy == (extra == 0 ? 1 : H - 2); }
        const char *ap = dy + (((long long)n * H + (ok ? ry : 0)) * W + col) * C * 4 + c128 * 512 + kg * 32;
        const __bf16 *bp = wb + (((long long)(kh * 3 + kw) * (C / 16) + c128 * 8) * CiP + ci) * 16 + kg * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ah[b][u] = zero; al[b][u] = zero;
            if (ok) { ah[b][u] = *(const cf_bf16x8 *)(ap + u * 64); al[b][u] = *(const cf_bf16x8 *)(ap + u * 64 + 16); }
            bh[b][u] = *(const cf_bf16x8 *)(bp + (long long)u * CiP * 16);
            bl[b][u] = *(const cf_bf16x8 *)(bp + w_lo_elems + (long long)u * CiP * 16);
        }
    };
    auto mma = [&](int b) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[b][u], bh[b][u], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[b][u], bl[b][u], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[b][u], bh[b][u], acc, 0, 0, 0);
        }
    };
    load(0, 0);
    for (int s = 0; s < nsteps; s += 2) {   // two steps per trip: the buffer index stays a compile-time constant
        if (s + 1 < nsteps) load(s + 1, 1);
        mma(0);
        if (s + 2 < nsteps) load(s + 2, 0);
        if (s + 1 < nsteps) mma(1);
    }
    if (ci < Cdx) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kg;
            colfix[(((long long)n * H + qy0 + row) * 2 + side) * Cdx + ci] = acc[r];
        }
    }
}
int acg_dgrad_colfix_launch(const acg_conv_desc *d, const void *dy, const float *wb, long long w_lo_elems, float *colfix, hipStream_t st)
{
    const int CiP = acg_ncols_pad(d->Ci);
    hipLaunchKernelGGL(dgrad_colfix_kernel, dim3(d->N * (d->Hi / 32), 2, CiP / 128), dim3(256), 0, st, (const char *)dy,
                       (const __bf16 *)wb, w_lo_elems, colfix, d->Hi, d->Wi, d->Co, CiP, d->Ci);
    ACG_CHECK_LAUNCH("dgrad_colfix_kernel");
    return ACG_OK;
}

// ---- reflection-pad adjoint: dxp[N][H+2p][W+2p][C] -> dx[N][H][W][C], folding mirrored borders ------------------------------
// (torch reflection_pad2d_backward).  float4 over channels.
__global__ void reflect_fold_kernel(const float *__restrict__ dxp, float *__restrict__ dx, int N, int H, int W, int C, int p)
{
    const int C4 = C / 4;
    const long long total = (long long)N * H * W * C4;
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int c4 = (int)(r % C4); r /= C4;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H); r /= H;
        const int n = (int)r;
        // padded rows that read input row y: y+p, plus mirrors p-y (1<=y<=p) and 2(H-1)-y+p (H-1-p<=y<=H-2)
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + p;
        if (y >= 1 && y <= p) ys[ny++] = p - y;
        if (y >= H - 1 - p && y <= H - 2) ys[ny++] = 2 * (H - 1) - y + p;
        xs[nx++] = x + p;
        if (x >= 1 && x <= p) xs[nx++] = p - x;
        if (x >= W - 1 - p && x <= W - 2) xs[nx++] = 2 * (W - 1) - x + p;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b)
                acc += *(const f32x4 *)(dxp + (((long long)n * Hp + ys[a]) * Wp + xs[b]) * C + c4 * 4);
        *(f32x4 *)(dx + i * 4) = acc;
    }
}

// The same fold restricted to the FRAME: the input pixels the pad ring mirrors onto (rows / columns 1..p and
// H-1-p..H-2).  Used when the data-gradient kernel already stored every other pixel straight into dx (Geom.fold_p):
// 2p rows x W plus 2p columns x (H - 2p) pixels per image instead of all H x W.
__global__ void reflect_fold_frame_kernel(const float *__restrict__ dxp, float *__restrict__ dx, int N, int H, int W, int C,
                                          int p, const float *__restrict__ addend, const float *__restrict__ relu_src,
                                          const unsigned *__restrict__ addend_mask, int out_s16, int relu_s16)
{
    const int C4 = C / 4;
    const int nrow = 2 * p * W, ncol = 2 * p * (H - 2 * p); // frame pixels per image: dirty rows, then dirty columns
    const long long total = (long long)N * (nrow + ncol) * C4;
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int c4 = (int)(r % C4); r /= C4;
        const int f = (int)(r % (nrow + ncol));
        const int n = (int)(r / (nrow + ncol));
        int y, x;
        if (f < nrow) { // dirty row k: rows 1..p then H-1-p..H-2
            const int k = f / W;
            x = f - k * W;
            y = k < p ? 1 + k : H - 1 - p + (k - p);
        } else {        // dirty column k of a clean row
            const int q = f - nrow, k = q / (H - 2 * p), yy = q - k * (H - 2 * p);
            x = k < p ? 1 + k : W - 1 - p + (k - p);
            y = yy == 0 ? 0 : (yy <= H - 2 - 2 * p ? p + yy : H - 1); // clean rows: 0, p+1..H-2-p, H-1
        }
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + p;
        if (y >= 1 && y <= p) ys[ny++] = p - y;
        if (y >= H - 1 - p && y <= H - 2) ys[ny++] = 2 * (H - 1) - y + p;
        xs[nx++] = x + p;
        if (x >= 1 && x <= p) xs[nx++] = p - x;
        if (x >= W - 1 - p && x <= W - 2) xs[nx++] = 2 * (W - 1) - x + p;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b)
                acc += *(const f32x4 *)(dxp + (((long long)n * Hp + ys[a]) * Wp + xs[b]) * C + c4 * 4);
        const long long o = (((long long)n * H + y) * W + x) * C + c4 * 4;
        // pre-split (S16) tensors: the 8-channel group of element o starts at byte 4 * (o & ~7); hi halves at +0, lo at +16
        const long long sb = 4 * (o & ~7LL) + 2 * (o & 7);
        if (relu_src != nullptr) { // same order as the convolution epilogue: mask, then addend
            if (relu_s16) {
                const uint2 sv = *(const uint2 *)((const char *)relu_src + sb);
                const unsigned h[4] = {sv.x & 0xffffu, sv.x >> 16, sv.y & 0xffffu, sv.y >> 16};
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = (h[q] - 1u) < 0x7fffu ? acc[q] : 0.f;
            } else {
                const f32x4 mv = *(const f32x4 *)(relu_src + o);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = mv[q] > 0.f ? acc[q] : 0.f;
            }
        }
        if (addend != nullptr) {
            f32x4 av = *(const f32x4 *)(addend + o);
            if (addend_mask != nullptr) {
                const long long f = o >> 2;
                const unsigned nb = (addend_mask[f >> 3] >> (4 * (int)(f & 7))) & 15u;
#pragma unroll
                for (int q = 0; q < 4; ++q) av[q] = (nb >> q) & 1u ? av[q] : 0.f;
            }
            acc += av;
        }
        if (out_s16) {
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            typedef float f32x2_t __attribute__((ext_vector_type(2)));
            uint2 hi, lo;
            unsigned *hp = &hi.x, *lp = &lo.x;
#pragma unroll
            for (int q = 0; q < 2; ++q) { // the arithmetic of acg_split8
                const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){acc[2 * q], acc[2 * q + 1]}, bf16x2_t));
                const float ha = __builtin_bit_cast(float, h << 16), hb = __builtin_bit_cast(float, h & 0xffff0000u);
                hp[q] = h;
                lp[q] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){acc[2 * q] - ha, acc[2 * q + 1] - hb}, bf16x2_t));
            }
            *(uint2 *)((char *)dx + sb) = hi;
            *(uint2 *)((char *)dx + sb + 16) = lo;
        } else {
            *(f32x4 *)(dx + o) = acc;
        }
    }
}
static int fold_blocks(long long total) { return acg_cdiv(total, 256) > 4096 ? 4096 : acg_cdiv(total, 256); }
int acg_reflect_fold_launch(const acg_conv_desc *d, const float *dxp, float *dx, hipStream_t st)
{
    const int blocks = fold_blocks((long long)d->N * d->Hi * d->Wi * (d->Ci / 4));
    hipLaunchKernelGGL(reflect_fold_kernel, dim3(blocks), dim3(256), 0, st, dxp, dx, d->N, d->Hi, d->Wi, d->Ci, d->pad);
    ACG_CHECK_LAUNCH("reflect_fold_kernel");
    return ACG_OK;
}
int acg_reflect_fold_frame_launch(const acg_conv_desc *d, const float *dxp, float *dx, const float *addend, const float *relu_src,
                                  const unsigned *addend_mask, int out_s16, int relu_s16, hipStream_t st)
{
    const int p = d->pad;
    const int blocks = fold_blocks((long long)d->N * (2 * p * d->Wi + 2 * p * (d->Hi - 2 * p)) * (d->Ci / 4));
    hipLaunchKernelGGL(reflect_fold_frame_kernel, dim3(blocks), dim3(256), 0, st, dxp, dx, d->N, d->Hi, d->Wi, d->Ci, p, addend,
                       relu_src, addend_mask, out_s16, relu_s16);
    ACG_CHECK_LAUNCH("reflect_fold_frame_kernel");
    return ACG_OK;
}

// ---- column sums (bias gradient): dy[M][C] -> db[c] (first Cr columns), two deterministic stages ----------------------------
#define COLSUM_ROWS 2048
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float *__restrict__ dy, long long M, int C, float *__restrict__ part)
{
    __shared__ float red[256 * 4];
    const int C4 = C / 4;             // <= 256
    const int lanes_per_row = C4;     // threads covering one row
    const int rows_par = 256 / lanes_per_row;
    const int c4 = threadIdx.x % lanes_per_row, rl = threadIdx.x / lanes_per_row;
    const long long r0 = (long long)blockIdx.x * COLSUM_ROWS;
    long long r1 = r0 + COLSUM_ROWS;
    if (r1 > M) r1 = M;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (rl < rows_par)
        for (long long r = r0 + rl; r < r1; r += rows_par) acc += *(const f32x4 *)(dy + r * C + c4 * 4);
    *(f32x4 *)&red[threadIdx.x * 4] = acc;
    __syncthreads();
    if (threadIdx.x < lanes_per_row) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < rows_par; ++k) s += *(const f32x4 *)&red[(k * lanes_per_row + threadIdx.x) * 4];
        *(f32x4 *)(part + (long long)blockIdx.x * C + threadIdx.x * 4) = s;
    }
}
// 16 channels x 16 partial-row lanes per block (channel c = c0 + (tid & 15), lane tid >> 4 sums rows lane, lane + 16, ... of
// part[nrows][Cp]), folded by a fixed-order LDS tree: deterministic.  db[c] is set or, with `accumulate`, added to (c < Cr)
__device__ __forceinline__ void bias_tree16(const float *__restrict__ part, int nrows, int Cp, int Cr, int c0, float *__restrict__ db, int accumulate, float *red)
{
    const int c = c0 + (threadIdx.x & 15);
    float s = 0.f;
    if (c < Cr)
        for (int k = threadIdx.x >> 4; k < nrows; k += 16) s += part[(long long)k * Cp + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st >= 16; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 16 && c < Cr) db[c] = (accumulate ? db[c] : 0.f) + red[threadIdx.x];
}
__global__ __launch_bounds__(256) void colsum_final_kernel(const float *__restrict__ part, int nblk, int C, int Cr,
                                                           float *__restrict__ db, int accumulate)
{
    __shared__ float red[256];
    bias_tree16(part, nblk, C, Cr, blockIdx.x * 16, db, accumulate, red);
}
size_t acg_colsum_ws_bytes(long long M, int C) { return (size_t)acg_cdiv(M, COLSUM_ROWS) * C * sizeof(float); }
int acg_colsum_launch(const float *dy, long long M, int C, int Cr, float *db, float *ws, hipStream_t st, int accumulate)
{
    ACG_REQUIRE(C % 4 == 0 && C / 4 <= 256, "colsum: C=%d unsupported", C);
    const int nblk = acg_cdiv(M, COLSUM_ROWS);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(nblk), dim3(256), 0, st, dy, M, C, ws);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(acg_cdiv(Cr, 16)), dim3(256), 0, st, ws, nblk, C, Cr, db, accumulate);
    ACG_CHECK_LAUNCH("colsum");
    return ACG_OK;
}

// ---- split-K reduction of weight-gradient partials -> torch OIHW (real Or x Ir) ---------------------------------------------
// part[nsplit][KK][CiP][CoP]
// thin: part[nsplit][1][CiP][CoP] with row = tap*4 + ci
// accumulate != 0: dw (and db) are ADDED to — the caller passes the parameter's .grad itself, so no separate accumulation
// kernel runs per parameter (torch's AccumulateGrad launched 564 five-microsecond adds per training step).
// The bias reduction rides in the same launch: blocks [wblocks, wblocks + ceil(Cr/16)) reduce bias_part[nsplit][Cp] -> db
// (16 channels per block, 16 split-lanes each, fixed-order tree: deterministic).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, int nsplit, int KK, int CiP, int CoP, int Or,
                                    int Ir, float *__restrict__ dw, int thin, int accumulate, int wblocks,
                                    const float *__restrict__ bias_part, int Cp, int Cr, float *__restrict__ db, int bias_slots,
                                    int el_log2)
{
    if ((int)blockIdx.x >= wblocks) {
        __shared__ float red[256];
        bias_tree16(bias_part, bias_slots, Cp, Cr, ((int)blockIdx.x - wblocks) * 16, db, accumulate, red);
        return;
    }
    // Weight part: a block is EL elements x (256 / EL) split-lanes; lane group kl sums the slabs k = kl, kl + KL, ... of its
    // element (coalesced over the EL elements), the groups fold through LDS in fixed order: deterministic.  An element is four
    // adjacent output channels where the layout allows (16-byte loads; the one-float-per-thread sequential version read a
    // 50 MB trunk slab set at 3.8 TB/s, 128 launches = 1.7 ms per step), else one.  `el_log2` = 6 (64 elements x 4 lanes), or 4
    // (16 x 16) when there are few elements and many slabs (the persistent thin-patch kernel leaves 768 of them).
    __shared__ f32x4 red4[256];
    const int EL = 1 << el_log2, KL = 256 >> el_log2;
    const int el = threadIdx.x & (EL - 1), kl = threadIdx.x >> el_log2;
    const bool quad = thin != 2 && (Or & 3) == 0 && (CoP & 3) == 0;
    const int On = quad ? Or >> 2 : Or;
    const long long total = (long long)KK * Ir * On;
    const long long i = (long long)blockIdx.x * EL + el;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    int o = 0, ci = 0, tap = 0;
    if (i < total) {
        long long r = i;
        o = (int)(r % On); r /= On;
        ci = (int)(r % Ir); r /= Ir;
        tap = (int)r;
        const long long stride = thin ? (long long)CiP * CoP : (long long)KK * CiP * CoP;
        const int oo = quad ? o * 4 : o;
        const float *p = thin == 2 ? part + ((long long)(tap * 4 + oo)) * CoP + ci   // rows (tap, co), columns ci
                       : thin == 1 ? part + ((long long)(tap * 4 + ci)) * CoP + oo  // rows (tap, ci), columns co
                                   : part + ((long long)tap * CiP + ci) * CoP + oo;
        if (quad) {
#pragma unroll 4
            for (int k = kl; k < nsplit; k += KL) sum += *(const f32x4 *)(p + k * stride);
        } else {
#pragma unroll 4
            for (int k = kl; k < nsplit; k += KL) sum[0] += p[k * stride];
        }
    }
    red4[threadIdx.x] = sum;
    __syncthreads();
    if (kl != 0 || i >= total) return;
    for (int k = 1; k < KL; ++k) sum += red4[k * EL + el];
    const int ne = quad ? 4 : 1;
    for (int e = 0; e < ne; ++e) {
        float *dst = dw + ((long long)((quad ? o * 4 : o) + e) * Ir + ci) * KK + tap;
        *dst = (accumulate ? *dst : 0.f) + sum[e];
    }
}
// dw (real Or x Ir, torch OIHW) from part[nsplit][...]; Cr > 0: also db[0 .. Cr) from bias_part[bias_slots][Cp]
int acg_wgrad_reduce_launch(const float *part, int nsplit, int KK, int CiP, int CoP, int Or, int Ir, float *dw, int thin,
                            int accumulate, const float *bias_part, int Cp, int Cr, float *db, int bias_slots, hipStream_t st)
{
    const bool quad = thin != 2 && Or % 4 == 0 && CoP % 4 == 0;   // the kernel's four-channels-per-element path
    const long long total = (long long)KK * Ir * (quad ? Or / 4 : Or);
    const int el_log2 = (total < 8192 && nsplit >= 64) ? 4 : 6;
    const int wblocks = acg_cdiv(total, 1 << el_log2);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(wblocks + acg_cdiv(Cr, 16)), dim3(256), 0, st, part, nsplit, KK, CiP, CoP, Or, Ir,
                       dw, thin, accumulate, wblocks, bias_part, Cp, Cr, db, bias_slots, el_log2);
    ACG_CHECK_LAUNCH("wgrad_reduce_kernel");
    return ACG_OK;
}
