// Radial and cross spectra of whole fields of any H x W in 16 .. 1024 (ops.field_spectrum, ops.field_cross_spectrum,
// model.translate_field_spectrum, test.py --metric field_spectrum).  Per field x[h, w] of one channel of one image:
// P = |fft2(x)|^2 / (H W), averaged over elliptical rings: with L = min(H, W) and signed wavenumbers (fy, fx) the ring radius of
// a cell is L sqrt((fy / H)^2 + (fx / W)^2) rounded to nearest, in integers: bin 0 is the cell fy = fx = 0, otherwise the largest
// b with b (b - 1) H^2 W^2 < L^2 (fy^2 W^2 + fx^2 H^2); bins 0 .. L/2, the cells beyond are dropped.  Ring b is "b cycles per L
// pixels" along either axis.  Per pair x, y and ring: the means of Pxx, Pyy and Cxy = Re(X conj Y) / (H W).  There is no
// reference call site; tests/field_spectrum_ref.py states the definition.  H = W = S a power of two is acg_radial_spectrum's
// and acg_cross_spectrum's own case and is forwarded to them: the same bits.
//
// Everything else takes four launches on the caller's stream, with nothing kept inside the library between calls:
//   setup   per axis whose length N is no power of two, into the head of the workspace: the chirp c[n] = exp(-i pi n^2 / N)
//           (n^2 reduced mod 2 N in integers, sincospi in double, rounded once) and the transformed filter of Bluestein's
//           chirp-z: the M-point transform of conj c[|n|] laid around 0, M the power of two >= 2 N - 1, times 1 / M.
//   rows    one workgroup per pair of rows of one field: z = row 2r + i row 2r+1 (an odd H leaves the last row alone with a zero
//           imaginary part), its W-point transform, untangled into the two rows' half spectra kx = 0 .. W/2 (an odd W has no
//           Nyquist column; nothing is packed), written to the workspace as [h][W/2 + 1].
//   cols    one workgroup per column kx of a field or pair: the H-point transform of that column of every field, then the
//           products w |X|^2 / (H W) (a pair: w |Y|^2 and w Re(X conj Y) behind it), w = 2 where the Hermitian twin is no stored
//           cell (0 < kx, 2 kx != W), into planes [kx][ky] of the workspace.
//   rings   one workgroup per field or pair, one work item per (ring, sign of fy): the item enumerates its ring's cells row
//           by row from the integer rule and sums every plane in double in that order, and counts the cells.  No float atomics:
//           a repeat gives the same bits, and no step depends on the input's layout.
// A transform of a power-of-two length is the radix-2 Stockham autosort of spectrum.hip on run-time lengths.  Any other length N
// is Bluestein on those stages: a[n] = x[n] c[n] padded with zeros to M, forward stages, times the transformed filter, the forward
// stages on the conjugate (the inverse), times c[k].  The two axes choose independently.  The two fields of a pair share every
// launch but never a complex transform, and each is transformed exactly as a single field is: Pxx of a pair has the bits of
// the field's own spectrum.
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "field.h"
#include "spectrum_shared.h"

#define FS_MIN 16
#define FS_MAX 1024
#define FS_THREADS 256
#define FS_MAX_BINS (FS_MAX / 2 + 1)

static bool fs_pow2(int n) { return (n & (n - 1)) == 0; }
static bool fs_extent_ok(int n) { return n >= FS_MIN && n <= FS_MAX; }
// the length of the transforms that carry a transform of length N: N itself, or the power of two >= 2 N - 1 (at most 2048)
static int fs_padded(int N)
{
    if (fs_pow2(N)) return N;
    int M = 1;
    while (M < 2 * N - 1) M <<= 1;
    return M;
}

// the products pinned as fused multiply-adds: a result keeps its bits between the one-field and the pair kernels only while
// both make the same choice
__device__ __forceinline__ float2 fs_cmul(float2 a, float2 b)
{
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float fs_dot2(float a, float b, float c, float d) { return fmaf(a, b, c * d); }

// the M-point transform of a (M a power of two), radix-2 Stockham autosort between a and b; returns the buffer of the result
__device__ __forceinline__ float2 *fs_fft(float2 *a, float2 *b, const float2 *tw, int M)
{
    const int half = M >> 1;
    for (int Ns = 1; Ns < M; Ns <<= 1) {
        for (int j = threadIdx.x; j < half; j += blockDim.x) {
            const int k = j & (Ns - 1), j0 = 2 * j - k;
            const float2 u = a[j], wv = fs_cmul(tw[Ns + k], a[j + half]);
            b[j0] = make_float2(u.x + wv.x, u.y + wv.y);
            b[j0 + Ns] = make_float2(u.x - wv.x, u.y - wv.y);
        }
        __syncthreads();
        float2 *t = a;
        a = b;
        b = t;
    }
    return a;
}

// The N-point transform of a[0 .. N), complete in LDS before the call: directly (M == N), or by Bluestein on M-point transforms
// with the axis' chirp[N] and transformed filter filt[M].  Returns the buffer (a or b) whose first N entries hold the result.
__device__ __forceinline__ float2 *fs_dft(float2 *a, float2 *b, const float2 *tw, int N, int M, const float2 *__restrict__ chirp,
                                          const float2 *__restrict__ filt)
{
    if (M == N) return fs_fft(a, b, tw, M);
    for (int n = threadIdx.x; n < M; n += blockDim.x) a[n] = n < N ? fs_cmul(a[n], chirp[n]) : make_float2(0.f, 0.f);
    __syncthreads();
    float2 *f = fs_fft(a, b, tw, M), *o = f == a ? b : a;
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        const float2 v = fs_cmul(f[k], filt[k]);
        f[k] = make_float2(v.x, -v.y);
    }
    __syncthreads();
    float2 *r = fs_fft(f, o, tw, M);
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const float2 v = r[k];
        r[k] = fs_cmul(make_float2(v.x, -v.y), chirp[k]);
    }
    __syncthreads();
    return r;
}

// one axis of a call: its length, its transforms' length, and where its chirp and filter lie in the head of the workspace
struct FsAxis {
    int N, M;
    long long chirp, filt;                                         // in float2 from the workspace's start
};
// blockIdx.x: the axis (0: W, 1: H).  Nothing to do for a power of two.
__global__ __launch_bounds__(FS_THREADS) void field_spectrum_setup_kernel(FsAxis ax0, FsAxis ax1, float2 *__restrict__ head)
{
    extern __shared__ __attribute__((aligned(16))) float2 fs_lds[];
    const FsAxis ax = blockIdx.x == 0 ? ax0 : ax1;
    const int N = ax.N, M = ax.M;
    if (M == N) return;
    float2 *a = fs_lds, *b = a + M, *tw = b + M;
    float2 *chirp = head + ax.chirp, *filt = head + ax.filt;
    spec_twiddles(tw, M);
    for (int n = threadIdx.x; n < M; n += blockDim.x) a[n] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const int r = (n * n) % (2 * N);
        double s, c;
        sincospi(-(double)r / (double)N, &s, &c);
        const float2 cn = make_float2((float)c, (float)s);
        chirp[n] = cn;
        a[n] = make_float2(cn.x, -cn.y);
        if (n) a[M - n] = make_float2(cn.x, -cn.y);
    }
    __syncthreads();
    const float2 *r = fs_fft(a, b, tw, M);
    const float inv = 1.f / (float)M;
    for (int k = threadIdx.x; k < M; k += blockDim.x) filt[k] = make_float2(r[k].x * inv, r[k].y * inv);
}

// blockIdx.x: the field or pair p; blockIdx.y: operand i and row pair q.  half: [p][i][h][W/2 + 1]
template <int NF>
__global__ __launch_bounds__(FS_THREADS) void field_spectrum_rows_kernel(FieldSrc<NF> src, int H, FsAxis ax, const float2 *__restrict__ head,
                                                                         float2 *__restrict__ half)
{
    extern __shared__ __attribute__((aligned(16))) float2 fs_lds[];
    const int W = ax.N, M = ax.M, WH = W / 2 + 1, RP = (H + 1) / 2;
    const int p = blockIdx.x, i = NF == 1 ? 0 : blockIdx.y / RP, q = blockIdx.y - i * RP;
    float2 *a = fs_lds, *b = a + M, *tw = b + M;
    const Field &f = src.f[i];
    int c;
    const float *xf = field_first(src, i, p, c);
    const bool two = 2 * q + 1 < H;
    spec_twiddles(tw, M);
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        const long long p0 = (long long)(2 * q) * W + w, p1 = p0 + W;
        float v0, v1 = 0.f;
        if (f.mode == FIELD_C4) {
            const float4 *x4 = reinterpret_cast<const float4 *>(xf);
            v0 = field_pick(x4[p0], c);
            if (two) v1 = field_pick(x4[p1], c);
        } else {
            v0 = xf[p0 * f.pix];
            if (two) v1 = xf[p1 * f.pix];
        }
        a[w] = make_float2(v0, v1);
    }
    __syncthreads();
    const float2 *z = fs_dft(a, b, tw, W, M, head + ax.chirp, head + ax.filt);
    // A[k] = (Z[k] + conj Z[W - k]) / 2, B[k] = (Z[k] - conj Z[W - k]) / 2i
    float2 *h0 = half + (((long long)p * NF + i) * H + 2 * q) * WH, *h1 = h0 + WH;
    for (int k = threadIdx.x; k < WH; k += blockDim.x) {
        const float2 u = z[k], v = z[k ? W - k : 0];
        h0[k] = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));
        if (two) h1[k] = make_float2(0.5f * (u.y + v.y), 0.5f * (v.x - u.x));
    }
}

// blockIdx.x: the field or pair p; blockIdx.y: the column kx.  planes: [p][K][kx][ky]
template <int NF>
__global__ __launch_bounds__(FS_THREADS) void field_spectrum_cols_kernel(const float2 *__restrict__ half, int W, FsAxis ax,
                                                                         const float2 *__restrict__ head, float *__restrict__ planes)
{
    extern __shared__ __attribute__((aligned(16))) float2 fs_lds[];
    constexpr int K = NF == 1 ? 1 : 3;
    const int H = ax.N, M = ax.M, WH = W / 2 + 1;
    const int p = blockIdx.x, kx = blockIdx.y;
    float2 *a = fs_lds, *b = a + M, *tw = b + M, *res = tw + M;    // res[NF][H]
    spec_twiddles(tw, M);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const float2 *hf = half + ((long long)p * NF + i) * H * WH + kx;
        for (int h = threadIdx.x; h < H; h += blockDim.x) a[h] = hf[(long long)h * WH];
        __syncthreads();
        const float2 *r = fs_dft(a, b, tw, H, M, head + ax.chirp, head + ax.filt);
        for (int ky = threadIdx.x; ky < H; ky += blockDim.x) res[i * H + ky] = r[ky];
        __syncthreads();
    }
    const float scale = (kx == 0 || 2 * kx == W ? 1.f : 2.f) / ((float)H * (float)W);
    float *pl = planes + ((long long)p * K * WH + kx) * H;
    for (int ky = threadIdx.x; ky < H; ky += blockDim.x) {
        const float2 u = res[ky], v = res[(NF - 1) * H + ky];
        pl[ky] = fs_dot2(u.x, u.x, u.y, u.y) * scale;
        if constexpr (NF == 2) {
            pl[(long long)WH * H + ky] = fs_dot2(v.x, v.x, v.y, v.y) * scale;
            pl[2ll * WH * H + ky] = fs_dot2(u.x, v.x, u.y, v.y) * scale;
        }
    }
}

// Ring b, rows of one sign of fy (neg: fy < 0; fy = 0 goes with the positive side): cell(ky, kx) for every stored cell
// 0 <= kx <= W/2 of the ring, row by row, left to right; cnt counts the cells of the whole plane they stand for.  With
// T = L^2 W^2 fy^2 a row holds the fx with b (b - 1) H^2 W^2 - T < fx^2 H^2 L^2 <= b (b + 1) H^2 W^2 - T; every term stays
// below 2^60.
template <class Cell>
__host__ __device__ inline void fs_ring_cells(int b, bool neg, int H, int W, int &cnt, Cell cell)
{
    if (b == 0) {
        if (!neg) {
            cell(0, 0);
            cnt += 1;
        }
        return;
    }
    const long long L = H < W ? H : W, HW2 = (long long)H * H * W * W, D = (long long)H * H * L * L, E = L * L * W * W;
    const long long up0 = (long long)b * (b + 1) * HW2, lo0 = (long long)b * (b - 1) * HW2 + 1;
    const int ymax = neg ? H / 2 : (H - 1) / 2, xcap = W / 2;
    for (int y = neg ? 1 : 0; y <= ymax; ++y) {
        const long long T = E * y * y;
        if (T > up0) break;
        const long long qu = (up0 - T) / D, lo = lo0 - T;
        const int xh = qu >= (long long)xcap * xcap ? xcap : spec_isqrt((int)qu);
        int xl = 0;
        if (lo > 0) {
            const long long ql = (lo + D - 1) / D;                 // fx^2 >= ql
            if (ql > (long long)xcap * xcap) continue;
            xl = spec_isqrt((int)ql - 1) + 1;
        }
        const int ky = neg ? H - y : y;
        for (int x = xl; x <= xh; ++x) {
            cell(ky, x);
            cnt += x == 0 || 2 * x == W ? 1 : 2;
        }
    }
}

// blockIdx.x: the field or pair p.  out[p][K][nb] = (the sum of the positive side + the sum of the negative side) / cells
template <int K>
__global__ __launch_bounds__(FS_THREADS) void field_spectrum_rings_kernel(const float *__restrict__ planes, int H, int W,
                                                                          float *__restrict__ out)
{
    __shared__ double fin[2 * FS_MAX_BINS][K];
    __shared__ int fcnt[2 * FS_MAX_BINS];
    const int WH = W / 2 + 1, nb = (H < W ? H : W) / 2 + 1;
    const float *pl = planes + (long long)blockIdx.x * K * WH * H;
    const long long plane = (long long)WH * H;
    for (int it = threadIdx.x; it < 2 * nb; it += blockDim.x) {
        double acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
        int cnt = 0;
        fs_ring_cells(it >> 1, it & 1, H, W, cnt, [&](int ky, int kx) {
            const float *cell = pl + (long long)kx * H + ky;
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += (double)cell[k * plane];
        });
#pragma unroll
        for (int k = 0; k < K; ++k) fin[it][k] = acc[k];
        fcnt[it] = cnt;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K * nb; t += blockDim.x) {
        const int k = t / nb, b = t - k * nb;
        out[(long long)blockIdx.x * K * nb + t] = (float)((fin[2 * b][k] + fin[2 * b + 1][k]) / (double)(fcnt[2 * b] + fcnt[2 * b + 1]));
    }
}

// ---- host side ----
static bool fs_forwarded(int H, int W) { return H == W && fs_pow2(H); }
static size_t fs_head_bytes(int H, int W) { return acg_round_up((size_t)(W + fs_padded(W) + H + fs_padded(H)) * sizeof(float2), 16); }
static size_t fs_half_bytes(size_t n, int NF, int H, int W) { return acg_round_up(n * NF * H * (W / 2 + 1) * sizeof(float2), 16); }
static size_t fs_plane_bytes(size_t n, int NF, int H, int W) { return acg_round_up(n * (NF == 1 ? 1 : 3) * H * (W / 2 + 1) * sizeof(float), 16); }

// head (chirps and filters) | the half spectra between the row and the column pass | the product planes
static size_t fs_workspace_bytes(int rows, int C, int H, int W, int NF)
{
    if (rows < 1 || C < 1 || !fs_extent_ok(H) || !fs_extent_ok(W)) return 0;
    if (fs_forwarded(H, W)) return NF == 1 ? acg_radial_spectrum_workspace_bytes(rows, C, H) : acg_cross_spectrum_workspace_bytes(rows, C, H);
    const size_t n = (size_t)rows * (size_t)C;
    return fs_head_bytes(H, W) + fs_half_bytes(n, NF, H, W) + fs_plane_bytes(n, NF, H, W);
}
extern "C" size_t acg_field_spectrum_workspace_bytes(int rows, int C, int H, int W) { return fs_workspace_bytes(rows, C, H, W, 1); }
extern "C" size_t acg_field_cross_spectrum_workspace_bytes(int rows, int C, int H, int W) { return fs_workspace_bytes(rows, C, H, W, 2); }

template <int NF>
static void fs_launch(hipStream_t st, FieldSrc<NF> src, int n, int H, int W, float *out, void *ws)
{
    FsAxis aw, ah;
    aw.N = W, aw.M = fs_padded(W), aw.chirp = 0, aw.filt = W;
    ah.N = H, ah.M = fs_padded(H), ah.chirp = W + aw.M, ah.filt = ah.chirp + H;
    float2 *head = (float2 *)ws;
    float2 *half = (float2 *)((char *)ws + fs_head_bytes(H, W));
    float *planes = (float *)((char *)half + fs_half_bytes(n, NF, H, W));
    const int Mmax = aw.M > ah.M ? aw.M : ah.M, WH = W / 2 + 1, RP = (H + 1) / 2;
    for (Field &f : src.f) f.mode = field_load_mode(f, src.C);
    if (aw.M != W || ah.M != H)
        hipLaunchKernelGGL(field_spectrum_setup_kernel, dim3(2), dim3(FS_THREADS), 3 * Mmax * sizeof(float2), st, aw, ah, head);
    hipLaunchKernelGGL(field_spectrum_rows_kernel<NF>, dim3(n, NF * RP), dim3(FS_THREADS), 3 * aw.M * sizeof(float2), st, src, H, aw,
                       (const float2 *)head, half);
    hipLaunchKernelGGL(field_spectrum_cols_kernel<NF>, dim3(n, WH), dim3(FS_THREADS), (3 * ah.M + NF * H) * sizeof(float2), st,
                       (const float2 *)half, W, ah, (const float2 *)head, planes);
    hipLaunchKernelGGL(field_spectrum_rings_kernel<(NF == 1 ? 1 : 3)>, dim3(n), dim3(FS_THREADS), 0, st, (const float *)planes, H, W, out);
    acg_note_kernel("%s_rows<W=%d,M=%d> + %s_cols<H=%d,M=%d> + rings", NF == 1 ? "field_spectrum" : "field_cross_spectrum", W, aw.M,
                    NF == 1 ? "field_spectrum" : "field_cross_spectrum", H, ah.M);
}

// what both entry points refuse first, under their own name fn: an extent they cannot serve, no rows or no channels
static int fs_shape_refused(const char *fn, int H, int W, int rows, int C)
{
    ACG_REQUIRE(fs_extent_ok(H) && fs_extent_ok(W), "%s: fields must be H x W with both extents in %d..%d (got %d x %d)", fn, FS_MIN,
                FS_MAX, H, W);
    return field_refuse_operands(fn, rows, C, nullptr, 0);
}

extern "C" int acg_field_spectrum(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride,
                                  long long chan_stride, float *psd, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_field_spectrum";
    ACG_REQUIRE(x != nullptr && psd != nullptr, "%s: null tensor", fn);
    const FieldSrc<1> src = {{{x, row_stride, chan_stride, pix_stride, FIELD_SCALAR}}, C, 1};
    FIELD_CHECK(fs_shape_refused(fn, H, W, rows, C));
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d)", fn, rows, C);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, src.f, 1));
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, fs_workspace_bytes(rows, C, H, W, 1)));
    if (fs_forwarded(H, W))                                        // nothing is left for it to refuse
        return acg_radial_spectrum(x, rows, C, H, row_stride, pix_stride, chan_stride, psd, ws, ws_bytes, stream);
    fs_launch<1>((hipStream_t)stream, src, rows * C, H, W, psd, ws);
    ACG_CHECK_LAUNCH("acg_field_spectrum");
    return ACG_OK;
}

extern "C" int acg_field_cross_spectrum(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W,
                                        long long x_row_stride, int x_pix_stride, long long x_chan_stride, long long y_row_stride,
                                        int y_pix_stride, long long y_chan_stride, float *out, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_field_cross_spectrum";
    ACG_REQUIRE(x != nullptr && y != nullptr && out != nullptr, "%s: null tensor", fn);
    const FieldSrc<2> src = {{{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}},
                             C, x_per_y};
    FIELD_CHECK(fs_shape_refused(fn, H, W, rows, C));
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d)", fn, rows, C);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, src.f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, rows));
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, fs_workspace_bytes(rows, C, H, W, 2)));
    if (fs_forwarded(H, W))
        return acg_cross_spectrum(x, y, rows, x_per_y, C, H, x_row_stride, x_pix_stride, x_chan_stride, y_row_stride, y_pix_stride,
                                  y_chan_stride, out, ws, ws_bytes, stream);
    fs_launch<2>((hipStream_t)stream, src, rows * C, H, W, out, ws);
    ACG_CHECK_LAUNCH("acg_field_cross_spectrum");
    return ACG_OK;
}
