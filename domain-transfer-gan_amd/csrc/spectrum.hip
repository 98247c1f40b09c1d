// Radially averaged power spectra of square fields (model.translate_spectrum, test.py --metric spectrum) and the paired
// cross-spectra of two (ops.cross_spectrum, model.translate_coherence, test.py --metric coherence).  Per field of one channel of
// one image, S x S real pixels: P = |fft2(x)|^2 / S^2 averaged over rings of integer wavenumber 0 .. S/2.  Per pair of fields
// x, y and ring: the means of Pxx = |X|^2 / S^2, Pyy = |Y|^2 / S^2 and the co-spectrum Cxy = Re(X conj Y) / S^2; the quadrature part
// Im(X conj Y) sums to 0 over every ring of two real fields (the twin cell holds the conjugate product) and is no output.
// There is no reference call site: the reference has no spectral code; tests/spectrum_ref.py and tests/cross_spectrum_ref.py
// state the definitions.
//
// One set of kernels, templated on the fields a workgroup carries: NF = 1 (a field, one sum per ring) or NF = 2 (a pair, three).
// A batched real 2-D FFT in fp32 with the products and the ring sums fused behind it, no vendor FFT:
//   rows     two real rows per complex transform (z = row 2r + i row 2r+1), radix-2 Stockham autosort in LDS (every stage reads
//            unit-stride and writes runs of the stage's width: no bit-reversal gather, no stride-2^k access), then the two rows'
//            half spectra are untangled.  Columns kx = 0 and kx = S/2 of a real row are real, so they travel packed in one
//            complex column (re: kx = 0, im: kx = S/2): the half spectrum is exactly S x S/2 complex, the field's own bytes.
//            The half spectra of a workgroup's NF fields lie side by side in one [ky][NF S/2] tile, X's columns in front and
//            Y's behind.  A pair shares every pass, but never a complex transform: tangled as z = x + i y, the rounding of the
//            stronger field would leak into the weaker one's spectrum at the stronger one's scale (a generator against a truth
//            1000 times fainter).
//   columns  the same Stockham stages down the columns of that tile with the lanes along kx, so every LDS access is
//            unit-stride across the wave and the twiddle is a broadcast.
//   products w |F|^2 / S^2 per cell (a pair: w |X|^2, w |Y|^2, w Re(X conj Y), each / S^2, into three planes), w = 2 for
//            0 < kx < S/2 (the Hermitian twin lies in the same ring), 1 for kx = 0 and S/2, whose packed column is untangled
//            here, for both fields of a pair before their product is taken.  Of the column kx = S/2 only the rows
//            |fy| < spec_nyq(S) / 2 are kept: a ring reaches no further (fy^2 <= S/2).
//   rings    ring b holds the cells with b (b - 1) < fx^2 + fy^2 <= b (b + 1) (integers: sqrt(s) rounded to nearest).  One
//            work item per (ring, sign of fy) enumerates its cells row by row from the integer rule and sums every plane in
//            double in that fixed order, and counts the cells; out[k][b] = (sum+ + sum-) / count.  No float atomics: two runs
//            give the same bits, and the arithmetic does not depend on the input's layout.
// While the NF half spectra fit one workgroup's LDS twice (S <= 128 for a field, S <= 64 for a pair), one workgroup per field or
// pair does all of it in LDS and writes nothing but its ring means.  Above, a row pass writes the tile to the workspace (S x NF S/2
// complex per field or pair) and a column pass (one workgroup per field or pair, SPEC_TILE / S columns at a time, an equal
// share of them from every field) reads it back and bins.
// Twiddles: sincospif on exact arguments, one table per stage laid out by butterfly index (unit-stride reads).
#include <math.h>
#include <stdint.h>
#include <type_traits>
#include "common.h"
#include "field.h"
#include "spectrum_shared.h"

#define SPEC_TILE 4096                   // complex elements of one LDS buffer of the two-pass kernels (32 KiB)
#define SPEC_MIN_S 16
#define SPEC_MAX_S 1024

// one workgroup does a field or pair in LDS while two buffers of NF half spectra (8 NF S^2 bytes) fit beside the twiddles:
// S <= 128 for a field, S <= 64 for a pair
__host__ __device__ constexpr bool spec_one_wg(int S, int NF) { return 8 * NF * S * S <= 128 * 1024; }
// threads of a workgroup: the one-workgroup kernel has four butterflies of a stage (NF S^2 / 4 of them) per thread, which is the
// widest workgroup at S = 128 (129 KiB of LDS: alone on the CU) and half of it for a pair at S = 64 (65 KiB: two share a CU), but
// no fewer than four waves, and one at S = 16.  The two passes share a CU two workgroups at a time (66-72 KiB of LDS each): 16
// waves of the row pass, all 32 of the column pass, whose one workgroup per field or pair is a serial chain of tiles and wants
// the widest workgroup
__host__ __device__ constexpr int spec_field_threads(int S, int NF) { return S <= 16 ? 64 : NF * S * S / 16 < 256 ? 256 : NF * S * S / 16; }
static_assert(spec_field_threads(16, 1) == 64 && spec_field_threads(32, 1) == 256 && spec_field_threads(64, 1) == 256 &&
              spec_field_threads(128, 1) == 1024 && spec_field_threads(16, 2) == 64 && spec_field_threads(32, 2) == 256 &&
              spec_field_threads(64, 2) == 512 && spec_one_wg(128, 1) && !spec_one_wg(256, 1) && spec_one_wg(64, 2) &&
              !spec_one_wg(128, 2), "the launch geometry of every size");
#define SPEC_ROWS_THREADS 512
#define SPEC_COLS_THREADS 1024
__host__ __device__ constexpr int spec_planes(int NF) { return NF == 1 ? 1 : 3; }   // |X|^2; with a second field |Y|^2 and Re(X conj Y)
// slots of the kept rows of the column kx = S/2: row fy in slot fy & (slots - 1); fy^2 <= S/2 <= 512 lies well inside
__host__ __device__ constexpr int spec_nyq(int S) { return S < 64 ? S : 64; }

__device__ __forceinline__ void spec_butterfly(float2 u, float2 v, float2 w, float2 &p, float2 &m)
{
    const float2 wv = make_float2(w.x * v.x - w.y * v.y, w.x * v.y + w.y * v.x);
    p = make_float2(u.x + wv.x, u.y + wv.y);
    m = make_float2(u.x - wv.x, u.y - wv.y);
}

// NSEQ transforms of length S along the contiguous index, layout [seq][S]; returns the buffer that holds the result
template <int S, int NSEQ>
__device__ __forceinline__ float2 *spec_fft_rows(float2 *a, float2 *b, const float2 *tw)
{
    for (int Ns = 1; Ns < S; Ns <<= 1) {
        for (int t = threadIdx.x; t < NSEQ * (S / 2); t += blockDim.x) {
            const int q = t / (S / 2), j = t & (S / 2 - 1), k = j & (Ns - 1), j0 = 2 * j - k;
            const float2 *in = a + q * S;
            float2 *out = b + q * S;
            float2 p, m;
            spec_butterfly(in[j], in[j + S / 2], tw[Ns + k], p, m);
            if (Ns == 1) {
                *reinterpret_cast<float4 *>(out + j0) = make_float4(p.x, p.y, m.x, m.y);   // neighbours: one 16-byte store
            } else {
                out[j0] = p;
                out[j0 + Ns] = m;
            }
        }
        __syncthreads();
        float2 *t2 = a;
        a = b;
        b = t2;
    }
    return a;
}

// KT transforms of length S down the rows of a [S][KT] tile, the lanes along the KT columns
template <int S, int KT>
__device__ __forceinline__ float2 *spec_fft_cols(float2 *a, float2 *b, const float2 *tw)
{
    for (int Ns = 1; Ns < S; Ns <<= 1) {
        for (int t = threadIdx.x; t < (S / 2) * KT; t += blockDim.x) {
            const int j = t / KT, c = t & (KT - 1), k = j & (Ns - 1), j0 = 2 * j - k;
            float2 p, m;
            spec_butterfly(a[j * KT + c], a[(j + S / 2) * KT + c], tw[Ns + k], p, m);
            b[j0 * KT + c] = p;
            b[(j0 + Ns) * KT + c] = m;
        }
        __syncthreads();
        float2 *t2 = a;
        a = b;
        b = t2;
    }
    return a;
}

// z[q][w] = x[2 (rp0 + q)][w] + i x[2 (rp0 + q) + 1][w] for NRP row pairs; four pixels of both rows per work item.
// xf: the field's first pixel (FIELD_C4: the image's, the channel picked from each pixel's 16 bytes).
template <int S, int NRP>
__device__ __forceinline__ void spec_load_rows(const float *__restrict__ xf, int pix_stride, int mode, int c, int rp0, float2 *z)
{
    for (int t = threadIdx.x; t < NRP * (S / 4); t += blockDim.x) {
        const int q = t / (S / 4), w = (t & (S / 4 - 1)) * 4;
        const long long p0 = (long long)(2 * (rp0 + q)) * S + w, p1 = p0 + S;
        float4 r0, r1;
        if (mode == FIELD_PLANAR) {
            r0 = *reinterpret_cast<const float4 *>(xf + p0);
            r1 = *reinterpret_cast<const float4 *>(xf + p1);
        } else if (mode == FIELD_C4) {
            const float4 *x4 = reinterpret_cast<const float4 *>(xf);
            r0 = make_float4(field_pick(x4[p0], c), field_pick(x4[p0 + 1], c), field_pick(x4[p0 + 2], c), field_pick(x4[p0 + 3], c));
            r1 = make_float4(field_pick(x4[p1], c), field_pick(x4[p1 + 1], c), field_pick(x4[p1 + 2], c), field_pick(x4[p1 + 3], c));
        } else {
            r0 = make_float4(xf[p0 * pix_stride], xf[(p0 + 1) * pix_stride], xf[(p0 + 2) * pix_stride], xf[(p0 + 3) * pix_stride]);
            r1 = make_float4(xf[p1 * pix_stride], xf[(p1 + 1) * pix_stride], xf[(p1 + 2) * pix_stride], xf[(p1 + 3) * pix_stride]);
        }
        float4 *dst = reinterpret_cast<float4 *>(z + q * S + w);
        dst[0] = make_float4(r0.x, r1.x, r0.y, r1.y);
        dst[1] = make_float4(r0.z, r1.z, r0.w, r1.w);
    }
}

// The spectra of the two real rows of z = a + i b at column k of the packed half spectrum (k < S/2):
// A = (Z[k] + conj Z[S-k]) / 2, B = (Z[k] - conj Z[S-k]) / 2i; k = 0 carries (A[0], A[S/2]) and (B[0], B[S/2]), all real.
template <int S>
__device__ __forceinline__ void spec_untangle(const float2 *z, int k, float2 &ha, float2 &hb)
{
    if (k == 0) {
        const float2 z0 = z[0], zn = z[S / 2];
        ha = make_float2(z0.x, zn.x);
        hb = make_float2(z0.y, zn.y);
    } else {
        const float2 u = z[k], v = z[S - k];
        ha = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));
        hb = make_float2(0.5f * (u.y + v.y), 0.5f * (v.x - u.x));
    }
}

// NRP transformed row pairs z[q][S] -> rows 2q, 2q + 1 of h (row stride ld complex; LDS or global), two columns per store
template <int S, int NRP>
__device__ __forceinline__ void spec_untangle_rows(const float2 *z, float2 *h, int ld = S / 2)
{
    for (int t = threadIdx.x; t < NRP * (S / 4); t += blockDim.x) {
        const int q = t / (S / 4), k = (t & (S / 4 - 1)) * 2;
        float2 a0, b0, a1, b1;
        spec_untangle<S>(z + q * S, k, a0, b0);
        spec_untangle<S>(z + q * S, k + 1, a1, b1);
        *reinterpret_cast<float4 *>(h + (long long)(2 * q) * ld + k) = make_float4(a0.x, a0.y, a1.x, a1.y);
        *reinterpret_cast<float4 *>(h + (long long)(2 * q + 1) * ld + k) = make_float4(b0.x, b0.y, b1.x, b1.y);
    }
}

// a b + c d of the packed column as one fused multiply-add behind the rounded c d: pinned, because the results keep their bits
// only while the compiler makes this choice, and beside the guarded store of the column kx = S/2 it does not make it by itself
__device__ __forceinline__ float spec_dot2(float a, float b, float c, float d) { return fmaf(a, b, c * d); }

// A transformed [S][NF KH] tile, columns kx0 .. kx0 + KH - 1 of X in front and of Y behind -> pl[K][S][KH]: the weighted |X|^2
// of every cell and, of a pair, |Y|^2 and Re(X conj Y) behind it; the tile of kx0 = 0 untangles the packed column of every
// field into kx = 0 (pl[.][ky][0]) and kx = S/2 (pn[K][spec_nyq(S)]: the kept rows), both of weight 1
template <int S, int KH, int NF>
__device__ __forceinline__ void spec_products(const float2 *f, int kx0, float *pl, float *pn)
{
    constexpr int KT = NF * KH, H = S / 2, NQ = spec_nyq(S);
    const float inv = 1.f / ((float)S * (float)S);
    for (int t = threadIdx.x; t < S * KH; t += blockDim.x) {
        const int ky = t / KH, c = t & (KH - 1);
        const float2 u = f[ky * KT + c], v = f[ky * KT + (NF - 1) * KH + c];   // v: the cell of Y (NF = 1: u again, unused)
        if (kx0 + c == 0) {
            const int kz = (S - ky) & (S - 1), fy = ky < H ? ky : ky - S;
            const float2 u2 = f[kz * KT], v2 = f[kz * KT + (NF - 1) * KH];
            const float xdr = u.x + u2.x, xdi = u.y - u2.y, xnr = u.x - u2.x, xni = u.y + u2.y;
            const float ydr = v.x + v2.x, ydi = v.y - v2.y, ynr = v.x - v2.x, yni = v.y + v2.y;
            pl[t] = spec_dot2(xdr, xdr, xdi, xdi) * (0.25f * inv);
            if constexpr (NF == 2) {
                pl[S * KH + t] = spec_dot2(ydr, ydr, ydi, ydi) * (0.25f * inv);
                pl[2 * S * KH + t] = spec_dot2(xdr, ydr, xdi, ydi) * (0.25f * inv);
            }
            if (fy > -NQ / 2 && fy < NQ / 2) {
                const int slot = fy & (NQ - 1);
                pn[slot] = spec_dot2(xnr, xnr, xni, xni) * (0.25f * inv);
                if constexpr (NF == 2) {
                    pn[NQ + slot] = spec_dot2(ynr, ynr, yni, yni) * (0.25f * inv);
                    pn[2 * NQ + slot] = spec_dot2(xnr, ynr, xni, yni) * (0.25f * inv);
                }
            }
        } else {
            pl[t] = (u.x * u.x + u.y * u.y) * (2.f * inv);
            if constexpr (NF == 2) {
                pl[S * KH + t] = (v.x * v.x + v.y * v.y) * (2.f * inv);
                pl[2 * S * KH + t] = (u.x * v.x + u.y * v.y) * (2.f * inv);
            }
        }
    }
}

__device__ __forceinline__ int spec_isqrt_ceil(int n) { return n <= 0 ? 0 : spec_isqrt(n - 1) + 1; }

// Ring b, rows of one sign of fy (neg: fy < 0; fy = 0 goes with the positive side), inside the tile's columns: the row range and
// each row's column range follow from b (b - 1) < fx^2 + fy^2 <= b (b + 1); the cells are visited row by row, left to right:
// cell(ky * KT + kx - kx0) for 0 <= kx < S/2, nyq(ky) for the column fx = -S/2
template <int S, int KT, class Cell, class Nyq>
__device__ __forceinline__ void spec_ring_cells(int b, bool neg, int kx0, int &cnt, Cell cell, Nyq nyq)
{
    constexpr int H = S / 2;
    const int kx1 = kx0 + KT - 1;
    if (b == 0) {
        if (!neg && kx0 == 0) {
            cell(0);
            cnt += 1;
        }
        return;
    }
    const int up = b * (b + 1), lo = b * (b - 1) + 1;
    if (up >= kx0 * kx0) {
        const int ymax = min(spec_isqrt(up - kx0 * kx0), neg ? H : H - 1);
        const int ymin = max(spec_isqrt_ceil(lo - kx1 * kx1), neg ? 1 : 0);
        for (int y = ymin; y <= ymax; ++y) {
            const int ky = neg ? S - y : y;
            const int xh = min(spec_isqrt(up - y * y), kx1), xl = max(spec_isqrt_ceil(lo - y * y), kx0);
            for (int x = xl; x <= xh; ++x) {
                cell(ky * KT + (x - kx0));
                cnt += x == 0 ? 1 : 2;
            }
        }
    }
    if (b == H && kx0 == 0) {                                     // the column fx = -S/2: H^2 + fy^2 <= H (H + 1)
        const int ylast = spec_isqrt(H);
        for (int y = neg ? 1 : 0; y <= ylast; ++y) {
            nyq(neg ? S - y : y);
            cnt += 1;
        }
    }
}

// The ring sums of a workgroup of T threads over K planes: one (ring, sign of fy) item per thread and turn
template <int S, int T, int K>
struct RingBins {
    static constexpr int NB = S / 2 + 1;
    static constexpr int NI = (2 * NB + T - 1) / T;    // (ring, sign) items per thread
    static constexpr size_t LDS_BYTES = 2 * NB * (K * sizeof(double) + sizeof(int));
    double acc[NI][K];
    int cnt[NI];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int k = 0; k < K; ++k) acc[i][k] = 0.0;
            cnt[i] = 0;
        }
    }
    // the cells of the tile of columns kx0 .. kx0 + KH - 1: pl[K][S][KH] and, of the column kx = S/2, pn[K][spec_nyq(S)]
    template <int KH>
    __device__ __forceinline__ void add_tile(int kx0, const float *pl, const float *pn)
    {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int it = threadIdx.x + i * T;
            if (it >= 2 * NB) continue;
            double(&a)[K] = acc[i];
            spec_ring_cells<S, KH>(
                it >> 1, it & 1, kx0, cnt[i],
                [&](int c) {
#pragma unroll
                    for (int k = 0; k < K; ++k) a[k] += (double)pl[k * S * KH + c];
                },
                [&](int ky) {
                    const int slot = (ky < S / 2 ? ky : ky - S) & (spec_nyq(S) - 1);
#pragma unroll
                    for (int k = 0; k < K; ++k) a[k] += (double)pn[k * spec_nyq(S) + slot];
                });
        }
    }
    // out[k][b] = (sum of the positive side + sum of the negative side) / cells; lds: LDS_BYTES, free to overwrite
    __device__ __forceinline__ void store(void *lds, float *__restrict__ out)
    {
        double *fin = reinterpret_cast<double *>(lds);
        int *fcnt = reinterpret_cast<int *>(fin + 2 * K * NB);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int it = threadIdx.x + i * T;
            if (it < 2 * NB) {
#pragma unroll
                for (int k = 0; k < K; ++k) fin[K * it + k] = acc[i][k];
                fcnt[it] = cnt[i];
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < K * NB; t += blockDim.x) {
            const int k = t / NB, b = t - k * NB;
            out[t] = (float)((fin[2 * K * b + k] + fin[2 * K * b + K + k]) / (double)(fcnt[2 * b] + fcnt[2 * b + 1]));
        }
    }
};

// 16-byte copies between the half spectra of a field or pair in the workspace, hf[ky][NF S/2], and a [ky][KT] LDS tile that
// holds columns kx0 .. kx0 + KT / NF - 1 of every field, X's in front and Y's behind
template <int S, int KT, int NF>
__device__ __forceinline__ long long spec_tile_cell(int ky, int cc, int kx0)
{
    constexpr int KH = KT / NF;
    static_assert(KH >= 2, "a 16-byte copy stays inside one field's columns");
    return (long long)ky * (NF * (S / 2)) + (NF == 1 || cc < KH ? kx0 + cc : S / 2 + kx0 + cc - KH);
}
template <int S, int KT, int NF>
__device__ __forceinline__ void spec_load_tile(const float2 *hf, int kx0, float2 *tile)
{
    for (int t = threadIdx.x; t < S * (KT / 2); t += blockDim.x) {
        const int ky = t / (KT / 2), cc = (t & (KT / 2 - 1)) * 2;
        *reinterpret_cast<float4 *>(tile + ky * KT + cc) = *reinterpret_cast<const float4 *>(hf + spec_tile_cell<S, KT, NF>(ky, cc, kx0));
    }
}
template <int S, int KT, int NF>
__device__ __forceinline__ void spec_store_tile(const float2 *tile, int kx0, float2 *hf)
{
    for (int t = threadIdx.x; t < S * (KT / 2); t += blockDim.x) {
        const int ky = t / (KT / 2), cc = (t & (KT / 2 - 1)) * 2;
        *reinterpret_cast<float4 *>(hf + spec_tile_cell<S, KT, NF>(ky, cc, kx0)) = *reinterpret_cast<const float4 *>(tile + ky * KT + cc);
    }
}

// spec_one_wg(S, NF): one workgroup per field or pair; nothing but out is written
template <int S, int NF>
__global__ __launch_bounds__(spec_field_threads(S, NF)) void spectrum_field_kernel(FieldSrc<NF> src, float *__restrict__ out)
{
    constexpr int H = S / 2, K = spec_planes(NF);
    using Bins = RingBins<S, spec_field_threads(S, NF), K>;
    __shared__ __attribute__((aligned(16))) float2 buf0[NF * H * S];
    __shared__ __attribute__((aligned(16))) float2 buf1[NF * H * S];
    __shared__ float2 tw[S];
    static_assert(K * (S * H + spec_nyq(S)) * sizeof(float) <= sizeof(buf0) && Bins::LDS_BYTES <= sizeof(buf0), "LDS");
    spec_twiddles(tw, S);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        int c;
        const float *xf = field_first(src, i, blockIdx.x, c);
        spec_load_rows<S, H>(xf, src.f[i].pix, src.f[i].mode, c, 0, buf0 + i * H * S);
    }
    __syncthreads();
    float2 *z = spec_fft_rows<S, NF * H>(buf0, buf1, tw);          // x's S/2 row pairs, then y's
    float2 *h = z == buf0 ? buf1 : buf0;
#pragma unroll
    for (int i = 0; i < NF; ++i) spec_untangle_rows<S, H>(z + i * H * S, h + i * H, NF * H);   // [ky][NF S/2]: the whole column tile
    __syncthreads();
    float2 *f = spec_fft_cols<S, NF * H>(h, z, tw);
    float *pl = reinterpret_cast<float *>(f == buf0 ? buf1 : buf0), *pn = pl + K * S * H;
    spec_products<S, H, NF>(f, 0, pl, pn);
    __syncthreads();
    Bins bins;
    bins.clear();
    bins.template add_tile<H>(0, pl, pn);
    bins.store(f, out + (long long)blockIdx.x * K * Bins::NB);
}

// above, first pass: SPEC_TILE / S row pairs of one field per workgroup (blockIdx.y: x's tiles, then y's) -> their rows of that
// field's side of the [ky][NF S/2] tile in the workspace
template <int S, int NF>
__global__ __launch_bounds__(SPEC_ROWS_THREADS) void spectrum_rows_kernel(FieldSrc<NF> src, float2 *__restrict__ half)
{
    constexpr int NRP = SPEC_TILE / S, TILES = (S / 2) / NRP, H = S / 2;
    __shared__ __attribute__((aligned(16))) float2 buf0[SPEC_TILE];
    __shared__ __attribute__((aligned(16))) float2 buf1[SPEC_TILE];
    __shared__ float2 tw[S];
    const int i = NF == 1 ? 0 : blockIdx.y / TILES, rp0 = (blockIdx.y - i * TILES) * NRP;
    int c;
    const float *xf = field_first(src, i, blockIdx.x, c);
    spec_twiddles(tw, S);
    spec_load_rows<S, NRP>(xf, src.f[i].pix, src.f[i].mode, c, rp0, buf0);
    __syncthreads();
    const float2 *z = spec_fft_rows<S, NRP>(buf0, buf1, tw);
    spec_untangle_rows<S, NRP>(z, half + ((long long)blockIdx.x * S + 2 * rp0) * (NF * H) + i * H, NF * H);
}

// above, second pass: one workgroup per field or pair walks its half spectra in tiles of SPEC_TILE / (NF S) columns of each
template <int S, int NF>
__global__ __launch_bounds__(SPEC_COLS_THREADS) void spectrum_cols_kernel(const float2 *__restrict__ half, float *__restrict__ out)
{
    constexpr int KT = SPEC_TILE / S, KH = KT / NF, H = S / 2, K = spec_planes(NF);
    using Bins = RingBins<S, SPEC_COLS_THREADS, K>;
    __shared__ __attribute__((aligned(16))) float2 buf0[SPEC_TILE];
    __shared__ __attribute__((aligned(16))) float2 buf1[SPEC_TILE];
    __shared__ float2 tw[S];
    static_assert(K * (S * KH + spec_nyq(S)) * sizeof(float) <= sizeof(buf0) && Bins::LDS_BYTES <= sizeof(buf0), "LDS");
    const float2 *hf = half + (long long)blockIdx.x * S * (NF * H);
    spec_twiddles(tw, S);
    Bins bins;
    bins.clear();
    float2 *f = buf0;
    for (int kx0 = 0; kx0 < H; kx0 += KH) {
        spec_load_tile<S, KT, NF>(hf, kx0, buf0);
        __syncthreads();
        f = spec_fft_cols<S, KT>(buf0, buf1, tw);
        float *pl = reinterpret_cast<float *>(f == buf0 ? buf1 : buf0), *pn = pl + K * S * KH;
        spec_products<S, KH, NF>(f, kx0, pl, pn);
        __syncthreads();
        bins.template add_tile<KH>(kx0, pl, pn);
        __syncthreads();                                           // pl may be buf0, which the next tile's load overwrites
    }
    bins.store(f, out + (long long)blockIdx.x * K * Bins::NB);
}

static bool spec_size_ok(int S) { return S >= SPEC_MIN_S && S <= SPEC_MAX_S && (S & (S - 1)) == 0; }

// what every entry point here refuses first, under its own name fn: a size it cannot serve, no rows or no channels
static int spec_shape_refused(const char *fn, int S, int rows, int C)
{
    ACG_REQUIRE(spec_size_ok(S), "%s: fields must be S x S with S a power of two in %d..%d (S=%d)", fn, SPEC_MIN_S, SPEC_MAX_S, S);
    return field_refuse_operands(fn, rows, C, nullptr, 0);
}

// f(std::integral_constant<int, S>) for the size S of a call that spec_shape_refused has let pass
template <class F>
static void spec_for_size(int S, F f)
{
    switch (S) {
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    case 64: f(std::integral_constant<int, 64>()); break;
    case 128: f(std::integral_constant<int, 128>()); break;
    case 256: f(std::integral_constant<int, 256>()); break;
    case 512: f(std::integral_constant<int, 512>()); break;
    default: f(std::integral_constant<int, 1024>()); break;
    }
}

// the workspace of n fields or pairs: their [ky][NF S/2] tiles between the two passes
static size_t spec_half_bytes(int rows, int C, int S, int NF)
{
    if (rows < 1 || C < 1 || !spec_size_ok(S) || spec_one_wg(S, NF)) return 0;
    return (size_t)rows * (size_t)C * (size_t)S * (size_t)(NF * (S / 2)) * sizeof(float2);
}
extern "C" size_t acg_radial_spectrum_workspace_bytes(int rows, int C, int S) { return spec_half_bytes(rows, C, S, 1); }
extern "C" size_t acg_cross_spectrum_workspace_bytes(int rows, int C, int S) { return spec_half_bytes(rows, C, S, 2); }

template <int S, int NF>
static void spec_launch(hipStream_t st, const FieldSrc<NF> &src, int n, float *out, float2 *half)
{
    if constexpr (spec_one_wg(S, NF)) {
        hipLaunchKernelGGL((spectrum_field_kernel<S, NF>), dim3(n), dim3(spec_field_threads(S, NF)), 0, st, src, out);
        acg_note_kernel(NF == 1 ? "spectrum_field<%d>" : "cross_spectrum_field<%d>", S);
    } else {
        constexpr int TILES = (S / 2) / (SPEC_TILE / S);           // of every field: x's, then y's
        hipLaunchKernelGGL((spectrum_rows_kernel<S, NF>), dim3(n, NF * TILES), dim3(SPEC_ROWS_THREADS), 0, st, src, half);
        hipLaunchKernelGGL((spectrum_cols_kernel<S, NF>), dim3(n), dim3(SPEC_COLS_THREADS), 0, st, (const float2 *)half, out);
        acg_note_kernel(NF == 1 ? "spectrum_rows<%d> + spectrum_cols<%d>" : "cross_spectrum_rows<%d> + cross_spectrum_cols<%d>", S, S);
    }
}

extern "C" int acg_radial_spectrum(const float *x, int rows, int C, int S, long long row_stride, int pix_stride,
                                   long long chan_stride, float *psd, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_radial_spectrum";
    ACG_REQUIRE(x != nullptr && psd != nullptr, "%s: null tensor", fn);
    FieldSrc<1> src = {{{x, row_stride, chan_stride, pix_stride, FIELD_SCALAR}}, C, 1};
    FIELD_CHECK(spec_shape_refused(fn, S, rows, C));
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d)", fn, rows, C);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, src.f, 1));
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_radial_spectrum_workspace_bytes(rows, C, S)));
    src.f[0].mode = field_load_mode(src.f[0], C, true);
    spec_for_size(S, [&](auto s) { spec_launch<decltype(s)::value, 1>((hipStream_t)stream, src, rows * C, psd, (float2 *)ws); });
    ACG_CHECK_LAUNCH("acg_radial_spectrum");
    return ACG_OK;
}

extern "C" int acg_cross_spectrum(const float *x, const float *y, int rows, int x_per_y, int C, int S, long long x_row_stride,
                                  int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                                  long long y_chan_stride, float *out, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_cross_spectrum";
    ACG_REQUIRE(x != nullptr && y != nullptr && out != nullptr, "%s: null tensor", fn);
    FieldSrc<2> src = {{{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}},
                       C, x_per_y};
    FIELD_CHECK(spec_shape_refused(fn, S, rows, C));
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL, "%s: too many pairs (rows=%d, C=%d)", fn, rows, C);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, src.f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, rows));
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_cross_spectrum_workspace_bytes(rows, C, S)));
    for (Field &f : src.f) f.mode = field_load_mode(f, C, true);
    spec_for_size(S, [&](auto s) { spec_launch<decltype(s)::value, 2>((hipStream_t)stream, src, rows * C, out, (float2 *)ws); });
    ACG_CHECK_LAUNCH("acg_cross_spectrum");
    return ACG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The data gradient (ops.RadialSpectrum.backward, ops.spectral_loss): for a cotangent g[b] per field and ring,
// gx = d sum_b g[b] psd[b] / dx = 2 Re ifft2(w F), w[ky, kx] = g[bin] / count[bin] (0 beyond ring S/2), ifft2 normalised by
// 1 / S^2.  w F is Hermitian, so ifft2(w F) = fft2(conj(w F)) / S^2 is real: the inverse runs on the forward's Stockham stages
// and twiddle tables, and every step stays inside the packed half spectrum:
//   scale    G = conj(w F) per cell, w recomputed from the integer ring rule; 2 / S^2 is folded into the ring weights (a power
//            of two: exact).  The packed column (kx = 0 and S/2, each Hermitian in ky) is untangled, scaled and re-tangled:
//            its column transform is then real + i real, the packed form of two real row coefficients again.
//   columns  the forward's column stages on G.
//   rows     row y of the result is Hermitian in kx; rows 2q and 2q + 1 are re-tangled into one complex row (the inverse of
//            spec_untangle), one complex transform gives row 2q in the real and row 2q + 1 in the imaginary part.
// The cells of a ring are counted from the integer rule by a launch of their own into the head of the workspace (integer
// atomics in LDS only).  No float atomics; the arithmetic does not depend on the layout.  NHWC: the workgroups of channel 0
// also write the zeros of the padded channels C .. Cp - 1.
// S <= 128: one workgroup per field (forward, scale, inverse, store in the forward's two LDS buffers).  Above: the forward's
// row pass, a column pass per tile (transform, scale, transform, written back in place) and an inverse row pass.
#define SPEC_COUNT_THREADS 256

__host__ __device__ constexpr size_t spec_counts_bytes(int S) { return ((size_t)(S / 2 + 1) * sizeof(int) + 15) / 16 * 16; }

// cnt[b]: the cells (fx, fy) in [-S/2, S/2 - 1]^2 of ring b; one workgroup per ring, the rows fy over its work items
__global__ __launch_bounds__(SPEC_COUNT_THREADS) void spectrum_ring_counts_kernel(int S, int *__restrict__ cnt)
{
    __shared__ int total;
    const int b = blockIdx.x, H = S / 2;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int n = 0;
    if (b == 0) {
        n = threadIdx.x == 0 ? 1 : 0;
    } else {
        const int up = b * (b + 1), lo = b * (b - 1) + 1;
        for (int y = threadIdx.x; y < S; y += blockDim.x) {
            const int fy = y < H ? y : y - S, hi = up - fy * fy;
            if (hi < 0) continue;
            const int xh = spec_isqrt(hi), xl = spec_isqrt_ceil(lo - fy * fy);
            n += max(0, min(xh, H - 1) - xl + 1);                   // 0 <= fx <= S/2 - 1
            n += max(0, min(xh, H) - max(xl, 1) + 1);               // -S/2 <= fx < 0
        }
    }
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) cnt[b] = total;
}

// gw[b] = g[b] (2 / S^2) / count[b]: the weight of every cell of ring b, the factor 2 and ifft2's 1 / S^2 included
template <int S>
__device__ __forceinline__ void spec_ring_weights(const float *__restrict__ g, const int *__restrict__ cnt, float *gw)
{
    const float k = 2.f / ((float)S * (float)S);
    for (int b = threadIdx.x; b <= S / 2; b += blockDim.x) gw[b] = g[b] * k / (float)cnt[b];
}

// the weight of the cell of signed wavenumbers (fx, fy): its ring by the integer rule, 0 beyond ring S/2
template <int S>
__device__ __forceinline__ float spec_cell_weight(const float *gw, int fx, int fy)
{
    const int s = fx * fx + fy * fy;
    int b = spec_isqrt(s);
    if (b * (b + 1) < s) ++b;
    return b <= S / 2 ? gw[b] : 0.f;
}

// A transformed [S][KT] tile of columns kx0 .. kx0 + KT - 1, in place: f <- conj(w f); the tile of kx0 = 0 untangles its
// packed column into kx = 0 and kx = S/2, scales both and packs conj(w0 F0) + i conj(wn Fn)
template <int S, int KT>
__device__ __forceinline__ void spec_scale_conj(float2 *f, int kx0, const float *gw)
{
    constexpr int H = S / 2;
    for (int t = threadIdx.x; t < S * KT; t += blockDim.x) {
        const int ky = t / KT, c = t & (KT - 1), fy = ky < H ? ky : ky - S;
        if (kx0 + c == 0) {
            if (ky > H) continue;                                   // the work item of ky writes S - ky as well
            const int kz = (S - ky) & (S - 1);
            const float2 u = f[t], v = f[kz * KT];
            const float ar = 0.5f * (u.x + v.x), ai = 0.5f * (u.y - v.y), br = 0.5f * (u.y + v.y), bi = 0.5f * (v.x - u.x);
            const float wa = spec_cell_weight<S>(gw, 0, fy), wb = spec_cell_weight<S>(gw, H, fy);
            f[t] = make_float2(wa * ar + wb * bi, wb * br - wa * ai);
            if (kz != ky) f[kz * KT] = make_float2(wa * ar - wb * bi, wb * br + wa * ai);
        } else {
            const float w = spec_cell_weight<S>(gw, kx0 + c, fy);
            const float2 u = f[t];
            f[t] = make_float2(w * u.x, -w * u.y);
        }
    }
}

// Rows 2q, 2q + 1 of the packed half spectrum h (row stride S/2 complex; LDS or global), each Hermitian in kx, -> the complex
// rows z[q][S] = row 2q + i row 2q+1 for NRP row pairs: the inverse of spec_untangle_rows
template <int S, int NRP>
__device__ __forceinline__ void spec_tangle_rows(const float2 *h, float2 *z)
{
    constexpr int H = S / 2;
    for (int t = threadIdx.x; t < NRP * H; t += blockDim.x) {
        const int q = t / H, k = t & (H - 1);
        const float2 a = h[(long long)(2 * q) * H + k], b = h[(long long)(2 * q + 1) * H + k];
        float2 *zq = z + q * S;
        if (k == 0) {
            zq[0] = make_float2(a.x, b.x);
            zq[H] = make_float2(a.y, b.y);
        } else {
            zq[k] = make_float2(a.x - b.y, a.y + b.x);
            zq[S - k] = make_float2(a.x + b.y, b.x - a.y);
        }
    }
}

// z[q][w] = row 2 (rp0 + q) + i row 2 (rp0 + q) + 1 -> gx, in x's layout; gf: the field's first pixel, gi: its image's.
// The work items of channel 0 (zero_ch > 0) also clear channels zero_from .. zero_from + zero_ch - 1 of their pixels.
template <int S, int NRP>
__device__ __forceinline__ void spec_store_rows(const float2 *z, float *__restrict__ gf, float *__restrict__ gi, int pix_stride,
                                                long long chan_stride, bool planar, int rp0, int zero_from, int zero_ch)
{
    for (int t = threadIdx.x; t < NRP * (S / 4); t += blockDim.x) {
        const int q = t / (S / 4), w = (t & (S / 4 - 1)) * 4;
        const long long p0 = (long long)(2 * (rp0 + q)) * S + w, p1 = p0 + S;
        const float4 lo = *reinterpret_cast<const float4 *>(z + q * S + w), hi = *reinterpret_cast<const float4 *>(z + q * S + w + 2);
        const float r0[4] = {lo.x, lo.z, hi.x, hi.z}, r1[4] = {lo.y, lo.w, hi.y, hi.w};
        if (planar) {
            *reinterpret_cast<float4 *>(gf + p0) = make_float4(r0[0], r0[1], r0[2], r0[3]);
            *reinterpret_cast<float4 *>(gf + p1) = make_float4(r1[0], r1[1], r1[2], r1[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gf[(p0 + i) * pix_stride] = r0[i];
                gf[(p1 + i) * pix_stride] = r1[i];
            }
        }
        for (int cc = zero_from; cc < zero_from + zero_ch; ++cc) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gi[(p0 + i) * pix_stride + cc * chan_stride] = 0.f;
                gi[(p1 + i) * pix_stride + cc * chan_stride] = 0.f;
            }
        }
    }
}

// what a workgroup needs to place its field's gradient in gx, laid out as x (src): the field's first pixel, its image's, and
// the padded channels it clears
struct SpecDst {
    float *gf, *gi;
    int zero_from, zero_ch;
};
__device__ __forceinline__ SpecDst spec_dst(float *gx, const FieldSrc<1> &src, int f, int Cp)
{
    const int row = f / src.C, c = f - row * src.C;
    SpecDst d;
    d.gi = gx + (long long)row * src.f[0].row;
    d.gf = d.gi + (long long)c * src.f[0].chan;
    d.zero_from = src.C;
    d.zero_ch = c == 0 ? Cp - src.C : 0;
    return d;
}

// S <= 128: one workgroup per field
template <int S>
__global__ __launch_bounds__(spec_field_threads(S, 1)) void spectrum_bwd_field_kernel(FieldSrc<1> src, const float *__restrict__ g,
                                                                             const int *__restrict__ cnt, int Cp,
                                                                             float *__restrict__ gx)
{
    constexpr int H = S / 2;
    __shared__ __attribute__((aligned(16))) float2 buf0[H * S];
    __shared__ __attribute__((aligned(16))) float2 buf1[H * S];
    __shared__ float2 tw[S];
    __shared__ float gw[H + 1];
    int c;
    const float *xf = field_first(src, 0, blockIdx.x, c);
    spec_twiddles(tw, S);
    spec_ring_weights<S>(g + (long long)blockIdx.x * (H + 1), cnt, gw);
    spec_load_rows<S, H>(xf, src.f[0].pix, src.f[0].mode, c, 0, buf0);
    __syncthreads();
    float2 *z = spec_fft_rows<S, H>(buf0, buf1, tw);
    float2 *h = z == buf0 ? buf1 : buf0;
    spec_untangle_rows<S, H>(z, h);
    __syncthreads();
    float2 *f = spec_fft_cols<S, H>(h, z, tw);
    spec_scale_conj<S, H>(f, 0, gw);
    __syncthreads();
    float2 *o = f == buf0 ? buf1 : buf0;
    float2 *t = spec_fft_cols<S, H>(f, o, tw);                     // [y][S/2]: every row's half spectrum
    o = t == buf0 ? buf1 : buf0;
    spec_tangle_rows<S, H>(t, o);
    __syncthreads();
    const float2 *r = spec_fft_rows<S, H>(o, t, tw);
    const SpecDst d = spec_dst(gx, src, blockIdx.x, Cp);
    spec_store_rows<S, H>(r, d.gf, d.gi, src.f[0].pix, src.f[0].chan, src.f[0].mode == FIELD_PLANAR, 0, d.zero_from, d.zero_ch);
}

// S > 128, second pass: one workgroup per tile of SPEC_TILE / S columns of a field's half spectrum, in place
template <int S>
__global__ __launch_bounds__(SPEC_COLS_THREADS) void spectrum_bwd_cols_kernel(float2 *__restrict__ half, const float *__restrict__ g,
                                                                         const int *__restrict__ cnt)
{
    constexpr int KT = SPEC_TILE / S, H = S / 2;
    __shared__ __attribute__((aligned(16))) float2 buf0[SPEC_TILE];
    __shared__ __attribute__((aligned(16))) float2 buf1[SPEC_TILE];
    __shared__ float2 tw[S];
    __shared__ float gw[H + 1];
    const int kx0 = blockIdx.y * KT;
    float2 *hf = half + (long long)blockIdx.x * S * H;
    spec_twiddles(tw, S);
    spec_ring_weights<S>(g + (long long)blockIdx.x * (H + 1), cnt, gw);
    spec_load_tile<S, KT, 1>(hf, kx0, buf0);
    __syncthreads();
    float2 *f = spec_fft_cols<S, KT>(buf0, buf1, tw);
    spec_scale_conj<S, KT>(f, kx0, gw);
    __syncthreads();
    const float2 *r = spec_fft_cols<S, KT>(f, f == buf0 ? buf1 : buf0, tw);
    spec_store_tile<S, KT, 1>(r, kx0, hf);
}

// S > 128, third pass: SPEC_TILE / S row pairs of one field per workgroup, half spectra -> the real rows of gx
template <int S>
__global__ __launch_bounds__(SPEC_ROWS_THREADS) void spectrum_bwd_rows_kernel(const float2 *__restrict__ half, FieldSrc<1> src, int Cp,
                                                                         float *__restrict__ gx)
{
    constexpr int NRP = SPEC_TILE / S;
    __shared__ __attribute__((aligned(16))) float2 buf0[SPEC_TILE];
    __shared__ __attribute__((aligned(16))) float2 buf1[SPEC_TILE];
    __shared__ float2 tw[S];
    const int rp0 = blockIdx.y * NRP;
    spec_twiddles(tw, S);
    spec_tangle_rows<S, NRP>(half + ((long long)blockIdx.x * S + 2 * rp0) * (S / 2), buf0);
    __syncthreads();
    const float2 *r = spec_fft_rows<S, NRP>(buf0, buf1, tw);
    const SpecDst d = spec_dst(gx, src, blockIdx.x, Cp);
    spec_store_rows<S, NRP>(r, d.gf, d.gi, src.f[0].pix, src.f[0].chan, src.f[0].mode == FIELD_PLANAR, rp0, d.zero_from, d.zero_ch);
}

extern "C" size_t acg_radial_spectrum_bwd_workspace_bytes(int rows, int C, int S)
{
    if (rows < 1 || C < 1 || !spec_size_ok(S)) return 0;
    return spec_counts_bytes(S) + acg_radial_spectrum_workspace_bytes(rows, C, S);
}

template <int S>
static void spec_bwd_launch(hipStream_t st, const FieldSrc<1> &src, const float *g, int fields, int Cp, float *gx, int *cnt,
                            float2 *half)
{
    hipLaunchKernelGGL(spectrum_ring_counts_kernel, dim3(S / 2 + 1), dim3(SPEC_COUNT_THREADS), 0, st, S, cnt);
    if constexpr (spec_one_wg(S, 1)) {
        hipLaunchKernelGGL(spectrum_bwd_field_kernel<S>, dim3(fields), dim3(spec_field_threads(S, 1)), 0, st, src, g, (const int *)cnt,
                           Cp, gx);
        acg_note_kernel("spectrum_bwd_field<%d>", S);
    } else {
        constexpr int TILES = (S / 2) / (SPEC_TILE / S);
        hipLaunchKernelGGL((spectrum_rows_kernel<S, 1>), dim3(fields, TILES), dim3(SPEC_ROWS_THREADS), 0, st, src, half);
        hipLaunchKernelGGL(spectrum_bwd_cols_kernel<S>, dim3(fields, TILES), dim3(SPEC_COLS_THREADS), 0, st, half, g,
                           (const int *)cnt);
        hipLaunchKernelGGL(spectrum_bwd_rows_kernel<S>, dim3(fields, TILES), dim3(SPEC_ROWS_THREADS), 0, st, (const float2 *)half, src,
                           Cp, gx);
        acg_note_kernel("spectrum_rows<%d> + spectrum_bwd_cols<%d> + spectrum_bwd_rows<%d>", S, S, S);
    }
}

extern "C" int acg_radial_spectrum_bwd(const float *x, const float *g, int rows, int C, int Cp, int S, long long row_stride,
                                       int pix_stride, long long chan_stride, float *gx, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_radial_spectrum_bwd";
    ACG_REQUIRE(x != nullptr && g != nullptr && gx != nullptr, "%s: null tensor", fn);
    FieldSrc<1> src = {{{x, row_stride, chan_stride, pix_stride, FIELD_SCALAR}}, C, 1};
    FIELD_CHECK(spec_shape_refused(fn, S, rows, C));
    ACG_REQUIRE(Cp >= C, "%s: the stored channels cannot be fewer than the valid ones (C=%d, Cp=%d)", fn, C, Cp);
    ACG_REQUIRE((long long)rows * C <= 0x7fffffffLL, "%s: too many fields (rows=%d, C=%d)", fn, rows, C);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, src.f, 1));
    ACG_REQUIRE(x != gx, "%s: gx must not alias x", fn);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_radial_spectrum_bwd_workspace_bytes(rows, C, S)));
    src.f[0].mode = field_load_mode(src.f[0], C, true, gx);
    int *cnt = (int *)ws;
    float2 *half = (float2 *)((char *)ws + spec_counts_bytes(S));
    spec_for_size(S, [&](auto s) { spec_bwd_launch<decltype(s)::value>((hipStream_t)stream, src, g, rows * C, Cp, gx, cnt, half); });
    ACG_CHECK_LAUNCH("acg_radial_spectrum_bwd");
    return ACG_OK;
}
