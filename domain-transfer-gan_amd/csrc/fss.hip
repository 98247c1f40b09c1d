// Neighbourhood fractions skill scores (ops.fss, model.translate_fss, test.py --metric fss; tests/fss_ref.py states the
// definition).  Per field x, paired truth y, channel, threshold t and odd window n: events b = [x >= t] (NaN is no event),
// window counts c(i, j) = sum of b over the cells of the centred n x n window inside the domain, and the triple
// (sum cf^2, sum co^2, sum cf co) over the H x W cells.  Everything after the comparison is integer: the results are exact,
// the same bits in every layout and launch order.  No atomics.
//   events  one wave per image row (C4 NHWC: all channels of a pixel from one 16-byte load; otherwise per channel): the
//           ballot of [x >= t] over 64 consecutive columns is one 64-bit word of the plane (row, c, t).  Rows are padded to
//           whole words (WW = ceil(W / 64) per row); next to every row go WW + 1 16-bit prefixes, the events in the words
//           before each.  Both live in the workspace: 10 bits per cell and threshold, never a plane per window.
//   counts  the events of row i in columns [a, b) are pref(i, b) - pref(i, a), pref(i, k) = prefix[k / 64] + popcount of the
//           low k % 64 bits of word k / 64: any window width costs two words and two prefixes.
//   box     one workgroup per (x row, c, t), one thread per column j.  Per window the thread walks down its column with the
//           running sums cf, co of the row counts of rows i - n/2 .. i + n/2 (one row enters, one leaves), and adds the three
//           products in 64-bit registers.  No barrier inside the walk; a block reduction and one store per triple end it.
//           Resident path (fss_box<lds>): the workgroup's planes and their prefixes, (8 WW + 2 (WW + 1)) H bytes each, are
//           copied into LDS first (up to FSS_LDS_MAX: two planes take 21 KiB at 256^2, 39 KiB at 321^2); above
//           (fss_box<global>) the walk reads them from the workspace through the caches.
//   ens     E = sum over the M members of cf_m = the window count of e = sum_m b_m (box sums are linear).  e is kept as
//           NS = bit_width(M) bit planes of the same format (fss_slices: per word a carry-save sum of the M member words, bit k
//           of e in plane k), so the row count of e is sum_k 2^k (row count of plane k) and the ensemble's walk is the box
//           kernel with NS planes on its x side, one workgroup per (truth row, c, t) (fss_ens<lds> while NS + 1 planes fit:
//           16 members at 256^2 take 63 KiB).  M = 1: e is the member's own plane, no slices.
// The intensity-scale triples of the same events (ops.fss_scales, --fss_scales; tests/fss_scales_ref.py; Casati et al. 2004):
//   scales  acg_fss_scales shares events and slices.  Level l = 0 .. L = ceil(log2(max(H, W))) cuts the plane into blocks of
//           2^l x 2^l cells anchored at cell (0, 0), the last ones cut by the domain; bf, bo are the events of a block and the
//           triple is (sum bf^2, sum bo^2, sum bf bo) over the blocks of a level.  One workgroup per (x row, c, t) (the ensemble:
//           per (truth row, c, t), bf the slices' sum_k 2^k count), a wave per 64 x 64 tile at a time: lane r holds the words
//           of tile row r, level 0 is popcounts, level 1 the 2-bit fields of x - ((x >> 1) & 0x55..), and each further level
//           adds neighbouring blocks in the lane and then the lane 2^(l-1) away (6 levels: 63 exchanges per side), the first
//           lane of every 2^l squaring.  The tile totals go to LDS; one thread per block forms levels 7 .. 10 from them.
// The reliability tables of the same events (ops.reliability, --fss_rel; include/acgan_verif.h; tests/reliability_ref.py):
//   rel     acg_reliability shares events.  The neighbourhood event of a cell is the OR of the events in its window (the
//           window count is positive); table[k][o] counts the cells where k of the M members and o of the truth have it.
//           One workgroup per (truth row, c, t, window), one thread per 64-bit word at a time: dilate the word of each of
//           the M + 1 planes (OR down the rows of the window, then shifts along the row with the two neighbouring words;
//           windows stop at 65), carry-save add the member words in registers, and per k add two popcounts to integer
//           counters in LDS.  fss_rel<lds> while the M + 1 planes' words fit FSS_REL_LDS_MAX, fss_rel<global> above.
#include "common.h"
#include "field.h"
#include "../../include/acgan_verif.h"
#include <stdint.h>

#define FSS_MAX_HW 1024
#define FSS_MAX_T 8
#define FSS_MAX_NW 8
#define FSS_MAX_M 64
#define FSS_LDS_MAX (64 * 1024 - 512)      // of the 64 KiB a workgroup gets by default; the reduction takes 384 bytes
#define FSS_MAX_NS 7                       // bit_width(FSS_MAX_M)
#define FSS_SLICE_THREADS 256
#define FSS_EVENT_THREADS 256
#define FSS_SCALE_THREADS 256
#define FSS_TILE_LEVELS 7                  // levels 0 .. 6 lie inside a 64 x 64 tile: one word per lane of a wave
#define FSS_MAX_TILES 256                  // (FSS_MAX_HW / 64)^2
#define FSS_REL_THREADS 1024
#define FSS_REL_MAX_WINDOW 65              // radius 32: a dilated word depends on itself and its two neighbours only
#define FSS_REL_LDS_MAX (FSS_LDS_MAX - 512) // fss_rel's counters take 520 bytes of static LDS

typedef unsigned long long u64;

struct FssPlanes {                       // event planes in the workspace: plane p at bits + p H WW, pref + p H (WW + 1)
    u64 *bits;
    unsigned short *pref;
};

static inline int fss_ww(int W) { return (W + 63) / 64; }
static size_t fss_bits_bytes(size_t planes, int H, int W) { return acg_round_up(planes * H * fss_ww(W) * sizeof(u64), 16); }
static size_t fss_pref_bytes(size_t planes, int H, int W)
{
    return acg_round_up(planes * H * (fss_ww(W) + 1) * sizeof(unsigned short), 16);
}

// One wave per (field row f, image row i [, channel]): words and prefixes of the planes (f, c, t), all t.  C4: x is FIELD_C4
// and the wave covers channels 0 .. C - 1 (C <= 4); otherwise blockIdx.y is the channel.
template <bool C4>
__global__ __launch_bounds__(FSS_EVENT_THREADS) void fss_events_kernel(Field x, int rows, int C, int H, int W,
                                                                     const float *__restrict__ thr, int T, FssPlanes pl)
{
    constexpr int NC = C4 ? 4 : 1;
    const int lane = threadIdx.x & 63, WW = (W + 63) >> 6;
    const long long item = (long long)blockIdx.x * (FSS_EVENT_THREADS / 64) + (threadIdx.x >> 6);
    if (item >= (long long)rows * H) return;                       // whole waves leave: the ballots below see full waves
    const int f = (int)(item / H), i = (int)(item - (long long)f * H);
    const int c0 = C4 ? 0 : blockIdx.y, nc = C4 ? C : 1;
    const float *__restrict__ xf = x.x + (long long)f * x.row;
    unsigned before = 0;                 // lane c FSS_MAX_T + t keeps the events of plane (c, t) in the words before w, and stores
    for (int w = 0; w <= WW; ++w) {
        const int j = w * 64 + lane;
        const bool in = w < WW && j < W;
        float v[NC];
        if constexpr (C4) {
            const float4 q = in ? reinterpret_cast<const float4 *>(xf)[(long long)i * W + j] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            v[0] = in ? xf[(long long)c0 * x.chan + ((long long)i * W + j) * x.pix] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c >= nc) continue;
            for (int t = 0; t < T; ++t) {
                const bool mine = lane == c * FSS_MAX_T + t;
                const long long p = ((long long)f * C + c0 + c) * T + t;
                if (mine) pl.pref[(p * H + i) * (WW + 1) + w] = (unsigned short)before;
                if (w == WW) continue;
                const u64 word = __ballot(in && v[c] >= thr[(c0 + c) * T + t]);   // NaN compares false: no event
                if (mine) {
                    pl.bits[(p * H + i) * WW + w] = word;
                    before += __popcll(word);
                }
            }
        }
    }
}

// events of one row (bits: its WW words, pref: its WW + 1 prefixes) in columns [0, k), 0 <= k <= W
__device__ __forceinline__ int fss_pref(const u64 *bits, const unsigned short *pref, int k)
{
    const int w = k >> 6, b = k & 63;
    int n = pref[w];
    if (b) n += __popcll(bits[w] & ((1ull << b) - 1ull));
    return n;
}
__device__ __forceinline__ int fss_row_count(const u64 *bits, const unsigned short *pref, int i, int WW, int lo, int hi)
{
    const u64 *b = bits + (long long)i * WW;
    const unsigned short *p = pref + (long long)i * (WW + 1);
    return fss_pref(b, p, hi) - fss_pref(b, p, lo);
}

struct FssWindows {
    int n, r[FSS_MAX_NW];                // radii n / 2, clamped to max(H, W) (the whole domain)
};

// sums of the workgroup's threads -> out[0..2] by thread 0; red: 3 * 16 words of LDS
__device__ __forceinline__ void fss_block_store(u64 a, u64 b, u64 c, u64 *red, long long *out)
{
    u64 v[3] = {a, b, c};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned lo = __shfl_down((unsigned)v[k], off), hi = __shfl_down((unsigned)(v[k] >> 32), off);
            v[k] += ((u64)hi << 32) | lo;
        }
    const int wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
    __syncthreads();                                               // red is reused window after window
    if ((threadIdx.x & 63) == 0) red[wave] = v[0], red[16 + wave] = v[1], red[32 + wave] = v[2];
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s0 = 0, s1 = 0, s2 = 0;
        for (int w = 0; w < nwaves; ++w) s0 += red[w], s1 += red[16 + w], s2 += red[32 + w];
        out[0] = (long long)s0, out[1] = (long long)s1, out[2] = (long long)s2;
    }
}

// The walk of one workgroup: the x side is the sum over nx planes of 2^k times plane k's counts (nx = 1: a member's events;
// nx = NS: the bit planes of an exceedance count), the y side one plane.  xsb, xsp: the words / prefixes between x planes.
__device__ __forceinline__ void fss_walk(const u64 *xb, const unsigned short *xp, int nx, long long xsb, long long xsp, const u64 *yb,
                                         const unsigned short *yp, int H, int W, const FssWindows &win, u64 *red, long long *out)
{
    const int j = threadIdx.x, WW = (W + 63) >> 6;
    for (int k = 0; k < win.n; ++k) {
        const int r = win.r[k];
        u64 sff = 0, soo = 0, sfo = 0;
        if (j < W) {
            const int lo = max(j - r, 0), hi = min(j + r, W - 1) + 1;
            auto xrow = [&](int i) {
                int n = 0;
                for (int m = 0; m < nx; ++m) n += fss_row_count(xb + m * xsb, xp + m * xsp, i, WW, lo, hi) << m;
                return n;
            };
            long long cf = 0, co = 0;
            for (int i = 0; i <= min(r, H - 1); ++i) {
                cf += xrow(i);
                co += fss_row_count(yb, yp, i, WW, lo, hi);
            }
            for (int i = 0; i < H; ++i) {
                sff += (u64)(cf * cf), soo += (u64)(co * co), sfo += (u64)(cf * co);
                const int enter = i + r + 1, leave = i - r;
                if (enter < H) {
                    cf += xrow(enter);
                    co += fss_row_count(yb, yp, enter, WW, lo, hi);
                }
                if (leave >= 0) {
                    cf -= xrow(leave);
                    co -= fss_row_count(yb, yp, leave, WW, lo, hi);
                }
            }
        }
        fss_block_store(sff, soo, sfo, red, out + 3 * k);
    }
}

// One workgroup per blockIdx.x = (x row f, c, t): its x side is the nx planes blockIdx.x nx .. of px, its truth plane
// (f / x_per_y, c, t) of py.  The members: nx = 1 on the event planes; the ensemble: nx = NS on the slices, x_per_y = 1.
// LDS: the nx + 1 planes are copied into dynamic LDS first (x's words, y's words, x's prefixes, y's prefixes).
template <bool LDS>
__global__ __launch_bounds__(FSS_MAX_HW) void fss_box_kernel(FssPlanes px, FssPlanes py, int nx, int CT, int x_per_y, int H, int W,
                                                            FssWindows win, long long *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fss_lds[];
    __shared__ u64 red[48];
    const int WW = (W + 63) >> 6;
    const long long p = blockIdx.x, f = p / CT, q = (f / x_per_y) * CT + (p - f * CT);
    const long long nb = (long long)H * WW, np = (long long)H * (WW + 1);
    const u64 *xb = px.bits + p * nx * nb, *yb = py.bits + q * nb;
    const unsigned short *xp = px.pref + p * nx * np, *yp = py.pref + q * np;
    long long *o = out + p * win.n * 3;
    if constexpr (LDS) {
        u64 *lb = reinterpret_cast<u64 *>(fss_lds);
        unsigned short *lp = reinterpret_cast<unsigned short *>(lb + (nx + 1) * nb);
        for (int t = threadIdx.x; t < nx * nb; t += blockDim.x) lb[t] = xb[t];
        for (int t = threadIdx.x; t < nb; t += blockDim.x) lb[nx * nb + t] = yb[t];
        for (int t = threadIdx.x; t < nx * np; t += blockDim.x) lp[t] = xp[t];
        for (int t = threadIdx.x; t < np; t += blockDim.x) lp[nx * np + t] = yp[t];
        __syncthreads();
        fss_walk(lb, lp, nx, nb, np, lb + nx * nb, lp + nx * np, H, W, win, red, o);
    } else {
        fss_walk(xb, xp, nx, nb, np, yb, yp, H, W, win, red, o);
    }
}

// e = the sum of the M member planes of a truth as NS bit planes: one thread per (truth plane q, image row i) adds the members'
// words with a carry-save counter (bit k of the count in s[k]) and writes the words and row prefixes of planes q NS + k
__global__ __launch_bounds__(FSS_SLICE_THREADS) void fss_slices_kernel(FssPlanes px, FssPlanes ps, long long planes_y, int CT, int M,
                                                                      int NS, int H, int W)
{
    const long long idx = (long long)blockIdx.x * FSS_SLICE_THREADS + threadIdx.x;
    if (idx >= planes_y * H) return;
    const long long q = idx / H, g = q / CT, p0 = g * M * CT + (q - g * CT);     // member m's plane lies m CT planes after p0
    const int i = (int)(idx - q * H), WW = (W + 63) >> 6;
    unsigned before[FSS_MAX_NS];
#pragma unroll
    for (int k = 0; k < FSS_MAX_NS; ++k) before[k] = 0;
    for (int w = 0; w <= WW; ++w) {
        u64 s[FSS_MAX_NS];
#pragma unroll
        for (int k = 0; k < FSS_MAX_NS; ++k) s[k] = 0;
        if (w < WW)
            for (int m = 0; m < M; ++m) {
                u64 carry = px.bits[((p0 + (long long)m * CT) * H + i) * WW + w];
#pragma unroll
                for (int k = 0; k < FSS_MAX_NS; ++k) {
                    const u64 t = s[k] & carry;
                    s[k] ^= carry;
                    carry = t;
                }
            }
#pragma unroll
        for (int k = 0; k < FSS_MAX_NS; ++k) {
            if (k >= NS) continue;
            const long long row = (q * NS + k) * H + i;
            ps.pref[row * (WW + 1) + w] = (unsigned short)before[k];
            if (w < WW) ps.bits[row * WW + w] = s[k];
            before[k] += __popcll(s[k]);
        }
    }
}

// The intensity-scale triples of one workgroup: blockIdx.x = (x row f, c, t) picks its planes as in fss_box_kernel (nx = 1: a
// member's events; nx = NS <= NX: the bit planes of an exceedance count, x_per_y = 1), out + blockIdx.x nl 3 takes the triples
// of levels 0 .. nl - 1.  Bits of a word past W and rows past H are masked here, whatever the workspace holds there.
template <int NX>
__global__ __launch_bounds__(FSS_SCALE_THREADS) void fss_scales_kernel(FssPlanes px, FssPlanes py, int nx, int CT, int x_per_y, int H,
                                                                      int W, int nl, long long *__restrict__ out)
{
    __shared__ unsigned tile_x[FSS_MAX_TILES], tile_o[FSS_MAX_TILES];      // the events of every 64 x 64 tile
    __shared__ u64 red[48];
    const int lane = threadIdx.x & 63, WW = (W + 63) >> 6, TH = (H + 63) >> 6;
    const long long p = blockIdx.x, f = p / CT, q = (f / x_per_y) * CT + (p - f * CT);
    const long long nb = (long long)H * WW;
    const u64 *xb = px.bits + p * nx * nb, *yb = py.bits + q * nb;
    u64 acc[FSS_TILE_LEVELS][3];
#pragma unroll
    for (int l = 0; l < FSS_TILE_LEVELS; ++l) acc[l][0] = acc[l][1] = acc[l][2] = 0;
    for (int tile = threadIdx.x >> 6; tile < TH * WW; tile += FSS_SCALE_THREADS / 64) {
        const int ti = tile / WW, tj = tile - ti * WW, i = ti * 64 + lane, left = W - tj * 64;
        const u64 keep = i >= H ? 0ull : left >= 64 ? ~0ull : (1ull << left) - 1ull;
        const u64 O = keep ? yb[(long long)i * WW + tj] & keep : 0ull;
        u64 F[NX];
#pragma unroll
        for (int k = 0; k < NX; ++k) F[k] = keep && k < nx ? xb[k * nb + (long long)i * WW + tj] & keep : 0ull;
        // level 0: the cells themselves, e = sum_k 2^k F[k]: e^2 = sum_k 4^k F[k] + 2 sum_{k < k'} 2^(k + k') F[k] F[k']
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            acc[0][0] += (u64)__popcll(F[k]) << (2 * k);
            acc[0][2] += (u64)__popcll(F[k] & O) << k;
#pragma unroll
            for (int k2 = k + 1; k2 < NX; ++k2) acc[0][0] += (u64)__popcll(F[k] & F[k2]) << (k + k2 + 1);
        }
        acc[0][1] += __popcll(O);
        // level 1 inside the lane: the events of the 32 column pairs of its row
        const u64 odd = 0x5555555555555555ull;
        unsigned cx[32], co[32];
        const u64 ho = O - ((O >> 1) & odd);
#pragma unroll
        for (int s = 0; s < 32; ++s) co[s] = (unsigned)(ho >> (2 * s)) & 3u, cx[s] = 0;
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const u64 hx = F[k] - ((F[k] >> 1) & odd);
#pragma unroll
            for (int s = 0; s < 32; ++s) cx[s] += ((unsigned)(hx >> (2 * s)) & 3u) << k;
        }
        // level l: cx[s], co[s] become the events of block (lane >> l, s) of the tile in every lane of its 2^l rows
#pragma unroll
        for (int l = 1; l < FSS_TILE_LEVELS; ++l) {
#pragma unroll
            for (int s = 0; s < (64 >> l); ++s) {
                if (l > 1) cx[s] = cx[2 * s] + cx[2 * s + 1], co[s] = co[2 * s] + co[2 * s + 1];
                cx[s] += __shfl_xor(cx[s], 1 << (l - 1));
                co[s] += __shfl_xor(co[s], 1 << (l - 1));
                if ((lane & ((1 << l) - 1)) == 0) {
                    acc[l][0] += (u64)cx[s] * cx[s];
                    acc[l][1] += (u64)co[s] * co[s];
                    acc[l][2] += (u64)cx[s] * co[s];
                }
            }
        }
        if (lane == 0) tile_x[tile] = cx[0], tile_o[tile] = co[0];
    }
#pragma unroll
    for (int l = 0; l < FSS_TILE_LEVELS; ++l)
        if (l < nl) fss_block_store(acc[l][0], acc[l][1], acc[l][2], red, out + (p * nl + l) * 3);
    __syncthreads();                                               // the tile totals of all waves
    for (int l = FSS_TILE_LEVELS; l < nl; ++l) {                   // blocks of tb x tb tiles: at most 8 x 8 of them
        const int tb = 1 << (l - FSS_TILE_LEVELS + 1), bw = (WW + tb - 1) / tb, bh = (TH + tb - 1) / tb;
        u64 ff = 0, oo = 0, fo = 0;
        if ((int)threadIdx.x < bh * bw) {
            const int bi = threadIdx.x / bw, bj = threadIdx.x - bi * bw;
            unsigned sx = 0, so = 0;                               // at most 64 * 2^20 events
            for (int ti = bi * tb; ti < min((bi + 1) * tb, TH); ++ti)
                for (int tj = bj * tb; tj < min((bj + 1) * tb, WW); ++tj) sx += tile_x[ti * WW + tj], so += tile_o[ti * WW + tj];
            ff = (u64)sx * sx, oo = (u64)so * so, fo = (u64)sx * so;
        }
        fss_block_store(ff, oo, fo, red, out + (p * nl + l) * 3);
    }
}

static int fss_slices(int M)             // bit_width(M): the planes of a count in 0 .. M; none of their own for M = 1
{
    int ns = 0;
    while (M >> ns) ++ns;
    return ns;
}

static bool fss_shape_ok(int rows, int x_per_y, int C, int H, int W, int T, int nw)
{
    return rows >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= FSS_MAX_HW && W <= FSS_MAX_HW && T >= 1 && T <= FSS_MAX_T && nw >= 1 &&
           nw <= FSS_MAX_NW && x_per_y >= 1 && x_per_y <= FSS_MAX_M && rows % x_per_y == 0 &&
           (long long)rows * C * T <= 0x7fffffffLL && (long long)rows * H <= 0x7fffffffLL;
}

// x's planes (words, prefixes), then y's, then with want_ens and x_per_y > 1 the bit_width(x_per_y) slices of every truth plane:
// about 10 bits per cell and plane, whatever the windows
static size_t fss_planes_bytes(int rows, int x_per_y, int C, int H, int W, int T, int want_ens)
{
    const size_t px = (size_t)rows * C * T, py = (size_t)(rows / x_per_y) * C * T;
    const size_t ps = want_ens && x_per_y > 1 ? py * fss_slices(x_per_y) : 0;
    return fss_bits_bytes(px, H, W) + fss_pref_bytes(px, H, W) + fss_bits_bytes(py, H, W) + fss_pref_bytes(py, H, W) +
           fss_bits_bytes(ps, H, W) + fss_pref_bytes(ps, H, W);
}
extern "C" size_t acg_fss_workspace_bytes(int rows, int x_per_y, int C, int H, int W, int T, int nw, int want_ens)
{
    return fss_shape_ok(rows, x_per_y, C, H, W, T, nw) ? fss_planes_bytes(rows, x_per_y, C, H, W, T, want_ens) : 0;
}

struct FssSpace {                        // the workspace of a call: the planes of x, of y and the slices of every truth plane
    FssPlanes px, py, ps;
};
static FssSpace fss_carve(void *ws, size_t npx, size_t npy, int NS, int H, int W)
{
    unsigned char *w8 = (unsigned char *)ws;
    FssSpace s;
    s.px.bits = (u64 *)w8, w8 += fss_bits_bytes(npx, H, W);
    s.px.pref = (unsigned short *)w8, w8 += fss_pref_bytes(npx, H, W);
    s.py.bits = (u64 *)w8, w8 += fss_bits_bytes(npy, H, W);
    s.py.pref = (unsigned short *)w8, w8 += fss_pref_bytes(npy, H, W);
    s.ps.bits = (u64 *)w8, w8 += fss_bits_bytes(npy * NS, H, W);
    s.ps.pref = (unsigned short *)w8;
    return s;
}

static void fss_events(hipStream_t st, const Field &x, int rows, int C, int H, int W, const float *thr, int T, FssPlanes pl)
{
    const unsigned blocks = (unsigned)acg_cdiv((long)rows * H, FSS_EVENT_THREADS / 64);
    if (x.mode == FIELD_C4)
        hipLaunchKernelGGL(fss_events_kernel<true>, dim3(blocks), dim3(FSS_EVENT_THREADS), 0, st, x, rows, C, H, W, thr, T, pl);
    else
        hipLaunchKernelGGL(fss_events_kernel<false>, dim3(blocks, C), dim3(FSS_EVENT_THREADS), 0, st, x, rows, C, H, W, thr, T, pl);
}

extern "C" int acg_fss(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                       int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                       const float *thr, int T, const int *windows, int nw, long long *out, long long *ens_out, void *ws,
                       size_t ws_bytes, void *stream)
{
    const char *fn = "acg_fss";
    ACG_REQUIRE(x != nullptr && y != nullptr && thr != nullptr && windows != nullptr, "acg_fss: null tensor");
    ACG_REQUIRE(out != nullptr || ens_out != nullptr, "acg_fss: out and ens_out are both NULL");
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= FSS_MAX_HW && W <= FSS_MAX_HW, "acg_fss: fields must be H x W with 1 <= H, W <= %d (got %d x %d)",
                FSS_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(T >= 1 && T <= FSS_MAX_T && nw >= 1 && nw <= FSS_MAX_NW, "acg_fss: need 1 <= T <= %d thresholds and 1 <= nw <= %d windows (T=%d, nw=%d)",
                FSS_MAX_T, FSS_MAX_NW, T, nw);
    ACG_REQUIRE((long long)rows * C * T <= 0x7fffffffLL && (long long)rows * H <= 0x7fffffffLL,
                "acg_fss: too many planes (rows=%d, C=%d, T=%d, H=%d)", rows, C, T, H);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, FSS_MAX_M));
    FssWindows win;
    win.n = nw;
    const int whole = H > W ? H : W;
    for (int k = 0; k < FSS_MAX_NW; ++k) win.r[k] = 0;
    for (int k = 0; k < nw; ++k) {
        const int n = windows[k];
        ACG_REQUIRE(n >= 1 && n % 2 == 1, "acg_fss: windows must be odd and positive (window %d is %d)", k, n);
        win.r[k] = n / 2 < whole ? n / 2 : whole;
        // the largest possible sum, every cell an event in every member: (v min(n, H) min(n, W))^2 H W, v = 1 or x_per_y
        const unsigned __int128 side = (unsigned __int128)(n < H ? n : H) * (unsigned)(n < W ? n : W) * (ens_out ? x_per_y : 1);
        ACG_REQUIRE(side * side * (unsigned)H * (unsigned)W < ((unsigned __int128)1 << 63),
                    "acg_fss: overflow: window %d on %d x %d with %d members per truth can reach 2^63", n, H, W, ens_out ? x_per_y : 1);
    }
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_fss_workspace_bytes(rows, x_per_y, C, H, W, T, nw, ens_out != nullptr)));
    for (Field &o : f) o.mode = field_load_mode(o, C);
    hipStream_t st = (hipStream_t)stream;
    const int rows_y = rows / x_per_y, CT = C * T;
    const size_t npx = (size_t)rows * CT, npy = (size_t)rows_y * CT;
    const int NS = fss_slices(x_per_y);
    const FssSpace space = fss_carve(ws, npx, npy, NS, H, W);
    const FssPlanes &px = space.px, &py = space.py, &ps = space.ps;
    fss_events(st, f[0], rows, C, H, W, thr, T, px);
    fss_events(st, f[1], rows_y, C, H, W, thr, T, py);
    const unsigned threads = (unsigned)acg_round_up(W, 64);
    const size_t plane = (size_t)H * fss_ww(W) * sizeof(u64) + (size_t)H * (fss_ww(W) + 1) * sizeof(unsigned short);
    auto box = [&](const FssPlanes &xs, int nx, size_t blocks, int per, long long *o) {   // -> whether the planes went into LDS
        const size_t lds = (nx + 1) * plane;
        if (lds <= FSS_LDS_MAX)
            hipLaunchKernelGGL(fss_box_kernel<true>, dim3((unsigned)blocks), dim3(threads), lds, st, xs, py, nx, CT, per, H, W, win, o);
        else
            hipLaunchKernelGGL(fss_box_kernel<false>, dim3((unsigned)blocks), dim3(threads), 0, st, xs, py, nx, CT, per, H, W, win, o);
        return lds <= FSS_LDS_MAX;
    };
    char path[96] = "";
    size_t len = 0;
    if (out != nullptr) len += snprintf(path + len, sizeof(path) - len, " + fss_box<%s>", box(px, 1, npx, x_per_y, out) ? "lds" : "global");
    if (ens_out != nullptr && x_per_y == 1) {                      // the member's own plane is the count plane
        len += snprintf(path + len, sizeof(path) - len, " + fss_ens<%s>", box(px, 1, npy, 1, ens_out) ? "lds" : "global");
    } else if (ens_out != nullptr) {
        hipLaunchKernelGGL(fss_slices_kernel, dim3((unsigned)acg_cdiv((long)npy * H, FSS_SLICE_THREADS)), dim3(FSS_SLICE_THREADS), 0, st,
                           px, ps, (long long)npy, CT, x_per_y, NS, H, W);
        len += snprintf(path + len, sizeof(path) - len, " + fss_slices + fss_ens<%s>", box(ps, NS, npy, 1, ens_out) ? "lds" : "global");
    }
    acg_note_kernel("fss_events<%s>%s", f[0].mode == FIELD_C4 ? "c4" : "strided", path);
    ACG_CHECK_LAUNCH("acg_fss");
    return ACG_OK;
}

static int fss_scale_levels(int H, int W)  // L + 1, L = ceil(log2(max(H, W)))
{
    int nl = 1;
    while ((1 << (nl - 1)) < (H > W ? H : W)) ++nl;
    return nl;
}

// acg_fss's workspace without the windows: the planes of x and y and, with want_ens and x_per_y > 1, the slices
extern "C" size_t acg_fss_scales_workspace_bytes(int rows, int x_per_y, int C, int H, int W, int T, int want_ens)
{
    return fss_shape_ok(rows, x_per_y, C, H, W, T, 1) ? fss_planes_bytes(rows, x_per_y, C, H, W, T, want_ens) : 0;
}

extern "C" int acg_fss_scales(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                              int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                              long long y_chan_stride, const float *thr, int T, long long *out, long long *ens_out, void *ws,
                              size_t ws_bytes, void *stream)
{
    const char *fn = "acg_fss_scales";
    ACG_REQUIRE(x != nullptr && y != nullptr && thr != nullptr, "acg_fss_scales: null tensor");
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, FSS_MAX_M));
    ACG_REQUIRE(out != nullptr || ens_out != nullptr, "acg_fss_scales: out and ens_out are both NULL");
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= FSS_MAX_HW && W <= FSS_MAX_HW,
                "acg_fss_scales: fields must be H x W with 1 <= H, W <= %d (got %d x %d)", FSS_MAX_HW, H, W);
    ACG_REQUIRE(T >= 1 && T <= FSS_MAX_T, "acg_fss_scales: need 1 <= T <= %d thresholds (T=%d)", FSS_MAX_T, T);
    ACG_REQUIRE((long long)rows * C * T <= 0x7fffffffLL && (long long)rows * H <= 0x7fffffffLL,
                "acg_fss_scales: too many planes (rows=%d, C=%d, T=%d, H=%d)", rows, C, T, H);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_fss_scales_workspace_bytes(rows, x_per_y, C, H, W, T, ens_out != nullptr)));
    for (Field &o : f) o.mode = field_load_mode(o, C);
    hipStream_t st = (hipStream_t)stream;
    const int rows_y = rows / x_per_y, CT = C * T, NS = fss_slices(x_per_y), nl = fss_scale_levels(H, W);
    const size_t npx = (size_t)rows * CT, npy = (size_t)rows_y * CT;
    const FssSpace space = fss_carve(ws, npx, npy, NS, H, W);
    fss_events(st, f[0], rows, C, H, W, thr, T, space.px);
    fss_events(st, f[1], rows_y, C, H, W, thr, T, space.py);
    if (out != nullptr)
        hipLaunchKernelGGL(fss_scales_kernel<1>, dim3((unsigned)npx), dim3(FSS_SCALE_THREADS), 0, st, space.px, space.py, 1, CT, x_per_y,
                           H, W, nl, out);
    if (ens_out != nullptr && x_per_y == 1) {                      // the member's own plane is the count plane
        hipLaunchKernelGGL(fss_scales_kernel<1>, dim3((unsigned)npy), dim3(FSS_SCALE_THREADS), 0, st, space.px, space.py, 1, CT, 1, H,
                           W, nl, ens_out);
    } else if (ens_out != nullptr) {
        hipLaunchKernelGGL(fss_slices_kernel, dim3((unsigned)acg_cdiv((long)npy * H, FSS_SLICE_THREADS)), dim3(FSS_SLICE_THREADS), 0, st,
                           space.px, space.ps, (long long)npy, CT, x_per_y, NS, H, W);
        hipLaunchKernelGGL(fss_scales_kernel<FSS_MAX_NS>, dim3((unsigned)npy), dim3(FSS_SCALE_THREADS), 0, st, space.ps, space.py, NS, CT,
                           1, H, W, nl, ens_out);
    }
    acg_note_kernel("fss_events<%s>%s%s", f[0].mode == FIELD_C4 ? "c4" : "strided", out != nullptr ? " + fss_scales" : "",
                    ens_out == nullptr ? "" : x_per_y == 1 ? " + fss_scales_ens" : " + fss_slices + fss_scales_ens");
    ACG_CHECK_LAUNCH("acg_fss_scales");
    return ACG_OK;
}

// ---- reliability tables of the same events (include/acgan_verif.h; ops.reliability, --fss_rel) ----

// One word of a plane's neighbourhood events: the OR of the events within r <= 32 rows and columns of each of the 64 cells
// of word w of row i, inside the domain.  plane: H rows of WW words whose bits past W are 0 (fss_events writes them so).
// Dilation separates: first the OR down the rows of the word and its two neighbours, then along the row by shifts; `valid`
// (the cells of the word inside W) takes off what the shifts carried past W.
__device__ __forceinline__ u64 fss_rel_dilate(const u64 *plane, int i, int w, int H, int WW, int r, u64 valid)
{
    const int i0 = max(i - r, 0), i1 = min(i + r, H - 1);
    u64 c = 0, l = 0, h = 0;                                       // the word, the one before it, the one after it
    if (r == 0) return plane[(long long)i * WW + w] & valid;
    for (int ii = i0; ii <= i1; ++ii) {
        const u64 *row = plane + (long long)ii * WW;
        c |= row[w];
        if (w > 0) l |= row[w - 1];
        if (w + 1 < WW) h |= row[w + 1];
    }
    u64 d = c;
    for (int s = 1; s <= r; ++s)                                   // 64 - s lies in 32 .. 63: no shift by the word's width
        d |= (c << s) | (l >> (64 - s)) | (c >> s) | (h << (64 - s));
    return d & valid;
}

// One workgroup per (truth plane q = (g, c, t), window blockIdx.y): table[k][o] of its H W cells, k the members among the
// M of truth row g whose neighbourhood event holds, o the truth's.  Thread by thread over the (row, word) items: the M
// dilated member words go through a carry-save counter (bit b of k in s[b], as in fss_slices_kernel), mask_k is the AND of
// the slices or their complements, and the two popcounts of every k go to 32-bit counters in LDS (integer adds: any order
// gives the same sums; a counter holds at most H W <= 2^20).  LDS: the M + 1 planes' words are copied into dynamic LDS
// first (members, then the truth).
template <bool LDS>
__global__ __launch_bounds__(FSS_REL_THREADS) void fss_rel_kernel(FssPlanes px, FssPlanes py, int CT, int M, int NS, int H, int W,
                                                                 FssWindows win, long long *__restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fss_lds[];
    __shared__ unsigned cnt[2 * (FSS_MAX_M + 1)];
    const int WW = (W + 63) >> 6, r = win.r[blockIdx.y];
    const long long q = blockIdx.x, g = q / CT, p0 = g * M * CT + (q - g * CT);  // member m's plane lies m CT planes after p0
    const long long nb = (long long)H * WW;
    const u64 *xb = px.bits + p0 * nb, *yb = py.bits + q * nb;
    long long xs = (long long)CT * nb;                             // the words between two members' planes
    for (int t = threadIdx.x; t < 2 * (M + 1); t += blockDim.x) cnt[t] = 0;
    if constexpr (LDS) {
        u64 *lb = reinterpret_cast<u64 *>(fss_lds);
        for (int m = 0; m < M; ++m)
            for (int t = threadIdx.x; t < nb; t += blockDim.x) lb[m * nb + t] = xb[m * xs + t];
        for (int t = threadIdx.x; t < nb; t += blockDim.x) lb[M * nb + t] = yb[t];
        xb = lb, yb = lb + M * nb, xs = nb;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < nb; item += blockDim.x) {
        const int i = item / WW, w = item - i * WW, left = W - w * 64;
        const u64 valid = left >= 64 ? ~0ull : (1ull << left) - 1ull;
        const u64 o = fss_rel_dilate(yb, i, w, H, WW, r, valid);
        u64 s[FSS_MAX_NS];
#pragma unroll
        for (int b = 0; b < FSS_MAX_NS; ++b) s[b] = 0;
        for (int m = 0; m < M; ++m) {
            u64 carry = fss_rel_dilate(xb + m * xs, i, w, H, WW, r, valid);
#pragma unroll
            for (int b = 0; b < FSS_MAX_NS; ++b) {
                const u64 t = s[b] & carry;
                s[b] ^= carry;
                carry = t;
            }
        }
        for (int k = 0; k <= M; ++k) {
            u64 mk = valid;
#pragma unroll
            for (int b = 0; b < FSS_MAX_NS; ++b)
                if (b < NS) mk &= (k >> b) & 1 ? s[b] : ~s[b];
            if (mk == 0) continue;
            const unsigned n1 = __popcll(mk & o), n0 = __popcll(mk & ~o);
            if (n0) atomicAdd(&cnt[2 * k], n0);
            if (n1) atomicAdd(&cnt[2 * k + 1], n1);
        }
    }
    __syncthreads();
    long long *out = table + (q * gridDim.y + blockIdx.y) * 2 * (M + 1);
    for (int t = threadIdx.x; t < 2 * (M + 1); t += blockDim.x) out[t] = (long long)cnt[t];
}

extern "C" int acg_verif_version(void) { return ACG_VERIF_VERSION; }

// acg_fss's planes of x and of y, no slices: the members are added word by word in registers
extern "C" size_t acg_reliability_workspace_bytes(int rows, int x_per_y, int C, int H, int W, int T, int nw)
{
    return fss_shape_ok(rows, x_per_y, C, H, W, T, nw) ? fss_planes_bytes(rows, x_per_y, C, H, W, T, 0) : 0;
}

extern "C" int acg_reliability(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                               int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                               long long y_chan_stride, const float *thr, int T, const int *windows, int nw, long long *table,
                               void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_reliability";
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, FSS_MAX_M));
    ACG_REQUIRE(x != nullptr && y != nullptr && thr != nullptr && windows != nullptr && table != nullptr, "acg_reliability: null tensor");
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= FSS_MAX_HW && W <= FSS_MAX_HW,
                "acg_reliability: fields must be H x W with 1 <= H, W <= %d (got %d x %d)", FSS_MAX_HW, H, W);
    ACG_REQUIRE(T >= 1 && T <= FSS_MAX_T, "acg_reliability: need 1 <= T <= %d thresholds (T=%d)", FSS_MAX_T, T);
    ACG_REQUIRE(nw >= 1 && nw <= FSS_MAX_NW, "acg_reliability: need 1 <= nw <= %d windows (nw=%d)", FSS_MAX_NW, nw);
    ACG_REQUIRE((long long)rows * C * T <= 0x7fffffffLL && (long long)rows * H <= 0x7fffffffLL,
                "acg_reliability: too many planes (rows=%d, C=%d, T=%d, H=%d)", rows, C, T, H);
    FssWindows win;
    win.n = nw;
    for (int k = 0; k < FSS_MAX_NW; ++k) win.r[k] = 0;
    for (int k = 0; k < nw; ++k) {
        const int n = windows[k];
        ACG_REQUIRE(n >= 1 && n % 2 == 1 && n <= FSS_REL_MAX_WINDOW,
                    "acg_reliability: windows must be odd and lie in 1..%d (window %d is %d)", FSS_REL_MAX_WINDOW, k, n);
        win.r[k] = n / 2;
    }
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_reliability_workspace_bytes(rows, x_per_y, C, H, W, T, nw)));
    for (Field &o : f) o.mode = field_load_mode(o, C);
    hipStream_t st = (hipStream_t)stream;
    const int rows_y = rows / x_per_y, CT = C * T, NS = fss_slices(x_per_y);
    const size_t npx = (size_t)rows * CT, npy = (size_t)rows_y * CT;
    const FssSpace space = fss_carve(ws, npx, npy, 0, H, W);
    fss_events(st, f[0], rows, C, H, W, thr, T, space.px);
    fss_events(st, f[1], rows_y, C, H, W, thr, T, space.py);
    const size_t lds = (size_t)(x_per_y + 1) * H * fss_ww(W) * sizeof(u64);
    const bool resident = lds <= FSS_REL_LDS_MAX;
    if (resident)
        hipLaunchKernelGGL(fss_rel_kernel<true>, dim3((unsigned)npy, nw), dim3(FSS_REL_THREADS), lds, st, space.px, space.py, CT,
                           x_per_y, NS, H, W, win, table);
    else
        hipLaunchKernelGGL(fss_rel_kernel<false>, dim3((unsigned)npy, nw), dim3(FSS_REL_THREADS), 0, st, space.px, space.py, CT,
                           x_per_y, NS, H, W, win, table);
    acg_note_kernel("fss_events<%s> + fss_rel<%s>", f[0].mode == FIELD_C4 ? "c4" : "strided", resident ? "lds" : "global");
    ACG_CHECK_LAUNCH("acg_reliability");
    return ACG_OK;
}
