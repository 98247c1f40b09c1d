// Minkowski functionals of excursion sets (ops.minkowski, model.translate_minkowski, test.py --metric minkowski;
// tests/minkowski_ref.py states the definition).  Per field x, channel c and the T non-decreasing thresholds thr[c][.]: the
// level of a pixel is L = #{t : thr[c][t] <= x} in 0 .. T (NaN: 0, the event convention of fss.hip), the excursion set at
// threshold t is {L >= t + 1}, and the field stands in a ring of level-0 cells.  Five multisets of levels - the pixels (F), the
// max / min over the two pixels of every unit edge (Emax, Emin) and over the four pixels of every vertex (Vmax, Vmin) - give,
// as (T + 1)-bin histograms followed by a suffix sum, the counts (nF, nE1, nE2, nV1, nV4) of faces, edges and vertices that
// touch the set / lie inside it, at all T thresholds from ONE pass over the field: area = nF, perimeter = nE1 - nE2,
// euler8 = nV1 - nE1 + nF, euler4 = nF - nE2 + nV4.  Everything after the comparison is integer: exact, the same bits in every
// layout and launch order.
//   hist    one workgroup per (field row, band of MK_BAND lattice rows [, channel]); C4 NHWC: all channels of a pixel from one
//           16-byte load, otherwise blockIdx carries the channel.  The channel's thresholds go into LDS and each pixel's level
//           comes from a branch-free bisection over them (log2 T steps); the band's levels go into an LDS byte tile of MK_BAND + 1 rows (the
//           row above the band is recomputed: bands are independent) by W + 2 columns (the ring).  Then one thread per corner
//           cell (i, j) of the (H + 1) x (W + 1) lattice, which owns pixel (i, j), the edge on its left, the edge above it and
//           the vertex at its top left; the lattice's last row and column hold ring cells only, whose levels are 0, so every
//           face, edge and vertex is counted once and no case needs a branch.  The histograms are u32 bins in LDS, bin 0 is
//           never added to.  Adds are aggregated over runs of equal levels in neighbouring lanes (one DPP shift, one ballot):
//           the head of a run adds the run's length with one LDS atomic, so a constant field costs four atomics per wave where
//           it would serialise 64, and a smooth field a few.  Integer adds: the order cannot show.  The workgroup stores its
//           5 T bins to the workspace with plain stores.
//   finish  one workgroup per (field row, channel): sums the bands' bins (a thread per bin), takes the suffix sums (a wave per
//           set) and stores the int64 counts.  No global atomics; nothing depends on what the outputs or the workspace held before.
#include "common.h"
#include "field.h"
#include <stdint.h>

#define MK_MAX_HW 1024
#define MK_MAX_T 255
#define MK_BAND 8
#define MK_THREADS 256
#define MK_SETS 5                          // F, Emax, Emin, Vmax, Vmin

typedef unsigned long long u64;

static inline int mk_bands(int H) { return (H + 1 + MK_BAND - 1) / MK_BAND; }
__host__ __device__ static inline int mk_tile_stride(int W) { return (W + 2 + 3) & ~3; }
// the dynamic LDS of a hist workgroup serving nc channels: thresholds, bins 0 .. T of the five sets, the level tile
static inline size_t mk_lds_bytes(int nc, int W, int T)
{
    return (size_t)nc * T * sizeof(float) + (size_t)nc * MK_SETS * (T + 1) * sizeof(unsigned) + (size_t)nc * (MK_BAND + 1) * mk_tile_stride(W);
}

// #{t : thr[t] <= x} for non-decreasing thr[0 .. T - 1]: a bisection without a branch, from s0 = the largest power of two <= T
// down (5 steps at T = 31, 8 at 255; the trip count is uniform); NaN compares false everywhere: 0
__device__ __forceinline__ int mk_level(const float *thr, int T, int s0, float x)
{
    int pos = 0;
    for (int s = s0; s > 0; s >>= 1) {
        const int k = pos + s;
        if (k <= T && thr[k - 1] <= x) pos = k;
    }
    return pos;
}

// hist[v] += 1 from every lane of a full wave, v in 0 .. T; bin 0 is skipped.  Lanes that follow a lane of the same v leave
// their add to the head of their run, which adds the run's length.  The neighbour's v comes by a DPP shift inside rows of 16
// lanes (row_shr:1, a VALU move: no LDS traffic), so a run ends at a row's end: at most four atomics a wave on a constant field.
__device__ __forceinline__ void mk_add(unsigned *hist, int v)
{
    const int lane = threadIdx.x & 63;
    const int prev = __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false);   // lane l - 1's v; a row's first lane keeps its own
    const bool head = (lane & 15) == 0 || prev != v;
    const u64 heads = __ballot(head);
    if (head && v != 0) {
        // the run's length: the distance to the next head of this row of 16 lanes, or to the row's end (the bit put at 16)
        const unsigned h32 = lane < 32 ? (unsigned)heads : (unsigned)(heads >> 32);
        const unsigned row = ((h32 >> (lane & 16)) & 0xffffu) | 0x10000u;
        atomicAdd(hist + v, (unsigned)__ffs((int)(row >> ((lane & 15) + 1))));
    }
}

// One workgroup per blockIdx.x = (g, band), g = the field row (C4: channels 0 .. C - 1 of FIELD_C4 pixels) or (field row,
// channel).  part: (rows, C, nb, 5, T) bins 1 .. T of the band's histograms, fully written.
template <bool C4>
__global__ __launch_bounds__(MK_THREADS) void mink_hist_kernel(Field x, int C, int H, int W, int nb, const float *__restrict__ thr, int T,
                                                              unsigned *__restrict__ part)
{
    constexpr int NC = C4 ? 4 : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char mk_lds[];
    const int nc = C4 ? C : 1, TS = mk_tile_stride(W), tid = threadIdx.x, s0 = 1 << (31 - __clz(T));
    float *sthr = reinterpret_cast<float *>(mk_lds);
    unsigned *hist = reinterpret_cast<unsigned *>(sthr + nc * T);
    unsigned char *tile = reinterpret_cast<unsigned char *>(hist + nc * MK_SETS * (T + 1));
    const long long g = blockIdx.x / nb;
    const int b = (int)(blockIdx.x - g * nb);
    const long long f = C4 ? g : g / C;
    const int c0 = C4 ? 0 : (int)(g - f * C);
    const int i0 = b * MK_BAND, nr = min(MK_BAND, H + 1 - i0);     // lattice rows i0 .. i0 + nr - 1
    for (int k = tid; k < nc * T; k += MK_THREADS) sthr[k] = thr[c0 * T + k];
    for (int k = tid; k < nc * MK_SETS * (T + 1); k += MK_THREADS) hist[k] = 0;
    __syncthreads();
    // tile row r holds pixel row i0 - 1 + r, tile column q pixel column q - 1; outside the domain the level is 0
    const float *__restrict__ xf = x.x + f * x.row + (C4 ? 0 : (long long)c0 * x.chan);
    for (int k = tid; k < (nr + 1) * TS; k += MK_THREADS) {        // k = r TS + q, the cell's place in a channel's tile
        const int r = k / TS, q = k - r * TS, i = i0 - 1 + r, j = q - 1;
        const bool in = i >= 0 && i < H && j >= 0 && j < W;
        const long long p = (long long)i * W + j;
        if constexpr (C4) {
            const float4 v = in ? reinterpret_cast<const float4 *>(xf)[p] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nc) tile[c * (MK_BAND + 1) * TS + k] = (unsigned char)(in ? mk_level(sthr + c * T, T, s0, field_pick(v, c)) : 0);
        } else {
            tile[k] = (unsigned char)(in ? mk_level(sthr, T, s0, xf[p * x.pix]) : 0);
        }
    }
    __syncthreads();
    // corner cell (i0 + r, j): a b over c d are the levels of pixels (i - 1, j - 1), (i - 1, j), (i, j - 1), (i, j)
    const int cells = nr * (W + 1);
    for (int base = 0; base < cells; base += MK_THREADS) {         // whole waves: mk_add shuffles and ballots
        const int k = base + tid;
        const bool ok = k < cells;
        const int r = ok ? k / (W + 1) : 0, j = ok ? k - r * (W + 1) : 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c >= nc) continue;
            const unsigned char *t0 = tile + (c * (MK_BAND + 1) + r) * TS + j;
            const int a = ok ? t0[0] : 0, bb = ok ? t0[1] : 0, cc = ok ? t0[TS] : 0, d = ok ? t0[TS + 1] : 0;
            unsigned *h = hist + c * MK_SETS * (T + 1);
            mk_add(h, d);
            mk_add(h + (T + 1), max(cc, d));
            mk_add(h + (T + 1), max(bb, d));
            mk_add(h + 2 * (T + 1), min(cc, d));
            mk_add(h + 2 * (T + 1), min(bb, d));
            mk_add(h + 3 * (T + 1), max(max(a, bb), max(cc, d)));
            mk_add(h + 4 * (T + 1), min(min(a, bb), min(cc, d)));
        }
    }
    __syncthreads();
    for (int k = tid; k < nc * MK_SETS * T; k += MK_THREADS) {
        const int c = k / (MK_SETS * T), rem = k - c * (MK_SETS * T), s = rem / T, l = rem - s * T;
        part[((((long long)f * C + c0 + c) * nb + b) * MK_SETS + s) * T + l] = hist[(c * MK_SETS + s) * (T + 1) + l + 1];
    }
}

// One workgroup per g = (field row, channel): out[g][t][s] = sum over the bands and the levels l >= t + 1 of set s's bins.
// The band sums: one thread per bin, the bands' loads independent of each other; the suffix sums: one wave per set, a lane
// holding four neighbouring bins, a shuffle scan over the lanes' totals.
__global__ __launch_bounds__(MK_THREADS) void mink_finish_kernel(const unsigned *__restrict__ part, int nb, int T, long long *__restrict__ out)
{
    __shared__ unsigned sm[MK_SETS][MK_THREADS];
    const int tid = threadIdx.x, lane = tid & 63;
    const long long g = blockIdx.x;
    const unsigned *__restrict__ p = part + g * nb * MK_SETS * T;
    for (int k = tid; k < MK_SETS * MK_THREADS; k += MK_THREADS) (&sm[0][0])[k] = 0;
    __syncthreads();
    for (int k = tid; k < MK_SETS * T; k += MK_THREADS) {
        unsigned v = 0;                                            // a field's counts stay below 2^32 (2 * 1025^2 at most)
#pragma unroll 8
        for (int b = 0; b < nb; ++b) v += p[(long long)b * MK_SETS * T + k];
        const int s = k / T;
        sm[s][k - s * T] = v;
    }
    __syncthreads();
    for (int s = tid >> 6; s < MK_SETS; s += MK_THREADS / 64) {
        unsigned a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = sm[s][4 * lane + i];
        a[2] += a[3], a[1] += a[2], a[0] += a[1];                  // within the lane; a[0] is the lane's total
        unsigned run = a[0];                                       // the totals of this lane and the lanes above it
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_down(run, off);
            if (lane + off < 64) run += o;
        }
        const unsigned above = run - a[0];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = 4 * lane + i;
            if (t < T) out[(g * T + t) * MK_SETS + s] = (long long)(a[i] + above);
        }
    }
}

static bool mk_shape_ok(int rows, int C, int H, int W, int T)
{
    return rows >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= MK_MAX_HW && W <= MK_MAX_HW && T >= 1 && T <= MK_MAX_T &&
           (long long)rows * C * mk_bands(H) <= 0x7fffffffLL && (long long)rows * C * T <= 0x7fffffffLL;
}

// the bands' histograms: (rows, C, bands, 5, T) 32-bit bins
extern "C" size_t acg_minkowski_workspace_bytes(int rows, int C, int H, int W, int T)
{
    if (!mk_shape_ok(rows, C, H, W, T)) return 0;
    return acg_round_up((size_t)rows * C * mk_bands(H) * MK_SETS * T * sizeof(unsigned), 16);
}

extern "C" int acg_minkowski(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                             const float *thr, int T, long long *out, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_minkowski";
    ACG_REQUIRE(x != nullptr && thr != nullptr && out != nullptr, "acg_minkowski: null tensor");
    Field f = {x, row_stride, chan_stride, pix_stride, FIELD_SCALAR};
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= MK_MAX_HW && W <= MK_MAX_HW, "acg_minkowski: fields must be H x W with 1 <= H, W <= %d (got %d x %d)",
                MK_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(T >= 1 && T <= MK_MAX_T, "acg_minkowski: need 1 <= T <= %d thresholds (T=%d)", MK_MAX_T, T);
    ACG_REQUIRE(mk_shape_ok(rows, C, H, W, T), "acg_minkowski: too many planes (rows=%d, C=%d, T=%d, H=%d)", rows, C, T, H);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, &f, 1));
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, acg_minkowski_workspace_bytes(rows, C, H, W, T)));
    f.mode = field_load_mode(f, C);
    hipStream_t st = (hipStream_t)stream;
    const int nb = mk_bands(H);
    unsigned *part = (unsigned *)ws;
    if (f.mode == FIELD_C4)
        hipLaunchKernelGGL(mink_hist_kernel<true>, dim3((unsigned)((long long)rows * nb)), dim3(MK_THREADS), mk_lds_bytes(C, W, T), st, f, C,
                           H, W, nb, thr, T, part);
    else
        hipLaunchKernelGGL(mink_hist_kernel<false>, dim3((unsigned)((long long)rows * C * nb)), dim3(MK_THREADS), mk_lds_bytes(1, W, T), st,
                           f, C, H, W, nb, thr, T, part);
    hipLaunchKernelGGL(mink_finish_kernel, dim3((unsigned)((long long)rows * C)), dim3(MK_THREADS), 0, st, part, nb, T, out);
    acg_note_kernel("mink_hist<%s> + mink_finish", f.mode == FIELD_C4 ? "c4" : "strided");
    ACG_CHECK_LAUNCH("acg_minkowski");
    return ACG_OK;
}
