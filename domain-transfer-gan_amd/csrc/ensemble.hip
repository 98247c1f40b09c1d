// Ensemble statistics of M translations per input (model.translate_ensemble, test.py --metric ensemble): per cell
// (input, pixel, channel) the member mean, unbiased standard deviation and linear-rule quantiles and, against a paired target,
// the CRPS, the rank of the target among the members and the per-input sums the scores are derived from.
// Members are the generator's NHWC output with Cp stored channels (C valid, the rest ignored), member m of input n at row
// n*M + m.  One lane per cell: consecutive lanes take consecutive (pixel, channel) cells of one image, so a wave reads one
// contiguous stretch of every member row.  The M values of a cell are sorted in registers by a fully unrolled bitonic network
// on a compile-time bucket of M (8 / 16 / 32 / 64, padded with +inf); quantiles are picked with wave-uniform indices through
// unrolled selects.  The float sums go through per-block partials in the workspace, folded in a fixed order: no float
// atomics, results are bit-identical on a repeat.
#include <math.h>
#include "common.h"

#define ENS_THREADS 256
#define ENS_PIX 256                      // pixels of one input per block; the block walks their C cells in C steps of 256
#define ENS_MAX_M 64
#define ENS_MAX_Q 8
#define ENS_REC 72                       // workspace words per (input, block): 4 float sums, coverage, M + 1 rank bins, padding

struct EnsQuant {
    int lo[ENS_MAX_Q], hi[ENS_MAX_Q];    // floor / ceil of h = (M - 1) q
    float frac[ENS_MAX_Q];               // h - floor(h)
    int nq;
};

static inline long long ens_chunks(size_t npix) { return ((long long)npix + ENS_PIX - 1) / ENS_PIX; }

template <int MB>
__device__ __forceinline__ void ens_sort(float (&v)[MB])
{
    // bitonic network: every index is a compile-time constant once the three loops are unrolled
#pragma unroll
    for (int k = 2; k <= MB; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = v[i], b = v[l];
                    const bool up = (i & k) == 0;
                    v[i] = up ? fminf(a, b) : fmaxf(a, b);
                    v[l] = up ? fmaxf(a, b) : fminf(a, b);
                }
            }
        }
    }
}

// v[idx] for a wave-uniform idx without a runtime-indexed register array (which goes to scratch): a multiplexer tree over
// the bits of idx, MB - 1 selects.  idx passes through an empty volatile asm first, so that neither the per-bit conditions
// are hoisted out of the cell loop (one SGPR pair per bit, level and quantile) nor the tree is folded back into an indexed
// load from a stack copy of v.
template <int MB>
__device__ __forceinline__ float ens_pick(const float (&v)[MB], int idx)
{
    asm volatile("" : "+v"(idx));
    float t[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) t[i] = v[i];
#pragma unroll
    for (int w = MB / 2, b = 0; w > 0; w >>= 1, ++b) {
        const bool hi = (idx >> b) & 1;
#pragma unroll
        for (int i = 0; i < w; ++i) t[i] = hi ? t[2 * i + 1] : t[2 * i];
    }
    return t[0];
}

template <int MB, bool HAS_Y>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_stats_kernel(const float *__restrict__ x, const float *__restrict__ y, int M,
                                                                     long long npix, int C, int Cp, EnsQuant Q,
                                                                     float *__restrict__ mean, float *__restrict__ stdev,
                                                                     float *__restrict__ quant, float *__restrict__ crps_map,
                                                                     int nchunk, unsigned *__restrict__ ws)
{
    __shared__ float red[4][ENS_THREADS];
    __shared__ unsigned hist[ENS_MAX_M + 1], cover;
    const int n = blockIdx.y, tid = threadIdx.x;
    if (HAS_Y) {
        for (int r = tid; r <= M; r += ENS_THREADS) hist[r] = 0u;
        if (tid == 0) cover = 0u;
        __syncthreads();
    }
    const long long p0 = (long long)blockIdx.x * ENS_PIX;
    const long long row = (long long)npix * Cp;                    // floats per image
    const float *xn = x + (long long)n * M * row;
    const float invM = 1.f / (float)M;
    float s_e1 = 0.f, s_e2 = 0.f, s_sq = 0.f, s_var = 0.f;
    unsigned my_cover = 0u;
    for (int it = 0; it < C; ++it) {
        const int cell = it * ENS_THREADS + tid;                    // (pixel, channel) inside the block's chunk
        const int dp = cell / C, c = cell - dp * C;
        const long long p = p0 + dp;
        if (p >= npix) continue;
        const long long off = p * Cp + c;
        // Only the loads test m < M (M re-read per cell: hoisted out of the loop, the MB compares are MB SGPR pairs that
        // spill).  The other loops tell a pad by its +inf value, a lane compare consumed at once.
        int Mc = M;
        asm volatile("" : "+s"(Mc));
        float v[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) v[m] = m < Mc ? xn[(long long)m * row + off] : INFINITY;
        // the mean from the deviations of the first member, the variance around it in a second pass: equal members (a
        // degenerate ensemble) give exactly their value and exactly 0
        float sd = 0.f;
#pragma unroll
        for (int m = 1; m < MB; ++m) sd += v[m] != INFINITY ? v[m] - v[0] : 0.f;
        const float mu = v[0] + sd * invM;
        float ss = 0.f;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float d = v[m] != INFINITY ? v[m] - mu : 0.f;
            ss += d * d;
        }
        const float var = M > 1 ? ss / (float)(M - 1) : 0.f;
        // E1 and E2 are summed in double: their float sums of up to 64 terms drift past 1e-6 of the float64 reference
        float yv = 0.f, e1 = 0.f;
        unsigned lt = 0u, eq = 0u;
        if (HAS_Y) {
            yv = y[(long long)n * row + off];
            double e1s = 0.0;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                e1s += v[m] != INFINITY ? (double)fabsf(v[m] - yv) : 0.0;
                lt += v[m] < yv ? 1u : 0u;                           // a pad (+inf) is never below or equal to y
                eq += v[m] == yv ? 1u : 0u;
            }
            e1 = (float)(e1s / M);
        }
        ens_sort<MB>(v);
        const long long o = ((long long)n * C + c) * npix + p;     // NCHW
        if (mean) mean[o] = mu;
        if (stdev) stdev[o] = sqrtf(var);
        float qlo = 0.f, qhi = 0.f;
#pragma unroll
        for (int k = 0; k < ENS_MAX_Q; ++k) {
            if (k < Q.nq) {
                const float a = ens_pick<MB>(v, Q.lo[k]), b = ens_pick<MB>(v, Q.hi[k]);
                const float qv = a + Q.frac[k] * (b - a);
                if (quant) quant[(((long long)n * Q.nq + k) * C + c) * npix + p] = qv;
                if (k == 0) qlo = qv;
                qhi = qv;
            }
        }
        if (HAS_Y) {
            // E2 = (2/M^2) sum_i (2i - M - 1) x_(i) (1-based i), summed by gaps: the gap x_(k) - x_(k-1) (0-based) lies between
            // k (M - k) pairs, so the sum is sum_{0 < k < M} k (M - k) (x_(k) - x_(k-1)) — non-negative terms, static indices
            double e2s = 0.0;
#pragma unroll
            for (int k = 1; k < MB; ++k) e2s += v[k] != INFINITY ? (double)(k * (M - k)) * (double)(v[k] - v[k - 1]) : 0.0;
            const double e2d = e2s * 2.0 / ((double)M * M);
            const float e2 = (float)e2d;
            if (crps_map) crps_map[o] = (float)((double)e1 - 0.5 * e2d);
            const float d = mu - yv;
            s_e1 += e1;
            s_e2 += e2;
            s_sq += d * d;
            s_var += var;
            my_cover += (qlo <= yv && yv <= qhi) ? 1u : 0u;
            atomicAdd(&hist[lt + eq / 2u], 1u);                    // LDS integer counts
        }
    }
    if (!HAS_Y) return;
    red[0][tid] = s_e1;
    red[1][tid] = s_e2;
    red[2][tid] = s_sq;
    red[3][tid] = s_var;
    if (my_cover) atomicAdd(&cover, my_cover);
    __syncthreads();
    for (int k = ENS_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[j][tid] += red[j][tid + k];
        }
        __syncthreads();
    }
    unsigned *rec = ws + ((long long)n * nchunk + blockIdx.x) * ENS_REC;
    if (tid < 4) rec[tid] = __float_as_uint(red[tid][0]);
    if (tid == 4) rec[4] = cover;
    for (int r = tid; r <= M; r += ENS_THREADS) rec[5 + r] = hist[r];
}

// sums[n] and rank_hist[n] from the block records of input n, folded in block order (floats in double)
__global__ __launch_bounds__(128) void ensemble_fold_kernel(const unsigned *__restrict__ ws, int nchunk, int M, float cells,
                                                            float *__restrict__ sums, unsigned *__restrict__ rank_hist)
{
    const int n = blockIdx.x, j = threadIdx.x;
    const unsigned *rec = ws + (long long)n * nchunk * ENS_REC;
    if (j < 4) {
        double s = 0.0;
        for (int k = 0; k < nchunk; ++k) s += (double)__uint_as_float(rec[(long long)k * ENS_REC + j]);
        if (sums) sums[n * 6 + j] = (float)s;
    } else if (j < 5 + M + 1) {
        unsigned s = 0u;
        for (int k = 0; k < nchunk; ++k) s += rec[(long long)k * ENS_REC + j];
        if (j == 4) {
            if (sums) {
                sums[n * 6 + 4] = (float)s;
                sums[n * 6 + 5] = cells;
            }
        } else if (rank_hist) {
            rank_hist[(long long)n * (M + 1) + (j - 5)] = s;
        }
    }
}

extern "C" size_t acg_ensemble_workspace_bytes(int N, size_t npix)
{
    return (size_t)(N > 0 ? N : 0) * (size_t)ens_chunks(npix) * ENS_REC * sizeof(unsigned);
}

template <int MB>
static void ensemble_launch(bool has_y, dim3 grid, hipStream_t st, const float *x, const float *y, int M, long long npix, int C,
                            int Cp, const EnsQuant &Q, float *mean, float *stdev, float *quant, float *crps_map, int nchunk,
                            unsigned *ws)
{
    if (has_y)
        hipLaunchKernelGGL((ensemble_stats_kernel<MB, true>), grid, dim3(ENS_THREADS), 0, st, x, y, M, npix, C, Cp, Q, mean, stdev,
                           quant, crps_map, nchunk, ws);
    else
        hipLaunchKernelGGL((ensemble_stats_kernel<MB, false>), grid, dim3(ENS_THREADS), 0, st, x, y, M, npix, C, Cp, Q, mean,
                           stdev, quant, crps_map, nchunk, ws);
}

extern "C" int acg_ensemble_stats(const float *x, const float *y, int N, int M, size_t npix, int C, int Cp, const float *q, int nq,
                                  float *mean, float *stdev, float *quant, float *crps_map, float *sums, unsigned *rank_hist,
                                  void *ws, size_t ws_bytes, void *stream)
{
    ACG_REQUIRE(x != nullptr, "acg_ensemble_stats: null members");
    ACG_REQUIRE(N >= 1 && npix >= 1, "acg_ensemble_stats: empty tensor (N=%d, npix=%zu)", N, npix);
    ACG_REQUIRE(M >= 1 && M <= ENS_MAX_M, "acg_ensemble_stats: need 1 <= M <= %d (M=%d)", ENS_MAX_M, M);
    ACG_REQUIRE((Cp == 4 || (Cp >= 16 && Cp % 16 == 0)) && C >= 1 && C <= Cp,
                "acg_ensemble_stats: need 1 <= C <= Cp, Cp 4 or a multiple of 16 (C=%d, Cp=%d)", C, Cp);
    ACG_REQUIRE(q != nullptr && nq >= 1 && nq <= ENS_MAX_Q, "acg_ensemble_stats: need 1 <= nq <= %d levels (nq=%d)", ENS_MAX_Q, nq);
    for (int k = 0; k < nq; ++k) {
        ACG_REQUIRE(q[k] >= 0.f && q[k] <= 1.f, "acg_ensemble_stats: quantile level %g outside [0, 1]", (double)q[k]);
        ACG_REQUIRE(k == 0 || q[k] >= q[k - 1], "acg_ensemble_stats: quantile levels must be sorted");
    }
    ACG_REQUIRE(y != nullptr || (crps_map == nullptr && sums == nullptr && rank_hist == nullptr),
                "acg_ensemble_stats: crps_map, sums and rank_hist need the target y");
    const long long nchunk = ens_chunks(npix);
    ACG_REQUIRE(nchunk <= 0x7fffffffLL && N <= 65535 && (long long)C * ENS_THREADS < 0x7fffffffLL,
                "acg_ensemble_stats: too large (N=%d, npix=%zu)", N, npix);
    if (y != nullptr && (ws == nullptr || ws_bytes < acg_ensemble_workspace_bytes(N, npix))) {
        acg_set_error("acg_ensemble_stats: workspace too small (%zu < %zu)", ws_bytes, acg_ensemble_workspace_bytes(N, npix));
        return ACG_ERR_WORKSPACE;
    }
    EnsQuant Q;
    for (int k = 0; k < ENS_MAX_Q; ++k) {
        const double h = k < nq ? (double)(M - 1) * (double)q[k] : 0.0;
        Q.lo[k] = (int)floor(h);
        Q.hi[k] = (int)ceil(h);
        Q.frac[k] = (float)(h - floor(h));
    }
    Q.nq = nq;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nchunk, (unsigned)N);
    const bool has_y = y != nullptr;
    unsigned *w = (unsigned *)ws;
    if (M <= 8)
        ensemble_launch<8>(has_y, grid, st, x, y, M, (long long)npix, C, Cp, Q, mean, stdev, quant, crps_map, (int)nchunk, w);
    else if (M <= 16)
        ensemble_launch<16>(has_y, grid, st, x, y, M, (long long)npix, C, Cp, Q, mean, stdev, quant, crps_map, (int)nchunk, w);
    else if (M <= 32)
        ensemble_launch<32>(has_y, grid, st, x, y, M, (long long)npix, C, Cp, Q, mean, stdev, quant, crps_map, (int)nchunk, w);
    else
        ensemble_launch<64>(has_y, grid, st, x, y, M, (long long)npix, C, Cp, Q, mean, stdev, quant, crps_map, (int)nchunk, w);
    if (has_y && (sums != nullptr || rank_hist != nullptr))
        hipLaunchKernelGGL(ensemble_fold_kernel, dim3(N), dim3(128), 0, st, (const unsigned *)w, (int)nchunk, M,
                           (float)((double)C * (double)npix), sums, rank_hist);
    ACG_CHECK_LAUNCH("acg_ensemble_stats");
    return ACG_OK;
}
