// Streaming per-cell statistics of an ensemble against its truth (ops.cell_stats, --metric ensemble --ens_maps 1;
// tests/cell_stats_ref.py states the definition, include/acgan_cell.h repeats it).  x holds rows = Ny M fields, member m of truth
// n at row n M + m (acg_ensemble_stats's order, x_per_y = M), y the Ny truths.  The state (mom, evt, hist_x, hist_y) is planar,
// one value per cell and plane, and every call adds to it.
//
// Ownership: one thread owns a cell for a whole launch.  It reads the cell's running sums from the state, walks the truth rows
// in ascending order and inside each the members in ascending order, and writes the sums back with plain stores: no atomics,
// no workspace, and the same bits whatever the split of the rows into calls or launches.  The lanes of a wave own neighbouring
// pixels, so the planar state and planar operands are read and written 256 or 512 bytes per wave and access.  Where an operand
// is an NHWC pixel of four stored channels on the 16-byte grid (FIELD_C4) the thread carries the pixel's channels and reads
// them with one 16-byte load per row; the other operand is then read channel by channel.  Otherwise a thread carries one
// channel.  What is loaded at once never changes the order of a sum.
//
// Three kernels, each a pass over the input (DESIGN.md §21 has the numbers):
//   cell_mom   the nine double sums; the members of a truth are loaded eight at a time before the first is used
//   cell_evt   (T > 0) per threshold the counts (k, o, k o, k k) in 32-bit registers, at most 2^19 truth rows per launch
//              (64^2 2^19 = 2^31), added to the 64-bit state at the end
//   cell_hist  (E > 0) one operand: private 16-bit counters in LDS laid out [channel][bin][thread], at most 65535 rows per
//              launch, one coalesced read-modify-write of the state per bin at the end; the bin #{e : edge_e <= v} by a
//              branch-free binary search of the ascending edges, which sit in LDS (a NaN compares false: bin 0)
//
// The file is compiled without floating-point contraction: every line of the definition is one rounded double operation.
#include "common.h"
#include "field.h"
#include "../../include/acgan_cell.h"
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

constexpr int CL_THREADS = 256, CL_MAX_HW = 1024, CL_MAX_M = 64, CL_MAX_T = 8, CL_MAX_E = 63;
constexpr int CL_UNROLL = 8;                       // member rows in flight per thread
constexpr int CL_EVT_ROWS = 1 << 19;               // truth rows per cell_evt launch: k k <= 4096 summed in 32 bits
constexpr int CL_HIST_ROWS = 65535;                // rows per cell_hist launch: 16-bit counters
constexpr int CL_HIST_LDS = 32 * 1024;             // of counters per workgroup

// the values of the thread's channels in pixel `cell` of row `row`: C4 one 16-byte load (NC = 4), else nc strided loads
template <bool C4, int NC>
__device__ __forceinline__ void cl_load(const Field &f, long long row, int cell, int c0, int nc, float (&v)[NC])
{
    const float *__restrict__ p = f.x + row * f.row;
    if constexpr (C4) {
        const float4 q = reinterpret_cast<const float4 *>(p)[cell];
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = c < nc ? p[(long long)(c0 + c) * f.chan + (long long)cell * f.pix] : 0.f;
    }
}

// blockIdx.x = channel group * blocks per plane + block of the plane -> the thread's pixel and first channel
template <int NC>
__device__ __forceinline__ int cl_owner(int HW, int C, int &c0, int &nc)
{
    const unsigned per = (unsigned)(HW + CL_THREADS - 1) / CL_THREADS, g = blockIdx.x / per;
    c0 = NC == 4 ? 0 : (int)g;
    nc = NC == 4 ? C : 1;
    return (int)(blockIdx.x - g * per) * CL_THREADS + (int)threadIdx.x;
}

template <bool XC4, bool YC4>
__global__ __launch_bounds__(CL_THREADS) void cell_mom_kernel(Field x, Field y, int Ny, int M, int C, int HW, double *__restrict__ mom)
{
    constexpr int NC = (XC4 || YC4) ? 4 : 1;
    int c0, nc;
    const int cell = cl_owner<NC>(HW, C, c0, nc);
    if (cell >= HW) return;
    double a[NC][9];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int p = 0; p < 9; ++p) a[c][p] = c < nc ? mom[((long long)p * C + c0 + c) * HW + cell] : 0.0;
    const double Md = (double)M;
    for (int n = 0; n < Ny; ++n) {
        float yf[NC];
        cl_load<YC4, NC>(y, n, cell, c0, nc, yf);
        double yv[NC], S[NC], Q[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            yv[c] = (double)yf[c];
            a[c][2] += yv[c];
            a[c][3] += yv[c] * yv[c];
            S[c] = 0.0, Q[c] = 0.0;
        }
        for (int m0 = 0; m0 < M; m0 += CL_UNROLL) {
            float xf[CL_UNROLL][NC];
#pragma unroll
            for (int u = 0; u < CL_UNROLL; ++u)
                if (m0 + u < M) cl_load<XC4, NC>(x, (long long)n * M + m0 + u, cell, c0, nc, xf[u]);
#pragma unroll
            for (int u = 0; u < CL_UNROLL; ++u) {
                if (m0 + u >= M) continue;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double xv = (double)xf[u][c];
                    const double xx = xv * xv;
                    a[c][0] += xv;
                    a[c][1] += xx;
                    a[c][4] += xv * yv[c];
                    a[c][5] += fabs(xv - yv[c]);
                    S[c] += xv;
                    Q[c] += xx;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double u = S[c] * S[c];
            a[c][6] += u;
            a[c][7] += S[c] * yv[c];
            const double t = Md * Q[c];
            const double v = t - u;
            a[c][8] += v;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int p = 0; p < 9; ++p)
            if (c < nc) mom[((long long)p * C + c0 + c) * HW + cell] = a[c][p];
}

template <bool XC4, bool YC4>
__global__ __launch_bounds__(CL_THREADS) void cell_evt_kernel(Field x, Field y, int Ny, int M, int C, int HW,
                                                            const float *__restrict__ thr, int T, long long *__restrict__ evt)
{
    constexpr int NC = (XC4 || YC4) ? 4 : 1;
    int c0, nc;
    const int cell = cl_owner<NC>(HW, C, c0, nc);
    if (cell >= HW) return;
    float th[NC][CL_MAX_T];
    unsigned acc[NC][CL_MAX_T][4];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int t = 0; t < CL_MAX_T; ++t) {
            th[c][t] = (c < nc && t < T) ? thr[(c0 + c) * T + t] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[c][t][q] = 0u;
        }
    for (int n = 0; n < Ny; ++n) {
        float yf[NC];
        cl_load<YC4, NC>(y, n, cell, c0, nc, yf);
        unsigned k[NC][CL_MAX_T];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int t = 0; t < CL_MAX_T; ++t) k[c][t] = 0u;
        for (int m0 = 0; m0 < M; m0 += CL_UNROLL) {
            float xf[CL_UNROLL][NC];
#pragma unroll
            for (int u = 0; u < CL_UNROLL; ++u)
                if (m0 + u < M) cl_load<XC4, NC>(x, (long long)n * M + m0 + u, cell, c0, nc, xf[u]);
#pragma unroll
            for (int u = 0; u < CL_UNROLL; ++u) {
                if (m0 + u >= M) continue;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int t = 0; t < CL_MAX_T; ++t)
                        if (t < T) k[c][t] += xf[u][c] >= th[c][t] ? 1u : 0u;      // float32; NaN compares false: no event
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int t = 0; t < CL_MAX_T; ++t) {
                if (t >= T) continue;
                const unsigned o = yf[c] >= th[c][t] ? 1u : 0u;
                acc[c][t][0] += k[c][t];
                acc[c][t][1] += o;
                acc[c][t][2] += o ? k[c][t] : 0u;
                acc[c][t][3] += k[c][t] * k[c][t];
            }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int t = 0; t < CL_MAX_T; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c < nc && t < T) evt[(((long long)(c0 + c) * T + t) * 4 + q) * HW + cell] += (long long)acc[c][t][q];
}

// LDS: NC rows of 64 edges, then the counters [channel][bin][thread]
template <bool C4>
__global__ __launch_bounds__(CL_THREADS) void cell_hist_kernel(Field x, int rows, int C, int HW, const float *__restrict__ edges,
                                                             int E, int *__restrict__ hist)
{
    constexpr int NC = C4 ? 4 : 1;
    extern __shared__ __align__(16) unsigned char cl_smem[];
    float *ed = reinterpret_cast<float *>(cl_smem);
    unsigned short *cnt = reinterpret_cast<unsigned short *>(cl_smem + NC * 64 * sizeof(float));
    const int threads = (int)blockDim.x, tid = (int)threadIdx.x, nb = E + 1;
    const unsigned per = (unsigned)(HW + threads - 1) / threads, g = blockIdx.x / per;
    const int c0 = NC == 4 ? 0 : (int)g, nc = NC == 4 ? C : 1;
    const int cell = (int)(blockIdx.x - g * per) * threads + tid;
    const bool active = cell < HW;
    for (int i = tid; i < nc * E; i += threads) ed[(i / E) * 64 + i % E] = edges[(long long)(c0 + i / E) * E + i % E];
    for (int i = 0; i < nc * nb; ++i) cnt[i * threads + tid] = 0;
    __syncthreads();
    if (!active) return;
    for (int r0 = 0; r0 < rows; r0 += CL_UNROLL) {
        float xf[CL_UNROLL][NC];
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u)
            if (r0 + u < rows) cl_load<C4, NC>(x, r0 + u, cell, c0, nc, xf[u]);
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) {
            if (r0 + u >= rows) continue;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (c >= nc) continue;
                const float v = xf[u][c];
                int b = 0;                                         // the largest b <= E with edge[b - 1] <= v
#pragma unroll
                for (int step = 32; step; step >>= 1) {
                    const int j = b + step;
                    if (j <= E && ed[c * 64 + j - 1] <= v) b = j;
                }
                cnt[(c * nb + b) * threads + tid] += 1;
            }
        }
    }
    for (int c = 0; c < nc; ++c)
        for (int b = 0; b < nb; ++b) hist[((long long)(c0 + c) * nb + b) * HW + cell] += (int)cnt[(c * nb + b) * threads + tid];
}

extern "C" int acg_cell_version(void) { return ACG_CELL_VERSION; }

static void cl_hist(hipStream_t st, Field f, int rows, int C, int HW, const float *edges, int E, int *hist)
{
    const int NC = f.mode == FIELD_C4 ? 4 : 1;
    int threads = CL_THREADS;
    while (threads > 64 && (size_t)NC * (E + 1) * threads * sizeof(unsigned short) > CL_HIST_LDS) threads >>= 1;
    const size_t lds = (size_t)NC * 64 * sizeof(float) + (size_t)NC * (E + 1) * threads * sizeof(unsigned short);
    const unsigned blocks = (unsigned)acg_cdiv(HW, threads) * (unsigned)(NC == 4 ? 1 : C);
    for (int r0 = 0; r0 < rows; r0 += CL_HIST_ROWS) {
        const int nr = rows - r0 < CL_HIST_ROWS ? rows - r0 : CL_HIST_ROWS;
        Field g = f;
        g.x += (long long)r0 * f.row;
        if (NC == 4)
            hipLaunchKernelGGL(cell_hist_kernel<true>, dim3(blocks), dim3(threads), lds, st, g, nr, C, HW, edges, E, hist);
        else
            hipLaunchKernelGGL(cell_hist_kernel<false>, dim3(blocks), dim3(threads), lds, st, g, nr, C, HW, edges, E, hist);
    }
}

extern "C" int acg_cell_stats(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                              int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride,
                              long long y_chan_stride, const float *thr, int T, const float *edges, int E, double *mom,
                              long long *evt, int *hist_x, int *hist_y, void *stream)
{
    const char *fn = "acg_cell_stats";
    Field f[2] = {{x, x_row_stride, x_chan_stride, x_pix_stride, FIELD_SCALAR}, {y, y_row_stride, y_chan_stride, y_pix_stride, FIELD_SCALAR}};
    FIELD_CHECK(field_refuse_operands(fn, rows, C, f, 2));
    FIELD_CHECK(field_refuse_pairing(fn, rows, x_per_y, CL_MAX_M));
    ACG_REQUIRE(x != nullptr && y != nullptr && mom != nullptr, "acg_cell_stats: null tensor (x, y or mom)");
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= CL_MAX_HW && W <= CL_MAX_HW && (long long)acg_cdiv((long)H * W, 64) * C <= 0x7fffffffLL,
                "acg_cell_stats: fields must be H x W with 1 <= H, W <= %d and fewer than 2^31 workgroups (got %d x %d, C=%d)",
                CL_MAX_HW, H, W, C);
    ACG_REQUIRE(T >= 0 && T <= CL_MAX_T && (T == 0 || (thr != nullptr && evt != nullptr)),
                "acg_cell_stats: need 0 <= T <= %d thresholds, and thr and evt with T > 0 (T=%d)", CL_MAX_T, T);
    ACG_REQUIRE(E >= 0 && E <= CL_MAX_E && (E == 0 || (edges != nullptr && hist_x != nullptr && hist_y != nullptr)),
                "acg_cell_stats: need 0 <= E <= %d edges, and edges, hist_x and hist_y with E > 0 (E=%d)", CL_MAX_E, E);
    ACG_REQUIRE((uintptr_t)mom % sizeof(double) == 0 && (T == 0 || (uintptr_t)evt % sizeof(long long) == 0) &&
                    (E == 0 || ((uintptr_t)hist_x % sizeof(int) == 0 && (uintptr_t)hist_y % sizeof(int) == 0)),
                "acg_cell_stats: a state buffer is not aligned to its element size");
    for (Field &o : f) o.mode = field_load_mode(o, C);
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, M = x_per_y, Ny = rows / M;
    const bool xc4 = f[0].mode == FIELD_C4, yc4 = f[1].mode == FIELD_C4;
    const unsigned blocks = (unsigned)acg_cdiv(HW, CL_THREADS) * (unsigned)((xc4 || yc4) ? 1 : C);
#define CL_PAIR(kernel, ...)                                                                                                  \
    do {                                                                                                                      \
        if (xc4 && yc4) hipLaunchKernelGGL((kernel<true, true>), dim3(blocks), dim3(CL_THREADS), 0, st, __VA_ARGS__);         \
        else if (xc4) hipLaunchKernelGGL((kernel<true, false>), dim3(blocks), dim3(CL_THREADS), 0, st, __VA_ARGS__);          \
        else if (yc4) hipLaunchKernelGGL((kernel<false, true>), dim3(blocks), dim3(CL_THREADS), 0, st, __VA_ARGS__);          \
        else hipLaunchKernelGGL((kernel<false, false>), dim3(blocks), dim3(CL_THREADS), 0, st, __VA_ARGS__);                  \
    } while (0)
    CL_PAIR(cell_mom_kernel, f[0], f[1], Ny, M, C, HW, mom);
    for (int n0 = 0; T > 0 && n0 < Ny; n0 += CL_EVT_ROWS) {
        Field gx = f[0], gy = f[1];
        gx.x += (long long)n0 * M * gx.row;
        gy.x += (long long)n0 * gy.row;
        CL_PAIR(cell_evt_kernel, gx, gy, Ny - n0 < CL_EVT_ROWS ? Ny - n0 : CL_EVT_ROWS, M, C, HW, thr, T, evt);
    }
#undef CL_PAIR
    if (E > 0) {
        cl_hist(st, f[0], rows, C, HW, edges, E, hist_x);
        cl_hist(st, f[1], Ny, C, HW, edges, E, hist_y);
    }
    acg_note_kernel("cell_mom<%s, %s>%s%s", xc4 ? "c4" : "strided", yc4 ? "c4" : "strided", T > 0 ? " + cell_evt" : "",
                    E > 0 ? " + cell_hist" : "");
    ACG_CHECK_LAUNCH("acg_cell_stats");
    return ACG_OK;
}
