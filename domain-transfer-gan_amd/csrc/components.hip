// Connected components of excursion sets (ops.components, model.translate_minkowski(components=), test.py --metric minkowski
// --mink_components; tests/components_ref.py states the definition).  A plane is one (field row, channel c, threshold t); its set
// is [x >= thr[c][t]] (x == thr inside, NaN outside, cells beyond the field outside: acg_minkowski's conventions).  Per plane the
// components of the set under 4- or 8-connectivity are labelled with a union-find forest over the H W cells and COMP_STATS int64
// values are written: n, area, sum of area^2, n_border, and the 21 bins of floor(log2(area)).
//   The forest: lab[i] is the row-major index of a cell of i's component that is <= i (-1 outside the set); a root has
// lab[i] == i.  A parent is always SMALLER than its child, so every chase strictly descends and ends, and the root of a finished
// tree is its component's first cell in row-major order: the labels are canonical and no result depends on arrival order.  A
// union finds both roots and hooks the larger under the smaller with a compare-and-swap that succeeds only while the larger
// still is a root; when it fails another lane has hooked that root, the chase goes on from its new (smaller) parent: a retry
// means another lane made progress and the larger of the two indices has fallen, so the loop ends.  Nothing ever waits.
//   label   one workgroup per (group of planes, CC_TH x CC_TW tile); a thread keeps its CC_PER consecutive cells of a tile row in
//           registers (C4 NHWC: all channels of a pixel from one 16-byte load, the group is the field row; otherwise the group is
//           (field row, channel)) and the workgroup walks the planes of its group that the pass holds.  Per plane: the forest of
//           the tile in LDS (runs inside a thread start linked; unions with the left, upper and, for 8-connectivity, diagonal
//           neighbours where no other cell's union already implies them), flattened, areas and border flags reduced per tile root
//           in LDS; then plain stores of lab (global indices) and acc (the tile root's area, bit 31: touches the border; 0 for
//           every other cell) for the whole tile, and zeros into the plane's out by tile 0.
//   merge   one thread per cell of a tile's first row / column: unions across the seam (the diagonals across it and across tile
//           corners for 8-connectivity).  Workgroups share lab here, so EVERY access to it is an agent-scope atomic (load, min,
//           compare-and-swap): L1 is bypassed and the L2s agree.  Only roots are hooked, so a tile root's parents stay tile roots.
//   root    one thread per cell: a tile root (acc != 0) finds its component's root r, points lab at it (atomic min) and adds its
//           area and border flag into acc[r] (integer atomics; the adds were reduced per tile in LDS by `label`).  No hooking
//           happens here, so the forest is final: after this kernel every tile root points at its root.
//   stats   one thread per cell: label = 1 + root (two hops), and every root bins its area; the workgroup reduces n, area,
//           area^2, n_border and the bins in LDS and adds what is non-zero to the plane's out (integer atomics).
// What a kernel writes plainly is read by the NEXT kernel only.  Launches only: capturable in a HIP graph.
//   The SAL moments (acg_sal, second half of the file) hang their per-object reductions on the same forest: cc_find, cc_unite,
// cc_tile_forest and comp_merge_kernel are shared, and acg_components' bits, kernel names and workspace sizes stay as they are.
#include "common.h"
#include "field.h"
#include <stdint.h>

#define CC_MAX_HW 1024
#define CC_MAX_T 255
#define CC_TH 32
#define CC_TW 64
#define CC_THREADS 256
#define CC_PER (CC_TH * CC_TW / CC_THREADS)   // 8 consecutive cells of one tile row per thread
#define CC_SEAM (CC_TW + CC_TH)               // a tile's first row, then its first column
#define CC_STATS 25
#define CC_BINS 21
#define CC_BORDER 0x80000000u
#define CC_CAP ((size_t)256 << 20)

typedef unsigned long long u64;

static_assert(CC_TW % CC_PER == 0 && CC_PER == 8 && CC_THREADS * CC_PER == CC_TH * CC_TW, "a thread's cells share a tile row");
static_assert(CC_STATS == 4 + CC_BINS && CC_MAX_HW * CC_MAX_HW < (2 << CC_BINS), "the largest area falls into the last bin");

__host__ __device__ static inline int cc_tiles_x(int W) { return (W + CC_TW - 1) / CC_TW; }
__host__ __device__ static inline int cc_tiles(int H, int W) { return ((H + CC_TH - 1) / CC_TH) * cc_tiles_x(W); }
// a plane of the workspace: lab, int32 H W, then acc, uint32 H W
static inline size_t cc_plane_bytes(int H, int W) { return acg_round_up((size_t)H * W * 8, 16); }

template <int SCOPE>
__device__ __forceinline__ int cc_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// the root of x; on the way x's parent is lowered to its grandparent (an atomic min: a parent only ever becomes an ancestor)
template <int SCOPE>
__device__ __forceinline__ int cc_find(int *lab, int x)
{
    int p = cc_load<SCOPE>(lab + x);
    while (p != x) {
        const int g = cc_load<SCOPE>(lab + p);
        if (g != p) __hip_atomic_fetch_min(lab + x, g, __ATOMIC_RELAXED, SCOPE);
        x = p, p = g;
    }
    return x;
}

// join the trees of a and b (both inside the set).  max(a, b) falls with every retry.
template <int SCOPE>
__device__ __forceinline__ void cc_unite(int *lab, int a, int b)
{
    a = cc_find<SCOPE>(lab, a), b = cc_find<SCOPE>(lab, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b, b = t; }
        int seen = a;
        if (__hip_atomic_compare_exchange_strong(lab + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
        a = cc_find<SCOPE>(lab, seen);                             // a has a parent now: seen < a
        b = cc_find<SCOPE>(lab, b);
    }
}

struct CompPass {
    long long p0, p1;                                              // the planes of this pass, plane = (row C + c) T + t
    char *ws;
    size_t plane_bytes;
    int C, H, W, T, conn;
};
__device__ __forceinline__ int *cc_lab(const CompPass &ps, long long p) { return reinterpret_cast<int *>(ps.ws + (size_t)(p - ps.p0) * ps.plane_bytes); }
__device__ __forceinline__ unsigned *cc_acc(const CompPass &ps, long long p) { return reinterpret_cast<unsigned *>(cc_lab(ps, p)) + ps.H * ps.W; }

// Where a label workgroup stands, blockIdx.x = (group - first group of the pass, tile), and its thread's CC_PER consecutive
// cells of a tile row, read once for all planes of the group (C4: the group is the field row, a pixel's channels from one
// 16-byte load; otherwise the group is (field row, channel)).  Cells beyond the field: NaN, outside every set.
template <bool C4>
struct CcCells {
    int tile, r0, c0, k0, lr, lc0, r, cc0;
    long long qa, qb;                                              // the group's planes that the pass holds
    float4 v4[C4 ? CC_PER : 1];
    float v1[C4 ? 1 : CC_PER];
    __device__ __forceinline__ CcCells(const Field &x, const CompPass &ps)
    {
        const int H = ps.H, W = ps.W, T = ps.T, C = ps.C;
        const int tiles = cc_tiles(H, W), tx = cc_tiles_x(W);
        const long long PG = C4 ? (long long)C * T : T;           // planes of a group
        const long long g = ps.p0 / PG + blockIdx.x / tiles;
        tile = blockIdx.x % tiles, r0 = (tile / tx) * CC_TH, c0 = (tile % tx) * CC_TW;
        k0 = threadIdx.x * CC_PER, lr = k0 / CC_TW, lc0 = k0 % CC_TW, r = r0 + lr, cc0 = c0 + lc0;
        const long long f = C4 ? g : g / C;
        const float *__restrict__ xf = x.x + f * x.row + (C4 ? 0 : (g - f * C) * x.chan);
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            const bool in = r < H && cc0 + j < W;
            const long long p = (long long)r * W + cc0 + j;
            if constexpr (C4) v4[j] = in ? reinterpret_cast<const float4 *>(xf)[p] : make_float4(nan, nan, nan, nan);
            else v1[j] = in ? xf[p * x.pix] : nan;
        }
        qa = max(ps.p0, g * PG), qb = min(ps.p1, (g + 1) * PG);
    }
    __device__ __forceinline__ float value(int j, int c) const { return C4 ? field_pick(v4[C4 ? j : 0], c) : v1[C4 ? 0 : j]; }
};

// The forest of one tile in LDS, by the tile's CC_THREADS threads: m, bit j + 1: cell k0 + j of mine (row lr of the tile, from
// column lc0) is in the set -> lab holds the flattened forest and root[j] the tile root of my cell j (-1 outside the set)
__device__ __forceinline__ void cc_tile_forest(int *lab, unsigned m, int k0, int lr, int lc0, int conn, int (&root)[CC_PER])
{
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    int start = k0;                                                // a run inside the thread starts linked to its first cell
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) {
        const bool in = (m >> (j + 1)) & 1;
        if (!((m >> j) & 1)) start = k0 + j;
        lab[k0 + j] = in ? start : -1;
    }
    __syncthreads();
    // membership of the row's neighbours left and right of my cells, and of the ten cells above (a sign never changes)
    if (lc0 > 0 && lab[k0 - 1] >= 0) m |= 1u;
    if (lc0 + CC_PER < CC_TW && lab[k0 + CC_PER] >= 0) m |= 1u << (CC_PER + 1);
    unsigned um = 0;
    if (lr > 0) {
#pragma unroll
        for (int j = -1; j <= CC_PER; ++j)
            if (lc0 + j >= 0 && lc0 + j < CC_TW && lab[k0 - CC_TW + j] >= 0) um |= 1u << (j + 1);
    }
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) {
        if (!((m >> (j + 1)) & 1)) continue;
        const int k = k0 + j;
        const bool left = (m >> j) & 1, right = (m >> (j + 2)) & 1;
        const bool up = (um >> (j + 1)) & 1, ul = (um >> j) & 1, ur = (um >> (j + 2)) & 1;
        if (j == 0 && left) cc_unite<WG>(lab, k, k - 1);
        if (up) {
            if (!(left && ul)) cc_unite<WG>(lab, k, k - CC_TW);    // else the cell on the left joins the two rows
        } else if (conn == 8) {
            if (ul && !left) cc_unite<WG>(lab, k, k - CC_TW - 1);  // a left neighbour in the set has ul above it
            if (ur && !right) cc_unite<WG>(lab, k, k - CC_TW + 1); // a right neighbour in the set has ur above it
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) root[j] = ((m >> (j + 1)) & 1) ? cc_find<WG>(lab, k0 + j) : -1;
}

// blockIdx.x = (group - first group of the pass, tile)
template <bool C4>
__global__ __launch_bounds__(CC_THREADS) void comp_label_kernel(Field x, CompPass ps, const float *__restrict__ thr, long long *__restrict__ out)
{
    __shared__ int lab[CC_TH * CC_TW];
    __shared__ unsigned cnt[CC_TH * CC_TW];
    const int H = ps.H, W = ps.W, T = ps.T, C = ps.C, tid = threadIdx.x;
    const CcCells<C4> my(x, ps);
    const int tile = my.tile, r0 = my.r0, c0 = my.c0, k0 = my.k0, lr = my.lr, lc0 = my.lc0, r = my.r, cc0 = my.cc0;
    const long long qa = my.qa, qb = my.qb;
    for (long long q = qa; q < qb; ++q) {
        const int c = (int)((q / T) % C), t = (int)(q % T);
        const float th = thr[c * T + t];
        unsigned m = 0;                                            // bit j + 1: cell j of mine is in the set
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            const float val = my.value(j, c);
            m |= (unsigned)(val >= th) << (j + 1);
        }
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) cnt[k0 + j] = 0;
        int root[CC_PER];
        cc_tile_forest(lab, m, k0, lr, lc0, ps.conn, root);
        // areas and border flags per tile root: one LDS add per run of equal roots among my cells
        int cur = -1;
        unsigned add = 0;
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            if (root[j] != cur) {
                if (cur >= 0) {
                    atomicAdd(cnt + cur, add & ~CC_BORDER);
                    if (add & CC_BORDER) atomicOr(cnt + cur, CC_BORDER);
                }
                cur = root[j], add = 0;
            }
            if (root[j] >= 0) {
                const int cj = cc0 + j;
                add += 1;
                if (r == 0 || r == H - 1 || cj == 0 || cj == W - 1) add |= CC_BORDER;
            }
        }
        if (cur >= 0) {
            atomicAdd(cnt + cur, add & ~CC_BORDER);
            if (add & CC_BORDER) atomicOr(cnt + cur, CC_BORDER);
        }
        __syncthreads();
        int *__restrict__ glab = cc_lab(ps, q);
        unsigned *__restrict__ gacc = cc_acc(ps, q);
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            if (r < H && cc0 + j < W) {
                const int gi = r * W + cc0 + j, kr = root[j];
                glab[gi] = kr < 0 ? -1 : (r0 + kr / CC_TW) * W + c0 + kr % CC_TW;
                gacc[gi] = kr == k0 + j ? cnt[kr] : 0u;
            }
        }
        if (tile == 0 && tid < CC_STATS) out[q * CC_STATS + tid] = 0;
        __syncthreads();                                           // cnt is read above and cleared by the next plane
    }
}

// blockIdx.x = (plane of the pass, tile); thread s < CC_TW: cell s of the tile's first row, else cell s - CC_TW of its first column
__global__ __launch_bounds__(128) void comp_merge_kernel(CompPass ps)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int H = ps.H, W = ps.W, tiles = cc_tiles(H, W), tx = cc_tiles_x(W);
    const long long p = ps.p0 + blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, r0 = (tile / tx) * CC_TH, c0 = (tile % tx) * CC_TW, s = threadIdx.x;
    if (s >= CC_SEAM) return;
    int *lab = cc_lab(ps, p);
    auto in = [&](int r, int c) { return r >= 0 && r < H && c >= 0 && c < W && cc_load<AG>(lab + r * W + c) >= 0; };
    if (s < CC_TW) {                                               // across the seam above: (r - 1, c - 1 .. c + 1)
        const int r = r0, c = c0 + s;
        if (r == 0 || !in(r, c)) return;
        const int k = r * W + c;
        const bool up = in(r - 1, c), ul = in(r - 1, c - 1), left = in(r, c - 1);
        if (up) {
            if (!(c > c0 && left && ul)) cc_unite<AG>(lab, k, k - W);    // inside the tile the cell on the left joins the two
        } else if (ps.conn == 8) {
            if (ul && !left) cc_unite<AG>(lab, k, k - W - 1);
            if (in(r - 1, c + 1) && !in(r, c + 1)) cc_unite<AG>(lab, k, k - W + 1);
        }
    } else {                                                       // across the seam on the left: (r - 1 .. r + 1, c - 1)
        const int r = r0 + s - CC_TW, c = c0;
        if (c == 0 || !in(r, c)) return;
        const int k = r * W + c;
        const bool left = in(r, c - 1), ul = in(r - 1, c - 1), up = in(r - 1, c);
        if (left) {
            if (!(r > r0 && up && ul)) cc_unite<AG>(lab, k, k - 1);      // a corner cell skips neither: the two rules lean on each other
        } else if (ps.conn == 8) {
            if (ul && !up) cc_unite<AG>(lab, k, k - W - 1);
            if (in(r + 1, c - 1) && !in(r + 1, c)) cc_unite<AG>(lab, k, k + W - 1);
        }
    }
}

// blockIdx.x = (plane of the pass, block of CC_THREADS cells)
__global__ __launch_bounds__(CC_THREADS) void comp_root_kernel(CompPass ps, int bpp)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const long long p = ps.p0 + blockIdx.x / bpp;
    const int i = (blockIdx.x % bpp) * CC_THREADS + threadIdx.x;
    if (i >= ps.H * ps.W) return;
    int *lab = cc_lab(ps, p);
    unsigned *acc = cc_acc(ps, p);
    const unsigned a = __hip_atomic_load(acc + i, __ATOMIC_RELAXED, AG);
    if (a == 0) return;                                            // not a tile root
    const int rt = cc_find<AG>(lab, i);
    if (rt == i) return;
    __hip_atomic_fetch_min(lab + i, rt, __ATOMIC_RELAXED, AG);
    __hip_atomic_fetch_add(acc + rt, a & ~CC_BORDER, __ATOMIC_RELAXED, AG);
    if (a & CC_BORDER) __hip_atomic_fetch_or(acc + rt, CC_BORDER, __ATOMIC_RELAXED, AG);
}

// blockIdx.x = (plane of the pass, block of CC_THREADS cells); labels: all planes' (P, H, W), or null
__global__ __launch_bounds__(CC_THREADS) void comp_stats_kernel(CompPass ps, int bpp, long long *__restrict__ out, int *__restrict__ labels)
{
    __shared__ u64 sm[CC_STATS];
    const long long p = ps.p0 + blockIdx.x / bpp;
    const int i = (blockIdx.x % bpp) * CC_THREADS + threadIdx.x, HW = ps.H * ps.W;
    if (threadIdx.x < CC_STATS) sm[threadIdx.x] = 0;
    __syncthreads();
    if (i < HW) {
        const int *__restrict__ lab = cc_lab(ps, p);
        int rt = lab[i];
        if (rt >= 0) {
            for (int up = lab[rt]; up != rt; up = lab[rt]) rt = up;    // the cell's tile root, then its root
            if (rt == i) {
                const unsigned a = cc_acc(ps, p)[i], area = a & ~CC_BORDER;
                atomicAdd(sm + 0, (u64)1);
                atomicAdd(sm + 1, (u64)area);
                atomicAdd(sm + 2, (u64)area * area);
                if (a & CC_BORDER) atomicAdd(sm + 3, (u64)1);
                atomicAdd(sm + 4 + (31 - __clz(area)), (u64)1);    // 1 <= area <= 2^20
            }
        }
        if (labels) labels[p * HW + i] = rt + 1;
    }
    __syncthreads();
    if (threadIdx.x < CC_STATS && sm[threadIdx.x] != 0) atomicAdd(reinterpret_cast<u64 *>(out) + p * CC_STATS + threadIdx.x, sm[threadIdx.x]);
}

static bool cc_shape_ok(int rows, int C, int H, int W, int T)
{
    return rows >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= CC_MAX_HW && W <= CC_MAX_HW && T >= 1 && T <= CC_MAX_T &&
           (long long)rows * C * T <= 0x7fffffffLL;
}

// all planes, at most CC_CAP (acg_components then runs in passes), at least one plane
extern "C" size_t acg_components_workspace_bytes(int rows, int C, int H, int W, int T)
{
    if (!cc_shape_ok(rows, C, H, W, T)) return 0;
    const size_t plane = cc_plane_bytes(H, W), all = (size_t)rows * C * T * plane;
    if (all <= CC_CAP) return all;
    return plane > CC_CAP ? plane : CC_CAP / plane * plane;
}

extern "C" int acg_components(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                              const float *thr, int T, int conn, long long *out, int *labels, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "acg_components";
    ACG_REQUIRE(x != nullptr && thr != nullptr && out != nullptr, "acg_components: null tensor");
    Field f = {x, row_stride, chan_stride, pix_stride, FIELD_SCALAR};
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= CC_MAX_HW && W <= CC_MAX_HW, "acg_components: fields must be H x W with 1 <= H, W <= %d (got %d x %d)",
                CC_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(T >= 1 && T <= CC_MAX_T, "acg_components: need 1 <= T <= %d thresholds (T=%d)", CC_MAX_T, T);
    ACG_REQUIRE(conn == 4 || conn == 8, "acg_components: connectivity must be 4 or 8 (conn=%d)", conn);
    ACG_REQUIRE(cc_shape_ok(rows, C, H, W, T), "acg_components: too many planes (rows=%d, C=%d, T=%d)", rows, C, T);
    const long long planes = (long long)rows * C * T;
    ACG_REQUIRE(labels == nullptr || planes * H * W <= 0x7fffffffLL, "acg_components: too many cells for labels (%lld planes of %d x %d)", planes,
                H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, &f, 1));
    const size_t plane = cc_plane_bytes(H, W);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, plane));
    f.mode = field_load_mode(f, C);
    hipStream_t st = (hipStream_t)stream;
    const int tiles = cc_tiles(H, W), bpp = acg_cdiv((long)H * W, CC_THREADS);
    long long per = (long long)(ws_bytes / plane);                 // planes of a pass: what the workspace holds, grids below 2^31
    const long long most = 0x7fffffffLL / (bpp > tiles ? bpp : tiles);
    per = per < most ? per : most;
    const long long PG = f.mode == FIELD_C4 ? (long long)C * T : T;
    for (long long p0 = 0; p0 < planes; p0 += per) {
        CompPass ps = {p0, p0 + per < planes ? p0 + per : planes, (char *)ws, plane, C, H, W, T, conn};
        const unsigned np = (unsigned)(ps.p1 - ps.p0), groups = (unsigned)((ps.p1 - 1) / PG - p0 / PG + 1);
        if (f.mode == FIELD_C4)
            hipLaunchKernelGGL(comp_label_kernel<true>, dim3(groups * tiles), dim3(CC_THREADS), 0, st, f, ps, thr, out);
        else
            hipLaunchKernelGGL(comp_label_kernel<false>, dim3(groups * tiles), dim3(CC_THREADS), 0, st, f, ps, thr, out);
        if (tiles > 1) {                                           // one tile: its roots are the plane's
            hipLaunchKernelGGL(comp_merge_kernel, dim3(np * tiles), dim3(128), 0, st, ps);
            hipLaunchKernelGGL(comp_root_kernel, dim3(np * bpp), dim3(CC_THREADS), 0, st, ps, bpp);
        }
        hipLaunchKernelGGL(comp_stats_kernel, dim3(np * bpp), dim3(CC_THREADS), 0, st, ps, bpp, out, labels);
    }
    acg_note_kernel(tiles > 1 ? "comp_label<%s> + comp_merge + comp_root + comp_stats" : "comp_label<%s> + comp_stats",
                    f.mode == FIELD_C4 ? "c4" : "strided");
    ACG_CHECK_LAUNCH("acg_components");
    return ACG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// SAL: the weighted moments of the objects (ops.sal, model.translate_sal, test.py --metric fss --fss_sal 1; tests/sal_ref.py states the
// definition).  The mass of a cell is the fixed-point integer q = clamp(rint((x - floor) 2^20), 0, 2^24) (fp32, each operation
// rounded on its own; NaN: 0), so every sum below is an exact integer, whatever its order.  On the forest above, per plane:
//   field   once per call, after a launch that zeroes `field`: one workgroup per (field row [, channel], chunk of 8192 cells)
//           sums q, q h, q w over ALL its cells (registers, wave shuffles, LDS) and adds what is non-zero to Q, QY, QX (64-bit
//           integer atomics at agent scope).
//   label   comp_label's walk with sal's reductions: per tile root, in LDS, R, Y, X = sum of q, q h, q w and the peak max q of
//           its cells (one LDS atomic per quantity and run of equal roots among a thread's cells); plain stores of lab and, in
//           acc's place, of pk for the whole tile (a tile root: SAL_TROOT | peak, every other cell 0), and of the three sums
//           of the tile roots ALONE into mom: no other cell's sums are ever read.  LDS: 2048 cells x (4 lab + 4 peak + 3 x 8
//           sums) = 64 KiB of a CU's 160, two workgroups per CU.
//   merge   comp_merge_kernel as it stands: lab is the first array of a plane here too.
//   root    one thread per cell: a tile root that is not its component's root points lab at it and adds its sums to the root's
//           (64-bit integer atomics) and its peak (32-bit max), at agent scope.
//   finish  one workgroup of SAL_FIN threads per plane: thread k walks cells k, k + SAL_FIN, ..; counts the cells of the set
//           and, at every root, n, Robj, Rmax (integers: wave shuffles, then LDS atomics) and the two double terms
//           R (R / P) and R sqrt((Y / R - QY / Q)^2 + (X / R - QX / Q)^2), each operation rounded on its own, summed per thread
//           in index order and then by a fixed LDS tree.  obj and shape are written plainly.  No floating-point atomics: the
//           same bits on every call, in every layout, for every workspace size and whatever the workspace held.
// A plane of the workspace: lab int32 H W, pk uint32 H W, mom 3 x uint64 H W.
#define SAL_TROOT 0x80000000u
#define SAL_QMAX 16777216.0f
#define SAL_FIN 1024
#define SAL_UNROLL 8                                           // cells a thread of field / finish loads before it uses the first
#define SAL_CHUNK (SAL_UNROLL * SAL_FIN)                       // cells of a field workgroup

static inline size_t sal_plane_bytes(int H, int W) { return acg_round_up((size_t)H * W * 32, 16); }
__device__ __forceinline__ u64 *sal_mom(const CompPass &ps, long long p) { return reinterpret_cast<u64 *>(cc_lab(ps, p) + 2 * ps.H * ps.W); }

__device__ __forceinline__ unsigned sal_quant(float v, float flr)
{
    const float s = rintf(__fmul_rn(__fsub_rn(v, flr), 1048576.0f));
    return (unsigned)fminf(fmaxf(s, 0.0f), SAL_QMAX);              // NaN: fmaxf gives the 0
}

__device__ __forceinline__ u64 sal_wave_sum(u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u64 sal_wave_max(u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(CC_THREADS) void sal_zero_kernel(long long *__restrict__ field, long long n)
{
    const long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < n) field[i] = 0;
}

// blockIdx.x = field row (C4: all its channels from 16-byte loads) or (field row, channel), blockIdx.y = chunk of SAL_CHUNK
// cells: thread k takes cells k, k + SAL_FIN, .. of the chunk; field (rows, C, 3), zeroed by sal_zero_kernel
template <bool C4>
__global__ __launch_bounds__(SAL_FIN) void sal_field_kernel(Field x, int C, int H, int W, float flr, long long *__restrict__ field)
{
    constexpr int NC = C4 ? 4 : 1;
    __shared__ u64 sm[NC * 3];
    const int tid = threadIdx.x, HW = H * W, i0 = blockIdx.y * SAL_CHUNK + tid;
    const long long f = C4 ? blockIdx.x : blockIdx.x / C;
    const float *__restrict__ xf = x.x + f * x.row + (C4 ? 0 : (blockIdx.x - f * C) * x.chan);
    if (tid < NC * 3) sm[tid] = 0;
    __syncthreads();
    u64 s[NC][3] = {};
    float v[SAL_UNROLL][NC];
#pragma unroll
    for (int u = 0; u < SAL_UNROLL; ++u) {                           // SAL_UNROLL independent loads in flight
        const int i = i0 + u * SAL_FIN;
        if constexpr (C4) {
            const float4 v4 = i < HW ? reinterpret_cast<const float4 *>(xf)[i] : make_float4(flr, flr, flr, flr);
            v[u][0] = v4.x, v[u][C4 ? 1 : 0] = v4.y, v[u][C4 ? 2 : 0] = v4.z, v[u][C4 ? 3 : 0] = v4.w;
        } else {
            v[u][0] = i < HW ? xf[(long long)i * x.pix] : flr;     // a cell at the floor weighs nothing
        }
    }
#pragma unroll
    for (int u = 0; u < SAL_UNROLL; ++u) {
        const int i = i0 + u * SAL_FIN, h = i / W, w = i - h * W;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const u64 q = sal_quant(v[u][c], flr);
            s[c][0] += q, s[c][1] += q * h, s[c][2] += q * w;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u64 a = sal_wave_sum(s[c][k]);
            if ((tid & 63) == 0 && a != 0) atomicAdd(sm + c * 3 + k, a);
        }
    __syncthreads();
    if ((C4 ? tid < C * 3 : tid < 3) && sm[tid] != 0)
        __hip_atomic_fetch_add(reinterpret_cast<u64 *>(field) + (long long)blockIdx.x * (C4 ? C : 1) * 3 + tid, sm[tid], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// blockIdx.x = (group - first group of the pass, tile), as comp_label_kernel
template <bool C4>
__global__ __launch_bounds__(CC_THREADS) void sal_label_kernel(Field x, CompPass ps, const float *__restrict__ thr, float flr)
{
    __shared__ u64 sR[CC_TH * CC_TW], sY[CC_TH * CC_TW], sX[CC_TH * CC_TW];
    __shared__ int lab[CC_TH * CC_TW];
    __shared__ unsigned sP[CC_TH * CC_TW];
    const int H = ps.H, W = ps.W, T = ps.T, C = ps.C, tid = threadIdx.x;
    const CcCells<C4> my(x, ps);
    const int tile = my.tile, r0 = my.r0, c0 = my.c0, k0 = my.k0, lr = my.lr, lc0 = my.lc0, r = my.r, cc0 = my.cc0;
#pragma unroll
    for (int j = 0; j < CC_PER; ++j) sR[k0 + j] = sY[k0 + j] = sX[k0 + j] = 0, sP[k0 + j] = 0;   // a tile root clears its own once it has stored them
    const long long qa = my.qa, qb = my.qb;
    for (long long q = qa; q < qb; ++q) {
        const int c = (int)((q / T) % C), t = (int)(q % T);
        const float th = thr[c * T + t];
        unsigned m = 0;                                            // bit j + 1: cell j of mine is in the set
        unsigned mass[CC_PER];
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            const float val = my.value(j, c);
            m |= (unsigned)(val >= th) << (j + 1);
            mass[j] = sal_quant(val, flr);
        }
        int root[CC_PER];
        cc_tile_forest(lab, m, k0, lr, lc0, ps.conn, root);
        // the moments per tile root: one LDS atomic per quantity and run of equal roots among my cells (they share row r)
        int cur = -1;
        u64 sq = 0, sx = 0;
        unsigned pk = 0;
        auto flush = [&]() {
            if (cur < 0) return;
            atomicMax(sP + cur, pk);
            if (sq != 0) atomicAdd(sR + cur, sq), atomicAdd(sY + cur, sq * (u64)r), atomicAdd(sX + cur, sx);
        };
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            if (root[j] != cur) {
                flush();
                cur = root[j], sq = sx = 0, pk = 0;
            }
            if (root[j] >= 0) {
                sq += mass[j], sx += (u64)mass[j] * (u64)(cc0 + j);
                pk = mass[j] > pk ? mass[j] : pk;
            }
        }
        flush();
        __syncthreads();
        int *__restrict__ glab = cc_lab(ps, q);
        unsigned *__restrict__ gpk = cc_acc(ps, q);
        u64 *__restrict__ gmom = sal_mom(ps, q);
        const int HW = H * W;
#pragma unroll
        for (int j = 0; j < CC_PER; ++j) {
            const int kr = root[j];
            const bool mine = kr == k0 + j;                        // a tile root lies inside the field
            if (r < H && cc0 + j < W) {
                const int gi = r * W + cc0 + j;
                glab[gi] = kr < 0 ? -1 : (r0 + kr / CC_TW) * W + c0 + kr % CC_TW;
                gpk[gi] = mine ? SAL_TROOT | sP[kr] : 0u;
                if (mine) gmom[gi] = sR[kr], gmom[HW + gi] = sY[kr], gmom[2 * HW + gi] = sX[kr];
            }
            if (mine) sR[kr] = sY[kr] = sX[kr] = 0, sP[kr] = 0;
        }
        __syncthreads();                                           // the sums are read above and added to by the next plane
    }
}

// blockIdx.x = (plane of the pass, block of CC_THREADS cells)
__global__ __launch_bounds__(CC_THREADS) void sal_root_kernel(CompPass ps, int bpp)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const long long p = ps.p0 + blockIdx.x / bpp;
    const int i = (blockIdx.x % bpp) * CC_THREADS + threadIdx.x, HW = ps.H * ps.W;
    if (i >= HW) return;
    int *lab = cc_lab(ps, p);
    unsigned *pk = cc_acc(ps, p);
    u64 *mom = sal_mom(ps, p);
    const unsigned a = __hip_atomic_load(pk + i, __ATOMIC_RELAXED, AG);
    if (a == 0) return;                                            // not a tile root
    const int rt = cc_find<AG>(lab, i);
    if (rt == i) return;                                           // nothing is added to a tile root that is no root: its sums stand
    __hip_atomic_fetch_min(lab + i, rt, __ATOMIC_RELAXED, AG);
    __hip_atomic_fetch_max(pk + rt, a, __ATOMIC_RELAXED, AG);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u64 v = __hip_atomic_load(mom + k * HW + i, __ATOMIC_RELAXED, AG);
        if (v != 0) __hip_atomic_fetch_add(mom + k * HW + rt, v, __ATOMIC_RELAXED, AG);
    }
}

// blockIdx.x = plane of the pass; obj (planes, 4): n, area, Robj, Rmax; shape (planes, 2): SV, SR
__global__ __launch_bounds__(SAL_FIN) void sal_finish_kernel(CompPass ps, const long long *__restrict__ field, long long *__restrict__ obj,
                                                             double *__restrict__ shape)
{
#pragma clang fp contract(off)
    __shared__ double sv[SAL_FIN], sr[SAL_FIN];
    __shared__ u64 si[4];
    const long long p = ps.p0 + blockIdx.x;
    const int tid = threadIdx.x, HW = ps.H * ps.W;
    const int *__restrict__ lab = cc_lab(ps, p);
    const unsigned *__restrict__ pk = cc_acc(ps, p);
    const u64 *__restrict__ mom = sal_mom(ps, p);
    const long long *__restrict__ fq = field + (p / ps.T) * 3;
    const double Q = (double)fq[0];
    const double cy = fq[0] > 0 ? (double)fq[1] / Q : 0.0, cx = fq[0] > 0 ? (double)fq[2] / Q : 0.0;
    if (tid < 4) si[tid] = 0;
    u64 n = 0, area = 0, robj = 0, rmax = 0;
    double v = 0.0, d = 0.0;
    for (int i0 = tid; i0 < HW; i0 += SAL_UNROLL * SAL_FIN) {          // SAL_UNROLL independent loads in flight, the cells still in order
        int ls[SAL_UNROLL];
#pragma unroll
        for (int u = 0; u < SAL_UNROLL; ++u) ls[u] = i0 + u * SAL_FIN < HW ? lab[i0 + u * SAL_FIN] : -1;
        u64 Rs[SAL_UNROLL], Ys[SAL_UNROLL], Xs[SAL_UNROLL];
        unsigned Ps[SAL_UNROLL];
#pragma unroll
        for (int u = 0; u < SAL_UNROLL; ++u) {                       // a root's sums: all loads of the block before any term
            const int i = i0 + u * SAL_FIN;
            const bool root = ls[u] == i;
            Rs[u] = root ? mom[i] : 0, Ys[u] = root ? mom[HW + i] : 0, Xs[u] = root ? mom[2 * HW + i] : 0, Ps[u] = root ? pk[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < SAL_UNROLL; ++u) {
            const int i = i0 + u * SAL_FIN, l = ls[u];
            if (l < 0) continue;
            ++area;
            if (l != i) continue;
            const u64 R = Rs[u];
            ++n, robj += R, rmax = R > rmax ? R : rmax;
            if (R == 0) continue;                                  // every cell at the floor: counted, no mass
            const double Rd = (double)R, Pd = (double)(Ps[u] & ~SAL_TROOT);
            const double dy = (double)Ys[u] / Rd - cy, dx = (double)Xs[u] / Rd - cx;
            v += Rd * (Rd / Pd);
            d += Rd * sqrt(dy * dy + dx * dx);
        }
    }
    sv[tid] = v, sr[tid] = d;
    __syncthreads();
    n = sal_wave_sum(n), area = sal_wave_sum(area), robj = sal_wave_sum(robj), rmax = sal_wave_max(rmax);
    if ((tid & 63) == 0) atomicAdd(si + 0, n), atomicAdd(si + 1, area), atomicAdd(si + 2, robj), atomicMax(si + 3, rmax);
    for (int s = SAL_FIN / 2; s > 0; s >>= 1) {
        if (tid < s) sv[tid] += sv[tid + s], sr[tid] += sr[tid + s];
        __syncthreads();
    }
    if (tid < 4) obj[p * 4 + tid] = (long long)si[tid];
    if (tid == 0) shape[p * 2] = sv[0], shape[p * 2 + 1] = sr[0];
}

// all planes, at most CC_CAP (acg_sal then runs in passes), at least one plane
extern "C" size_t acg_sal_workspace_bytes(int rows, int C, int H, int W, int T)
{
    if (!cc_shape_ok(rows, C, H, W, T)) return 0;
    const size_t plane = sal_plane_bytes(H, W), all = (size_t)rows * C * T * plane;
    if (all <= CC_CAP) return all;
    return plane > CC_CAP ? plane : CC_CAP / plane * plane;
}

extern "C" int acg_sal(const float *x, int rows, int C, int H, int W, long long row_stride, int pix_stride, long long chan_stride,
                       const float *thr, int T, int conn, float floor, long long *field, long long *obj, double *shape, void *ws,
                       size_t ws_bytes, void *stream)
{
    const char *fn = "acg_sal";
    ACG_REQUIRE(x != nullptr && thr != nullptr && field != nullptr && obj != nullptr && shape != nullptr, "acg_sal: null tensor");
    Field f = {x, row_stride, chan_stride, pix_stride, FIELD_SCALAR};
    ACG_REQUIRE(H >= 1 && W >= 1 && H <= CC_MAX_HW && W <= CC_MAX_HW, "acg_sal: fields must be H x W with 1 <= H, W <= %d (got %d x %d)",
                CC_MAX_HW, H, W);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, nullptr, 0));
    ACG_REQUIRE(T >= 1 && T <= CC_MAX_T, "acg_sal: need 1 <= T <= %d thresholds (T=%d)", CC_MAX_T, T);
    ACG_REQUIRE(conn == 4 || conn == 8, "acg_sal: connectivity must be 4 or 8 (conn=%d)", conn);
    ACG_REQUIRE(floor - floor == 0.0f, "acg_sal: the floor must be finite (floor=%g)", (double)floor);
    ACG_REQUIRE(cc_shape_ok(rows, C, H, W, T), "acg_sal: too many planes (rows=%d, C=%d, T=%d)", rows, C, T);
    FIELD_CHECK(field_refuse_operands(fn, rows, C, &f, 1));
    const size_t plane = sal_plane_bytes(H, W);
    FIELD_CHECK(field_refuse_workspace(fn, ws, ws_bytes, plane));
    f.mode = field_load_mode(f, C);
    hipStream_t st = (hipStream_t)stream;
    const bool c4 = f.mode == FIELD_C4;
    const int tiles = cc_tiles(H, W), bpp = acg_cdiv((long)H * W, CC_THREADS);
    const long long planes = (long long)rows * C * T;
    long long per = (long long)(ws_bytes / plane);                 // planes of a pass: what the workspace holds, grids below 2^31
    const long long most = 0x7fffffffLL / (bpp > tiles ? bpp : tiles);
    per = per < most ? per : most;
    const long long PG = c4 ? (long long)C * T : T;
    const long long nfield = (long long)rows * C * 3;
    const int chunks = acg_cdiv((long)H * W, SAL_CHUNK);
    hipLaunchKernelGGL(sal_zero_kernel, dim3((unsigned)((nfield + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st, field, nfield);
    if (c4)
        hipLaunchKernelGGL(sal_field_kernel<true>, dim3(rows, chunks), dim3(SAL_FIN), 0, st, f, C, H, W, floor, field);
    else
        hipLaunchKernelGGL(sal_field_kernel<false>, dim3(rows * C, chunks), dim3(SAL_FIN), 0, st, f, C, H, W, floor, field);
    for (long long p0 = 0; p0 < planes; p0 += per) {
        CompPass ps = {p0, p0 + per < planes ? p0 + per : planes, (char *)ws, plane, C, H, W, T, conn};
        const unsigned np = (unsigned)(ps.p1 - ps.p0), groups = (unsigned)((ps.p1 - 1) / PG - p0 / PG + 1);
        if (c4)
            hipLaunchKernelGGL(sal_label_kernel<true>, dim3(groups * tiles), dim3(CC_THREADS), 0, st, f, ps, thr, floor);
        else
            hipLaunchKernelGGL(sal_label_kernel<false>, dim3(groups * tiles), dim3(CC_THREADS), 0, st, f, ps, thr, floor);
        if (tiles > 1) {                                           // one tile: its roots are the plane's
            hipLaunchKernelGGL(comp_merge_kernel, dim3(np * tiles), dim3(128), 0, st, ps);
            hipLaunchKernelGGL(sal_root_kernel, dim3(np * bpp), dim3(CC_THREADS), 0, st, ps, bpp);
        }
        hipLaunchKernelGGL(sal_finish_kernel, dim3(np), dim3(SAL_FIN), 0, st, ps, field, obj, shape);
    }
    acg_note_kernel(tiles > 1 ? "sal_field<%s> + sal_label<%s> + comp_merge + sal_root + sal_finish" : "sal_field<%s> + sal_label<%s> + sal_finish",
                    c4 ? "c4" : "strided", c4 ? "c4" : "strided");
    ACG_CHECK_LAUNCH("acg_sal");
    return ACG_OK;
}
