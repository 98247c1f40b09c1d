// The operand of the field metrics and losses (spectrum.hip, field_spectrum.hip, ssim.hip, fss.hip, marginal.hip): rows x C
// fields of H x W pixels, addressed by (row, pixel, channel) strides in floats.  The one place that knows how such an operand
// is described, which layouts get 16-byte accesses, and what is refused of it before a launch.
#pragma once
#include <stdint.h>
#include "common.h"

// how a field's pixels are read: one by one; four pixels of a planar row at once; a pixel's (up to) four channels at once
enum { FIELD_SCALAR = 0, FIELD_PLANAR = 1, FIELD_C4 = 2 };

// one operand of a launch: where its fields lie and how their pixels are loaded.  An entry point fills it as the caller
// describes it, {x, row, chan, pix, FIELD_SCALAR}; the load mode follows (field_load_mode) once the call has been let pass
struct Field {
    const float *x;
    long long row, chan;                                           // strides in floats
    int pix, mode;
};
// what a launch reads: field or pair p is channel c of row r of operand 0 and, of a pair, channel c of row r / x_per_y of operand 1
template <int NF>
struct FieldSrc {
    Field f[NF];
    int C, x_per_y;
};

// the first pixel of field or pair p in operand i (FIELD_C4: the image's; c: the channel to pick)
template <int NF>
__device__ __forceinline__ const float *field_first(const FieldSrc<NF> &s, int i, int p, int &c)
{
    int row = p / s.C;
    c = p - row * s.C;
    if (i == 1) row /= s.x_per_y;
    const Field &f = s.f[i];
    return f.x + (long long)row * f.row + (f.mode == FIELD_C4 ? 0 : (long long)c * f.chan);
}

// channel c of a FIELD_C4 pixel's 16 bytes
__device__ __forceinline__ float field_pick(float4 v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// 16-byte accesses where the layout allows them: a pixel's channels of an NHWC operand of four stored channels, or (planar_ok:
// for a caller whose kernels read it) four pixels of a planar row.  also: a second tensor of the same strides that is accessed
// the same way (the gradient), or null.  An operand off the 16-byte grid, or whose rows leave it, is read pixel by pixel.
static inline int field_load_mode(const Field &f, int C, bool planar_ok = false, const void *also = nullptr)
{
    const bool aligned = (uintptr_t)f.x % 16 == 0 && (uintptr_t)also % 16 == 0 && f.row % 4 == 0;
    if (planar_ok && f.pix == 1 && f.chan % 4 == 0 && aligned) return FIELD_PLANAR;
    if (f.pix == 4 && f.chan == 1 && C <= 4 && aligned) return FIELD_C4;
    return FIELD_SCALAR;
}

// What an entry point refuses of its operands, under its own name fn; each returns ACG_OK or the status after acg_set_error.
// An entry point lists them among its own refusals in the order it reports them: FIELD_CHECK(field_refuse_...(...)).
#define FIELD_CHECK(call)                    \
    do {                                     \
        if (const int rc__ = (call)) return rc__; \
    } while (0)

// rows and channels to work on, and positive strides of the nf operands f (x, then y); nf = 0: the counts alone, for an entry
// point with refusals of its own between the two
static inline int field_refuse_operands(const char *fn, int rows, int C, const Field *f, int nf)
{
    ACG_REQUIRE(rows >= 1 && C >= 1, "%s: need rows >= 1 and C >= 1 (rows=%d, C=%d)", fn, rows, C);
    for (int i = 0; i < nf; ++i)
        ACG_REQUIRE(f[i].row >= 1 && f[i].pix >= 1 && f[i].chan >= 1, "%s: strides must be positive (%s: row %lld, pixel %d, channel %lld)",
                    fn, i ? "y" : "x", f[i].row, f[i].pix, f[i].chan);
    return ACG_OK;
}

// row r of x pairs with row r / x_per_y of y: x_per_y in 1 .. max_per, dividing the rows of x
static inline int field_refuse_pairing(const char *fn, int rows, int x_per_y, int max_per)
{
    ACG_REQUIRE(x_per_y >= 1 && x_per_y <= max_per && rows % x_per_y == 0,
                "%s: x_per_y must lie in 1..%d and divide the rows of x (rows=%d, x_per_y=%d)", fn, max_per, rows, x_per_y);
    return ACG_OK;
}

// a workspace of `need` bytes (0: none is looked at): missing or too small is ACG_ERR_WORKSPACE, off the 16-byte grid invalid
static inline int field_refuse_workspace(const char *fn, const void *ws, size_t ws_bytes, size_t need)
{
    if (need != 0 && (ws == nullptr || ws_bytes < need)) {
        acg_set_error("%s: workspace too small (%zu < %zu)", fn, ws_bytes, need);
        return ACG_ERR_WORKSPACE;
    }
    ACG_REQUIRE(need == 0 || (uintptr_t)ws % 16 == 0, "%s: the workspace must be 16-byte aligned", fn);
    return ACG_OK;
}
