/* acgan_verif.h - verification-only entry points of libacgan_hip.so.
 *
 * The training ABI is include/acgan_hip.h; a caller that binds the training step does not need this header and does not
 * have to rebind when the evaluator gains a score.  The entry points here are compiled into the same shared object, return
 * the same status codes (ACG_OK, ACG_ERR_INVALID = -1, ACG_ERR_WORKSPACE = -2, ACG_ERR_LAUNCH = -3) and report through the
 * same acg_last_error() / acg_last_kernel() of acgan_hip.h.  They carry a version of their own: check
 * acg_verif_version() == ACG_VERIF_VERSION after loading, as acg_version() is checked against ACG_VERSION.
 */
#ifndef ACGAN_VERIF_H
#define ACGAN_VERIF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACG_VERIF_VERSION 1

/* ACG_VERIF_VERSION of the build */
int acg_verif_version(void);

/* ---- reliability tables of ensemble events (ops.reliability, model.translate_fss(reliability=...), test.py --metric fss
 *      --fss_rel 1; no reference call site: the reference has no verification code, tests/reliability_ref.py states the
 *      definition; Murphy 1973, Ferro 2014, Schwartz & Sobash 2017) ----
 * x, y, rows, x_per_y, the strides (in floats), thr (C, T) on the device, windows (nw odd widths in HOST memory, read before
 * the launch) and the pairing rule are acg_fss's: row r of x pairs with row r / x_per_y of y, M = x_per_y members share a
 * truth.  The events are acg_fss's, b = [x >= thr[c][t]] (NaN is no event).  For an odd window n the neighbourhood event
 * b^n(i, j) is 1 iff any cell |i' - i| <= n/2, |j' - j| <= n/2 inside the domain is an event (acg_fss's window count is
 * positive); n = 1 is the cell itself, a window that covers the domain is the whole domain.  With k(i, j) = the number of
 * members whose b^n(i, j) is 1 and o(i, j) = b^n of the truth
 *   table (rows / x_per_y, C, T, nw, M + 1, 2) int64: table[k][o] = the number of the H W cells with that pair.
 * It is fully written; every (M + 1) x 2 block sums to H W; with M = 1 it is the 2 x 2 contingency table of the neighbourhood
 * events.  Brier score, its decomposition, the reliability diagram and the ROC follow from it on the host
 * (ops.reliability_summary).  Everything after the comparison is integer: exact, no floating-point atomics, the same bits for
 * every layout and launch order and whatever the workspace held.  Nothing is read back; capturable in a HIP graph.
 * Limits: 1 <= H, W <= 1024, 1 <= T <= 8, 1 <= nw <= 8, each window odd with 1 <= n <= 65, 1 <= x_per_y <= 64.
 * Refused before a launch (-1, acg_last_error starts with "acg_reliability"), in this order: rows < 1 or C < 1; a stride < 1;
 * x_per_y outside 1..64 or not dividing rows; a null x, y, thr, windows or table; an extent outside 1..1024; T outside 1..8;
 * nw outside 1..8 (and more than 2^31 - 1 planes or rows); a window that is even, non-positive or above 65; a misaligned
 * workspace (16 bytes).  A workspace below acg_reliability_workspace_bytes returns -2; the query returns 0 for a size that
 * the call refuses.
 * The workspace holds acg_fss's event planes of x and of y (one bit per cell in rows of WW = ceil(W / 64) 64-bit words, with
 * their row prefixes): 16-byte rounded 8 P H WW + 2 P H (WW + 1) bytes for the P = rows C T planes of x, then the same for
 * y; it does not depend on nw.  Kernels: fss_events as in acg_fss, then fss_rel, one workgroup per (truth row, c, t, window):
 * per 64-bit word it ORs the words of the rows of the window and their two neighbouring words (windows stop at 65, so a word
 * needs no more), dilates along the row by shifts, masks the bits past W, carry-save adds the M member words into
 * bit_width(M) slices in registers and adds popcount(mask_k & o), popcount(mask_k & ~o) for every k into 32-bit counters in
 * LDS; one 64-bit store per table entry ends it.  The M + 1 planes are copied into LDS first when they fit 63 KiB
 * (fss_rel<lds>: 6 members at 256^2), else read from the workspace (fss_rel<global>). */
size_t acg_reliability_workspace_bytes(int rows, int x_per_y, int C, int H, int W, int T, int nw);
int acg_reliability(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                    int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                    const float *thr, int T, const int *windows, int nw, long long *table, void *workspace, size_t ws_bytes,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ACGAN_VERIF_H */
