/* acgan_cell.h - per-cell (climatology map) entry points of libacgan_hip.so.
 *
 * The training ABI is include/acgan_hip.h, the verification tables are include/acgan_verif.h; a caller that binds either does
 * not need this header and does not have to rebind when the evaluator gains a per-cell score.  The entry points here are
 * compiled into the same shared object, return the same status codes (ACG_OK, ACG_ERR_INVALID = -1, ACG_ERR_WORKSPACE = -2,
 * ACG_ERR_LAUNCH = -3) and report through the same acg_last_error() / acg_last_kernel() of acgan_hip.h.  They carry a
 * version of their own: check acg_cell_version() == ACG_CELL_VERSION after loading.
 */
#ifndef ACGAN_CELL_H
#define ACGAN_CELL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACG_CELL_VERSION 1

/* ACG_CELL_VERSION of the build */
int acg_cell_version(void);

/* ---- streaming per-cell statistics of an ensemble against its truth (ops.cell_stats, model.translate_ensemble(cell_stats=...),
 *      test.py --metric ensemble --ens_maps 1; no reference call site; tests/cell_stats_ref.py states the definition) ----
 * x, y, rows, x_per_y, the strides (in floats) and the pairing rule are acg_fss's: row r of x pairs with row r / x_per_y of y,
 * M = x_per_y members share a truth, Ny = rows / M.  thr (C, T) and edges (C, E) are float32 on the device, edges ascending
 * per channel (the caller's contract).
 * The state buffers are the caller's, zeroed once; every call ADDS to them.  They are planar:
 *   mom (9, C, H, W) float64; evt (C, T, 4, H, W) int64; hist_x, hist_y (C, E + 1, H, W) int32.
 * For cell (c, i, j), over n = 0 .. Ny - 1 in that order and inside each n over m = 0 .. M - 1 in that order, every float
 * converted to double first and every line one IEEE double operation rounded once (no contraction):
 *   yv = Y[n];  Sy += yv;  Syy += yv*yv;  S = 0;  Q = 0
 *   for m:  xv = X[n*M+m];  Sx += xv;  Sxx += xv*xv;  Sxy += xv*yv;  Sad += |xv - yv|;  S += xv;  Q += xv*xv
 *   u = S*S;  SS += u;  SSy += S*yv;  t = M*Q;  v = t - u;  Sw += v          (no division on the device)
 * mom planes, in order: Sx, Sxx, Sy, Syy, Sxy, Sad, SS, SSy, Sw.  The running sums start from what mom holds, so the result
 * has the same bits whatever the split of the rows into calls, as long as the rows arrive in the same order, and in every
 * layout.  NaN and +-inf propagate as IEEE says; subnormal float32 inputs are outside the equality claim.
 * Events: per threshold t the comparison is made in float32 and NaN is no event, as in acg_fss: k = #{m : X >= thr[c][t]},
 * o = [Y >= thr[c][t]], evt[c][t] += (k, o, k o, k k).  Histograms: the bin of a value v is #{e : edges[c][e] <= v}, NaN falls
 * into bin 0; hist_x[c][bin(xv)] += 1 per member, hist_y[c][bin(yv)] += 1 per truth.  An int32 histogram count holds 2^31 - 1
 * rows per cell over the life of a state: the caller keeps a split times its members below that.
 * T = 0 (thr and evt null) turns the events off, E = 0 (edges, hist_x, hist_y null) the histograms; the moments are always
 * computed.  No workspace, nothing read back, launches only (capturable in a HIP graph), no atomics: one thread owns a cell
 * for a whole launch and writes it with plain vector stores.
 * Limits: 1 <= H, W <= 1024, 1 <= x_per_y <= 64, 0 <= T <= 8, 0 <= E <= 63.
 * Refused before a launch (-1, acg_last_error starts with "acg_cell_stats"), in this order: rows < 1 or C < 1; a stride < 1;
 * x_per_y outside 1..64 or not dividing rows; a null x, y or mom; an extent outside 1..1024 (or 2^31 workgroups); T outside
 * 0..8, or T > 0 with a null thr or evt; E outside 0..63, or E > 0 with a null edges, hist_x or hist_y; a state buffer that
 * is not aligned to its element size.
 * Kernels: cell_mom (the moments; a thread carries a pixel's four channels where an operand is a 16-byte NHWC pixel, else one
 * channel), then cell_evt if T > 0 (32-bit counters in registers, at most 2^19 truth rows per launch, added to evt at the
 * end), then cell_hist on x and on y if E > 0 (private 16-bit counters in LDS laid out [bin][thread], at most 65535 rows per
 * launch, one coalesced flush per bin; the bin by a binary search of the edges in LDS). */
int acg_cell_stats(const float *x, const float *y, int rows, int x_per_y, int C, int H, int W, long long x_row_stride,
                   int x_pix_stride, long long x_chan_stride, long long y_row_stride, int y_pix_stride, long long y_chan_stride,
                   const float *thr, int T, const float *edges, int E, double *mom, long long *evt, int *hist_x, int *hist_y,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ACGAN_CELL_H */
