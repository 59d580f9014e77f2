/* gdyn_dcov.h -- C-ABI of the displacement covariance maps of libgdyn: for every pair of bins of beads, the sum behind the covariance
 * of their displacements over a lag, C_IJ(tau) = <D_I(tau) . D_J(tau)> ("which loci move together"), or, with lag 0, of their positions
 * about the time mean (the "essential dynamics" matrix whose leading eigenvectors are the collective modes).  Nothing in the reference
 * computes either: this is a capability beyond it.  Summed over the beads of a bin the map is a symmetric product S = A A^T of a row
 * matrix A (bins x 3 origins) in fp64: dense matrix work, done on the matrix cores (csrc/gdyn_dcov.hip).
 *
 * History.  A gd_dcov handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the
 * precision it was given.  A history with a non-finite coordinate is refused (GD_EINVAL) and leaves the handle without one.
 *
 * Bins.  B ranges [start_b, end_b) of beads: ascending, non-empty, not overlapping, end <= N.  Beads in no bin take no part.
 * With no bins set every bead is its own bin (B = N).  Bins belong to a history: they are set after it (GD_ESTATE before),
 * kept by a new history of the same N and dropped by one of another N.
 *
 * Columns.  gd_dcov_prepare builds the row matrix A[b, c] in fp64 and keeps it on the device.  Every operation is rounded on its
 * own (no contraction, no fast-math).
 *   Displacement mode (lag >= 1): the origins are f_k = first + k stride, k < count; count == 0 takes all origins with
 *     f_k + lag < F.  An explicit origin with f_k + lag >= F, or stride 0, is GD_EINVAL.  Column c = 3 k + axis holds
 *     D[i] = double(X[f_k + lag, i, axis]) - double(X[f_k, i, axis]).  Nothing is unwrapped or reduced: periodic systems store
 *     unwrapped coordinates, as for gdyn_dcorr.h.
 *   Fluctuation mode (lag == 0): the frames are f_k = first + k stride, k < count; count == 0 takes all with f_k < F.  Column
 *     c = 3 k + axis holds D[i] = double(X[f_k, i, axis]) - mean[i, axis], where mean is the serial sum of double(X[f_k, i, axis])
 *     over k ascending, from +0, divided by the number of frames.
 *   A preparation with no column is GD_EINVAL.
 *   Raw rows.  A bin is cut into pieces of GD_DCOV_PIECE_BEADS beads from its start.  A piece's sum is serial over its beads
 *     ascending, from +0; raw[b, c] is the serial sum of the pieces ascending, from +0.
 *   Drift removal (remove_drift != 0).  m[c] = (raw[b, c] added serially over the bins ascending, from +0) / double(number of
 *     binned beads);  A[b, c] = raw[b, c] - double(|b|) * m[c], the product and the difference each rounded once.  Without it A = raw.
 *   A new history or new bins drop the preparation; gd_dcov_rows and gd_dcov_map are GD_ESTATE without one.
 *   gd_dcov_rows returns rows of A: a bin's displacement series, a result in its own right.
 *
 * Map.  For bins I, J:   sum[I, J] = sum over the columns c of A[I, c] * A[J, c];
 *     count[I, J] = (columns / 3) |I| |J|, a closed form computed on the host.
 *   Mean covariance = sum / count; the correlation of a rectangle = sum / sqrt(diag_rows (x) diag_cols), where diag_rows and
 *   diag_cols hold the cells (I, I) of the rectangle's row bins and column bins: the caller's divisions.
 *
 * Summation order.  The columns are padded with zeros to a multiple of 4 (K columns) and cut into ranges of
 * GD_DCOV_COLUMN_RANGE columns counted from column 0.  Within a range a cell is ONE accumulator: it starts at +0 and is updated by
 * one 16x16x4 fp64 matrix instruction (v_mfma_f64_16x16x4_f64) per group of four columns, groups ascending; within a group the order
 * is the instruction's own.  The partial sums of the ranges are then added serially, ascending, from +0, by a second kernel.  No
 * floating-point atomic is used.  Only cells with I <= J are computed; the cell (J, I) is a copy of (I, J).  Bins are tiled from bin 0
 * on, so where a cell sits in its instruction depends on (I, J) alone.  What follows:
 *   1. results are bit-identical from run to run, for every columns_per_stage, and between a host-fed and a live-fed float32
 *      history;
 *   2. a cell does not know its rectangle: gd_dcov_map over any rectangle equals, byte for byte, the same slice of the map over
 *      all bins, and its diag_rows and diag_cols equal the whole map's diagonal;
 *   3. M[I, J] and M[J, I] are byte-equal in one call and across calls; this rests on the copy, not on a property of the hardware;
 *   4. every cell lies within gamma * sum_c |A[I, c]| |A[J, c]| of the exact sum of products of the device's own rows, with
 *      gamma = (K + 1) u / (1 - (K + 1) u), u = 2^-53: the bound of K rounded products and their additions in any order, which
 *      holds whether the instruction fuses its multiply-adds or not.  Whether it fuses, and in which order it takes its four columns,
 *      is not documented and has not been measured, so no more than this bound is promised;
 *   5. in displacement mode, integer-valued coordinates with |x| < 2^10, bins of at most 64 beads, at most 2^10 origins and no drift
 *      removal make every row entry (|.| < 2^17) and every sum (< 3 * 2^10 * 2^34 < 2^46) an exactly representable integer: the map
 *      is then exact.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_DCOV_H
#define GDYN_DCOV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_DCOV_ABI_VERSION 1
#define GD_DCOV_PIECE_BEADS 32       /* beads of one piece of a bin */
#define GD_DCOV_COLUMN_RANGE 768     /* columns of one accumulator: 256 origins */

typedef struct gd_dcov gd_dcov;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                /* HIP device ordinal */
    uint32_t columns_per_stage;     /* columns staged in LDS at once, rounded up to a multiple of 4; 0: automatic; no result depends on it */
} gd_dcov_desc;

int gd_dcov_abi_version(void);
int gd_dcov_create(const gd_dcov_desc *desc, gd_dcov **out);
int gd_dcov_destroy(gd_dcov *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_dcov_set_history(gd_dcov *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_dcov_set_history_live(gd_dcov *h, gd_live_history *history, uint32_t replica);
/* ranges: (B, 2) [start, end) pairs, ascending, non-empty, not overlapping, end <= N; NULL with n_bins == 0: every bead its own bin.
 * GD_ESTATE without a history */
int gd_dcov_set_bins(gd_dcov *h, const uint32_t *ranges, uint32_t n_bins);
/* Builds A (see Columns).  lag 0: fluctuation mode.  GD_ESTATE without a history; GD_EINVAL: stride 0, an origin past the history, no
 * column; GD_ENOMEM: A does not fit on the device.  A failed call keeps the last preparation. */
int gd_dcov_prepare(gd_dcov *h, uint32_t lag, uint32_t first, uint32_t stride, uint32_t count, int remove_drift);
/* the columns of the preparation, 3 per origin; 0 without one */
uint32_t gd_dcov_columns(const gd_dcov *h);
/* Device times in milliseconds, between events on the handle's stream: of the last successful gd_dcov_prepare (stage 1), and of the
 * product kernel and of the merge kernel of the last successful gd_dcov_map that computed cells (summed over its launches).  0 before
 * the first.  Each pointer may be NULL.  What tools/bench_dcov.py reports. */
int gd_dcov_last_times(const gd_dcov *h, double *stage1_ms, double *product_ms, double *merge_ms);
/* out: (n_bins, columns) doubles, the rows [first_bin, first_bin + n_bins) of A.  GD_EINVAL: no row or rows past B */
int gd_dcov_rows(gd_dcov *h, uint32_t first_bin, uint32_t n_bins, double *out);
/* The cells [row_first, row_first + n_rows) x [col_first, col_first + n_cols) of the map.  sum (double), count (uint64): (n_rows, n_cols);
 * diag_rows (n_rows) and diag_cols (n_cols) doubles, the cells (I, I) of the rows' and the columns' bins.  Each of the four may be NULL.
 * GD_EINVAL: an empty rectangle or one past B.  GD_ENOMEM: the outputs do not fit on the device. */
int gd_dcov_map(gd_dcov *h, uint32_t row_first, uint32_t n_rows, uint32_t col_first, uint32_t n_cols, double *sum, uint64_t *count, double *diag_rows,
                double *diag_cols);

#ifdef __cplusplus
}
#endif

#endif
