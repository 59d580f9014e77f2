/* gdyn_dmap.h -- C-ABI of the distance and contact-frequency maps of libgdyn: for every pair of bins of beads, the sums behind
 * the mean spatial distance (what chromatin tracing and FISH report), the rms distance and the contact frequency at thresholds
 * chosen after the run, over the frames of a history.  Nothing in the reference computes either: this is a capability beyond it.
 * The work is dense all-pairs arithmetic (csrc/gdyn_dmap.hip).
 *
 * History.  A gd_dmap handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the
 * precision it was given.  A history with a non-finite coordinate is refused (GD_EINVAL) and leaves the handle without one.
 *
 * Arithmetic.  fp64 on the widened coordinates, every operation rounded on its own (no contraction, no fast-math).
 *
 * Bins.  B ranges [start_b, end_b) of beads: ascending, non-empty, not overlapping, end <= N.  Beads in no bin take no part.
 * With no bins set every bead is its own bin (B = N).  Bins belong to a history: they are set after it (GD_ESTATE before),
 * checked against its N then and again at the call, kept by a new history of the same N and dropped by one of another N.
 *
 * Pair term.  For beads i != j in a frame f:
 *     d = double(X[f,i]) - double(X[f,j]) per axis; with box != NULL reduced by d -= box * nearbyint(d / box) (round half to
 *     even), the rule of gdyn_rdf.h and gdyn_dcorr.h;   r2 = (dx*dx + dy*dy) + dz*dz;   r = sqrt(r2), correctly rounded.
 *   r2 and r do not change when i and j change places: negation is exact and nearbyint is odd.
 *
 * Outputs.  For bins I, J and the frames [first_frame, first_frame + n_frames):
 *     sum1[I,J]    = sum over f, i in I, j in J, j != i of r;      sum2[I,J] likewise of r2;
 *     hits[t][I,J] = the number of those terms with r2 < thr_t * thr_t (uint64): strict, the product rounded once;
 *                    up to GD_DMAP_MAX_THRESHOLDS thresholds, each positive and finite;
 *     count[I,J]   = n_frames * (|I| |J| - [I = J] |I|), a closed form computed on the host.
 *   Mean distance = sum1 / count, rms distance = sqrt(sum2 / count), contact frequency = hits / count: the caller's divisions.
 *
 * Summation order.  A bin is cut into pieces of GD_DMAP_PIECE_BEADS beads from its start, the frames into ranges
 * [k R, (k + 1) R) with R = GD_DMAP_FRAME_RANGE, counted from frame 0 of the history.  With a <= b the bin indices of a cell,
 * the partial sum of a frame range is ONE serial sum, in this order of its loops from the outermost: pieces u of bin a ascending,
 * pieces v of bin b ascending, frames of the range that lie in the window ascending, beads i of piece u ascending, beads j of
 * piece v ascending.  The partial sums of the ranges are then added serially in ascending order.  The order therefore depends on
 * (the bins, the frame window) alone, and no floating-point atomic is used.  What follows:
 *   1. results are bit-identical from run to run, for every max_frames_per_stage, and between a host-fed and a live-fed
 *      float32 history;
 *   2. a cell does not know its region: gd_dmap_map over any rectangle equals, byte for byte, the same slice of the map over
 *      all bins;
 *   3. M[I,J] and M[J,I] are byte-equal in sum1, sum2, hits and count, in one call and across calls (the lower bin index is
 *      always the outer loop);
 *   4. hits equal a restatement that computes r2 by the same rounded operations, exactly;
 *   5. all terms are non-negative, so sum2 is within (2 count + 8) 2^-53 (relative) of any other order of summation of the
 *      same terms, and so is sum1 given that sqrt is correctly rounded (it is: the device library's fp64 sqrt refines
 *      v_rsq_f64 with fused steps to the correctly rounded result when, as here, no fast-math flag is given; gdyn_rdf.h and
 *      gdyn_dcorr.h rest their bin indices on the same fact);
 *   6. integer coordinates on a line with |x| < 2^11 make r an integer and every sum exact.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_DMAP_H
#define GDYN_DMAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_DMAP_ABI_VERSION 1
#define GD_DMAP_MAX_THRESHOLDS 4
#define GD_DMAP_FRAME_RANGE 64      /* frames of one serial partial sum */
#define GD_DMAP_PIECE_BEADS 32      /* beads of one piece of a bin */

typedef struct gd_dmap gd_dmap;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                /* HIP device ordinal */
    uint32_t max_frames_per_stage;  /* frames staged in LDS at once; 0: automatic; no result depends on it */
} gd_dmap_desc;

int gd_dmap_abi_version(void);
int gd_dmap_create(const gd_dmap_desc *desc, gd_dmap **out);
int gd_dmap_destroy(gd_dmap *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_dmap_set_history(gd_dmap *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_dmap_set_history_live(gd_dmap *h, gd_live_history *history, uint32_t replica);
/* ranges: (B, 2) [start, end) pairs, ascending, non-empty, not overlapping, end <= N; NULL with n_bins == 0: every bead its own bin.
 * GD_ESTATE without a history */
int gd_dmap_set_bins(gd_dmap *h, const uint32_t *ranges, uint32_t n_bins);
/* The cells [row_first, row_first + n_rows) x [col_first, col_first + n_cols) of the map over the frames [first_frame, first_frame +
 * n_frames).  box: 3 periods or NULL (open).  sum1, sum2 (double), count (uint64): (n_rows, n_cols); hits (uint64): (n_thresholds,
 * n_rows, n_cols).  sum1, sum2 and hits may each be NULL (then nothing is computed for them).  GD_EINVAL: an empty region or one past
 * B, n_frames == 0 or a window past F, more than GD_DMAP_MAX_THRESHOLDS thresholds or one that is not positive and finite, a period
 * that is not.  GD_ENOMEM: the outputs do not fit on the device. */
int gd_dmap_map(gd_dmap *h, uint32_t row_first, uint32_t n_rows, uint32_t col_first, uint32_t n_cols, uint32_t first_frame, uint32_t n_frames,
                const double *box, const double *thresholds, uint32_t n_thresholds, double *sum1, double *sum2, uint64_t *hits, uint64_t *count);

#ifdef __cplusplus
}
#endif

#endif
