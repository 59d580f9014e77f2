/* gdyn_dwell.h -- C-ABI of the contact dwell times of libgdyn: for given pairs of beads of a history, for how long a contact lasts, how
 * long two beads wait until they first meet, and the contact autocorrelation (the time-domain observables of pairs; the contact
 * frequency itself is gdyn_dmap.h's).  Nothing in the reference computes any of it: this is a capability beyond it
 * (csrc/gdyn_dwell.hip).  Every output is an integer.
 *
 * History.  A gd_dwell handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the precision
 * it was given.  A history with a non-finite coordinate is refused (GD_EINVAL) and leaves the handle without one.
 *
 * Chains.  Ranges [start, end) of beads, ascending and not overlapping, end <= N; empty ranges are allowed.  With none set there is
 * one chain [0, N).  Chains belong to a history: they are set after it (GD_ESTATE before), kept by a new history of the same N and
 * dropped by one of another N.
 *
 * Frames.  Every call selects the frames f_k = first + k stride, k < count; count == 0 takes all with f_k < F.  An explicit frame
 * with f_k >= F, stride 0 or a selection of no frame is GD_EINVAL.  K is the number of selected frames; run lengths and lags are
 * counted in selected frames.
 *
 * Pair term (that of gdyn_dmap.h).  fp64 on the widened coordinates, every operation rounded on its own (no contraction, no
 * fast-math).  For beads i != j in a frame f:
 *     d = double(X[f,i]) - double(X[f,j]) per axis; with box != NULL reduced by d -= box * nearbyint(d / box) (round half to even);
 *     r2 = (dx*dx + dy*dy) + dz*dz.
 *   No sqrt is taken anywhere.  r2 does not change when i and j change places: negation is exact and nearbyint is odd.
 *
 * State.  A rule has two radii 0 < r_on <= r_off, finite.  With on_k = r2 < r_on * r_on and hold_k = r2 < r_off * r_off at the
 * frame f_k (strict, each product rounded once):
 *     c_0 = on_0,     c_k = c_{k-1} ? hold_k : on_k.
 *   r_on == r_off is the plain threshold, r_on < r_off the usual hysteresis against recrossing.  A pair exactly at r_on does not
 *   enter; a pair exactly at r_off leaves.
 *
 * Runs.  A run is a maximal stretch of selected frames of one pair in one state c (0 apart, 1 in contact).  Its length l is counted
 * in selected frames; its kind is
 *     0 complete:        touches neither end of the selection;
 *     1 left-censored:   begins at k = 0 and ends before K - 1;
 *     2 right-censored:  begins after k = 0 and ends at K - 1;
 *     3 both:            the whole selection is one run.
 *   State-0 runs of kind 1 are first-passage times, state-0 runs of kind 3 pairs that never met.
 *
 * Bins.  B + 1 ascending edges, 1 <= e_0 < ... < e_B, 1 <= B <= GD_DWELL_MAX_BINS.  A length falls in bin b when e_b <= l < e_{b+1}.
 *
 * Rows.  The outputs are accumulated per row.  In gd_dwell_separations row m is the separation s_m: up to
 * GD_DWELL_MAX_SEPARATIONS separations, each >= 1, not necessarily distinct; the row's pairs are all (i, i + s_m) with both beads
 * inside one chain.  In gd_dwell_pairs the caller gives (P, 2) bead pairs, i != j, in any order, duplicates allowed; chains play no
 * part; row[P] in [0, R) names the row of every pair, and row == NULL makes every pair its own row, R = P.  A row without a pair is
 * all zero.
 *
 * Outputs, all uint64, each pointer may be NULL:
 *     runs[R, 2, 4, B]       the number of runs by row, state, kind and bin;
 *     outside[R, 2, 4]       runs whose length lies in no bin;
 *     length_sum[R, 2, 4]    the sum of l;
 *     hits[R, L]             for up to GD_DWELL_MAX_LAGS lags (0 allowed): the sum over the row's pairs and over k with k + lag < K
 *                            of c_k * c_{k+lag}; a lag with no such k gives 0;
 *     pairs[R]               the number of pairs of the row, a closed form computed on the host.
 *   The contact autocorrelation is hits[lag] / (pairs (K - lag)), the mean dwell time length_sum / sum of runs: the caller's
 *   divisions (dwell.py).
 *
 * gd_dwell_states returns c itself as (K, P) uint8, the contact kymograph of the given pairs.
 *
 * Only integer atomics are used.  What follows:
 *   1. every output equals the numpy restatement (tests/dwell_restatement.py) exactly, for float32 and float64 histories;
 *   2. results do not depend on pairs_per_launch, on what else the call lists (other separations, lags or bins) or on whether a
 *      float32 history was fed from the host or from a recorder;
 *   3. a frame selection knows only itself: selecting (first, stride, count) equals selecting all frames of the history cut to those
 *      frames by the caller;
 *   4. gd_dwell_pairs over the pairs (i, i + s) of the chains with row = the index of the separation equals gd_dwell_separations;
 *   5. per row, the sum of length_sum over states and kinds is K * pairs;
 *   6. per row, the runs of kinds 1 and 3 over both states, outside included, number pairs; so do the runs of kinds 2 and 3;
 *   7. hits at lag 0 is the sum over the kinds of length_sum of state 1;
 *   8. results are bit-identical from run to run.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_DWELL_H
#define GDYN_DWELL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_DWELL_ABI_VERSION 1
#define GD_DWELL_MAX_BINS 64             /* bins of the run lengths of one call */
#define GD_DWELL_MAX_LAGS 64             /* lags of one call */
#define GD_DWELL_MAX_SEPARATIONS 32      /* separations of one gd_dwell_separations */
#define GD_DWELL_PLANE_BYTES 268435456   /* the states of one launch (one bit per pair and selected frame, 64 frames to a word) stay
                                            within 256 MiB when pairs_per_launch is automatic */

typedef struct gd_dwell gd_dwell;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;               /* HIP device ordinal */
    uint32_t pairs_per_launch;     /* pairs of one kernel launch (gd_dwell_separations: first beads i, each with every separation);
                                      0: automatic (GD_DWELL_PLANE_BYTES); no result depends on it */
} gd_dwell_desc;

typedef struct {
    double r_on, r_off;            /* 0 < r_on <= r_off, finite */
    const double *box;             /* 3 periods, positive and finite, or NULL (open) */
    uint32_t first, stride, count; /* the frame selection (see Frames) */
} gd_dwell_rule;

typedef struct {
    const uint32_t *edges;         /* n_bins + 1 edges; NULL with n_bins == 0 only when neither runs nor outside is asked for */
    uint32_t n_bins;
    const uint32_t *lags;          /* n_lags lags; NULL with n_lags == 0: no hits */
    uint32_t n_lags;
} gd_dwell_spec;

typedef struct {
    uint64_t *runs, *outside, *length_sum, *hits, *pairs;      /* see Outputs; each may be NULL */
} gd_dwell_out;

int gd_dwell_abi_version(void);
int gd_dwell_create(const gd_dwell_desc *desc, gd_dwell **out);
int gd_dwell_destroy(gd_dwell *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_dwell_set_history(gd_dwell *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_dwell_set_history_live(gd_dwell *h, gd_live_history *history, uint32_t replica);
/* ranges: (C, 2) [start, end) pairs, ascending, not overlapping, empty allowed, end <= N; NULL with n_chains == 0: one chain [0, N).
 * GD_ESTATE without a history */
int gd_dwell_set_chains(gd_dwell *h, const uint32_t *ranges, uint32_t n_chains);
/* separations: n_separations values >= 1, 1 <= n_separations <= GD_DWELL_MAX_SEPARATIONS; R = n_separations.  GD_ESTATE without a
 * history; GD_EINVAL: the rule (radii, periods, frames), edges that do not ascend or e_0 == 0, too many bins, lags or separations, a
 * separation of 0, a NULL that is not optional; GD_ENOMEM: the outputs do not fit on the device */
int gd_dwell_separations(gd_dwell *h, const uint32_t *separations, uint32_t n_separations, const gd_dwell_rule *rule, const gd_dwell_spec *spec,
                         const gd_dwell_out *out);
/* pairs: (P, 2) beads, P >= 1, i != j, both < N; row: P rows in [0, n_rows), or NULL: every pair its own row, R = P (n_rows is not
 * read).  Errors as gd_dwell_separations, and GD_EINVAL: P == 0, i == j, a bead >= N, a row >= n_rows */
int gd_dwell_pairs(gd_dwell *h, const uint32_t *pairs, uint32_t n_pairs, const uint32_t *row, uint32_t n_rows, const gd_dwell_rule *rule,
                   const gd_dwell_spec *spec, const gd_dwell_out *out);
/* out: (K, P) uint8, c_k of pair p.  Errors as gd_dwell_pairs */
int gd_dwell_states(gd_dwell *h, const uint32_t *pairs, uint32_t n_pairs, const gd_dwell_rule *rule, uint8_t *out);
/* Device times in milliseconds, between events on the handle's stream, of the three kernels of the last successful
 * gd_dwell_separations or gd_dwell_pairs, summed over its launches: the states, the runs and the correlation (gd_dwell_states: the
 * states alone, the others 0).  0 before the first.  Each pointer may be NULL.  What tools/bench_dwell.py reports. */
int gd_dwell_last_times(const gd_dwell *h, double *states_ms, double *runs_ms, double *corr_ms);

#ifdef __cplusplus
}
#endif

#endif
