/* gdyn_vanhove.h -- C-ABI of the van Hove functions of libgdyn: the distribution of the displacements of single beads over a lag
 * (the self part G_s(r, tau): what single-locus tracking reports, and what shows two populations where the moments of gdyn_msd.h
 * cannot), and the density of OTHER beads at distance r from where a bead was tau ago (the distinct part G_d(r, tau), whose tau = 0
 * slice is gdyn_rdf.h's).  Nothing in the reference computes either: this is a capability beyond it (csrc/gdyn_vanhove.hip).  Every
 * output is an integer count.
 *
 * History.  A gd_vanhove handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the
 * precision it was given.  A history with a non-finite coordinate is refused (GD_EINVAL) and leaves the handle without one.
 *
 * Labels.  label[i] in [-1, K), K <= GD_VANHOVE_MAX_LABELS; a bead with label -1 takes no part.  Without labels there is one label
 * of all beads.  Labels belong to a history: they are set after it (GD_ESTATE before), kept by a new history of the same N and
 * dropped by one of another N.
 *
 * Origins.  Origin k is the frame f_k = first + k stride, k < count; count == 0 takes all with f_k < F.  O is the number selected.
 * An origin takes part in lag tau when f_k + tau < F.  Lags are in frames of the history, as in gdyn_dcorr.h.  A lag with no
 * origin is legal and gives zeros.  stride == 0, an explicit origin >= F and a lag listed twice are GD_EINVAL.  At most
 * GD_VANHOVE_MAX_LAGS lags a call.
 *
 * Edges.  B + 1 finite edges, 0 <= e_0 < ... < e_B, 1 <= B <= GD_VANHOVE_MAX_BINS.  A squared distance r2 falls in bin b when
 * e_b * e_b <= r2 < e_{b+1} * e_{b+1}, each product rounded once (fp64).  No sqrt is taken anywhere: the counts can equal numpy's
 * exactly, and linear and logarithmic radial bins follow one rule.
 *
 * Arithmetic.  fp64 on the widened coordinates, every operation rounded on its own (no contraction, no fast-math).
 *
 * Self part, gd_vanhove_self.  Lags >= 1.  axes is a non-zero mask of the components that enter (x = 1, y = 2, z = 4; 3 is the
 * microscope's projection).  For a selected bead i, per axis d = double(X[f+tau, i]) - double(X[f, i]);
 *     r2 = (tx + ty) + tz,   t_a = d_a * d_a for a masked axis and +0.0 otherwise.
 *   Outputs, all uint64, each pointer may be NULL:
 *     counts[L, K, B]         pooled over the origins of the lag;
 *     below[L, K]             r2 < e_0 * e_0;
 *     above[L, K]             r2 >= e_B * e_B;
 *     per_origin[L, O, K, B]  per origin; the rows of origins that do not take part in a lag are zero;
 *     origins[L]              the number of origins that take part, a closed form computed on the host.
 *   Per lag and label:  sum_b counts + below + above = members(label) * origins(lag).
 *   The overlap Q(tau) and chi_4(tau) are the caller's cumulative sums of per_origin (vanhove.py).
 *
 * Distinct part, gd_vanhove_distinct.  Lags >= 0, an optional box of three periods, always 3D.  For an ORDERED pair of distinct
 * selected beads (i, j), i != j, per axis d = double(X[f+tau, j]) - double(X[f, i]); with box != NULL reduced by
 * d -= box * nearbyint(d / box) (round half to even; the history is unwrapped, as everywhere);  r2 = (dx*dx + dy*dy) + dz*dz.
 *   The pair counts when e_0 * e_0 <= r2 < e_B * e_B, once per ordered pair and at its minimum image for any e_B in a periodic
 *   box (the rule of gdyn_rdf.h and gdyn_dcorr.h).  A bead that sits at tau exactly where another sat at 0 has r2 = 0 and counts
 *   when e_0 = 0.  The class of a pair is a * K + b, a the label of i (the bead at the origin frame), b that of j.
 *   Outputs, uint64:  counts[L, K * K, B] pooled over the origins of the lag, and origins[L] (may be NULL).
 *   (a, b) and (b, a) differ for tau > 0; at tau = 0 the table is symmetric and its diagonal classes are twice the unordered pair
 *   counts.
 *
 * Only integer atomics are used.  What follows:
 *   1. every output equals the numpy restatement (tests/vanhove_restatement.py) exactly, for float32 and float64 histories;
 *   2. results do not depend on max_frames_per_tile or max_frames_per_launch, nor on the code path (block histogram or direct);
 *   3. results of a lag do not depend on what else the call lists (other lags, their order) and results of a label not on the beads
 *      of other labels;
 *   4. results do not depend on whether a float32 history was fed from the host or from a recorder;
 *   5. an origin selection equals the history cut by the caller where that is expressible: (first, 1, 0) equals all origins of
 *      the frames [first, F), and (0, stride, 0) with lags that stride divides equals every stride-th frame with the lags
 *      divided by stride;
 *   6. per lag and label the self identity above holds; per_origin summed over origins is counts;
 *   7. the distinct table at tau = 0 is symmetric under (a, b) <-> (b, a) and equals twice gdyn_rdf.h's / gdyn_dcorr.h's unordered
 *      counts on its diagonal classes where no pair lies on an edge (those take sqrt; this header takes none);
 *   8. results are bit-identical from run to run.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_VANHOVE_H
#define GDYN_VANHOVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_VANHOVE_ABI_VERSION 1
#define GD_VANHOVE_MAX_LAGS 32           /* lags of one call */
#define GD_VANHOVE_MAX_BINS 256          /* radial bins of one call */
#define GD_VANHOVE_MAX_LABELS 8
#define GD_VANHOVE_LDS_CELLS 6144        /* a block histogram of up to this many uint32 cells lives in LDS (self: lags x labels x
                                            (bins + 2); distinct: labels^2 x bins); above it counts go straight to the global table.
                                            No result depends on it */
#define GD_VANHOVE_AXES_X 1u
#define GD_VANHOVE_AXES_Y 2u
#define GD_VANHOVE_AXES_Z 4u

typedef struct gd_vanhove gd_vanhove;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                  /* HIP device ordinal */
    uint32_t max_frames_per_tile;     /* self part: frames of one LDS window of a tile of beads; 0: automatic (all that fit); no
                                         result depends on it */
    uint32_t max_frames_per_launch;   /* distinct part: (origin, lag) frame pairs of one batch; 0: automatic; no result depends on it */
} gd_vanhove_desc;

typedef struct {
    const uint32_t *lags;             /* n_lags distinct lags, in any order */
    uint32_t n_lags;                  /* 1 .. GD_VANHOVE_MAX_LAGS */
    const double *edges;              /* n_bins + 1 edges */
    uint32_t n_bins;                  /* 1 .. GD_VANHOVE_MAX_BINS */
    uint32_t first, stride, count;    /* the origins (see Origins) */
} gd_vanhove_spec;

typedef struct {
    uint64_t *counts, *below, *above, *per_origin, *origins;      /* see Self part; each may be NULL */
} gd_vanhove_self_out;

int gd_vanhove_abi_version(void);
int gd_vanhove_create(const gd_vanhove_desc *desc, gd_vanhove **out);
int gd_vanhove_destroy(gd_vanhove *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_vanhove_set_history(gd_vanhove *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_vanhove_set_history_live(gd_vanhove *h, gd_live_history *history, uint32_t replica);
/* label: N values in [-1, n_labels), n_labels <= GD_VANHOVE_MAX_LABELS; NULL with n_labels <= 1: one label of all beads.  GD_ESTATE
 * without a history */
int gd_vanhove_set_labels(gd_vanhove *h, const int32_t *label, uint32_t n_labels);
/* the number of origins a selection makes of the handle's history (O); 0 for an illegal one */
uint32_t gd_vanhove_origins(const gd_vanhove *h, uint32_t first, uint32_t stride, uint32_t count);
/* GD_ESTATE without a history; GD_EINVAL: stride 0, an origin >= F, lag 0, a lag twice, no or too many lags or bins, edges that are
 * not finite, negative or not ascending, axes 0 or > 7, a NULL spec, out, lags or edges */
int gd_vanhove_self(gd_vanhove *h, const gd_vanhove_spec *spec, uint32_t axes, const gd_vanhove_self_out *out);
/* box: 3 periods, positive and finite, or NULL (open).  counts must not be NULL.  Errors as gd_vanhove_self (lag 0 is legal) */
int gd_vanhove_distinct(gd_vanhove *h, const gd_vanhove_spec *spec, const double *box, uint64_t *counts, uint64_t *origins);
/* Device times in milliseconds, between events on the handle's stream, of the last successful gd_vanhove_self or
 * gd_vanhove_distinct, summed over its launches: the counting kernel (k_vh_self, k_vh_pairs), the cell index of the distinct part
 * (0 for the self part) and the clearing of the self part's tables (0 for the distinct part).  0 before the first, and after a
 * call in which no lag had an origin.  Each pointer may be NULL.  What tools/bench_vanhove.py reports. */
int gd_vanhove_last_times(const gd_vanhove *h, double *count_ms, double *index_ms, double *other_ms);

#ifdef __cplusplus
}
#endif

#endif
