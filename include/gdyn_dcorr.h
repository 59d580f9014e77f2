/* gdyn_dcorr.h -- C-ABI of the spatial correlation of bead displacements of libgdyn, C(r, tau): the mean of
 * D_i(tau) . D_j(tau) over pairs of beads a distance r apart, where D_i(tau) is the displacement of bead i over the lag tau.
 * The reference has no such analysis: this is a capability beyond it.  The pair search is gdyn_rdf.h's, the history handling
 * gdyn_msd.h's; the kernels are csrc/gdyn_dcorr.hip.
 *
 * A gd_dcorr handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64 as given.  All
 * arithmetic is fp64 on the widened coordinates, every operation rounded on its own (no contraction, no fast-math).
 *
 * Displacement, for a lag tau >= 1 and an origin frame f with f + tau < F:
 *     D[i] = double(X[f+tau,i]) - double(X[f,i]) per axis;   t2[i] = (Dx*Dx + Dy*Dy) + Dz*Dz.
 *   Nothing is subtracted: no drift, no centroid, no rotation (a caller who wants one removed subtracts it from a host-fed
 *   history).  Periodic systems store unwrapped coordinates.
 *
 * Selection and pair classes:
 *     label[i] in [-1, K), K <= GD_DCORR_MAX_LABELS; a bead with label -1 takes no part.  No labels set: one label (K = 1)
 *     of all beads.  chain[i]: an optional uint32 that splits pairs into same chain and different chain.
 *     The class of an unordered pair with labels a <= b is p = a*K - a*(a-1)/2 + (b - a); with chains set it is
 *     2*p + (chain_i != chain_j).  P = K*(K+1)/2, doubled with chains (gd_dcorr_classes).
 *
 * Pairs: the unordered pairs {i, j} of distinct selected beads, taken at the origin frame f, by the rules of gdyn_rdf.h:
 *     d = X[f,i] - X[f,j] per axis; in a periodic box (box != NULL) reduced by the minimum image d -= box * nearbyint(d / box),
 *     in an open box (box == NULL) used as it is;
 *     a pair counts when (dx*dx + dy*dy) + dz*dz < max_distance * max_distance (strict);
 *     bin = (uint64)(sqrt(r2) * (1 / bin_width)); a bin at or past n_bins = ceil(max_distance / bin_width) is dropped;
 *     coincident beads count in bin 0; each pair is counted once, for any max_distance in a periodic box.
 *
 * Term:  dot = (Dx_i*Dx_j + Dy_i*Dy_j) + Dz_i*Dz_j;   q = llrint(dot * 2^S), round half to even.
 *   Per origin f, class p and bin b:  count[f,p,b] (uint64) and sum[f,p,b] = sum of q (int64).  The sums are integers: the
 *   result does not depend on the order of arrival, on max_frames_per_launch or on the code path, and is bit-identical from
 *   run to run.  <D_i . D_j>(r) = sum / 2^S / count; that division and C(r) / C(0) are the caller's.
 *
 * Scale S and the overflow guard.  M: the largest t2 over the selected beads and origins of the call; n: the number of selected
 *   beads.  |dot| <= M (Cauchy-Schwarz), so a call is legal when  max(n*(n-1)/2, 1) * (M * 2^S + 1) < 2^62, evaluated exactly.
 *   scale_bits == 0 asks for the largest legal S in [0, GD_DCORR_MAX_SCALE_BITS]; scale_bits in [1, GD_DCORR_MAX_SCALE_BITS] is
 *   S itself and GD_DCORR_SCALE_UNIT is S = 0 (quantum 1: integer-valued displacements); an S that is not legal, or no legal
 *   S, is GD_EINVAL before any pair is walked.  The sums are per origin, so the guard does not tighten with the number of frames.
 *
 * Self terms, for normalisation: per origin and label, self_count (uint64) and self_sum = sum of llrint(t2 * 2^S) (int64).
 *
 * Origins are first_origin + k * origin_stride, k < n_origins; n_origins == 0: all that fit (gd_dcorr_origins tells how many,
 * possibly none: a lag >= F is legal then).  An explicit origin with f + lag >= F, lag 0 and origin_stride 0 are GD_EINVAL.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  Labels and chains belong to a history: they are set after it
 * (GD_ESTATE before), kept by a new history of the same N and dropped by one of another N.  This header has its own version:
 * the symbols below are not part of gdyn.h's ABI. */
#ifndef GDYN_DCORR_H
#define GDYN_DCORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_DCORR_ABI_VERSION 1

#define GD_DCORR_MAX_LABELS 8
#define GD_DCORR_MAX_SCALE_BITS 40
#define GD_DCORR_SCALE_UNIT (-1)
/* up to this many cells P * n_bins a block keeps its histogram in LDS (uint32 counts, 64-bit sums) and flushes its non-zero cells
 * with one 64-bit integer atomic each; above it every pair goes to the global tables directly.  (Also direct: 2^24 selected beads
 * or more, where a block's uint32 counters could overflow, and a device that grants too little LDS for the table.) */
#define GD_DCORR_LDS_BINS 8192
#define GD_DCORR_MAX_BINS (1u << 24)

typedef struct gd_dcorr gd_dcorr;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t max_frames_per_launch;  /* origins binned, sorted and paired per launch; 0: automatic; no result depends on it */
} gd_dcorr_desc;

int gd_dcorr_abi_version(void);
int gd_dcorr_create(const gd_dcorr_desc *desc, gd_dcorr **out);
int gd_dcorr_destroy(gd_dcorr *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_dcorr_set_history(gd_dcorr *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_dcorr_set_history_live(gd_dcorr *h, gd_live_history *history, uint32_t replica);
/* label: N values in [-1, n_labels), n_labels in [1, GD_DCORR_MAX_LABELS]; NULL (n_labels 0 or 1): one label of all beads */
int gd_dcorr_set_labels(gd_dcorr *h, const int32_t *label, uint32_t n_labels);
/* chain_id: N values, or NULL: pairs are not split by chain */
int gd_dcorr_set_chains(gd_dcorr *h, const uint32_t *chain_id);
/* n_bins of (bin_width, max_distance), or 0 when they are not positive and finite or n_bins exceeds GD_DCORR_MAX_BINS */
uint32_t gd_dcorr_bins(double bin_width, double max_distance);
/* P of the labels and chains in force (1 for a handle without a history; 0 for NULL) */
uint32_t gd_dcorr_classes(const gd_dcorr *h);
/* how many origins a call with these arguments covers (0 also for an invalid handle or stride) */
uint32_t gd_dcorr_origins(const gd_dcorr *h, uint32_t lag, uint32_t first_origin, uint32_t n_origins, uint32_t origin_stride);
/* box: the three periods (positive, finite), or NULL: open.  scale_used: the S of the sums.  count_out, sum_out: (origins, P, n_bins);
 * self_count_out, self_sum_out: (origins, K), or NULL */
int gd_dcorr_pairs(gd_dcorr *h, uint32_t lag, uint32_t first_origin, uint32_t n_origins, uint32_t origin_stride, const double *box,
                   double bin_width, double max_distance, int32_t scale_bits, int32_t *scale_used, uint64_t *count_out, int64_t *sum_out,
                   uint64_t *self_count_out, int64_t *self_sum_out);

#ifdef __cplusplus
}
#endif

#endif
