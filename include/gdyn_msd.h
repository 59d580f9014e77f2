/* gdyn_msd.h -- C-ABI of the lag statistics of libgdyn: the mean squared displacement of beads against lag time, MSD(tau),
 * and the mean squared spatial distance of beads against their separation along a chain, R2(s).  Neither exists in the
 * reference: this is a capability beyond it.  Both are sums of squared differences between items a fixed lag apart in a
 * sequence (one bead's trajectory along the frame axis; one chain of one frame along the bead axis), and one kernel family
 * (csrc/gdyn_msd.hip) serves both.
 *
 * A gd_msd handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the precision
 * it was given.  The term of two items is computed in fp64, every operation rounded on its own (no contraction):
 *     d = double(b) - double(a) per axis;   t2(a, b) = (dx*dx + dy*dy) + dz*dz;   t4 = t2*t2
 *
 * Along time, for a lag tau >= 1 and bead i:
 *     m2[i, tau] = sum over f = 0 .. F-1-tau of t2(X[f,i], X[f+tau,i]);   m4 likewise of t4.
 *   gd_msd_time takes group[i] in [-1, G) (-1: in no group; no groups set: one group of all beads) and returns
 *     sum2[g, l] = sum over the beads of g of m2[i, lag_l], sum4 likewise, count[g, l] = |g| * max(0, F - lag_l).
 *   A lag >= F is legal (count 0, sums 0); lag 0 and a lag listed twice are GD_EINVAL.  MSD = sum2 / count, and the
 *   non-Gaussian parameter is 3 (sum4/count) / (5 (sum2/count)^2) - 1: both divisions are the caller's.
 *   gd_msd_time_per_bead(lag) returns m2[:, lag] (and m4), the mobility profile along the genome; lag >= F is GD_EINVAL.
 *
 * Along the chain, for chains [start_c, end_c) (ascending, not overlapping, end <= N), a separation s >= 1 and the frames
 * [first_frame, first_frame + n_frames):
 *     c2[c, s] = sum over the frames f and i = start_c .. end_c-1-s of t2(X[f,i], X[f,i+s]);   c4 likewise of t4;
 *     count[c, s] = n_frames * max(0, len_c - s)   (a separation at least as long as the chain: count 0, sums 0).
 *   Rg^2 of a chain follows from all its separations (sum over i<j of r_ij^2 / n^2), averaged over the frames; there is no separate call
 *   here.  Per frame, with the tensor, and for sliding windows: include/gdyn_gyr.h.
 *
 * Nothing is subtracted: no drift, no centroid.  Periodic systems store unwrapped coordinates, so MSD across box images is
 * already right.
 *
 * Summation.  All terms are non-negative, so any order is within count * 2^-53 (relative) of the exact sum.  The order used
 * depends only on the shapes (F, N, chains, groups): results are bit-identical from run to run, for every
 * max_items_per_tile, for a lag whatever other lags the call lists and in whatever order, and between a host-fed and a
 * live-fed history.  Integer-valued coordinates with |x| < 2^11 make every sum exact.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a
 * history with a non-finite coordinate leaves the handle without one.  Groups and chains belong to a history: they are set
 * after it (GD_ESTATE before: a group array has the history's N entries), checked against its N then and again at the call,
 * kept by a new history of the same N and dropped by one of another N.  This header has its own version: the symbols below
 * are not part of gdyn.h's ABI. */
#ifndef GDYN_MSD_H
#define GDYN_MSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_MSD_ABI_VERSION 1

typedef struct gd_msd gd_msd;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;              /* HIP device ordinal */
    uint32_t max_items_per_tile;  /* items of a sequence staged at once; 0: automatic; no result depends on it */
} gd_msd_desc;

int gd_msd_abi_version(void);
int gd_msd_create(const gd_msd_desc *desc, gd_msd **out);
int gd_msd_destroy(gd_msd *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_msd_set_history(gd_msd *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_msd_set_history_live(gd_msd *h, gd_live_history *history, uint32_t replica);
/* group: N values in [-1, n_groups), or NULL (then n_groups must be 0 or 1): one group of all beads.  GD_ESTATE without a history */
int gd_msd_set_groups(gd_msd *h, const int32_t *group, uint32_t n_groups);
/* ranges: (C, 2) [start, end) pairs, ascending, not overlapping, end <= N.  GD_ESTATE without a history */
int gd_msd_set_chains(gd_msd *h, const uint32_t *ranges, uint32_t n_chains);
/* sum2, sum4 (or NULL), count: (G, n_lags) each */
int gd_msd_time(gd_msd *h, const uint32_t *lags, uint32_t n_lags, double *sum2, double *sum4, uint64_t *count);
/* m2, m4 (or NULL): N each */
int gd_msd_time_per_bead(gd_msd *h, uint32_t lag, double *m2, double *m4);
/* sum2, sum4 (or NULL), count: (C, n_seps) each */
int gd_msd_chain(gd_msd *h, const uint32_t *seps, uint32_t n_seps, uint32_t first_frame, uint32_t n_frames, double *sum2, double *sum4,
                 uint64_t *count);

#ifdef __cplusplus
}
#endif

#endif
