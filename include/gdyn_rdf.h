/* gdyn_rdf.h -- C-ABI of the radial distribution analyses of libgdyn (device-side restatement of the pair search of the
 * reference's 4-sim-ab/box/src/rdf_analysis and rdf_analysis_hetero, distance_histogram.cc).
 *
 * A gd_rdf handle holds one selection of beads on one device:
 *   gd_rdf_set_selection  the centre indices and, in cross mode, the target indices into frames of n_points beads;
 *   gd_rdf_counts         per frame, the number of pairs in each distance bin, as uint64 (F, n_bins) row-major.
 * Self mode (target_idx == NULL): unordered pairs {i, j} of distinct centres (rdf_analysis: neighbor_searcher::search).
 * Cross mode: (centre, target) pairs (rdf_analysis_hetero: one neighbor_searcher::query per centre); the two lists must not
 * share an index.
 *
 * The rules, all arithmetic in fp64 on the (widened) input coordinates, without contraction:
 *   minimum image  d[k] -= box[k] * nearbyint(d[k] / box[k]) per axis, on the unwrapped coordinates as given;
 *   cutoff         a pair counts when (d0*d0 + d1*d1) + d2*d2 < max_distance * max_distance (strict);
 *   bin            (uint64)(sqrt(d0*d0 + d1*d1 + d2*d2) * (1 / bin_width)); a bin at or past n_bins is dropped;
 *   n_bins         ceil(max_distance / bin_width) (gd_rdf_bins);
 *   each pair is counted at most once, at its minimum-image distance, for any max_distance (also above box/2).
 * A pair with a non-finite coordinate is never counted.  Counts are integers: bit-identical from run to run and for every
 * max_frames_per_launch.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not
 * part of gdyn.h's ABI. */
#ifndef GDYN_RDF_H
#define GDYN_RDF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_RDF_ABI_VERSION 1

/* up to this many bins a block counts in LDS (uint32) and flushes its non-zero bins with one integer atomic each; above it every
 * pair is added to the global uint64 counts directly.  (Also direct: more than 2^24 partners per frame, where a block's uint32
 * counters could overflow.) */
#define GD_RDF_LDS_BINS 8192
#define GD_RDF_MAX_BINS (1u << 24)

typedef struct gd_rdf gd_rdf;

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t max_frames_per_launch;  /* frames binned and counted per launch; 0: automatic */
} gd_rdf_desc;

int gd_rdf_abi_version(void);
int gd_rdf_create(const gd_rdf_desc *desc, gd_rdf **out);
int gd_rdf_destroy(gd_rdf *h);
/* indices < n_points; either list may be empty (every count is then 0).  target_idx NULL: self mode (n_target ignored);
 * cross mode with an index in both lists: GD_EINVAL.  (A repeated index is a second, coincident point.) */
int gd_rdf_set_selection(gd_rdf *h, uint32_t n_points, const uint32_t *center_idx, uint32_t n_center, const uint32_t *target_idx,
                         uint32_t n_target);
/* n_bins of (bin_width, max_distance), or 0 when they are not positive and finite or n_bins exceeds GD_RDF_MAX_BINS */
uint32_t gd_rdf_bins(double bin_width, double max_distance);
/* xyz: frames * n_points * 3 values, float when is_f64 == 0, double otherwise; box: the three periods (positive, finite);
 * counts_out: frames * n_bins uint64 */
int gd_rdf_counts(gd_rdf *h, const void *xyz, int is_f64, uint32_t frames, const double box[3], double bin_width, double max_distance,
                  uint64_t *counts_out);

#ifdef __cplusplus
}
#endif

#endif
