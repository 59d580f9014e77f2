/* gdyn_cluster.h -- C-ABI of the connected clusters of libgdyn: per frame of a history, which selected beads form one domain in
 * real space (the connected components of the graph whose edges are the pairs of beads closer than a distance), how many domains
 * there are, how large the largest is and how their sizes are distributed.  The reference has no such analysis: this is a
 * capability beyond it.  The pair search is gdyn_rdf.h's, the history handling gdyn_msd.h's, the selection and the pair classes
 * gdyn_dcorr.h's; the kernels are csrc/gdyn_cluster.hip.
 *
 * A gd_cluster handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64 as given.  All
 * arithmetic is fp64 on the widened coordinates, every operation rounded on its own (no contraction, no fast-math).
 *
 * Selection and link classes:
 *     label[i] in [-1, K), K <= GD_CLUSTER_MAX_LABELS; a bead with label -1 takes no part.  No labels set: one label (K = 1)
 *     of all beads.
 *     The class of an unordered pair with labels a <= b is p = a*K - a*(a-1)/2 + (b - a), gd_dcorr's formula; P = K*(K+1)/2
 *     (gd_cluster_classes).
 *     A 64-bit link mask says which classes may link: bit p set, pairs of class p may link.  The default is all P classes.  A
 *     mask with a bit at or past P, or an empty mask, is GD_EINVAL.
 *     Labels and mask belong to a history: they are set after it (GD_ESTATE before), kept by a new history of the same N and
 *     dropped by one of another N.  A new label set resets the mask to all classes.
 *
 * Edges of frame f: the unordered pairs {i, j} of distinct selected beads with
 *     d = X[f,i] - X[f,j] per axis; in a periodic box (box != NULL) reduced by the minimum image d -= box * nearbyint(d / box),
 *     exactly as gdyn_rdf.h states it, in an open box (box == NULL) used as it is;
 *     (dx*dx + dy*dy) + dz*dz < distance * distance (strict), and the mask bit of the pair's class set.
 *     Coincident beads are linked.  distance must be positive and finite, and so must every period of the box.
 *
 * Result per frame f of the call:
 *     root[f, i] (int32): the smallest bead index of the connected component of bead i, -1 for a bead that is not selected.  This
 *         canonical form makes the output unique.
 *     summary[f, 0..3] (uint64): the number of selected beads, the number of clusters, the size of the largest cluster and the
 *         sum of s*s over the clusters of sizes s.  The weight-average size is summary[3] / summary[0]; that division is the
 *         caller's.  All four are 0 in a frame without a selected bead.
 *     hist[f, b] (uint64, b < n_size_bins): the number of clusters with min(s, n_size_bins) - 1 == b: sizes are counted exactly
 *         up to n_size_bins - 1 and the last bin collects the rest.  n_size_bins is 1 to GD_CLUSTER_MAX_SIZE_BINS.
 *     root and hist may each be NULL.
 *
 * Frames are first_frame + k * frame_stride, k < n_frames; n_frames == 0: all that fit (gd_cluster_frames tells how many).  An
 * explicit frame past the history and frame_stride 0 are GD_EINVAL.  A history of 2^31 beads or more is GD_EINVAL.
 *
 * Determinism.  Every output is an integer that depends on the graph alone, not on the order in which its edges are found or
 * joined.  The results are therefore bit-identical from run to run, for every max_frames_per_launch, for a frame whatever other
 * frames the call lists, and between a host-fed and a live-fed history.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_CLUSTER_H
#define GDYN_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_CLUSTER_ABI_VERSION 1

#define GD_CLUSTER_MAX_LABELS 8
#define GD_CLUSTER_MAX_SIZE_BINS (1u << 20)

typedef struct gd_cluster gd_cluster;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t max_frames_per_launch;  /* frames sorted, linked and counted per launch; 0: automatic; no result depends on it */
} gd_cluster_desc;

int gd_cluster_abi_version(void);
int gd_cluster_create(const gd_cluster_desc *desc, gd_cluster **out);
int gd_cluster_destroy(gd_cluster *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_cluster_set_history(gd_cluster *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_cluster_set_history_live(gd_cluster *h, gd_live_history *history, uint32_t replica);
/* label: N values in [-1, n_labels), n_labels in [1, GD_CLUSTER_MAX_LABELS]; NULL (n_labels 0 or 1): one label of all beads */
int gd_cluster_set_labels(gd_cluster *h, const int32_t *label, uint32_t n_labels);
/* link_mask: bit p set, pairs of class p may link; only bits below P, at least one */
int gd_cluster_set_links(gd_cluster *h, uint64_t link_mask);
/* P of the labels in force (1 for a handle without a history; 0 for NULL) */
uint32_t gd_cluster_classes(const gd_cluster *h);
/* how many frames a call with these arguments covers (0 also for an invalid handle or stride, or a first frame past the history) */
uint32_t gd_cluster_frames(const gd_cluster *h, uint32_t first_frame, uint32_t n_frames, uint32_t frame_stride);
/* box: the three periods (positive, finite), or NULL: open.  root_out: (frames, N) or NULL; summary_out: (frames, 4);
 * hist_out: (frames, n_size_bins) or NULL */
int gd_cluster_components(gd_cluster *h, uint32_t first_frame, uint32_t n_frames, uint32_t frame_stride, const double *box, double distance,
                          uint32_t n_size_bins, int32_t *root_out, uint64_t *summary_out, uint64_t *hist_out);

#ifdef __cplusplus
}
#endif

#endif
