/* gdyn_cmap.h -- C-ABI of the contact-map analyses of libgdyn: the accumulations of the reference's stage-5 analyses that
 * read the stored contact maps (/snapshots/interphase/<step>/contact_map, uint32 (M, 3) rows (i, j, count)):
 *   contact_map         collect_contact_matrix   (contact_map.py:44-95)            -> a region target
 *   gw_contact_matrix   collect_contacts         (gw_contact_matrix/command.py:87-100) -> a binned target
 *   nad_profile         collect_nucleolus_contacts (nad_profile.py:88-94)          -> a nucleolus profile target
 *   power_law           collect_contact_profile  (power_law.py:61-82)              -> a separation profile target
 *
 * A gd_cmap handle is bound to one device.  It owns device-resident int32 accumulators ("targets", at most
 * GD_CMAP_MAX_TARGETS) and gd_cmap_accumulate streams rows through every one of them in one pass.  With v the count of a
 * row (i, j, v):
 *   region(beg, end)             dense (end - beg)^2; a row with beg <= i, j < end adds v at [i - beg, j - beg].
 *                                gd_cmap_finish replaces the matrix by M + M^T and then sets its diagonal to the maximum of
 *                                that sum (the last two lines of collect_contact_matrix).
 *   binned(rebin_map[n], n_bins) dense n_bins^2; rows with i >= n or j >= n are ignored, the others add v at [b_i, b_j] and
 *                                at [b_j, b_i] (a pair inside one bin adds 2 v to the diagonal).
 *   nucleolus profile(beg, end, is_nucleolus[n_particles])
 *                                length end - beg; [i - beg] += v where beg <= i < end and j is nucleolar, and
 *                                [j - beg] += v where beg <= j < end and i is nucleolar.  These are true sums
 *                                (np.add.at): the reference's fancy-index += keeps one row per repeated index of an HDF5
 *                                chunk and so depends on the file's chunk layout (rule 3).
 *   separation profile(chain_id[n_particles], size)
 *                                length size; [|i - j|] += v where chain_id[i] == chain_id[j] != -1.
 * An index at or beyond n_particles is neither nucleolar nor in a chain.
 *
 * Every sum is a 32-bit integer sum (the reference's outputs are int32): results are byte-identical from run to run and for
 * every max_rows_per_launch.  A cell whose count exceeds 2^31 - 1 is outside the contract.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not
 * part of gdyn.h's ABI. */
#ifndef GDYN_CMAP_H
#define GDYN_CMAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_CMAP_ABI_VERSION 1
#define GD_CMAP_MAX_TARGETS 16
/* profile bins of a handle that are privatised in one LDS histogram per block (48 KiB); the bins of profiles added beyond
 * this budget are updated with global atomics */
#define GD_CMAP_LDS_BINS 12288
/* largest side of a dense target */
#define GD_CMAP_MAX_SIDE 131072

typedef struct gd_cmap gd_cmap;

typedef struct {
    int32_t  device;               /* HIP device ordinal */
    uint32_t max_rows_per_launch;  /* rows uploaded and accumulated at a time; 0: automatic */
} gd_cmap_desc;

int gd_cmap_abi_version(void);
int gd_cmap_create(const gd_cmap_desc *desc, gd_cmap **out);
int gd_cmap_destroy(gd_cmap *h);
/* Each gd_cmap_add_* creates a zeroed target and stores its index in *target.  The arrays are copied. */
int gd_cmap_add_region(gd_cmap *h, uint32_t beg, uint32_t end, int32_t *target);
/* rebin_map: n values in [0, n_bins) */
int gd_cmap_add_binned(gd_cmap *h, const int32_t *rebin_map, uint32_t n, uint32_t n_bins, int32_t *target);
int gd_cmap_add_nucleolus_profile(gd_cmap *h, uint32_t beg, uint32_t end, const uint8_t *is_nucleolus, uint32_t n_particles,
                                  int32_t *target);
/* chain_id: -1 for beads outside every chain.  GD_EINVAL when two beads of one chain lie size or more apart. */
int gd_cmap_add_separation_profile(gd_cmap *h, const int32_t *chain_id, uint32_t n_particles, uint32_t size, int32_t *target);
/* rows: n_rows * 3 uint32 (i, j, count).  n_rows == 0 is a no-op. */
int gd_cmap_accumulate(gd_cmap *h, const uint32_t *rows, uint64_t n_rows);
/* a region target: M <- M + M^T, then diagonal <- max(M).  GD_EINVAL for any other kind. */
int gd_cmap_finish(gd_cmap *h, int32_t target);
/* the number of int32 values gd_cmap_fetch writes for the target */
int gd_cmap_target_size(gd_cmap *h, int32_t target, uint64_t *count);
int gd_cmap_fetch(gd_cmap *h, int32_t target, int32_t *out);
/* zeroes every accumulator and the counters; the targets stay */
int gd_cmap_reset(gd_cmap *h);
/* removes every target */
int gd_cmap_clear(gd_cmap *h);
/* out[0]: updates of binned targets requested by the rows since the last reset (one per row that counts and binned target);
 * out[1]: global atomics issued for them after equal keys of adjacent rows were combined in the wave */
int gd_cmap_counters(gd_cmap *h, uint64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif
