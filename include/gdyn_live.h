/* gdyn_live.h -- C-ABI of the bridge between a running stepper (gd_system, gdyn.h) and the device analyses of libgdyn
 * (gdyn_cmap.h, gdyn_lamina.h, gdyn_rdf.h): the analyses read the stepper's device-resident state in place of host arrays.
 *
 * Each call is defined by the host-fed sequence it replaces, and its results equal that sequence byte for byte
 * (DESIGN.md section 7g):
 *   gd_live_contacts(sys, r, cm)     gd_contacts_fetch(sys, r, rows, ...), then gd_cmap_accumulate(cm, rows, n); for
 *                                    GD_ALL_REPLICAS that sequence for r = 0 .. R - 1.  The words of the contact tables are
 *                                    read in place and empty words are skipped: nothing is compacted, sorted or copied, and
 *                                    the tables are not modified.  A table that was never updated, or was cleared, adds
 *                                    nothing.  gd_cmap_counters' out[0] grows as in the host-fed sequence; out[1] depends on
 *                                    the order of the rows and only satisfies 0 < out[1] <= out[0].
 *   gd_live_lamina_distances         gd_get_positions_f32(sys, xyz, quantize), the semiaxes of gd_get_context(sys, r) for
 *                                    every replica, then gd_lamina_distances(lam, xyz, 0, R, N, semiaxes, out, out_is_f64).
 *   gd_live_lamina_contacts          those distances as float32, kept on the device, then gd_lamina_contacts(lam, dist, R, N,
 *                                    contact_distance, contacts_out): the handle's sum, call count and shape rule behave as
 *                                    in the host-fed call.  contacts_out == NULL: only the sum is updated.
 *   gd_live_rdf_counts               gd_get_positions_f32(sys, xyz, quantize), then gd_rdf_counts(rdf, xyz, 0, R, the
 *                                    system's periods, bin_width, max_distance, counts_out) with the handle's selection.
 * Frames are the R replicas at the present step.
 *
 * The flow analyses (gdyn_flow.h) need a history of frames, not the present one.  A gd_live_history records it on the device
 * (DESIGN.md section 7h): float32 (F, N, 3) per selected replica, 12 bytes per bead and frame, in blocks of frames_per_block
 * frames that are allocated as needed and never moved.
 *   gd_live_history_record           appends, for every selected replica, what gd_get_positions_f32(sys, ., quantize) gives for
 *                                    it at the present step.  The system is not modified.  GD_ENOMEM when a new block cannot be
 *                                    allocated: the frames recorded so far stay valid and the count does not change.
 *   gd_live_history_fetch            frames [first, first + count) of one recorded replica, float32 (count, N, 3)
 *   gd_live_flow_set_history         gd_flow_set_history(flow, the F recorded frames of that replica, F, N, 0): earlier
 *                                    velocities are forgotten, GD_ESTATE when no frame was recorded, GD_EINVAL for a non-finite
 *                                    coordinate (the handle is then left without a history).  The frames are widened to the
 *                                    handle's fp64 copy on the device.
 *
 * Every call is synchronous: it waits for the stepper's stream before it reads, and its result is complete when it returns.
 * The two handles of a call must live on one device.  The lamina calls need a system with an ellipsoid wall, the rdf call a
 * periodic system and a selection over the system's N beads.  The argument checks of the host-fed calls apply unchanged.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not
 * part of gdyn.h's ABI. */
#ifndef GDYN_LIVE_H
#define GDYN_LIVE_H

#include <stdint.h>

#include "gdyn.h"
#include "gdyn_cmap.h"
#include "gdyn_flow.h"
#include "gdyn_lamina.h"
#include "gdyn_rdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_LIVE_ABI_VERSION 2

int gd_live_abi_version(void);
/* the current contents of the contact table of one replica, or of all (GD_ALL_REPLICAS), streamed through every target of cm */
int gd_live_contacts(gd_system *sys, uint32_t replica, gd_cmap *cm);
/* out: R * N doubles when out_is_f64 != 0, else floats; NULL: nothing is copied back */
int gd_live_lamina_distances(gd_system *sys, gd_lamina *lam, int quantize, void *out, int out_is_f64);
/* contacts_out: R * N bytes (0 / 1), or NULL */
int gd_live_lamina_contacts(gd_system *sys, gd_lamina *lam, int quantize, double contact_distance, uint8_t *contacts_out);
/* counts_out: R * gd_rdf_bins(bin_width, max_distance) values */
int gd_live_rdf_counts(gd_system *sys, gd_rdf *rdf, int quantize, double bin_width, double max_distance, uint64_t *counts_out);

typedef struct gd_live_history gd_live_history;
/* a recorder on the system's device for systems of its N and R.  replicas: n_replicas distinct ids below R, in any order;
 * n_replicas == 0: all R.  frames_per_block == 0: blocks of about 256 MiB, at least one frame */
int gd_live_history_create(gd_system *sys, const uint32_t *replicas, uint32_t n_replicas, uint32_t frames_per_block, gd_live_history **out);
int gd_live_history_destroy(gd_live_history *h);
int gd_live_history_record(gd_live_history *h, gd_system *sys, int quantize);
int gd_live_history_frames(const gd_live_history *h, uint32_t *frames);
/* out: count * N * 3 floats */
int gd_live_history_fetch(gd_live_history *h, uint32_t replica, uint32_t first, uint32_t count, float *out);
/* keeps the blocks and sets the frame count to 0 */
int gd_live_history_clear(gd_live_history *h);
int gd_live_flow_set_history(gd_live_history *h, uint32_t replica, gd_flow *flow);

#ifdef __cplusplus
}
#endif

#endif
