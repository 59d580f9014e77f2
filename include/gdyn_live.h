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
#include "gdyn_lamina.h"
#include "gdyn_rdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_LIVE_ABI_VERSION 1

int gd_live_abi_version(void);
/* the current contents of the contact table of one replica, or of all (GD_ALL_REPLICAS), streamed through every target of cm */
int gd_live_contacts(gd_system *sys, uint32_t replica, gd_cmap *cm);
/* out: R * N doubles when out_is_f64 != 0, else floats; NULL: nothing is copied back */
int gd_live_lamina_distances(gd_system *sys, gd_lamina *lam, int quantize, void *out, int out_is_f64);
/* contacts_out: R * N bytes (0 / 1), or NULL */
int gd_live_lamina_contacts(gd_system *sys, gd_lamina *lam, int quantize, double contact_distance, uint8_t *contacts_out);
/* counts_out: R * gd_rdf_bins(bin_width, max_distance) values */
int gd_live_rdf_counts(gd_system *sys, gd_rdf *rdf, int quantize, double bin_width, double max_distance, uint64_t *counts_out);

#ifdef __cplusplus
}
#endif

#endif
