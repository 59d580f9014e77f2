// gdyn_live.hpp -- the seams of the live bridge (gdyn_live.hip, include/gdyn_live.h): what the stepper and the analyses
// hand each other inside libgdyn.  C++ linkage and hidden: none of it is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/gdyn.h"
#include "../../include/gdyn_cmap.h"
#include "../../include/gdyn_flow.h"
#include "../../include/gdyn_lamina.h"
#include "../../include/gdyn_live.h"
#include "../../include/gdyn_rdf.h"
#include "gdyn_types.h"

#define GD_SEAM __attribute__((visibility("hidden")))

// ---- the stepper (gdyn_capi.hip; the contact tables: gdyn_capi_contacts.hip).  Each call makes the system's device current and returns with its stream idle: what it
// hands out is not written again until the next call on the system.
struct gd_live_shape {
    int device;
    uint32_t N, R;
    bool periodic, has_wall;
    double box[3];
};
GD_SEAM gd_live_shape gd_live_shape_of(const gd_system *s);
// the contact tables (cap == 0: never updated) and the host mirror of their occupancy ([R], or NULL with cap == 0)
GD_SEAM int gd_live_contact_tab(gd_system *s, ContactTab *tab, const unsigned **occupancy);
// float32 (R, N, 3) in bead order in a device buffer of the system; quantize as in gd_get_positions_f32
GD_SEAM int gd_live_positions(gd_system *s, int quantize, const float **xyz);

// ---- the analyses.  who: the gd_live_* call the messages name.
GD_SEAM int gd_cmap_device(const gd_cmap *h);
GD_SEAM int gd_lamina_device(const gd_lamina *h);
GD_SEAM int gd_rdf_device(const gd_rdf *h);
// the table words of replicas r0 .. r0 + nr - 1 through every target; rows: their occupied words (host mirror)
GD_SEAM int gd_cmap_accumulate_tab(gd_cmap *h, const char *who, const ContactTab &tab, uint32_t r0, uint32_t nr, uint64_t rows);
// gd_lamina_distances / gd_lamina_contacts on float32 frames that lie on the handle's device
GD_SEAM int gd_lamina_distances_dev(gd_lamina *h, const char *who, const float *xyz_dev, uint32_t frames, uint32_t n_points,
                                    const double *semiaxes, void *out, int out_is_f64);
GD_SEAM int gd_lamina_contacts_dev(gd_lamina *h, const char *who, const float *xyz_dev, uint32_t frames, uint32_t n_points,
                                   const double *semiaxes, double contact_distance, uint8_t *contacts_out);
// gd_rdf_counts on float32 frames that lie on the handle's device; n_points must equal the selection's
GD_SEAM int gd_rdf_counts_dev(gd_rdf *h, const char *who, const float *xyz_dev, uint32_t frames, uint32_t n_points, const double box[3],
                              double bin_width, double max_distance, uint64_t *counts_out);
GD_SEAM int gd_flow_device(const gd_flow *h);
// a device-side gd_flow_set_history in two halves.  begin: the argument checks of the host-fed call, earlier velocities forgotten,
// and the handle's fp64 (frames, n_beads, 3) copy with the handle's stream, for the caller to fill there.  end, once that stream is
// idle: the handle holds the history, or none when the caller found it unusable (ok == false).
GD_SEAM int gd_flow_history_begin(gd_flow *h, const char *who, uint32_t frames, uint32_t n_beads, double **x, hipStream_t *stream);
GD_SEAM void gd_flow_history_end(gd_flow *h, uint32_t frames, uint32_t n_beads, bool ok);

// ---- the recorder (gdyn_live.hip), for an analysis that takes its frames as recorded (gdyn_history.hip): float32, frame f of a slot
// at gd_live_history_frame(h, f, slot), the frames of one block frame_stride floats apart.  The blocks are not written while the
// recorder's stream is idle, which every gd_live_history_* call leaves it.
struct gd_live_history_shape {
    int device;
    uint32_t N, frames, frames_per_block;
    size_t frame_stride;
};
GD_SEAM gd_live_history_shape gd_live_history_shape_of(const gd_live_history *h);
GD_SEAM int gd_live_history_slot(const gd_live_history *h, const char *who, uint32_t replica, uint32_t *slot);
GD_SEAM const float *gd_live_history_frame(const gd_live_history *h, uint32_t f, uint32_t slot);
