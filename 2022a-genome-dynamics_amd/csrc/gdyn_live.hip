// gdyn_live.hip -- the bridge of include/gdyn_live.h: the device analyses fed from a running stepper's device-resident state.
// It checks that the two handles of a call fit each other and joins the seams of gdyn_live.hpp: the stepper hands out its contact
// tables or its positions in bead order with its stream idle, and the analysis runs its own kernels on them on its own
// stream (k_cmap_accumulate_tab in gdyn_cmap.hip; the distance, contact and pair-count kernels of gdyn_lamina.hip and
// gdyn_rdf.hip, which take the frames from device memory).  Every call returns with the analysis stream idle too, so the
// next gd_run finds the buffers unread.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/gdyn_live.h"
#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"

using namespace gd;

namespace {

int same_device(const char *who, const gd_live_shape &v, int device)
{
    if (v.device != device) return fail(GD_EINVAL, "%s: the system is on device %d, the analysis handle on device %d", who, v.device, device);
    return GD_OK;
}

// the semiaxes gd_get_context reports, replica by replica
int wall_semiaxes(gd_system *sys, const gd_live_shape &v, std::vector<double> &semiaxes)
{
    semiaxes.resize((size_t)v.R * 3);
    for (uint32_t r = 0; r < v.R; r++) {
        gd_context c;
        if (int rc = gd_get_context(sys, r, &c)) return rc;
        for (int k = 0; k < 3; k++) semiaxes[3 * (size_t)r + k] = c.semiaxes[k];
    }
    return GD_OK;
}

int lamina_frames(const char *who, gd_system *sys, gd_lamina *lam, int quantize, gd_live_shape *v, std::vector<double> &semiaxes, const float **xyz)
{
    if (!sys || !lam) return fail(GD_EINVAL, "%s: NULL handle", who);
    *v = gd_live_shape_of(sys);
    if (int rc = same_device(who, *v, gd_lamina_device(lam))) return rc;
    if (!v->has_wall) return fail(GD_EINVAL, "%s: the system has no ellipsoid wall", who);
    if (int rc = wall_semiaxes(sys, *v, semiaxes)) return rc;
    return gd_live_positions(sys, quantize, xyz);
}

}  // namespace

extern "C" {

int gd_live_abi_version(void) { return GD_LIVE_ABI_VERSION; }

int gd_live_contacts(gd_system *sys, uint32_t replica, gd_cmap *cm)
{
    if (!sys || !cm) return fail(GD_EINVAL, "gd_live_contacts: NULL handle");
    gd_live_shape const v = gd_live_shape_of(sys);
    if (replica != GD_ALL_REPLICAS && replica >= v.R) return fail(GD_EINVAL, "gd_live_contacts: replica %u of %u", replica, v.R);
    if (int rc = same_device("gd_live_contacts", v, gd_cmap_device(cm))) return rc;
    ContactTab tab;
    const unsigned *occupancy = nullptr;
    if (int rc = gd_live_contact_tab(sys, &tab, &occupancy)) return rc;
    if (tab.cap == 0) return GD_OK;                          // never updated
    uint32_t const r0 = replica == GD_ALL_REPLICAS ? 0 : replica, nr = replica == GD_ALL_REPLICAS ? v.R : 1;
    uint64_t rows = 0;
    for (uint32_t r = r0; r < r0 + nr; r++) rows += occupancy[r];
    return gd_cmap_accumulate_tab(cm, "gd_live_contacts", tab, r0, nr, rows);
}

int gd_live_lamina_distances(gd_system *sys, gd_lamina *lam, int quantize, void *out, int out_is_f64)
{
    gd_live_shape v;
    std::vector<double> semiaxes;
    const float *xyz = nullptr;
    if (int rc = lamina_frames("gd_live_lamina_distances", sys, lam, quantize, &v, semiaxes, &xyz)) return rc;
    return gd_lamina_distances_dev(lam, "gd_live_lamina_distances", xyz, v.R, v.N, semiaxes.data(), out, out_is_f64);
}

int gd_live_lamina_contacts(gd_system *sys, gd_lamina *lam, int quantize, double contact_distance, uint8_t *contacts_out)
{
    gd_live_shape v;
    std::vector<double> semiaxes;
    const float *xyz = nullptr;
    if (int rc = lamina_frames("gd_live_lamina_contacts", sys, lam, quantize, &v, semiaxes, &xyz)) return rc;
    return gd_lamina_contacts_dev(lam, "gd_live_lamina_contacts", xyz, v.R, v.N, semiaxes.data(), contact_distance, contacts_out);
}

int gd_live_rdf_counts(gd_system *sys, gd_rdf *rdf, int quantize, double bin_width, double max_distance, uint64_t *counts_out)
{
    if (!sys || !rdf) return fail(GD_EINVAL, "gd_live_rdf_counts: NULL handle");
    gd_live_shape const v = gd_live_shape_of(sys);
    if (int rc = same_device("gd_live_rdf_counts", v, gd_rdf_device(rdf))) return rc;
    if (!v.periodic) return fail(GD_EINVAL, "gd_live_rdf_counts: the system's box is open");
    const float *xyz = nullptr;
    if (int rc = gd_live_positions(sys, quantize, &xyz)) return rc;
    return gd_rdf_counts_dev(rdf, "gd_live_rdf_counts", xyz, v.R, v.N, v.box, bin_width, max_distance, counts_out);
}

}  // extern "C"
