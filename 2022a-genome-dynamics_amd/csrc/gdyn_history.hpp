// gdyn_history.hpp -- the trajectory history of an analysis handle (gd_msd, gd_dcorr, gd_dmap, gd_sq, gd_cluster, gd_dcov, gd_gyr): (F, N, 3) coordinates on the
// device in the precision they came in, fed from the host or from a recorder (gdyn_live.hip), and held only when every
// coordinate is finite.  gdyn_history.hip; C++ linkage and hidden, like the seams of gdyn_live.hpp: none of it is exported.
#pragma once
#include <functional>

#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"

namespace gd {

struct GD_SEAM History {
    unsigned F = 0, N = 0;         // F == 0: no history; N stays, for what the handle keeps per bead
    bool is_f64 = false;
    dbuf<float> xf;
    dbuf<double> xd;
    dbuf<unsigned long long> first_bad;

    const void *x() const { return is_f64 ? (const void *)xd.p : (const void *)xf.p; }
    size_t elem() const { return is_f64 ? sizeof(double) : sizeof(float); }
    unsigned frames() const { return F; }
    unsigned beads() const { return N; }

    // What a handle keeps per bead follows the bead count: rebind(n_beads) runs once the new history is on the device and finite,
    // while beads() is still the last history's.  When it fails the handle holds no history.
    using Rebind = std::function<int(unsigned n_beads)>;

    // The body of gd_<x>_set_history and gd_<x>_set_history_live (`who`) of a handle on `device` with `stream`.  A refusal of the
    // arguments leaves the history as it was; from then on it is gone until the call has succeeded.  Returns with the stream idle.
    int set_host(const char *who, int device, hipStream_t stream, const void *xyz, uint32_t frames, uint32_t n_beads, bool f64, const Rebind &rebind);
    int set_live(const char *who, int device, hipStream_t stream, gd_live_history *history, uint32_t replica, const Rebind &rebind);

private:
    int finish(const char *who, hipStream_t stream, unsigned frames, unsigned n_beads, bool f64, const Rebind &rebind);
};

// `count` [start, end) ranges of N beads (`noun`: "chain", "bin"): ascending and not overlapping, none reversed and, unless
// empty_allowed, none empty
GD_SEAM int check_ranges(const char *who, const char *noun, bool empty_allowed, const uint32_t *r, unsigned count, unsigned N);

}  // namespace gd
