// gdyn_history.hpp -- the trajectory history of an analysis handle (gd_msd, gd_dcorr, gd_dmap, gd_sq, gd_cluster, gd_dcov, gd_gyr): (F, N, 3) coordinates on the
// device in the precision they came in, fed from the host or from a recorder (gdyn_live.hip), and held only when every
// coordinate is finite; and what those handles keep per bead of it: the label selection (gd_dcorr, gd_cluster), the check of a label
// array (gd_sq and gd_msd too) and ranges of beads (gd_dmap, gd_dcov).  gdyn_history.hip; C++ linkage and hidden, like the seams of gdyn_live.hpp: none of it is exported.
#pragma once
#include <functional>
#include <vector>

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

// `label` of N beads with K labels (`noun`: "label", "group"): every value in [-1, K), -1 for a bead that takes no part.  Without an
// array there is one label of all beads, so K is at most 1
GD_SEAM int check_labels(const char *who, const char *noun, const int32_t *label, unsigned N, unsigned K);

// The beads of a history that take part in gd_dcorr and gd_cluster and their labels: all beads under one label, or those whose label
// is not -1.  A call that fails leaves the selection as it was.
struct GD_SEAM LabelSelection {
    unsigned K = 1, n_sel = 0;
    bool have_labels = false;
    std::vector<uint64_t> members;      // beads per label
    dbuf<unsigned> sel;                 // the selected beads, ascending
    dbuf<int> label_dev;

    const int *labels() const { return have_labels ? label_dev.p : nullptr; }
    int select_all(unsigned N);
    // the body of gd_<x>_set_labels (`who`) of a handle on `device` that holds a history of N beads; at most max_labels labels
    int set(const char *who, int device, const int32_t *label, uint32_t n_labels, unsigned max_labels, unsigned N);
};

// Ascending ranges of the beads of a history that a handle holds on the host and on the device (`noun`: "bin"): the caller's
// (have) or every bead its own range.  The device copy is replaced only when the new one has been made.
struct GD_SEAM BeadRanges {
    bool have = false;
    std::vector<uint32_t> host;      // (count, 2)
    dbuf<uint32_t> dev;

    unsigned count() const { return (unsigned)(host.size() / 2); }
    uint32_t length(size_t r) const { return host[2 * r + 1] - host[2 * r]; }
    int every_bead(unsigned N);
    // the body of gd_<x>_set_<noun>s (`who`) of a handle on `device` that holds a history of N beads; at most 2^limit_bits ranges,
    // none empty; n == 0: every bead its own range again
    int set(const char *who, const char *noun, int device, const uint32_t *ranges, uint32_t n, unsigned limit_bits, unsigned N);
    int check(const char *who, const char *noun, unsigned N) const { return check_ranges(who, noun, false, host.data(), count(), N); }

private:
    int install(std::vector<uint32_t> ranges, bool have_now);
};

}  // namespace gd
