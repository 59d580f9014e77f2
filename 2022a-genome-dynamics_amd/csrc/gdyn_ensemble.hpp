// gdyn_ensemble.hpp -- host side of the per-replica A/B tables (include/gdyn_ensemble.h): which (a, b) factors every replica of a
// handle carries, which replicas hold the same table, and the two decisions finalize_topology takes from them.  Plain C++: no HIP
// runtime, no handle, no environment (tests/native/test_ensemble_ab.cpp drives it alone).
//
// A handle has one SHARED table (gd_set_bead_params) and, per replica and column, either nothing -- the replica refers to the shared
// column -- or a column of its own.  A column that is set to the values of the shared one is dropped again, so a handle whose
// replicas were all set back is in the state of one that was never touched.
//   homogeneous()  every replica's table equals every other's, however that came about: one table of N entries serves the handle
//                  and the bond records can be mixed per bond on the host
//   fp16_exact()   every value of every replica is exact in fp16: the factors ride in pos.w
#ifndef GDYN_ENSEMBLE_HPP
#define GDYN_ENSEMBLE_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gd {

// v == (double)(fp16)v.  Binary16: 11 significant bits, normal exponents -14 .. 15, subnormals in units of 2^-24; both infinities.
inline bool exact_in_fp16(double v)
{
    if (std::isnan(v)) return false;
    if (std::isinf(v) || v == 0.0) return true;
    int e = 0;
    const double m = std::frexp(std::fabs(v), &e);      // |v| = m 2^e, m in [0.5, 1)
    if (e > 16) return false;
    const double units = e >= -13 ? std::ldexp(m, 11) : std::ldexp(std::fabs(v), 24);
    return units == std::floor(units);
}

class EnsembleAB {
public:
    void reset(uint32_t n_beads, uint32_t n_replicas)
    {
        N = n_beads; R = n_replicas;
        shared_[0].assign(N, 0.0); shared_[1].assign(N, 0.0);
        own_.assign(R, Rep{});
    }
    uint32_t beads() const { return N; }
    uint32_t replicas() const { return R; }
    // gd_set_bead_params: a non-NULL column replaces that column of EVERY replica
    void set_shared(const double *a, const double *b)
    {
        const double *src[2] = {a, b};
        for (int c = 0; c < 2; c++) {
            if (!src[c]) continue;
            shared_[c].assign(src[c], src[c] + N);
            for (auto &rep : own_) rep.col[c].clear();
        }
    }
    // One replica's columns (NULL: kept).  0, or 1 + the index of the first non-finite value; a refused set changes nothing.
    size_t set(uint32_t r, const double *a, const double *b)
    {
        const double *src[2] = {a, b};
        for (int c = 0; c < 2; c++)
            for (uint32_t i = 0; src[c] && i < N; i++) if (!std::isfinite(src[c][i])) return (size_t)i + 1;
        for (int c = 0; c < 2; c++) {
            if (!src[c]) continue;
            bool same = true;
            for (uint32_t i = 0; same && i < N; i++) same = src[c][i] == shared_[c][i];
            if (same) own_[r].col[c].clear();
            else own_[r].col[c].assign(src[c], src[c] + N);
        }
        return 0;
    }
    // column c (0: a, 1: b) of replica r as the next evaluation uses it
    const double *column(uint32_t r, int c) const { return own_[r].col[c].empty() ? shared_[c].data() : own_[r].col[c].data(); }
    double a(uint32_t r, uint32_t i) const { return column(r, 0)[i]; }
    double b(uint32_t r, uint32_t i) const { return column(r, 1)[i]; }
    void get(uint32_t r, double *a_out, double *b_out) const
    {
        double *dst[2] = {a_out, b_out};
        for (int c = 0; c < 2; c++)
            for (uint32_t i = 0; dst[c] && i < N; i++) dst[c][i] = column(r, c)[i];
    }
    // class_of[R]: replicas with equal tables share a class; classes are numbered by first appearance.  Returns their number.
    uint32_t classes(uint32_t *class_of) const
    {
        std::vector<uint32_t> first;      // the first replica of every class
        std::vector<uint64_t> hash(R);
        for (uint32_t r = 0; r < R; r++) {
            hash[r] = table_hash(r);
            uint32_t k = 0;
            while (k < first.size() && !(hash[first[k]] == hash[r] && same_table(first[k], r))) k++;
            if (k == first.size()) first.push_back(r);
            class_of[r] = k;
        }
        return (uint32_t)first.size();
    }
    bool homogeneous() const
    {
        for (uint32_t r = 1; r < R; r++) if (!same_table(0, r)) return false;
        return true;
    }
    bool fp16_exact() const
    {
        for (int c = 0; c < 2; c++) {
            bool shared_used = false;
            for (auto &rep : own_) {
                if (rep.col[c].empty()) { shared_used = true; continue; }
                for (double v : rep.col[c]) if (!exact_in_fp16(v)) return false;
            }
            if (shared_used) for (double v : shared_[c]) if (!exact_in_fp16(v)) return false;
        }
        return true;
    }

private:
    struct Rep { std::vector<double> col[2]; };      // empty: the shared column
    bool same_table(uint32_t p, uint32_t q) const
    {
        for (int c = 0; c < 2; c++) {
            const double *x = column(p, c), *y = column(q, c);
            if (x == y) continue;
            for (uint32_t i = 0; i < N; i++) if (x[i] != y[i]) return false;
        }
        return true;
    }
    // FNV-1a over the values (0.0 and -0.0 compare equal, so they hash alike)
    uint64_t table_hash(uint32_t r) const
    {
        uint64_t h = 1469598103934665603ull;
        for (int c = 0; c < 2; c++) {
            const double *x = column(r, c);
            for (uint32_t i = 0; i < N; i++) {
                const double v = x[i] == 0.0 ? 0.0 : x[i];
                uint64_t w;
                static_assert(sizeof w == sizeof v, "64-bit doubles");
                __builtin_memcpy(&w, &v, sizeof w);
                h = (h ^ w) * 1099511628211ull;
            }
        }
        return h;
    }
    uint32_t N = 0, R = 0;
    std::vector<double> shared_[2];
    std::vector<Rep> own_;
};

}      // namespace gd

#endif
