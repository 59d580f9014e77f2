// gdyn_glue.hpp -- the pure logic of the device glue kinetics (include/gdyn_glue.h): the probabilities'
// integer thresholds, how a pair becomes a sort key and a Philox counter, how a replica's seed becomes the Philox key, the argument
// checks, and Philox4x32-10 itself.  Plain C++: no HIP runtime and no handle (tests/native/test_glue.cpp drives it alone); the
// kernels of gdyn_glue.hip compile the functions marked GD_GLUE_HD for the device too, so host and device share one text.
#ifndef GDYN_GLUE_HPP
#define GDYN_GLUE_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define GD_GLUE_HD __host__ __device__ inline
#else
#define GD_GLUE_HD inline
#endif

namespace gd {

constexpr uint32_t GLUE_KEY_TAG = 0x474C5545u;      // "GLUE": separates the glue draws from the integrator's, which use the bare seed

// Philox4x32-10 (Salmon et al., SC'11)
GD_GLUE_HD void glue_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4])
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// What one pair draws at one update: counter (i, j, epoch), key from the replica's seed
struct GlueDraw {
    uint32_t release, fire;      // compared with the thresholds below
    uint64_t sel;                // the selection key when more pairs fire than fit
};
GD_GLUE_HD GlueDraw glue_draw(uint32_t i, uint32_t j, uint64_t epoch, uint64_t seed)
{
    uint32_t w[4];
    glue_philox4x32_10(i, j, (uint32_t)(epoch & 0xffffffffull), (uint32_t)(epoch >> 32), (uint32_t)(seed & 0xffffffffull),
                       (uint32_t)(seed >> 32) ^ GLUE_KEY_TAG, w);
    return GlueDraw{w[0], w[1], (uint64_t)w[2] << 32 | w[3]};
}

// a pair (i < j) as one sortable word, and back
GD_GLUE_HD uint64_t glue_pack(uint32_t i, uint32_t j) { return (uint64_t)i << 32 | j; }
GD_GLUE_HD uint32_t glue_i(uint64_t key) { return (uint32_t)(key >> 32); }
GD_GLUE_HD uint32_t glue_j(uint64_t key) { return (uint32_t)(key & 0xffffffffull); }

// An event of probability p happens when a 32-bit draw is below min(2^32, floor(p 2^32)): p = 0 never, p = 1 always
inline uint64_t glue_threshold(double p)
{
    if (!(p > 0)) return 0;
    if (p >= 1) return 1ull << 32;
    return std::min<uint64_t>(1ull << 32, (uint64_t)std::floor(p * 4294967296.0));
}
// ... of a rate over dt: p = 1 - exp(-rate dt)
inline uint64_t glue_rate_threshold(double rate, double dt) { return glue_threshold(-std::expm1(-rate * dt)); }

// NULL, or what is wrong with the parameters of gd_glue_define (every max_glues is valid: 0 holds no pair)
inline const char *glue_check_params(double reach, double binding_rate, double unbinding_rate)
{
    if (!(reach > 0) || !std::isfinite(reach)) return "reach must be positive and finite";
    if (!std::isfinite(binding_rate) || binding_rate < 0) return "binding_rate must be finite and not negative";
    if (!std::isfinite(unbinding_rate) || unbinding_rate < 0) return "unbinding_rate must be finite and not negative";
    return nullptr;
}

// A caller's list (n pairs, flat) as a sorted key set: NULL and `keys` filled, or what is wrong (keys untouched)
inline const char *glue_normalise(const uint32_t *pairs, uint32_t n, uint32_t n_beads, uint32_t max_glues, std::vector<uint64_t> &keys)
{
    if (n > max_glues) return "more pairs than max_glues";
    std::vector<uint64_t> k(n);
    for (uint32_t q = 0; q < n; q++) {
        const uint32_t a = pairs[2 * q], b = pairs[2 * q + 1];
        if (a >= n_beads || b >= n_beads) return "bead id out of range";
        if (a == b) return "a pair of a bead with itself";
        k[q] = glue_pack(std::min(a, b), std::max(a, b));
    }
    std::sort(k.begin(), k.end());
    if (std::adjacent_find(k.begin(), k.end()) != k.end()) return "a pair is listed twice";
    keys.swap(k);
    return nullptr;
}

}      // namespace gd

#endif
