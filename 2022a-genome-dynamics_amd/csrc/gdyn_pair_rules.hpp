// gdyn_pair_rules.hpp -- the pair rules of the cell-based analyses, once: the wrapped position, the cell of a
// coordinate and the minimum image.  gdyn_rdf.hip includes this alone, gdyn_dcorr.hip and gdyn_cluster.hip through gdyn_cells.hpp.
// Defined in an anonymous namespace: each translation unit keeps its own object code under its own flags, so min_image carries the
// contraction pragma that a file built without -ffp-contract=off needs.
#pragma once
#include <hip/hip_runtime.h>

namespace gd {
namespace {

// position in [0, L]: fmod is exact, so the error is at most half an ulp of L whatever the magnitude of x (unwrapped input)
__device__ inline double wrap(double x, double L)
{
    double const w = fmod(x, L);
    return w < 0.0 ? w + L : w;
}

__device__ inline int cell_of(double w, double inv_side, int n) { return (int)fmin(fmax(floor(w * inv_side), 0.0), (double)(n - 1)); }      // (NaN -> 0)

__device__ inline double min_image(double d, double L)     // DESIGN.md 7b; |d| <= L/2 already gives nearbyint(d/L) = 0
{
#pragma clang fp contract(off)
    return fabs(d) > 0.5 * L ? d - L * nearbyint(d / L) : d;
}

}  // namespace
}  // namespace gd
