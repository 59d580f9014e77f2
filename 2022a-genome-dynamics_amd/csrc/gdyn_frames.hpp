// gdyn_frames.hpp -- the arithmetic that the history analyses share and that needs no device: which frames of a history a call
// selects (gd_dcorr, gd_cluster, gd_dcov, gd_gyr) and which tiles of a symmetric map a rectangle of it touches (gd_dmap, gd_dcov).
// Plain C++ in the manner of gdyn_policy.hpp: no HIP call, no handle, no error reporting; tests/native/test_frames.cpp drives it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace gd {

// how many of the frames first + k * stride (k = 0, 1, ...) of a history of F frames have a partner `lag` frames later (f + lag < F)
inline uint64_t frames_fit(uint32_t F, uint32_t first, uint32_t stride, uint32_t lag = 0)
{
    if (!stride || (uint64_t)first + lag >= F) return 0;
    return ((uint64_t)F - 1 - lag - first) / stride + 1;
}

// the frames a call serves: the `count` it asks for, or with count 0 all that fit
inline uint64_t frames_served(uint64_t fit, uint32_t count) { return count ? count : fit; }

// The tiles (lo, hi), lo <= hi, of `tile` x `tile` cells of a symmetric map that a call computes, ascending and each once: with `rect`
// those that the rectangle of n_rows x n_cols cells (both >= 1) from (row_first, col_first) or its mirror image touches, with
// diag_rows / diag_cols the diagonal tiles of its rows / columns.
inline std::vector<std::pair<uint32_t, uint32_t>> tile_cover(uint32_t tile, uint32_t row_first, uint32_t n_rows, uint32_t col_first, uint32_t n_cols,
                                                             bool rect = true, bool diag_rows = false, bool diag_cols = false)
{
    uint32_t const ti0 = row_first / tile, ti1 = (uint32_t)(((uint64_t)row_first + n_rows - 1) / tile);
    uint32_t const tj0 = col_first / tile, tj1 = (uint32_t)(((uint64_t)col_first + n_cols - 1) / tile);
    std::vector<std::pair<uint32_t, uint32_t>> tiles;
    if (rect) {
        tiles.reserve((size_t)(ti1 - ti0 + 1) * (tj1 - tj0 + 1));
        for (uint32_t ti = ti0; ti <= ti1; ti++)
            for (uint32_t tj = tj0; tj <= tj1; tj++) tiles.emplace_back(std::min(ti, tj), std::max(ti, tj));
    }
    if (diag_rows)
        for (uint32_t t = ti0; t <= ti1; t++) tiles.emplace_back(t, t);
    if (diag_cols)
        for (uint32_t t = tj0; t <= tj1; t++) tiles.emplace_back(t, t);
    std::sort(tiles.begin(), tiles.end());
    tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
    return tiles;
}

}  // namespace gd
