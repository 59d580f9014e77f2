// gdyn_frames.hpp -- the arithmetic that the history analyses share and that needs no device: which frames of a history a call
// selects (gd_dcorr, gd_cluster, gd_dcov, gd_gyr), which tiles of a symmetric map a rectangle of it touches (gd_dmap, gd_dcov), the
// windows of the lag walk (gdyn_lagwalk.hpp) that an LDS budget holds and the order of a call's lags (gd_msd, gd_vanhove).
// Plain C++ in the manner of gdyn_policy.hpp: no HIP call, no handle, no error reporting; tests/native/test_frames.cpp drives it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
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

struct LagWindows {
    unsigned W, windows;      // items of a window; 1: the longest sequence fits in one window and partners lie in it, else 2
};

// The windows of the lag walk in `budget` bytes of LDS of which `fixed` lie in front of them: `row` bytes an item, sequences of at most
// `longest` items, W at most `knob` (0: no bound).  Where fewer than two rows fit, W = 1 with two windows.
inline LagWindows lag_windows(size_t budget, size_t fixed, size_t row, unsigned longest, unsigned knob)
{
    unsigned const fit = (unsigned)std::min<size_t>((budget > fixed ? budget - fixed : 0) / row, 1u << 28);
    unsigned const want = knob ? std::min(knob, longest) : longest;
    if (want > fit) return {std::max(fit / 2, 1u), 2};
    unsigned const W = std::max(want, 1u);
    if (W >= longest) return {W, 1};
    return {2 * (size_t)W > fit ? std::max(fit / 2, 1u) : W, 2};
}

struct LagOrder {      // the indices of a call's lags by ascending lag, the least lag (none: 2^32 - 1) and, if one is listed twice, the least such
    std::vector<uint32_t> order;
    uint32_t least = 0xffffffffu, repeated = 0;
    bool twice = false;
};

inline LagOrder sort_lags(const uint32_t *lags, uint32_t n)
{
    LagOrder r;
    r.order.resize(n);
    std::iota(r.order.begin(), r.order.end(), 0u);
    std::sort(r.order.begin(), r.order.end(), [&](uint32_t a, uint32_t b) { return lags[a] < lags[b]; });
    if (n) r.least = lags[r.order[0]];
    for (uint32_t k = 1; k < n && !r.twice; k++)
        if (lags[r.order[k]] == lags[r.order[k - 1]]) {
            r.twice = true;
            r.repeated = lags[r.order[k]];
        }
    return r;
}

}  // namespace gd
