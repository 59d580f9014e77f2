// test_frames.cpp -- csrc/gdyn_frames.hpp on the CPU against brute-force loops: how many frames of a history a selection holds and
// serves, which tiles of a symmetric map a rectangle touches, the windows of the lag walk that an LDS budget holds, and the order
// of a call's lags.  Prints "frames: ok" and returns 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "gdyn_frames.hpp"

namespace {

int failures = 0;

#define CHECK(cond, ...)                             \
    do {                                             \
        if (!(cond)) {                               \
            failures++;                              \
            std::printf("FAILED %s: ", #cond);       \
            std::printf(__VA_ARGS__);                \
            std::printf("\n");                       \
        }                                            \
    } while (0)

constexpr uint32_t kMax = 0xffffffffu;

// the frames f = first + k * stride, k = 0, 1, ..., with f + lag < F, counted one by one in 64 bits (F is small here)
uint64_t brute_fit(uint32_t F, uint32_t first, uint32_t stride, uint32_t lag)
{
    if (!stride) return 0;
    uint64_t n = 0;
    for (uint64_t f = first; f + lag < F; f += stride) n++;
    return n;
}

void check_fit(uint32_t F, uint32_t first, uint32_t stride, uint32_t lag)
{
    uint64_t const got = gd::frames_fit(F, first, stride, lag), want = brute_fit(F, first, stride, lag);
    CHECK(got == want, "F %u first %u stride %u lag %u: %llu, brute force %llu", F, first, stride, lag, (unsigned long long)got, (unsigned long long)want);
    if (lag == 0) CHECK(gd::frames_fit(F, first, stride) == want, "F %u first %u stride %u: the default lag is 0", F, first, stride);
}

void test_frame_counts()
{
    // every small case, which holds F = 1, first >= F, lag >= F, first + lag = F - 1 (exactly one fits) and stride > F
    for (uint32_t F = 0; F <= 9; F++)
        for (uint32_t first = 0; first <= 11; first++)
            for (uint32_t stride = 0; stride <= 11; stride++)
                for (uint32_t lag = 0; lag <= 11; lag++) check_fit(F, first, stride, lag);
    // the edges by name
    CHECK(gd::frames_fit(1, 0, 1, 0) == 1, "one frame holds itself");
    CHECK(gd::frames_fit(1, 0, 1, 1) == 0, "one frame has no partner");
    CHECK(gd::frames_fit(7, 7, 1, 0) == 0 && gd::frames_fit(7, 0, 1, 7) == 0, "first >= F and lag >= F hold nothing");
    CHECK(gd::frames_fit(7, 4, 1, 2) == 1 && gd::frames_fit(7, 4, 1, 3) == 0, "first + lag = F - 1 holds exactly one");
    CHECK(gd::frames_fit(7, 2, 8, 0) == 1, "stride > F holds the first frame alone");
    CHECK(gd::frames_fit(7, 0, 0, 0) == 0, "stride 0 holds nothing");
    // first, stride and lag at 2^32 - 1: sums are taken in 64 bits and do not wrap round
    for (uint32_t F : {1u, 2u, 1000u, kMax - 1, kMax}) {
        CHECK(gd::frames_fit(F, kMax, 1, 0) == 0, "F %u: first 2^32 - 1 lies beyond every history", F);
        CHECK(gd::frames_fit(F, 0, 1, kMax) == 0, "F %u: lag 2^32 - 1 has no partner", F);
        CHECK(gd::frames_fit(F, 1, 1, kMax) == 0 && gd::frames_fit(F, kMax, 1, 1) == 0 && gd::frames_fit(F, kMax, kMax, kMax) == 0,
              "F %u: first + lag past 2^32 does not wrap round", F);
        CHECK(gd::frames_fit(F, 0, kMax, 0) == 1, "F %u: stride 2^32 - 1 holds the first frame alone", F);
    }
    CHECK(gd::frames_fit(kMax, 0, 1, 0) == kMax, "the longest history, every frame");
    CHECK(gd::frames_fit(kMax, kMax - 1, 1, 0) == 1 && gd::frames_fit(kMax, 0, 1, kMax - 1) == 1, "the longest history, exactly one");
    CHECK(gd::frames_fit(kMax, 0, kMax - 1, 0) == 2, "the longest history, its first and last frame");
    // what a call serves: the count asked for, whatever fits (the caller refuses count > fit), or all that fit
    for (uint64_t fit : {0ull, 1ull, 5ull, (unsigned long long)kMax}) {
        CHECK(gd::frames_served(fit, 0) == fit, "count 0 serves all %llu", (unsigned long long)fit);
        if (fit && fit <= kMax) CHECK(gd::frames_served(fit, (uint32_t)fit) == fit, "count = fit");
        if (fit < kMax) CHECK(gd::frames_served(fit, (uint32_t)fit + 1) == fit + 1, "count = fit + 1 is the caller's to refuse");
    }
}

typedef std::pair<uint32_t, uint32_t> Tile;

// cell by cell: the tile of every cell of the rectangle, of every diagonal cell of its rows and of its columns
std::set<Tile> brute_cover(uint32_t tile, uint32_t r0, uint32_t nr, uint32_t c0, uint32_t nc, bool rect, bool diag_rows, bool diag_cols)
{
    std::set<Tile> out;
    for (uint32_t r = r0; r < r0 + nr; r++) {
        if (diag_rows) out.insert({r / tile, r / tile});
        for (uint32_t c = c0; rect && c < c0 + nc; c++) out.insert({std::min(r / tile, c / tile), std::max(r / tile, c / tile)});
    }
    for (uint32_t c = c0; diag_cols && c < c0 + nc; c++) out.insert({c / tile, c / tile});
    return out;
}

void check_cover(uint32_t tile, uint32_t r0, uint32_t nr, uint32_t c0, uint32_t nc, bool rect, bool diag_rows, bool diag_cols)
{
    std::vector<Tile> const got = gd::tile_cover(tile, r0, nr, c0, nc, rect, diag_rows, diag_cols);
    std::set<Tile> const want = brute_cover(tile, r0, nr, c0, nc, rect, diag_rows, diag_cols);
    bool good = got.size() == want.size() && std::vector<Tile>(want.begin(), want.end()) == got;      // a set is ascending and unique
    for (Tile const &t : got) good = good && t.first <= t.second;
    CHECK(good, "tile %u rows %u+%u cols %u+%u rect %d diag %d %d: %zu tiles, brute force %zu", tile, r0, nr, c0, nc, rect, diag_rows, diag_cols, got.size(),
          want.size());
}

void test_tile_cover()
{
    // B = 50 cells in tiles of 16: three full tiles and a last partial one of 2 cells
    uint32_t const B = 50;
    for (uint32_t tile : {16u, 7u})
        for (int flags = 1; flags < 8; flags++)
            for (uint32_t r0 = 0; r0 < B; r0 += 5)
                for (uint32_t nr : {1u, 3u, 16u, 17u, 50u})
                    for (uint32_t c0 = 0; c0 < B; c0 += 7)
                        for (uint32_t nc : {1u, 2u, 15u, 33u, 50u})
                            if (r0 + nr <= B && c0 + nc <= B) check_cover(tile, r0, nr, c0, nc, flags & 1, flags & 2, flags & 4);
    // the edges by name, tiles of 16
    CHECK(gd::tile_cover(16, 17, 3, 20, 5) == std::vector<Tile>({{1, 1}}), "a rectangle inside one tile");
    CHECK(gd::tile_cover(16, 14, 4, 1, 2) == std::vector<Tile>({{0, 0}, {0, 1}}), "a rectangle across a tile boundary");
    // a row range wholly above the column range: the keys are those of the mirror image, canonical and each once
    CHECK(gd::tile_cover(16, 32, 18, 0, 20) == std::vector<Tile>({{0, 2}, {0, 3}, {1, 2}, {1, 3}}), "rows above the columns");
    CHECK(gd::tile_cover(16, 32, 18, 0, 20) == gd::tile_cover(16, 0, 20, 32, 18), "a rectangle and its mirror image");
    CHECK(gd::tile_cover(16, 0, 50, 0, 50).size() == 10, "the whole map: the upper triangle of 4 x 4 tiles");
    CHECK(gd::tile_cover(16, 32, 18, 0, 20, true, true, true) == std::vector<Tile>({{0, 0}, {0, 2}, {0, 3}, {1, 1}, {1, 2}, {1, 3}, {2, 2}, {3, 3}}),
          "with the diagonal tiles of rows and columns");
    CHECK(gd::tile_cover(16, 32, 18, 0, 20, false, true, false) == std::vector<Tile>({{2, 2}, {3, 3}}), "the diagonal tiles of the rows alone");
    CHECK(gd::tile_cover(16, 0, 4, 0, 4, false, false, false).empty(), "nothing asked for");
    CHECK(gd::tile_cover(16, 48, 2, 48, 2) == std::vector<Tile>({{3, 3}}), "the last partial tile");
    CHECK(gd::tile_cover(16, 49, 1, 0, 1, true, false, true) == std::vector<Tile>({{0, 0}, {0, 3}}), "the last cell against the first");
}

// the windows by search: the largest W <= the knob and the longest sequence whose one window (W >= longest) or two fit the rows that
// the budget holds after `fixed`; (1, 2) where nothing fits
gd::LagWindows brute_windows(size_t budget, size_t fixed, size_t row, unsigned longest, unsigned knob)
{
    size_t const fit = budget > fixed ? (budget - fixed) / row : 0;
    for (unsigned W = knob ? std::min(knob, longest) : longest; W >= 1; W--) {
        unsigned const windows = W >= longest ? 1 : 2;
        if ((size_t)windows * W <= fit) return {W, windows};
    }
    return {1, 2};
}

void check_windows(size_t budget, size_t fixed, size_t row, unsigned longest)
{
    size_t const fit = budget > fixed ? (budget - fixed) / row : 0;
    gd::LagWindows const free = gd::lag_windows(budget, fixed, row, longest, 0);
    for (unsigned knob : {0u, 1u, 2u, 3u, 8u, 36u, 37u, 416u, 417u, 418u, 834u, 835u, 836u, 5000u}) {
        gd::LagWindows const got = gd::lag_windows(budget, fixed, row, longest, knob), want = brute_windows(budget, fixed, row, longest, knob);
        CHECK(got.W == want.W && got.windows == want.windows, "budget %zu fixed %zu row %zu longest %u knob %u: (%u, %u), by search (%u, %u)", budget, fixed, row,
              longest, knob, got.W, got.windows, want.W, want.windows);
        CHECK(got.W >= 1 && (got.windows == 1 || got.windows == 2), "budget %zu longest %u knob %u: W %u windows %u", budget, longest, knob, got.W, got.windows);
        CHECK(got.W <= free.W, "budget %zu longest %u: knob %u raises W from %u to %u", budget, longest, knob, free.W, got.W);
        if (knob) CHECK(got.W <= knob, "budget %zu longest %u: W %u beyond the knob %u", budget, longest, got.W, knob);
        if (fit < 2 && !(fit == 1 && longest == 1)) {      // less than two rows: one item a window and two of them, whatever the budget
            CHECK(got.W == 1 && got.windows == 2, "budget %zu fixed %zu row %zu longest %u knob %u: (%u, %u) where %zu rows fit", budget, fixed, row, longest, knob,
                  got.W, got.windows, fit);
            continue;
        }
        CHECK((got.windows == 1) == (got.W >= longest), "budget %zu longest %u knob %u: W %u with %u windows", budget, longest, knob, got.W, got.windows);
        CHECK((size_t)got.windows * got.W * row + fixed <= budget, "budget %zu fixed %zu row %zu longest %u knob %u: %u windows of %u rows", budget, fixed, row, longest,
              knob, got.windows, got.W);
    }
}

void test_lag_windows()
{
    // small budgets, every one: rows of 3 and 7 bytes, with and without bytes in front, budgets below `fixed` and below one and two rows
    for (size_t row : {3u, 7u})
        for (size_t fixed : {0u, 5u})
            for (size_t budget = 0; budget <= 80; budget++)
                for (unsigned longest = 1; longest <= 30; longest++) check_windows(budget, fixed, row, longest);
    // the two real cases: 160 KiB of rows of 49 float32 or float64
    size_t const lds = 160 * 1024;
    CHECK(lds / (49 * 4) == 835 && lds / (49 * 8) == 417, "the rows of 160 KiB");
    for (size_t row : {49u * 4u, 49u * 8u})
        for (size_t fixed : {(size_t)0, (size_t)(65 * 8 + 1024 * 4)})
            for (unsigned longest : {1u, 2u, 200u, 408u, 409u, 416u, 417u, 418u, 701u, 811u, 812u, 834u, 835u, 836u, 1670u, 8199u, 100000u})
                check_windows(lds, fixed, row, longest);
    gd::LagWindows w = gd::lag_windows(lds, 0, 49 * 4, 835, 0);
    CHECK(w.W == 835 && w.windows == 1, "835 float32 items are one window");
    w = gd::lag_windows(lds, 0, 49 * 4, 836, 0);
    CHECK(w.W == 417 && w.windows == 2, "836 float32 items are walked in windows of 417");
    w = gd::lag_windows(lds, 0, 49 * 8, 417, 0);
    CHECK(w.W == 417 && w.windows == 1, "417 float64 items are one window");
    w = gd::lag_windows(lds, 0, 49 * 8, 8199, 0);
    CHECK(w.W == 208 && w.windows == 2, "a long float64 history is walked in windows of 208");
    w = gd::lag_windows(lds, 0, 49 * 8, 8199, 37);
    CHECK(w.W == 37 && w.windows == 2, "the knob bounds the window");
    // fewer than two rows
    w = gd::lag_windows(49 * 8 + 100, 0, 49 * 8, 701, 0);
    CHECK(w.W == 1 && w.windows == 2, "one row fits: (%u, %u)", w.W, w.windows);
    w = gd::lag_windows(100, 0, 49 * 8, 701, 0);
    CHECK(w.W == 1 && w.windows == 2, "no row fits: (%u, %u)", w.W, w.windows);
    w = gd::lag_windows(100, 200, 49 * 8, 701, 5);
    CHECK(w.W == 1 && w.windows == 2, "the fixed bytes alone exceed the budget: (%u, %u)", w.W, w.windows);
}

void test_sort_lags()
{
    uint32_t const lags[] = {7, 1, 4096, 3, 2};
    gd::LagOrder lo = gd::sort_lags(lags, 5);
    CHECK(lo.order == std::vector<uint32_t>({1, 4, 3, 0, 2}) && lo.least == 1 && !lo.twice, "five distinct lags in ascending order");
    uint32_t const twice[] = {9, 0, 5, 9, 5};
    lo = gd::sort_lags(twice, 5);
    CHECK(lo.least == 0 && lo.twice && lo.repeated == 5, "the least lag and the least repeated one: %u, %u", lo.least, lo.repeated);
    lo = gd::sort_lags(nullptr, 0);
    CHECK(lo.order.empty() && lo.least == kMax && !lo.twice, "no lags");
}

}  // namespace

int main()
{
    test_frame_counts();
    test_tile_cover();
    test_lag_windows();
    test_sort_lags();
    if (failures) {
        std::printf("frames: %d checks failed\n", failures);
        return 1;
    }
    std::printf("frames: ok\n");
    return 0;
}
