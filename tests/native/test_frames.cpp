// test_frames.cpp -- csrc/gdyn_frames.hpp on the CPU against brute-force loops: how many frames of a history a selection holds and
// serves, and which tiles of a symmetric map a rectangle touches.  Prints "frames: ok" and returns 0 when every check holds.
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

}  // namespace

int main()
{
    test_frame_counts();
    test_tile_cover();
    if (failures) {
        std::printf("frames: %d checks failed\n", failures);
        return 1;
    }
    std::printf("frames: ok\n");
    return 0;
}
