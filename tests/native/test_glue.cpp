// The pure logic of the device glue kinetics (csrc/gdyn_glue.hpp) alone: Philox4x32-10 against the Random123 vectors, the integer
// thresholds at p = 0, 1 and a tiny p, the pair packing, a draw's counter and key, the argument checks and the normalisation of a
// caller's list.  Driven by tests/test_glue_host.py (plain, and under AddressSanitizer + UBSan).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "gdyn_glue.hpp"

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static void test_philox()
{
    struct Vec { uint32_t c[4], k[2], o[4]; };
    const Vec vecs[] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    for (const Vec &v : vecs) {
        uint32_t w[4];
        gd::glue_philox4x32_10(v.c[0], v.c[1], v.c[2], v.c[3], v.k[0], v.k[1], w);
        CHECK(w[0] == v.o[0] && w[1] == v.o[1] && w[2] == v.o[2] && w[3] == v.o[3]);
    }
    // a draw: counter (i, j, epoch lo, epoch hi), key (seed lo, seed hi ^ tag); sel = w[2] << 32 | w[3]
    const uint64_t epoch = 0x13198a2e03707344ull ^ 0x1000000000ull, seed = 0x299f31d0a4093822ull;
    uint32_t w[4];
    gd::glue_philox4x32_10(7, 9, (uint32_t)epoch, (uint32_t)(epoch >> 32), 0xa4093822u, 0x299f31d0u ^ 0x474C5545u, w);
    const gd::GlueDraw d = gd::glue_draw(7, 9, epoch, seed);
    CHECK(d.release == w[0] && d.fire == w[1] && d.sel == ((uint64_t)w[2] << 32 | w[3]));
    // with the third vector's counter and a seed whose high word undoes the tag: the vector's own output
    const gd::GlueDraw e = gd::glue_draw(0x243f6a88u, 0x85a308d3u, 0x0370734413198a2eull, (uint64_t)(0x299f31d0u ^ gd::GLUE_KEY_TAG) << 32 | 0xa4093822u);
    CHECK(e.release == 0xd16cfe09u && e.fire == 0x94fdccebu && e.sel == 0x5001e42024126ea1ull);
    CHECK(gd::glue_draw(7, 9, epoch, seed).sel != gd::glue_draw(7, 9, epoch + 1, seed).sel);
    CHECK(gd::glue_draw(7, 9, epoch, seed).sel != gd::glue_draw(9, 7, epoch, seed).sel);
}

static void test_thresholds()
{
    const uint64_t one = 1ull << 32;
    CHECK(gd::glue_threshold(0.0) == 0);                     // never: no 32-bit word is below 0
    CHECK(gd::glue_threshold(1.0) == one);                   // always: every 32-bit word is below 2^32
    CHECK(gd::glue_threshold(0.5) == one / 2);
    CHECK(gd::glue_threshold(1e-12) == 0);                   // floor(4.3e-3)
    CHECK(gd::glue_threshold(1.0 / 4294967296.0) == 1);
    CHECK(gd::glue_threshold(std::nextafter(1.0, 0.0)) == one - 1);
    CHECK(gd::glue_threshold(-0.0) == 0);
    CHECK(gd::glue_rate_threshold(0.0, 1.0) == 0);
    CHECK(gd::glue_rate_threshold(1e3, 1.0) == one);         // exp(-1000) = 0: p = 1
    CHECK(gd::glue_rate_threshold(1e-15, 1.0) == 0);         // tiny: p = 1e-15 through expm1, no cancellation
    CHECK(gd::glue_rate_threshold(std::log(2.0), 1.0) == (uint64_t)std::floor(-std::expm1(-std::log(2.0)) * 4294967296.0));
    CHECK(gd::glue_rate_threshold(0.3, 2.0) == gd::glue_rate_threshold(0.6, 1.0));
}

static void test_packing()
{
    CHECK(gd::glue_pack(0, 1) == 1ull);
    CHECK(gd::glue_pack(3, 0xffffffffu) == 0x3ffffffffull);
    CHECK(gd::glue_pack(1, 0) > gd::glue_pack(0, 0xffffffffu));      // ascending words = ascending (i, j)
    const uint64_t k = gd::glue_pack(0xfffffffeu, 0xffffffffu);
    CHECK(gd::glue_i(k) == 0xfffffffeu && gd::glue_j(k) == 0xffffffffu);
}

static void test_checks()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(gd::glue_check_params(1.5, 0.0, 0.0) == nullptr);
    CHECK(gd::glue_check_params(1.5, 2.0, 3.0) == nullptr);
    for (double reach : {0.0, -1.0, inf, nan}) CHECK(gd::glue_check_params(reach, 1.0, 1.0) != nullptr);
    for (double rate : {-1e-9, inf, nan}) {
        CHECK(gd::glue_check_params(1.5, rate, 1.0) != nullptr);
        CHECK(gd::glue_check_params(1.5, 1.0, rate) != nullptr);
    }
    // normalisation: orientation and order fixed; a bad list leaves the previous keys
    std::vector<uint64_t> keys{42};
    const uint32_t ok[] = {5, 2, 0, 9, 2, 3};
    CHECK(gd::glue_normalise(ok, 3, 10, 3, keys) == nullptr);
    CHECK((keys == std::vector<uint64_t>{gd::glue_pack(0, 9), gd::glue_pack(2, 3), gd::glue_pack(2, 5)}));
    const std::vector<uint64_t> before = keys;
    const uint32_t twice[] = {5, 2, 2, 5}, self[] = {4, 4}, range[] = {1, 10};
    CHECK(gd::glue_normalise(twice, 2, 10, 3, keys) != nullptr && keys == before);
    CHECK(gd::glue_normalise(self, 1, 10, 3, keys) != nullptr && keys == before);
    CHECK(gd::glue_normalise(range, 1, 10, 3, keys) != nullptr && keys == before);
    CHECK(gd::glue_normalise(ok, 3, 10, 2, keys) != nullptr && keys == before);      // more than max_glues
    CHECK(gd::glue_normalise(nullptr, 0, 10, 0, keys) == nullptr && keys.empty());
}

int main()
{
    test_philox();
    test_thresholds();
    test_packing();
    test_checks();
    if (failures) { std::printf("glue: %d failure(s)\n", failures); return 1; }
    std::printf("glue: ok\n");
    return 0;
}
