// The host logic of the per-replica A/B tables (csrc/gdyn_ensemble.hpp) alone: the tables a replica carries, the partition into
// classes, the fp16 test over all replicas and the homogeneous / heterogeneous decision.  Driven by tests/test_ensemble_ab.py (plain,
// and under AddressSanitizer + UBSan).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "gdyn_ensemble.hpp"

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using Col = std::vector<double>;

static std::vector<uint32_t> classes_of(const gd::EnsembleAB &e, uint32_t *n = nullptr)
{
    std::vector<uint32_t> c(e.replicas(), 99u);
    const uint32_t k = e.classes(c.data());
    if (n) *n = k;
    return c;
}

static bool holds(const gd::EnsembleAB &e, uint32_t r, const Col &a, const Col &b)
{
    Col ga(e.beads(), -1.0), gb(e.beads(), -1.0);
    e.get(r, ga.data(), gb.data());
    return ga == a && gb == b;
}

static void test_fp16()
{
    for (double v : {0.0, -0.0, 0.5, 1.0, 5.0, -2.0, 0.25, 1024.0, 2047.0, 2048.0, 65504.0, 6.103515625e-05 /* 2^-14 */,
                     5.9604644775390625e-08 /* 2^-24 */, 1.0 + 1.0 / 1024})
        CHECK(gd::exact_in_fp16(v));
    for (double v : {0.3, 0.1, 2049.0, 65520.0, 65536.0, 1.0 + 1.0 / 2048, 2.98023223876953125e-08 /* 2^-25 */, 1e-30,
                     6.103515625e-05 + 2.98023223876953125e-08, std::numeric_limits<double>::quiet_NaN()})
        CHECK(!gd::exact_in_fp16(v));
    CHECK(gd::exact_in_fp16(std::numeric_limits<double>::infinity()));      // (binary16 has both infinities)
}

static void test_single_replica()
{
    gd::EnsembleAB e;
    e.reset(4, 1);
    uint32_t n = 0;
    CHECK(classes_of(e, &n) == std::vector<uint32_t>{0} && n == 1);
    CHECK(e.homogeneous() && e.fp16_exact());
    const Col a = {1, 0, 0.5, 1}, b = {0, 1, 0.5, 0};
    CHECK(e.set(0, a.data(), b.data()) == 0);
    CHECK(classes_of(e, &n) == std::vector<uint32_t>{0} && n == 1 && e.homogeneous());      // one replica: one table, whatever it holds
    CHECK(holds(e, 0, a, b));
}

static void test_classes()
{
    const uint32_t N = 5, R = 6;
    const Col a0 = {1, 1, 0, 0, 0.5}, b0 = {0, 0, 1, 1, 0.5};
    const Col a1 = {0, 1, 1, 0, 0.5}, b1 = {1, 0, 0, 1, 0.5};
    const Col a2 = {1, 0, 1, 0, 1}, b2 = {0, 1, 0, 1, 0};
    gd::EnsembleAB e;
    e.reset(N, R);
    e.set_shared(a0.data(), b0.data());
    uint32_t n = 0;
    CHECK((classes_of(e, &n) == std::vector<uint32_t>{0, 0, 0, 0, 0, 0}) && n == 1 && e.homogeneous());
    for (uint32_t r = 0; r < R; r++) CHECK(holds(e, r, a0, b0));
    // equal tables set in another order of calls, and column by column: T0 T1 T2 T1 T0 T2
    CHECK(e.set(5, a2.data(), b2.data()) == 0);
    CHECK(e.set(3, a1.data(), nullptr) == 0);
    CHECK(e.set(1, a1.data(), b1.data()) == 0);
    CHECK(e.set(2, nullptr, b2.data()) == 0);
    CHECK(e.set(3, nullptr, b1.data()) == 0);
    CHECK(e.set(2, a2.data(), nullptr) == 0);
    CHECK((classes_of(e, &n) == std::vector<uint32_t>{0, 1, 2, 1, 0, 2}) && n == 3 && !e.homogeneous());
    CHECK(holds(e, 1, a1, b1) && holds(e, 2, a2, b2) && holds(e, 3, a1, b1) && holds(e, 4, a0, b0) && holds(e, 5, a2, b2));
    CHECK(e.a(3, 1) == 1 && e.b(3, 0) == 1 && e.a(0, 0) == 1);
    // numbered by first appearance: replica 0 changes, the rest move up
    CHECK(e.set(0, a2.data(), b2.data()) == 0);
    CHECK((classes_of(e, &n) == std::vector<uint32_t>{0, 1, 0, 1, 2, 0}) && n == 3);
    // all different
    gd::EnsembleAB d;
    d.reset(N, 3);
    d.set_shared(a0.data(), b0.data());
    CHECK(d.set(1, a1.data(), b1.data()) == 0 && d.set(2, a2.data(), b2.data()) == 0);
    CHECK((classes_of(d, &n) == std::vector<uint32_t>{0, 1, 2}) && n == 3 && !d.homogeneous());
    // a column left out is kept: a of T1 with b of T0 is a table of its own
    gd::EnsembleAB k;
    k.reset(N, 2);
    k.set_shared(a0.data(), b0.data());
    CHECK(k.set(1, a1.data(), nullptr) == 0);
    CHECK(holds(k, 1, a1, b0) && !k.homogeneous());
    CHECK(k.set(1, nullptr, b1.data()) == 0);
    CHECK(holds(k, 1, a1, b1));
}

static void test_homogeneous_again()
{
    const uint32_t N = 3, R = 3;
    const Col a0 = {1, 0, 0.5}, b0 = {0, 1, 0.5}, a1 = {0, 1, 0.5}, b1 = {1, 0, 0.5};
    gd::EnsembleAB e;
    e.reset(N, R);
    e.set_shared(a0.data(), b0.data());
    CHECK(e.set(1, a1.data(), b1.data()) == 0 && !e.homogeneous());
    CHECK(e.set(1, a0.data(), b0.data()) == 0);      // back to the shared table
    uint32_t n = 0;
    CHECK(e.homogeneous() && (classes_of(e, &n) == std::vector<uint32_t>{0, 0, 0}) && n == 1);
    // every replica set to one table that is NOT the shared one: homogeneous as well, and replica 0 holds the handle's table
    for (uint32_t r = 0; r < R; r++) CHECK(e.set(r, a1.data(), b1.data()) == 0);
    CHECK(e.homogeneous() && holds(e, 0, a1, b1) && e.a(0, 1) == 1);
    // gd_set_bead_params: the column replaces that column of every replica
    CHECK(e.set(2, a0.data(), nullptr) == 0 && !e.homogeneous());
    e.set_shared(a0.data(), nullptr);
    CHECK(e.homogeneous());
    for (uint32_t r = 0; r < R; r++) CHECK(holds(e, r, a0, b1));      // (b: what the replicas had, all b1)
    e.set_shared(nullptr, b0.data());
    for (uint32_t r = 0; r < R; r++) CHECK(holds(e, r, a0, b0));
    // -0.0 and 0.0 are one value
    const Col am = {1, -0.0, 0.5};
    CHECK(e.set(1, am.data(), nullptr) == 0 && e.homogeneous());
}

static void test_refused_set()
{
    const uint32_t N = 3;
    const Col a0 = {1, 0, 0.5}, b0 = {0, 1, 0.5}, a1 = {0, 1, 0.5};
    gd::EnsembleAB e;
    e.reset(N, 2);
    e.set_shared(a0.data(), b0.data());
    CHECK(e.set(1, a1.data(), nullptr) == 0);
    Col bad = {0, 1, std::numeric_limits<double>::quiet_NaN()};
    CHECK(e.set(1, a0.data(), bad.data()) == 3);      // (1 + the index; a is not taken either)
    CHECK(holds(e, 1, a1, b0));
    bad = {std::numeric_limits<double>::infinity(), 0, 0};
    CHECK(e.set(0, bad.data(), nullptr) == 1);
    CHECK(holds(e, 0, a0, b0));
}

static void test_fp16_over_replicas()
{
    const uint32_t N = 4, R = 3;
    const Col a0 = {1, 0, 0.5, 5}, b0 = {0, 1, 0.5, 0};
    gd::EnsembleAB e;
    e.reset(N, R);
    e.set_shared(a0.data(), b0.data());
    CHECK(e.fp16_exact());
    Col b2 = b0;
    b2[3] = 0.3;      // one value of one replica
    CHECK(e.set(2, nullptr, b2.data()) == 0);
    CHECK(!e.fp16_exact());
    CHECK(e.set(2, nullptr, b0.data()) == 0);
    CHECK(e.fp16_exact());
    // a shared column that no replica refers to does not count
    Col as = a0;
    as[0] = 0.3;
    e.set_shared(as.data(), nullptr);
    CHECK(!e.fp16_exact());
    for (uint32_t r = 0; r < R; r++) CHECK(e.set(r, a0.data(), nullptr) == 0);
    CHECK(e.fp16_exact() && e.homogeneous());
}

static void test_one_bead()
{
    gd::EnsembleAB e;
    e.reset(1, 3);
    const double one = 1.0, zero = 0.0, third = 1.0 / 3;
    e.set_shared(&one, &zero);
    CHECK(e.set(1, &zero, &one) == 0);
    uint32_t n = 0;
    CHECK((classes_of(e, &n) == std::vector<uint32_t>{0, 1, 0}) && n == 2 && !e.homogeneous() && e.fp16_exact());
    CHECK(e.set(2, &third, nullptr) == 0);
    CHECK((classes_of(e, &n) == std::vector<uint32_t>{0, 1, 2}) && n == 3 && !e.fp16_exact());
    CHECK(e.a(2, 0) == third && e.b(2, 0) == 0.0);
}

int main()
{
    test_fp16();
    test_single_replica();
    test_classes();
    test_homogeneous_again();
    test_refused_set();
    test_fp16_over_replicas();
    test_one_bead();
    if (failures) { std::printf("ensemble ab: %d failure(s)\n", failures); return 1; }
    std::printf("ensemble ab: ok\n");
    return 0;
}
