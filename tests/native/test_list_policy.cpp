// CPU unit test of the list policy of libgdyn (csrc/gdyn_policy.hpp): synthetic build reports and accepted chunks in, the decisions
// of the rules out -- tile class, dense states, row width, the row pool of tiled lists, single-class lists, memory guard, width by
// tile class, interval adaptation and the auto_skin sweep.  Built and run by tests/test_list_policy.py (plain g++, no HIP runtime).
#include <cmath>
#include <cstdio>
#include <vector>

#include "gdyn_policy.hpp"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using gd::ListPolicy;

// the list in use: cutoff 1, list radius 1 + skin (bead scale 1), tiled at capacity `cap`
static gd::ListState tiled_list(const ListPolicy &p, uint32_t cap = 3312)
{
    gd::ListState l;
    l.cut = 1.0; l.rv = (float)(1.0 + p.skin); l.tiled = true; l.tile_cap = cap; l.W = 0; l.pool_used = 1000; l.pool_kib = 2000;
    l.rows = 16.0 * 30208; l.can_tile = true;
    return l;
}
static gd::ListState generic_list(const ListPolicy &p)
{
    gd::ListState l = tiled_list(p);
    l.tiled = false; l.W = p.W;
    return l;
}
static gd::BuildReport fits(unsigned need_t, unsigned need_w = 300)
{
    gd::BuildReport r;
    r.need_t = need_t; r.need_w = need_w; r.ncell = 4096;
    return r;
}
static gd::BuildReport overflow(unsigned bits, unsigned need_w)
{
    gd::BuildReport r;
    r.bits = bits; r.over = bits != 0; r.class_over = (bits & 2u) != 0; r.need_w = need_w;
    return r;
}
static gd::BuildReport tile_overflow(unsigned need_t)
{
    gd::BuildReport r;
    r.tile_over = true; r.need_t = need_t;
    return r;
}
// an accepted chunk that holds a complete interval; on a search list unless `adapt` (no interval adaptation)
static gd::Accepted chunk(float maxd2 = 0, bool adapt = false, double ms = 1.0, int64_t steps = 100)
{
    gd::Accepted a;
    a.ms = ms; a.steps = steps; a.maxd2 = maxd2; a.full_interval = true; a.on_search_list = !adapt;
    return a;
}
static auto unit_scale = [](uint32_t) { return 1.0; };

static void test_summarize()
{
    std::vector<unsigned> f(3 * GD_NFLAGS, 0u);
    const float d2[3] = {0.25f, 0.5f, 0.125f};
    for (int r = 0; r < 3; r++) memcpy(&f[r * GD_NFLAGS + GD_FLAG_MAXDISP2], &d2[r], 4);
    f[0 * GD_NFLAGS + GD_FLAG_OVERFLOW] = 1; f[2 * GD_NFLAGS + GD_FLAG_OVERFLOW] = 2;
    f[1 * GD_NFLAGS + GD_FLAG_NEED_W] = 700; f[2 * GD_NFLAGS + GD_FLAG_NEED_W] = 500;
    f[0 * GD_NFLAGS + GD_FLAG_NEED_TILE] = 3000; f[2 * GD_NFLAGS + GD_FLAG_NEED_TILE] = 3100;
    f[1 * GD_NFLAGS + GD_FLAG_NCELL] = 999; f[2 * GD_NFLAGS + GD_FLAG_VIOLATION] = 1;
    gd::BuildReport r = gd::summarize(f.data(), 3);
    CHECK(r.bits == 3u && r.over && r.class_over && !r.tile_over && r.violated);
    CHECK(r.need_w == 700 && r.need_t == 3100 && r.ncell == 999 && r.maxd2 == 0.5f);
    f[1 * GD_NFLAGS + GD_FLAG_TILE_OVERFLOW] = 1;
    r = gd::summarize(f.data(), 2);      // (replicas 0, 1 only)
    CHECK(r.bits == 1u && !r.class_over && r.tile_over && !r.violated && r.need_t == 3000);
}

static void test_tile_class()
{
    ListPolicy p;
    CHECK(p.tile_cap == 3312u);
    const unsigned expect[][2] = {{3300, 4080}, {3200, 3312}, {3300, 4080}, {3000, 3312}, {4100, 5072}, {6000, 8192}, {9000, 8192}, {1000, 3312}};
    for (auto &e : expect) { CHECK(!p.on_report(tiled_list(p), fits(e[0]))); CHECK(p.tile_cap == e[1]); }      // (need + 24 picks the class)
    CHECK(p.last_need_t == 1000 && p.ncell_seen == 4096);
    // an overflow: one class up (need + need/32 + 32), held for 4 chunks before a smaller class is taken again
    CHECK(p.on_report(tiled_list(p), tile_overflow(3500)));
    CHECK(p.tile_cap == 4080u && p.tile_hold == 4u);
    for (int i = 0; i < 4; i++) { p.on_report(tiled_list(p, 4080), fits(3000)); CHECK(p.tile_cap == 4080u); }
    p.on_report(tiled_list(p, 4080), fits(3000));
    CHECK(p.tile_cap == 3312u);
    // at the wide class width the capacity does not step up into the two-block class (class_skin narrows the list instead) ...
    p.skin = 0.9;
    p.on_report(tiled_list(p), fits(3400));
    CHECK(p.tile_cap == 3312u);
    // ... but does with the droplet term, a fixed skin, auto_skin or another width
    gd::ListState l = tiled_list(p); l.droplet = true;
    p.on_report(l, fits(3400)); CHECK(p.tile_cap == 4080u);
    p.tile_cap = 3312; p.skin_fixed = true; p.on_report(tiled_list(p), fits(3400)); CHECK(p.tile_cap == 4080u);
    p.tile_cap = 3312; p.skin_fixed = false; p.tuner.enabled = true; p.on_report(tiled_list(p), fits(3400)); CHECK(p.tile_cap == 4080u);
    p.tile_cap = 3312; p.tuner.enabled = false; p.skin = 0.8; p.on_report(tiled_list(p), fits(3400)); CHECK(p.tile_cap == 4080u);
    // generic lists leave the class alone; GDYN_TILE_CAPS replaces the list
    p.tile_cap = 3312; p.on_report(generic_list(p), fits(3400)); CHECK(p.tile_cap == 3312u);
    ListPolicy q; q.tile_caps = {2000u, 8192u};
    q.on_report(tiled_list(q), fits(1900)); CHECK(q.tile_cap == 2000u);
}

static void test_dense_tile()
{
    // free skin: the width narrows until the largest tile fits, K <= 4, the tiled path kept
    ListPolicy p;
    p.K = 20;
    gd::ListState l = tiled_list(p);
    CHECK(p.on_report(l, tile_overflow(20000)));
    const double ratio = std::min(0.97, std::max(0.5, std::sqrt(0.85 * 8192.0 / 20000.0)));
    CHECK(p.skin == std::max(0.15, l.rv * ratio / 1.0 - (l.rv / 1.0 - 0.75)));
    CHECK(p.skin == 0.15 && p.skin_dense_from == 0.75 && p.dense_by_tile && p.K == 4u && p.tile_cap == 8192u && p.tile_hold == 4u);
    CHECK(p.tiled_ok && p.a2_ema == 0 && p.skin_next == 0);
    ListPolicy m;      // a milder state: the narrowed width is the formula's, not the floor
    m.K = 3;
    l = tiled_list(m);
    m.on_report(l, tile_overflow(9000));
    const double r2 = std::min(0.97, std::max(0.5, std::sqrt(0.85 * 8192.0 / 9000.0)));
    CHECK(m.skin == std::max(0.15, l.rv * r2 - (l.rv - 0.75)) && m.skin > 0.15 && m.skin < 0.75 && m.K == 3u);

    // easing back: steps of at most x 1.35 + 0.02 while the largest tile, scaled to the next width, fits 0.85 of 8192
    p.skin_next = 0;
    p.on_report(tiled_list(p, 8192), fits(7900));      // too large to widen
    p.on_accepted(tiled_list(p, 8192), chunk(), unit_scale);
    CHECK(p.skin_next == 0);
    double skin = p.skin;
    int steps = 0;
    while (p.skin_dense_from > 0 && steps < 20) {
        p.on_report(tiled_list(p, 8192), fits(3000));
        p.on_accepted(tiled_list(p, 8192), chunk(), unit_scale);
        const double target = std::min(0.75, skin * 1.35 + 0.02);
        CHECK(p.skin_next == target);
        p.take_pending_skin(1.0);
        CHECK(p.skin == target && p.skin_next == 0);
        skin = p.skin; steps++;
    }
    CHECK(steps == 5 && p.skin == 0.75 && !p.dense_by_tile);      // (0.15, 0.2225, 0.320, 0.453, 0.631, 0.75)

    // fixed skin: off the tiled path, retried after 8, 16, ... 1024 accepted chunks at the largest class
    ListPolicy f;
    f.skin_fixed = true;
    for (unsigned expect : {8u, 16u, 32u, 64u, 128u, 256u, 512u, 1024u, 1024u}) {
        CHECK(f.on_report(tiled_list(f), tile_overflow(20000)));
        CHECK(!f.tiled_ok && f.tiled_off == 1 && !f.want_tiled(true) && f.skin == 0.75);
        unsigned n = 0;
        while (!f.tiled_ok && n < 5000) { f.on_accepted(generic_list(f), chunk(), unit_scale); n++; }
        CHECK(n == expect && f.tile_cap == 8192u && f.want_tiled(true) && !f.want_tiled(false));
    }
    f.on_accepted(tiled_list(f), chunk(), unit_scale);      // a tiled chunk resets the back-off
    CHECK(f.tiled_backoff == 8u);
}

static void test_generic_rows()
{
    ListPolicy p;
    p.W = 96;
    CHECK(p.on_report(generic_list(p), overflow(1, 300)));
    CHECK(p.W == 300u + 300u / 16 + 8);
    p.on_report(generic_list(p), overflow(1, 300));
    CHECK(p.W == 326u + 8);      // at least 8 more
    // given back when twice the new width is at most W
    p.W = 1000;
    CHECK(!p.on_report(generic_list(p), fits(0, 100)));
    CHECK(p.W == ((100u + 25 + 16 + 7) & ~7u));
    p.W = 200;
    p.on_report(generic_list(p), fits(0, 100));
    CHECK(p.W == 200u);
    // single-class lists: on at a far class beyond the record, off once the longest list fits its field
    p.on_report(tiled_list(p), overflow(2, 600));
    CHECK(p.all_near && p.W == 200u);
    p.on_report(tiled_list(p), fits(3000, 505)); CHECK(p.all_near);
    p.on_report(tiled_list(p), fits(3000, GD_TILED_MAX_FAR)); CHECK(!p.all_near);
    // a near class beyond the record: rows too wide for tiled lists
    p.on_report(tiled_list(p), overflow(2, GD_TILED_MAX_NEAR + 8));
    CHECK(!p.all_near && p.W == GD_TILED_MAX_W + 8u && !p.want_tiled(true));
    // ... generic lists then: they give the width back once the near class has passed (to what the longest list needs, as any width)
    p.on_report(generic_list(p), fits(0, 2000));
    CHECK(p.W == ListPolicy::want_width(2000) && p.W == 2520u && p.want_tiled(true));
    // the repair queue: pool bit with room in the pool -> 16 chunks of a repair block per wave
    gd::ListState l = tiled_list(p);
    p.on_report(l, overflow(4, 300));
    CHECK(p.repair_wide == 16u);
    p.on_accepted(l, chunk(), unit_scale);
    CHECK(p.repair_wide == 15u);
    ListPolicy q; l.pool_used = 3000;
    q.on_report(l, overflow(4, 300));
    CHECK(q.repair_wide == 0u);
}

// the width of tiled lists (the guess of a build without history) follows the lists, and the row pool is sized from it
static void test_tiled_width_and_pool()
{
    const size_t waves = 128 * 30208 / 64;      // the benchmark shape: 128 replicas of 30 208 slots
    // a generic excursion grows W to 4000 (within the tiled record: the tiled path is taken again) ...
    ListPolicy p;
    p.W = 96;
    CHECK(p.on_report(generic_list(p), overflow(1, 3750)));
    CHECK(p.W == 3750u + 3750u / 16 + 8 && p.W <= GD_TILED_MAX_W && p.want_tiled(true));
    p.W = 4000;
    // ... and tiled builds that report lists of 40 entries bring it back by the rule of the generic rows
    CHECK(!p.on_report(tiled_list(p), fits(3000, 40)));
    CHECK(p.W == ListPolicy::want_width(40) && p.W == 72u);
    p.on_report(tiled_list(p), fits(3000, 40));
    CHECK(p.W == 72u);
    // a build without history then asks for what lists of 40 entries need, within the stated margins: 5 chunks (KiB) per wave,
    // want_width's quarter + 16 entries (9 chunks), the pool's eighth + 2 KiB per wave -- not for rows of 4000 entries (500 KiB per wave)
    gd::PoolPlan pl = gd::plan_pool(0, 0, waves, p.W, false);
    CHECK(pl.used == 9 * waves && pl.want == 9 * waves + 9 * waves / 8 + 2 * waves && pl.resize && pl.alloc_kib == pl.want + pl.want / 16);
    CHECK(pl.want >= 5 * waves && pl.alloc_kib <= 14 * waves && pl.alloc_kib * 1024 < ((size_t)1 << 30));
    CHECK(gd::plan_pool(0, 0, waves, 4000, false).alloc_kib * 1024 > ((size_t)32 << 30));      // (what the width left behind would have asked for)
    // a caller's list_width within the tiled record is honoured once, then replaced by the measured need
    ListPolicy c;
    CHECK(c.set_tuning(0, 0, 1, 1200, false) && c.W == 1200u && c.want_tiled(true));
    CHECK(gd::plan_pool(0, 0, waves, c.W, false).used == 150 * waves);
    c.on_report(tiled_list(c), fits(3000, 40));
    CHECK(c.W == 72u);
    // a width within twice the need stays (no flapping), the default 96 too; tiled lists do not widen W (their rows are repaired)
    ListPolicy k; k.W = 96;
    k.on_report(tiled_list(k), fits(3000, 40)); CHECK(k.W == 96u);
    k.on_report(tiled_list(k), fits(3000, 400)); CHECK(k.W == 96u);
    k.W = 1000; k.on_report(tiled_list(k), fits(3000, 400)); CHECK(k.W == 1000u);      // (want 520: more than half)
    // the pool rule: with history the use of the last build, at least a KiB per wave; an eighth + 2 KiB per wave on top;
    // kept while it is within [want, 2 want + 4 waves], reallocated with a sixteenth more otherwise
    pl = gd::plan_pool(10000, 20000, 1000, 4000, true);
    CHECK(pl.used == 10000 && pl.want == 10000 + 1250 + 2000 && !pl.resize);
    CHECK(gd::plan_pool(10000, 13249, 1000, 96, true).resize && !gd::plan_pool(10000, 13250, 1000, 96, true).resize);
    CHECK(!gd::plan_pool(10000, 2 * 13250 + 4000, 1000, 96, true).resize && gd::plan_pool(10000, 2 * 13250 + 4001, 1000, 96, true).resize);
    CHECK(gd::plan_pool(10000, 0, 1000, 96, true).alloc_kib == 13250 + 13250 / 16);
    CHECK(gd::plan_pool(10, 0, 1000, 96, true).used == 1000);          // (a KiB per wave)
    CHECK(gd::plan_pool(10, 0, 1000, 96, false).used == 12000 && gd::plan_pool(50000, 0, 1000, 96, false).used == 50000);
    CHECK(gd::plan_pool(0, 0, 1000, 0, false).used == 1000);           // (at least one chunk per wave, as alloc_rows)
}

static void test_memory_guard()
{
    ListPolicy p;
    p.W = 1200; p.K = 12;
    gd::ListState l = generic_list(p);
    l.rows = 1.0e6;
    p.on_report(l, overflow(1, 1000));      // no device size known: no guard
    CHECK(p.skin == 0.75);
    p.mem_total = (size_t)16 << 30;
    p.on_report(l, overflow(1, 1000));
    const double budget = (double)(p.mem_total / 16), bytes = 1000.0 * 4.0 * 1.0e6;
    CHECK(p.dense_budget == (uint32_t)std::max(64.0, 1000.0 * budget / bytes));
    CHECK(p.skin == std::max(0.15, l.rv * std::cbrt(0.9 * budget / bytes) - (l.rv - 0.75)));
    CHECK(p.skin < 0.75 && p.skin_dense_from == 0.75 && !p.dense_by_tile && p.K == 4u);
    CHECK(p.W == std::max(64u, p.dense_budget & ~7u));
    // back once the longest list, scaled with the cube of the radius, fits 0.8 of the budget
    l = generic_list(p);
    const double ratio = (1.0 + 0.75) / (1.0 + p.skin);
    const unsigned small = (unsigned)(0.8 * p.dense_budget / (ratio * ratio * ratio)) - 1;
    p.on_report(l, fits(0, small + 40));
    p.on_accepted(l, chunk(), unit_scale);
    CHECK(p.skin_next == 0);
    p.on_report(l, fits(0, small));
    p.on_accepted(l, chunk(), unit_scale);
    CHECK(p.skin_next == 0.75 && p.skin_dense_from == 0);
    // tiled lists: the pool's use counts, and only above 4 GB of rows without an overflow
    ListPolicy t; t.mem_total = (size_t)16 << 30;
    gd::ListState lt = tiled_list(t); lt.pool_used = 2u << 20;      // 2 GiB
    t.on_report(lt, fits(3000, 1000)); CHECK(t.skin == 0.75);
    lt.pool_used = 5u << 20;
    t.on_report(lt, fits(3000, 1000)); CHECK(t.skin < 0.75);
    // not with a fixed skin, nor for short lists
    ListPolicy f; f.mem_total = (size_t)16 << 30; f.skin_fixed = true;
    f.on_report(l, overflow(1, 1000)); CHECK(f.skin == 0.75 && f.dense_budget == 0);
    f.skin_fixed = false; f.on_report(l, overflow(1, 512)); CHECK(f.skin == 0.75);
}

static void test_class_width()
{
    ListPolicy p;
    auto accept = [&](unsigned need_t, uint32_t cap = 3312, bool droplet = false) {
        gd::ListState l = tiled_list(p, cap); l.droplet = droplet;
        p.on_report(l, fits(need_t));
        p.on_accepted(l, chunk(), unit_scale);
    };
    accept(2900); accept(2900);
    CHECK(p.skin_next == 0 && p.skin_streak == 2);
    accept(3200);      // (the estimate at 0.9 does not fit: the streak starts again)
    CHECK(p.skin_streak == 0);
    accept(2900); accept(2900); accept(2900);
    CHECK(p.skin_next == 0.9);
    p.take_pending_skin(1.0);
    CHECK(p.skin == 0.9);
    accept(3200);
    CHECK(p.skin_next == 0);
    accept(3300);      // within 24 entries of the class: back to 0.75, then 64 chunks of hold
    CHECK(p.skin_next == 0.75 && p.skin_hold == 64u && p.tile_cap == 3312u);
    p.take_pending_skin(1.0);
    for (int i = 0; i < 64; i++) accept(2900);
    CHECK(p.skin_hold == 0 && p.skin_next == 0 && p.skin_streak == 0);
    accept(2900); accept(2900); accept(2900);
    CHECK(p.skin_next == 0.9);
    // not with a fixed skin, auto_skin or the droplet term; not on a chunk without a complete interval
    for (int k = 0; k < 3; k++) {
        ListPolicy q;
        if (k == 0) q.skin_fixed = true;
        if (k == 1) q.tuner.enabled = true;
        for (int i = 0; i < 6; i++) {
            gd::ListState l = tiled_list(q); l.droplet = k == 2;
            q.on_report(l, fits(2900));
            q.on_accepted(l, chunk(), unit_scale);
        }
        CHECK(q.skin_next == 0 && q.skin == 0.75);
    }
    ListPolicy q;
    gd::Accepted a = chunk(); a.full_interval = false;
    for (int i = 0; i < 6; i++) { q.on_report(tiled_list(q), fits(2900)); q.on_accepted(tiled_list(q), a, unit_scale); }
    CHECK(q.skin_next == 0);
}

// the adaptation rule: aim at k_target of the margin, at most 2K + 1, in [1, 200]
static uint32_t adapted(double target, double lim, double ema, uint32_t K)
{
    return (uint32_t)std::max(1.0, std::min(200.0, std::floor(std::min(target * lim * target * lim / ema, 2.0 * K + 1))));
}

static void test_interval()
{
    ListPolicy p;
    p.K = 10;
    gd::ListState l = tiled_list(p);      // lim = (rv - cut) / 2 = 0.375
    const double lim = 0.5 * (l.rv - 1.0);
    p.on_accepted(l, chunk(0.01f, true), unit_scale);
    const double d1 = std::sqrt((double)0.01f), a1 = d1 * d1 / 10;
    CHECK(p.a2_ema == a1);
    const uint32_t k1 = adapted(0.9, lim, a1, 10);
    CHECK(p.K == k1 && k1 == 21u);      // (the rate admits 113: at most 2K + 1)
    p.on_accepted(l, chunk(0.04f, true), unit_scale);
    const double d2 = std::sqrt((double)0.04f), a2 = 0.6 * a1 + 0.4 * (d2 * d2 / k1);
    CHECK(p.a2_ema == a2 && p.K == adapted(0.9, lim, a2, k1) && p.K == 43u);
    // the developer target; the bead scale of the cutoff shrinks the margin
    const double d3 = std::sqrt((double)0.1f), a3 = d3 * d3 / 10;
    ListPolicy t; t.K = 10; t.k_target = 0.5;
    t.on_accepted(l, chunk(0.1f, true), unit_scale);
    CHECK(t.a2_ema == a3 && t.K == adapted(0.5, lim, a3, 10) && t.K == 3u);
    ListPolicy b; b.K = 10;
    gd::Accepted ab = chunk(0.1f, true); ab.scale_now = 1.2;
    b.on_accepted(l, ab, unit_scale);
    CHECK(b.K == adapted(0.9, 0.5 * (l.rv - 1.2), a3, 10) && b.K == 6u && adapted(0.9, lim, a3, 10) == 11u);
    // a zero displacement doubles K, up to 200
    ListPolicy z; z.K = 150;
    z.on_accepted(l, chunk(0.0f, true), unit_scale); CHECK(z.K == 200u);
    z.K = 7; z.on_accepted(l, chunk(0.0f, true), unit_scale); CHECK(z.K == 14u);
    // not without adaptation, a complete interval or on a search list
    ListPolicy n; n.K = 10; n.adapt = 0;
    n.on_accepted(l, chunk(0.01f, true), unit_scale); CHECK(n.K == 10u && n.a2_ema == 0);
    n.adapt = 1; n.on_accepted(l, chunk(0.01f, false), unit_scale); CHECK(n.K == 10u && n.a2_ema == 0);
    // a violation: K - K/4, remembered for 64 chunks
    ListPolicy v; v.K = 20; v.a2_ema = 1e-4;
    CHECK(v.on_violation());
    CHECK(v.K == 15u && v.K_bad == 20u && v.K_bad_ttl == 64u && v.a2_ema == 0);
    v.on_accepted(l, chunk(1e-6f, true), unit_scale);      // (the rate admits far more)
    CHECK(v.K == 19u && v.K_bad_ttl == 63u);
    v.K_bad_ttl = 1;
    v.on_accepted(l, chunk(1e-6f, true), unit_scale);
    CHECK(v.K_bad_ttl == 0 && v.K == 19u);
    v.on_accepted(l, chunk(1e-6f, true), unit_scale);
    CHECK(v.K == 39u);
    ListPolicy v3; v3.K = 3; v3.on_violation(); CHECK(v3.K == 2u);
    // at K = 1 the skin widens by 1.5 until it would cover more than 8 cutoffs
    ListPolicy w; w.K = 1;
    int widen = 0;
    while (w.on_violation() && widen < 50) widen++;
    CHECK(w.skin > 8 && w.skin == 0.75 * std::pow(1.5, widen) && widen == 6);
    // a chunk gd_run gives up returns the width and the interval its rollbacks changed, as they stood before the first of them:
    // the skin that no longer covers one step ...
    ListPolicy g; g.K = 1;
    do g.hold_for_retries(); while (g.on_violation());
    CHECK(g.skin > 8 && g.K == 1u && g.retries.held);
    g.retries_over(true);
    CHECK(g.skin == 0.75 && g.K == 1u && !g.retries.held);
    // ... and the interval of a chunk rolled back 25 times (1166: the smallest from which 24 cuts end above 1)
    ListPolicy h; h.K = 1166; h.K_bad = 7; h.K_bad_ttl = 3;
    for (int cuts = 0; cuts < 24; cuts++) { h.hold_for_retries(); CHECK(h.K >= 2u && h.on_violation()); }
    CHECK(h.K == 2u && h.K_bad == 3u && h.K_bad_ttl == 64u && h.skin == 0.75);
    ListPolicy h2; h2.K = 1165; for (int cuts = 0; cuts < 24; cuts++) h2.on_violation();
    CHECK(h2.K == 1u);
    h.hold_for_retries(); h.retries_over(true);
    CHECK(h.K == 1166u && h.K_bad == 7u && h.K_bad_ttl == 3u && h.skin == 0.75 && !h.retries.held);
    // an accepted chunk keeps what its retries arrived at, and the next chunk holds from there
    ListPolicy k; k.K = 20;
    k.hold_for_retries(); k.on_violation(); k.retries_over(false);
    CHECK(k.K == 15u && k.K_bad == 20u && !k.retries.held);
    k.retries_over(true);      // (nothing held: nothing returned)
    CHECK(k.K == 15u && k.K_bad == 20u);
    k.K_bad_ttl = 10; k.hold_for_retries(); k.on_violation(); CHECK(k.K == 12u && k.K_bad == 15u);
    k.retries_over(true);
    CHECK(k.K == 15u && k.K_bad == 20u && k.K_bad_ttl == 10u);
    // a width that an overflow narrowed for a dense state between two violations stays narrowed
    ListPolicy d; d.K = 1;
    d.hold_for_retries(); d.on_violation(); CHECK(d.skin == 0.75 * 1.5);
    d.skin = 0.3; d.retries_over(true);
    CHECK(d.skin == 0.3 && d.K == 1u);
    // a pending skin: K by ratio^2 (x 0.9 on the way up), not beyond the measured rate
    ListPolicy s; s.K = 20; s.skin_next = 0.9;
    s.take_pending_skin(1.0);
    CHECK(s.skin == 0.9 && s.K == 20u && s.K_bad_ttl == 0);      // (no measured rate: not above the interval in use)
    s.skin_next = 0.45; s.take_pending_skin(1.0);
    CHECK(s.K == (uint32_t)std::floor(20 * 0.5 * 0.5));
    ListPolicy r; r.K = 20; r.skin_next = 0.9; r.a2_ema = 0.005; r.K_bad_ttl = 5;
    r.take_pending_skin(1.0);
    const uint32_t rate = (uint32_t)std::floor(0.9 * 0.45 * 0.9 * 0.45 / 0.005);
    CHECK(rate == 32u && r.K == 25u && r.K_bad_ttl == 0);      // (floor(20 x 1.2^2 x 0.9) = 25)
    // chunk lengths: 12 intervals in [32, 256]
    ListPolicy c; c.K = 10;
    CHECK(c.chunk_steps(1000) == 120 && c.chunk_steps(50) == 50);
    c.K = 1; CHECK(c.chunk_steps(1000) == 32);
    c.K = 100; CHECK(c.chunk_steps(1000) == 256);
}

// the auto_skin sweep: chunk times from a cost per step that depends on the skin
static void test_auto_skin()
{
    for (int variant = 0; variant < 2; variant++) {
        ListPolicy p;
        CHECK(!p.set_tuning(0, 0, 1, 0, true));
        CHECK(p.tuner.enabled);
        p.K = 20; p.a2_ema = 1e-4;
        // variant 0: 0.5 x the width 6.5 % cheaper (taken); variant 1: only 5.5 % cheaper (the width in use kept)
        auto cost = [&](double skin) { return std::fabs(skin - 0.375) < 1e-12 ? (variant == 0 ? 0.935 : 0.945) : 1.0; };
        std::vector<double> seen;
        int drops = 0;
        for (int i = 0; i < 4 + 3 + 4 * 4; i++) {
            gd::ListState l = tiled_list(p);
            const double s0 = p.skin;
            seen.push_back(s0);
            drops += p.on_accepted(l, chunk(0, false, cost(s0) * 100, 100), unit_scale);
            if (i == 4) CHECK(p.tuner.cand.size() == 5 && p.chunk_steps(1000) == std::min<int64_t>(128, std::max<int64_t>(32, 4ll * p.K)));
        }
        const double c[5] = {0.75, 0.9, 0.525, 0.375, 0.2625};
        CHECK(std::fabs(p.tuner.cand[1] - c[1]) < 1e-12 && p.tuner.cand[2] == 0.7 * 0.75 && p.tuner.cand[3] == 0.5 * 0.75 && p.tuner.cand[4] == 0.35 * 0.75);
        // 4 chunks of wait and 3 measured at the width in use, then per candidate 1 settle + 3 measured
        for (int i = 0; i < 7; i++) CHECK(seen[i] == 0.75);
        for (int k = 1; k < 5; k++)
            for (int i = 0; i < 4; i++) CHECK(seen[7 + 4 * (k - 1) + i] == p.tuner.cand[k]);
        CHECK(p.tuner.done && p.tuner.wait == 50 && drops == 5);      // (four candidates, then the selected width)
        CHECK(p.skin == (variant == 0 ? 0.5 * 0.75 : 0.75));
        if (variant == 1) continue;
        // a rollback while measuring: the candidate settles again
        // drift: once the wait is over, a third more (or less) K starts a second round around the width in use
        const uint32_t K_ref = p.tuner.K_ref;
        CHECK(K_ref == p.interval_for_skin(1.0, 0.375));
        p.K = K_ref;
        for (int i = 0; i < 50; i++) p.on_accepted(tiled_list(p), chunk(), unit_scale);
        CHECK(p.tuner.done && p.tuner.wait == 0);
        p.K = (uint32_t)(0.7 * K_ref);
        p.on_accepted(tiled_list(p), chunk(), unit_scale);
        CHECK(!p.tuner.done && p.tuner.rounds == 2 && p.tuner.cand.size() == 4);
        CHECK(p.tuner.cand[0] == 0.375 && p.tuner.cand[1] == std::min(1.2 * 0.375, 1.0) && p.tuner.cand[2] == 0.85 * 0.375 && p.tuner.cand[3] == 0.7 * 0.375);
        CHECK(p.tuner.measured == 1);
        p.on_rollback(false);
        CHECK(p.tuner.measured == 0 && p.tuner.settle == 1 && p.tuner.acc_steps == 0);
    }
    // a grown tile class restarts it as well (the class is taken once the wait is down to 45)
    ListPolicy g;
    g.set_tuning(0, 0, 1, 0, true);
    g.K = 20; g.a2_ema = 1e-4;
    for (int i = 0; i < 4 + 3 + 16; i++) g.on_accepted(tiled_list(g), chunk(0, false, 100, 100), unit_scale);
    CHECK(g.tuner.done && g.skin == 0.75);
    for (int i = 0; i < 10; i++) g.on_accepted(tiled_list(g), chunk(), unit_scale);
    CHECK(g.tuner.done && g.tuner.cap_ref == 3312u);
    g.on_accepted(tiled_list(g, 4080), chunk(), unit_scale);
    CHECK(!g.tuner.done && g.tuner.rounds == 2);
    // no sweep with a fixed cadence
    ListPolicy f;
    f.set_tuning(0, 0, 0, 0, true);
    CHECK(!f.tuner.enabled && f.adapt == 0);
}

static void test_set_tuning()
{
    ListPolicy p;
    p.skin_dense_from = 0.75; p.dense_by_tile = true; p.skin = 0.3; p.tiled_ok = false; p.tiled_off = 1; p.a2_ema = 1;
    CHECK(!p.set_tuning(-1, 0, 1, 0, false));
    CHECK(p.skin == 0.75 && !p.skin_fixed && p.skin_dense_from == 0 && !p.dense_by_tile && p.tiled_ok && p.tiled_off == 0 && p.a2_ema == 0);
    CHECK(p.set_tuning(0.6, 9, 1, 200, false));
    CHECK(p.skin == 0.6 && p.skin_fixed && p.K == 9u && p.W == 200u);
    CHECK(!p.set_tuning(0, 0, 1, 200, false) && p.skin == 0.6 && p.K == 9u);
}

int main()
{
    test_summarize();
    test_tile_class();
    test_dense_tile();
    test_generic_rows();
    test_tiled_width_and_pool();
    test_memory_guard();
    test_class_width();
    test_interval();
    test_auto_skin();
    test_set_tuning();
    if (failures) { printf("policy: %d failures\n", failures); return 1; }
    printf("policy: ok\n");
    return 0;
}
