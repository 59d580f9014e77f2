// CPU unit test of the resident list of a handle (csrc/gdyn_list.hpp): gd::ResidentList alone, one event after another -- the
// transition table of DESIGN.md row by row, the row-width prediction at its fp32 boundary, both arms of the freshness condition, the
// guard of the pool read-back, the list fields of gd_context in every state they distinguish.  Built and run by
// tests/test_resident_list.py (plain g++, no HIP runtime).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "gdyn_list.hpp"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using gd::ResidentList;

// every member, for "nothing else changed"
static bool same(const ResidentList &a, const ResidentList &b)
{
    return a.valid == b.valid && a.tiled == b.tiled && a.W == b.W && a.tile_cap == b.tile_cap && a.rv == b.rv && a.rn == b.rn &&
           a.steps_since_build == b.steps_since_build && a.search_list == b.search_list && a.verified_serial == b.verified_serial &&
           a.w_packed == b.w_packed && a.bbox_cur == b.bbox_cur && a.bbox_valid == b.bbox_valid && a.need_valid == b.need_valid &&
           a.need_rv == b.need_rv && a.need_all_near == b.need_all_near && a.order_valid == b.order_valid && a.pool_used == b.pool_used &&
           a.repairs == b.repairs;
}

static ResidentList::Build tiled_build(float rv = 0.525f, bool predicted = false)
{
    ResidentList::Build b;
    b.rv = rv; b.rn = 0.45f; b.with_list = true; b.tiled = true; b.W = 96; b.tile_cap = 3312; b.packed_ab = true; b.all_near = false;
    b.predicted = predicted; b.pool_guess = 720;
    return b;
}
static ResidentList::Build generic_build(float rv = 0.525f)
{
    ResidentList::Build b;
    b.rv = rv; b.rn = rv; b.with_list = true; b.tiled = false; b.W = 104; b.tile_cap = 3312; b.packed_ab = false;
    return b;
}
// a tiled list in use, three steps old, its pool use and repairs read back, verified at serial 7
static ResidentList list_in_use()
{
    ResidentList l;
    l.build_enqueued(tiled_build());
    l.enter_use(true);
    l.stepped(3);
    const unsigned used[3] = {500, 640, 2};
    l.chunk_read(used);
    l.run_ended(true, 0.3, 0.f, 7);
    return l;
}

static void test_initial_state()
{
    const ResidentList l;
    CHECK(!l.valid && !l.tiled && l.W == 0 && l.tile_cap == 0 && l.rv == 0 && l.rn == 0 && l.steps_since_build == 0 && !l.search_list);
    CHECK(l.verified_serial == 0 && !l.w_packed && l.bbox_cur == 0 && !l.bbox_valid && !l.need_valid && l.pool_used == 0 && l.repairs == 0);
    CHECK(!l.order_valid && !l.orders_by_history());      // (a handle's first build orders k_step's threads by slot)
    CHECK(!l.fresh(0) && !l.fresh(1) && !l.serves_search(0.1) && !l.predicts(0.5f, false));
}

// model, cutoff, scale or tuning changed; the sweep moved the skin; a search met a moved bead: not valid, nothing else
static void test_drop()
{
    const ResidentList l0 = list_in_use();
    CHECK(l0.valid && l0.search_list && l0.w_packed && l0.bbox_valid && l0.need_valid && l0.order_valid && l0.verified_serial == 7);
    ResidentList l = l0, want = l0;
    l.drop();
    want.valid = false;
    CHECK(same(l, want));
    CHECK(l.orders_by_history());      // (the same beads where they were: the order key still describes them)
    l.drop();      // (idempotent)
    CHECK(same(l, want));
}

// positions from the caller: not valid; w_packed, box, row history and order key cleared
static void test_positions_set()
{
    const ResidentList l0 = list_in_use();
    ResidentList l = l0, want = l0;
    l.positions_set();
    want.valid = false; want.w_packed = false; want.bbox_valid = false; want.need_valid = false; want.order_valid = false;
    CHECK(same(l, want));
    CHECK(!l.orders_by_history());         // (... and orders its threads by slot: nothing of the handle's earlier state decides a result)
    CHECK(l.need_rv == l0.need_rv && l.pool_used == 640 && l.bbox_cur == l0.bbox_cur);
    CHECK(!l.predicts(l0.rv, false));      // (the next tiled build has no history)
}

// new topology: not valid; w_packed cleared; box and history kept
static void test_topology_changed()
{
    const ResidentList l0 = list_in_use();
    ResidentList l = l0, want = l0;
    l.topology_changed();
    want.valid = false; want.w_packed = false;
    CHECK(same(l, want));
    CHECK(l.bbox_valid && l.need_valid && l.predicts(l0.rv, false) && l.orders_by_history());
}

// rollback: not valid; box and order key cleared; w_packed restored to the value before the chunk; history and pool_used kept
static void test_rolled_back()
{
    for (int before = 0; before < 2; before++) {
        const ResidentList l0 = list_in_use();
        ResidentList l = l0, want = l0;
        l.rolled_back(before != 0);
        want.valid = false; want.bbox_valid = false; want.w_packed = before != 0; want.order_valid = false;
        CHECK(same(l, want));
        CHECK(l.need_valid && l.pool_used == 640 && l.repairs == 2 && l.steps_since_build == 3);
        CHECK(l.predicts(l0.rv, false) && !l.orders_by_history());      // (rows from the history, threads by slot)
        // the retry's build writes a key again; a second rollback takes it back again
        l.build_enqueued(tiled_build(0.525f, true));
        CHECK(l.orders_by_history());
        l.rolled_back(before != 0);
        CHECK(!l.orders_by_history());
    }
    {   // the value before the chunk, whatever the chunk's builds made of it: plain positions stay plain
        ResidentList l;
        const bool snap = l.w_packed;
        l.build_enqueued(tiled_build());
        CHECK(l.w_packed);
        l.rolled_back(snap);
        CHECK(!l.w_packed);
    }
}

// a build outside gd_run refused, to be run again on the same positions: the order key it wrote is not used; nothing else
static void test_build_refused()
{
    ResidentList l;
    l.build_enqueued(tiled_build());
    CHECK(l.orders_by_history());
    ResidentList want = l;
    l.build_refused();
    want.order_valid = false;
    CHECK(same(l, want));
    CHECK(l.need_valid && l.predicts(0.525f, false) && l.pool_used == 720);      // (the retry's rows are predicted from what the refused build counted)
    l.build_refused();      // (idempotent)
    CHECK(same(l, want));
    l.build_enqueued(tiled_build(0.525f, true));      // the retry: accepted, in use, and the build after it is ordered by its key
    l.enter_use(false);
    CHECK(l.orders_by_history());
}

// a build enqueued
static void test_build_enqueued()
{
    {   // the first tiled build: no history, the guessed pool use stands in
        ResidentList l;
        const ResidentList::Build b = tiled_build();
        CHECK(!l.predicts(b.rv, b.all_near));
        l.build_enqueued(b);
        CHECK(!l.valid);      // (not in use yet)
        CHECK(l.rv == b.rv && l.rn == b.rn && l.tiled && l.tile_cap == 3312 && l.W == 96 && l.w_packed);
        CHECK(l.bbox_cur == 1 && l.bbox_valid && l.steps_since_build == 0);
        CHECK(l.need_valid && l.need_rv == b.rv && !l.need_all_near && l.pool_used == 720);
        CHECK(l.order_valid);      // (it writes the key the next build orders by)
        CHECK(!l.search_list && l.verified_serial == 0 && l.repairs == 0);
    }
    {   // a predicted tiled build keeps the pool use that was read back; the history moves to its radius and class mode
        ResidentList l = list_in_use();
        ResidentList::Build b = tiled_build(0.53f, true);
        b.all_near = true; b.tile_cap = 4080; b.W = 64;
        CHECK(l.bbox_cur == 1);
        l.build_enqueued(b);
        CHECK(l.pool_used == 640 && l.need_valid && l.need_rv == 0.53f && l.need_all_near);
        CHECK(l.bbox_cur == 0 && l.bbox_valid && l.steps_since_build == 0 && l.tile_cap == 4080 && l.W == 64 && l.rv == 0.53f);
        CHECK(l.valid && l.search_list && l.verified_serial == 7 && l.repairs == 2);      // (in use as it was until enter_use says otherwise)
    }
    {   // a generic build: no box for the next build, the history and the pool use are not touched, W is the uniform row width
        ResidentList l = list_in_use();
        l.build_enqueued(generic_build(0.6f));
        CHECK(!l.tiled && l.W == 104 && l.rv == 0.6f && l.rn == 0.6f && !l.w_packed && l.bbox_cur == 0 && !l.bbox_valid);
        CHECK(l.need_valid && l.need_rv == 0.525f && l.pool_used == 640 && l.steps_since_build == 0);
        CHECK(l.order_valid);      // (a generic build writes no key: the one of the last tiled build stands, as it was ...)
        ResidentList n;
        n.build_enqueued(generic_build());
        CHECK(!n.order_valid);     // (... also when there is none)
        ResidentList r = list_in_use();
        r.rolled_back(true);
        r.build_enqueued(generic_build());
        CHECK(!r.order_valid);     // (a key taken back stays taken back across a generic build)
    }
    {   // without a list (no pair term): the counting sort alone -- the row width of the list before stays, everything else as above
        ResidentList l = list_in_use();
        ResidentList::Build b;
        b.rv = 1.f; b.rn = 1.f; b.with_list = false; b.tiled = false; b.W = 0; b.tile_cap = 3312; b.packed_ab = true;
        l.build_enqueued(b);
        CHECK(l.W == 96 && !l.tiled && l.rv == 1.f && l.rn == 1.f && l.w_packed && !l.bbox_valid && l.bbox_cur == 0 && l.steps_since_build == 0);
        CHECK(l.need_valid && l.pool_used == 640 && l.order_valid);
        ResidentList l1;
        l1.build_enqueued(b);
        CHECK(l1.W == 0 && !l1.serves_search(0.5));      // (W == 0: a search builds a list first, whatever the radius)
        l1.enter_use(false);
        CHECK(!l1.serves_search(0.5));
    }
}

// the build's list enters use: valid, search_list as given -- one transition
static void test_enter_use()
{
    for (int by_search = 0; by_search < 2; by_search++) {
        ResidentList l;
        l.build_enqueued(tiled_build());
        ResidentList want = l;
        l.enter_use(by_search != 0);
        want.valid = true; want.search_list = by_search != 0;
        CHECK(same(l, want));
    }
    ResidentList l = list_in_use();      // (a search list is replaced by a force list)
    l.build_enqueued(tiled_build(0.525f, true));
    l.enter_use(false);
    CHECK(l.valid && !l.search_list);
}

static void test_stepped()
{
    ResidentList l;
    l.build_enqueued(generic_build());
    l.enter_use(false);
    ResidentList want = l;
    l.stepped(5); l.stepped(3);
    want.steps_since_build = 8;
    CHECK(same(l, want));
    l.build_enqueued(generic_build());
    CHECK(l.steps_since_build == 0);
}

// chunk read back: pool use and repairs taken over only when tiled and the cursor is non-zero
static void test_chunk_read()
{
    const unsigned used[3] = {300, 450, 7}, later_peak[3] = {450, 300, 1}, zero_cursor[3] = {0, 900, 9};
    {
        ResidentList l;
        l.build_enqueued(tiled_build());
        ResidentList want = l;
        l.chunk_read(used);
        want.pool_used = 450; want.repairs = 7;      // max(used[0], used[1]), used[2]
        CHECK(same(l, want));
        l.chunk_read(later_peak);
        CHECK(l.pool_used == 450 && l.repairs == 1);
        const ResidentList before = l;
        l.chunk_read(zero_cursor);      // (no tiled build ran in the chunk: nothing to take over)
        CHECK(same(l, before));
    }
    {   // a generic list ignores the cursor
        ResidentList l = list_in_use();
        l.build_enqueued(generic_build());
        const ResidentList before = l;
        l.chunk_read(used);
        CHECK(same(l, before) && l.pool_used == 640 && l.repairs == 2);
    }
}

// run ended verified: verified_serial = state_serial, under gd_run's condition
static void test_run_ended()
{
    const double cut = 0.3;
    auto stepped_list = [](const ResidentList::Build &b) { ResidentList l; l.build_enqueued(b); l.enter_use(false); l.stepped(8); return l; };
    const ResidentList t = stepped_list(tiled_build(0.5f));
    const double lim = 0.5 * (0.5 - cut);      // 0.1
    float inside = (float)(lim * lim);      // the largest fp32 bound inside the margin, and the next one
    if ((double)inside > lim * lim) inside = std::nextafterf(inside, 0.f);
    const float outside = std::nextafterf(inside, 1.f);
    CHECK((double)inside <= lim * lim && (double)outside > lim * lim);
    {
        ResidentList l = t, want = t;
        l.run_ended(true, cut, inside, 42);
        want.verified_serial = 42;
        CHECK(same(l, want));
        CHECK(l.fresh(42) && !l.fresh(43));
    }
    { ResidentList l = t; l.run_ended(true, cut, outside, 42); CHECK(same(l, t)); }      // the last step's positions beyond the margin
    { ResidentList l = t; l.run_ended(false, cut, 0.f, 42); CHECK(same(l, t)); }        // scales moved behind the last step, droplet, no steps
    { ResidentList l = t; l.run_ended(true, 0.5, 0.f, 42); CHECK(same(l, t)); }         // no margin: lim == 0
    { ResidentList l = t; l.run_ended(true, 0.6, 0.f, 42); CHECK(same(l, t)); }         // cutoff beyond the list radius
    { ResidentList l = t; l.drop(); const ResidentList d = l; l.run_ended(true, cut, 0.f, 42); CHECK(same(l, d)); }      // list dropped by the last chunk
    { const ResidentList g = stepped_list(generic_build(0.5f)); ResidentList l = g; l.run_ended(true, cut, 0.f, 42); CHECK(same(l, g)); }   // generic: observations build
}

// The prediction test: valid history, the same class mode, |rv / need_rv - 1| <= 0.02 in fp32.  With a history at radius 1 the
// quotient is rv itself and rv - 1 is exact in fp32 for rv in [0.5, 2): the boundary is the last multiple of 2^-23 (2^-24 below 1)
// that is not beyond 0.02f = 0.0199999995529651641845703125.
static void test_predicts()
{
    ResidentList l;
    l.build_enqueued(tiled_build(1.f));
    CHECK(l.predicts(1.f, false));
    const float up = 1.f + 167772.f / 8388608.f, up_next = std::nextafterf(up, 2.f);
    CHECK((double)up - 1.0 <= (double)0.02f && (double)up_next - 1.0 > (double)0.02f && std::fabs((double)up - 1.02) < 2e-7);
    CHECK(l.predicts(up, false));
    CHECK(!l.predicts(up_next, false));
    const float down = 1.f - 335544.f / 16777216.f, down_next = std::nextafterf(down, 0.f);
    CHECK(1.0 - (double)down <= (double)0.02f && 1.0 - (double)down_next > (double)0.02f && std::fabs((double)down - 0.98) < 1e-7);
    CHECK(l.predicts(down, false));
    CHECK(!l.predicts(down_next, false));
    CHECK(!l.predicts(1.f, true));      // another class mode
    l.positions_set();
    CHECK(!l.predicts(1.f, false));     // no history
    ResidentList z;
    z.build_enqueued(tiled_build(0.f));
    CHECK(z.need_valid && !z.predicts(0.f, false));      // a history at radius 0 predicts nothing (no division by it)
    ResidentList g;
    g.build_enqueued(generic_build(1.f));
    CHECK(!g.predicts(1.f, false));     // generic builds leave no history
    ResidentList m;      // a history at another radius: relative, not absolute
    m.build_enqueued(tiled_build(0.525f));
    CHECK(m.predicts(0.525f, false) && m.predicts(0.525f * 1.019f, false) && !m.predicts(0.525f * 1.021f, false) && !m.predicts(0.525f * 0.979f, false));
}

// fresh for an observation: valid and (nothing has stepped on it, or the last run verified it at this serial)
static void test_fresh()
{
    ResidentList l;
    l.build_enqueued(tiled_build(0.5f));
    CHECK(!l.fresh(5));      // built, not in use
    l.enter_use(false);
    CHECK(l.fresh(5) && l.fresh(6));      // arm 1: no step since the build, whatever the serial
    l.stepped(1);
    CHECK(!l.fresh(5));
    l.run_ended(true, 0.3, 0.f, 5);
    CHECK(l.fresh(5));       // arm 2: verified at this serial
    CHECK(!l.fresh(6));      // ... and not at a later one (positions or model changed since)
    l.drop();
    CHECK(!l.fresh(5));      // neither arm without a valid list
    l.build_enqueued(tiled_build(0.5f)); l.enter_use(false);
    CHECK(l.fresh(99));
}

// serves a pair search at dcut: valid, dcut (as fp32) within the list radius, rows allocated
static void test_serves_search()
{
    ResidentList l;
    l.build_enqueued(tiled_build(0.5f));
    CHECK(!l.serves_search(0.4));
    l.enter_use(false);
    CHECK(l.serves_search(0.4) && l.serves_search(0.5) && l.serves_search(0.5 + 1e-9) && !l.serves_search(0.51));      // (0.5 + 1e-9 rounds to 0.5f)
    CHECK(!l.serves_search(std::nan("")));
    l.stepped(4);
    CHECK(l.serves_search(0.4));      // (how far the beads have moved is the search kernel's business)
    l.drop();
    CHECK(!l.serves_search(0.4));
}

static void test_state()
{
    const ResidentList l = list_in_use();
    const gd::ListState s = l.state(0.3, 2000, 16.0 * 30208, true, false);
    CHECK(s.cut == 0.3 && s.rv == l.rv && s.tiled && s.tile_cap == 3312 && s.W == 96 && s.pool_used == 640 && s.pool_kib == 2000);
    CHECK(s.rows == 16.0 * 30208 && s.droplet && !s.can_tile);
    ResidentList g;
    g.build_enqueued(generic_build());
    const gd::ListState t = g.state(0.0, 0, 1536.0, false, true);
    CHECK(t.cut == 0.0 && !t.tiled && t.W == 104 && t.pool_used == 0 && t.pool_kib == 0 && !t.droplet && t.can_tile);
}

// the list fields of gd_context; everything else in it is the caller's
static gd_context context_of(const ResidentList &l, uint64_t rebuilds, uint64_t near = 4444, uint32_t largest = 2930, uint64_t rows = 2 * 1536)
{
    gd_context o;
    memset(&o, 0, sizeof o);
    o.step = 17; o.rebuilds = 1234; o.rebuild_interval = 9; o.list_entries = 55; o.compensated = 1; o.callback_pending = 1;
    l.fill_context(&o, rebuilds, near, largest, rows);
    CHECK(o.step == 17 && o.rebuilds == 1234 && o.rebuild_interval == 9 && o.list_entries == 55 && o.compensated == 1 && o.callback_pending == 1);
    return o;
}
static void test_fill_context()
{
    {   // before any build
        const gd_context o = context_of(ResidentList{}, 0);
        CHECK(o.list_path == 0 && o.tile_capacity == 0 && o.largest_tile == 0 && o.row_repairs == 0 && o.near_entries == 0 && o.list_bytes == 0);
        CHECK(o.list_radius == 0.0);
    }
    {   // valid, tiled: list_bytes = 1024 x pool_used
        const ResidentList l = list_in_use();
        const gd_context o = context_of(l, 1);
        CHECK(o.list_path == 2 && o.tile_capacity == 3312 && o.largest_tile == 2930 && o.row_repairs == 2 && o.near_entries == 4444);
        CHECK(o.list_bytes == 1024ull * 640 && o.list_radius == (double)l.rv);
        ResidentList big = l;      // (beyond 32 bits)
        const unsigned used[3] = {0xfffffff0u, 5, 0};
        big.chunk_read(used);
        CHECK(context_of(big, 1).list_bytes == 1024ull * 0xfffffff0ull);
    }
    {   // valid, generic: list_bytes = W x R x Np x 4
        ResidentList l = list_in_use();
        l.build_enqueued(generic_build(0.6f));
        l.enter_use(false);
        const gd_context o = context_of(l, 2);
        CHECK(o.list_path == 1 && o.tile_capacity == 0 && o.largest_tile == 0 && o.row_repairs == 0 && o.near_entries == 0);
        CHECK(o.list_bytes == 104ull * 2 * 1536 * 4 && o.list_radius == (double)0.6f);
        CHECK(context_of(l, 2, 0, 0, (uint64_t)128 * 30208).list_bytes == 104ull * 128 * 30208 * 4);      // (1.6 GB: beyond 32 bits)
    }
    {   // dropped after a tiled build: the path and the radius of the last build stay, and so do row_repairs and near_entries (they
        // follow the path, not validity); what describes the list in use is 0
        ResidentList l = list_in_use();
        l.drop();
        const gd_context o = context_of(l, 1);
        CHECK(o.list_path == 2 && o.tile_capacity == 0 && o.largest_tile == 0 && o.list_bytes == 0);
        CHECK(o.row_repairs == 2 && o.near_entries == 4444 && o.list_radius == (double)l.rv);
    }
    {   // dropped after a generic build
        ResidentList l;
        l.build_enqueued(generic_build());
        l.enter_use(false);
        l.positions_set();
        const gd_context o = context_of(l, 1);
        CHECK(o.list_path == 1 && o.tile_capacity == 0 && o.largest_tile == 0 && o.list_bytes == 0 && o.row_repairs == 0 && o.near_entries == 0);
    }
    {   // list_path is 0 only before the first build: a build that is not in use yet counts
        ResidentList l;
        l.build_enqueued(tiled_build());
        CHECK(context_of(l, 1).list_path == 2 && context_of(l, 1).list_bytes == 0);
        CHECK(context_of(ResidentList{}, 3).list_path == 1);      // (rebuilds alone decide; no path recorded: generic)
    }
}

int main()
{
    test_initial_state();
    test_drop();
    test_positions_set();
    test_topology_changed();
    test_rolled_back();
    test_build_refused();
    test_build_enqueued();
    test_enter_use();
    test_stepped();
    test_chunk_read();
    test_run_ended();
    test_predicts();
    test_fresh();
    test_serves_search();
    test_state();
    test_fill_context();
    if (failures) { fprintf(stderr, "resident list: %d check(s) failed\n", failures); return 1; }
    printf("resident list: ok\n");
    return 0;
}
