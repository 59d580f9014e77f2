// gdyn_policy.hpp -- the list policy of libgdyn: what the next list build and the next chunk of gd_run look like.
//
// Verlet skin (pending, dense and class-selected widths), rebuild interval K and its adaptation, generic row width W, LDS tile class and
// the tiled path, single-class lists, the repair-queue width, the opt-in timing sweep (auto_skin).  Plain C++ (no HIP runtime, handle or
// environment): gdyn_capi.hip hands it what builds and chunks reported and the list in use; tests/native/test_list_policy.cpp drives it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gdyn_types.h"

namespace gd {

// The flags of a build or chunk (R x GD_NFLAGS words, gdyn_types.h), over all replicas
struct BuildReport {
    unsigned bits = 0;                  // GD_FLAG_OVERFLOW bits, ORed
    bool over = false, class_over = false, tile_over = false, violated = false;
    unsigned need_w = 0, need_t = 0, ncell = 0;      // largest NEED_W, NEED_TILE, NCELL
    float maxd2 = 0;                    // largest MAXDISP2
};

inline BuildReport summarize(const unsigned *flags, uint32_t R)
{
    BuildReport b;
    for (const unsigned *f = flags; f < flags + (size_t)R * GD_NFLAGS; f += GD_NFLAGS) {
        b.bits |= f[GD_FLAG_OVERFLOW]; b.tile_over |= f[GD_FLAG_TILE_OVERFLOW] != 0; b.violated |= f[GD_FLAG_VIOLATION] != 0;
        b.need_w = std::max(b.need_w, f[GD_FLAG_NEED_W]); b.need_t = std::max(b.need_t, f[GD_FLAG_NEED_TILE]); b.ncell = std::max(b.ncell, f[GD_FLAG_NCELL]);
        float d2; memcpy(&d2, &f[GD_FLAG_MAXDISP2], 4); b.maxd2 = std::max(b.maxd2, d2);
    }
    b.over = b.bits != 0; b.class_over = (b.bits & 2u) != 0;
    return b;
}

// The list in use and the handle, as the policy sees them
struct ListState {
    double cut = 0;                     // pair cutoff (0: no pair term, no lists)
    float rv = 0;                       // list radius
    bool tiled = false;                 // tiled (LDS) lists
    uint32_t tile_cap = 0, W = 0;       // tile capacity / generic row width the list was built with
    uint32_t pool_used = 0; size_t pool_kib = 0;      // KiB of the row pool the last build took / the pool holds
    double rows = 0;                    // R x Np
    bool droplet = false, can_tile = false;      // droplet attraction on; the kernel path and the pair form admit tiled lists
};

// An accepted chunk of gd_run: device time, steps, largest squared displacement at the end of an interval, bead-scale factor of the
// cutoff now; whether it holds the last step of a complete K-step interval, whether it began on a (wider) contact-search list
struct Accepted { double ms = 0; int64_t steps = 0; float maxd2 = 0; double scale_now = 1; bool full_interval = false, on_search_list = false; };

// The row pool of tiled lists (KiB: one chunk of a k_step wave's rows, 64 lanes x 16 bytes) before a build.  With history
// (predict: every bead's row is predicted from what it needed at the build before) the pool follows the use of the last build, at
// least a chunk per wave; without (first build, positions from the caller, another list radius or class mode) every wave gets rows
// of W entries, W / 8 chunks.  Margin: an eighth + 2 KiB per wave on top of that use (the builds between two readbacks grow with
// the lists, repaired waves take fresh rows); the pool is reallocated -- with a sixteenth more, so that it is not reallocated at
// every build of a growing state -- when it is smaller than that, and given back when it is larger than twice that + 4 KiB per wave.
struct PoolPlan {
    size_t used = 0;        // KiB the build is expected to take (what stands in for the use until a readback brings the real one)
    size_t want = 0;        // KiB the pool has to hold: used + the margin
    bool resize = false;    // the pool is outside [want, 2 want + 4 waves]
    size_t alloc_kib = 0;   // ... and is reallocated at this size
};
inline PoolPlan plan_pool(size_t pool_used, size_t pool_kib, size_t waves, uint32_t W, bool predict)
{
    PoolPlan pl;
    pl.used = std::max<size_t>(pool_used, predict ? waves : waves * std::max<size_t>(W / 8u, 1u));
    pl.want = pl.used + pl.used / 8 + 2 * waves;
    pl.resize = pool_kib < pl.want || pool_kib > 2 * pl.want + 4 * waves;
    pl.alloc_kib = pl.want + pl.want / 16;
    return pl;
}

// ---- Replica groups of the step launches between two builds (gd_run, enqueue_chunk).  Replicas are independent:
// the k_step launches of an interval may run as two launches per step, replicas [0, A) on the handle's stream and [A, R) on a second
// one, so that the blocks of one group fill the CUs the other leaves idle while its rounds drain.  Results do not depend on it: every
// word a stepping launch reads or writes is addressed by the global replica or by a bead of it.  The rule is a function of the state
// alone, never of a clock.
enum : uint32_t { STEP_GROUPS_RULE = 0, STEP_GROUPS_ONE = 1, STEP_GROUPS_TWO = 2 };      // gd_set_step_groups (include/gdyn_groups.h)
struct StepGroupState {
    uint32_t R = 0, nblk = 0;           // replicas of the handle, blocks per replica
    bool tiled = false;                 // the list in use is tiled
    bool post_step = false;             // a kernel runs behind k_step (droplet term, per-replica pairs): it covers all replicas of a step
    bool device_noise = true;           // the noise is drawn on the device (injected noise is staged per step for all replicas)
    bool whole_replica_map = false;     // the handle maps whole replicas to XCDs (StepParams.cpb == 0)
    bool fast_pair = false;             // the pair form has a specialised kernel (StepParams.pk != 0): only those variants take a group offset
};
// blocks the smaller group must have for mode 0 to split, and group A's share of the replicas in sixteenths.  384 = half a round of the
// device (256 CUs x 3 resident blocks): a launch that splits is more than one round, a one-round grid stays on one launch.  Measured
// (DESIGN.md section 7l, 16 replicas in 8 + 8): groups of 472 blocks (30 000 beads) gain 9 %, groups of 240 gain 5 % -- a one-round
// grid, kept on one launch all the same --, groups of 120 and of 48 lose 10 %; the equal split against 7 : 9 and 9 : 7 sixteenths there
constexpr uint32_t STEP_GROUPS_MIN_BLOCKS = 384u;
constexpr uint32_t STEP_GROUPS_A16 = 8u;
// Replicas of group A (group B: the rest), or 0: one launch.  Both sizes are multiples of 8, so that each group keeps the block map
// it would have alone (block_map with cpb == 0: XCD x runs replicas x, x + 8, ... of the group).
inline uint32_t step_group_split(uint32_t mode, const StepGroupState &st, uint32_t min_blocks = STEP_GROUPS_MIN_BLOCKS, uint32_t a16 = STEP_GROUPS_A16)
{
    if (mode != STEP_GROUPS_RULE && mode != STEP_GROUPS_TWO) return 0;
    if (!st.tiled || st.post_step || !st.device_noise || !st.whole_replica_map || !st.fast_pair) return 0;
    if (st.R < 2 * GD_XCDS || st.R % GD_XCDS != 0 || st.nblk == 0) return 0;
    a16 = std::min(std::max(a16, 1u), 15u);
    uint32_t ra = (uint32_t)(((uint64_t)st.R * a16 + 8u * GD_XCDS) / (16u * GD_XCDS)) * GD_XCDS;      // the multiple of 8 nearest to R a16 / 16
    ra = std::min(std::max(ra, (uint32_t)GD_XCDS), st.R - GD_XCDS);
    const uint32_t small = std::min(ra, st.R - ra);
    if (mode == STEP_GROUPS_RULE && (uint64_t)small * st.nblk < min_blocks) return 0;
    return ra;
}

// ---- Prepared contexts (include/gdyn_prep.h).  In a span that runs in two groups, each step of each group may be
// k_ctx_prep -> k_step on the group's stream: one wave per replica applies the pending callback and derives the step's float constants,
// and the stepping blocks copy them instead of each computing them in front of its barrier.  The extra launch costs its stream a drain
// and a launch per step, which only the other group's k_step can cover: never in a span that steps in one launch.  ra: what
// step_group_split returned for the span.  prep: CTX_PREP_RULE in the product; the developer library's GDYN_CTX_PREP sets the others.
enum : uint32_t { CTX_PREP_NEVER = 0, CTX_PREP_RULE = 1, CTX_PREP_ALWAYS = 2 };
// blocks the smaller group must have under mode 0.  Measured (one handle, prepared against in-kernel contexts
// alternating): groups of 1 888 blocks (30 000 beads x 64 replicas) gain 2.5 % of the wall time per step, groups of 944 lose 5 %, of 472
// lose 17 %, of 240 lose 22 % -- the preparation launch is 8 us on its stream, and the shorter the other group's k_step, the less of it is
// covered.  The threshold is the smallest size measured to win; the headline (128 replicas: groups of 3 776 blocks) gains 3.7 %.
constexpr uint32_t CTX_PREP_MIN_BLOCKS = 1888u;
inline bool ctx_prepared(uint32_t group_mode, uint32_t ra, const StepGroupState &st, uint32_t prep = CTX_PREP_RULE, uint32_t min_blocks = CTX_PREP_MIN_BLOCKS)
{
    if (ra == 0 || ra >= st.R || prep == CTX_PREP_NEVER) return false;      // one launch per step: the kernel as it was
    if (prep == CTX_PREP_ALWAYS || group_mode == STEP_GROUPS_TWO) return true;
    if (group_mode != STEP_GROUPS_RULE) return false;
    return (uint64_t)std::min(ra, st.R - ra) * st.nblk >= min_blocks;
}

struct ListPolicy {
    // developer hooks (gd_create)
    std::vector<unsigned> tile_caps = {3312u, 4080u, 5072u, 8192u};      // (4080: the largest tile with byte-offset list entries)
    double k_target = 0.90;             // share of the skin the largest displacement of an interval aims at
    FILE *trace = nullptr;
    size_t mem_total = 0;               // device memory (bytes; 0: unknown, no memory guard)
    double skin = 0.75;   // relative to the pair cutoff; 0.65..0.8 are within 3% of each other on S-genome-30k, smaller tiles leave more LDS margin
    bool skin_fixed = false;            // the caller chose a skin (gd_tuning.skin > 0): keep it
    double skin_next = 0;               // width the next list build moves to (the list in use serves out its interval; 0: none pending)
    double skin_dense_from = 0;         // > 0: the width was narrowed because a build met a dense state; the width to return to
    bool dense_by_tile = false;         // ... because the largest tile did not fit the LDS: returns by tile size
    uint32_t dense_budget = 0;          // dense_guard: longest list (entries) the memory budget admits
    uint32_t skin_streak = 0, skin_hold = 0;      // class_skin: chunks the wider width has fitted / to wait before it looks again
    uint32_t K = 4, adapt = 1, K_bad = 0, K_bad_ttl = 0;      // rebuild interval, adapted or not; one that violated the skin lately: stay below it
    double a2_ema = 0;                  // running mean of (largest displacement)^2 per step of an interval (0: none yet)
    uint32_t W = 0, tile_cap = 3312, tile_hold = 0;      // generic row width / tile capacity of the next build; chunks to keep a larger class
    bool all_near = false;              // single-class lists: a build met a far class beyond the tiled record's 504 entries (until below)
    bool tiled_ok = true; uint32_t tiled_off = 0;      // why the tiled path is off: 0 on, 1 a tile overflowed (dense transient: retried later), 2 by design
    uint32_t tiled_wait = 0, tiled_backoff = 8;     // accepted chunks since / until the next retry of the tiled path
    uint32_t repair_wide = 0;           // > 0: accepted chunks still to run with a repair block for EVERY wave (a build queued more than GD_REPAIR_GRID)
    uint32_t last_need_w = 0, last_need_t = 0;      // longest list (entries, padded) the last build reported / largest tile reported last
    uint32_t ncell_seen = 0;            // largest cell grid of the last build that reported one (sizes k_scan's launch)
    // Skin selection by measured cost (per workload, tune_skin): a few candidate widths are each run for a few verified chunks once
    // the rebuild interval has settled, the device time per step decides.  Results do not depend on the skin, only the cost does.
    struct SkinTuner {
        bool enabled = false, done = false;     // opt-in: gd_tuning.auto_skin
        std::vector<double> cand, cost; size_t idx = 0;
        int settle = 0, measured = 0, wait = 4, rounds = 0;      // wait: accepted chunks before the (next) sweep may start
        uint32_t K_ref = 0, cap_ref = 0;                         // rebuild interval / tile class when the last sweep ended
        double acc_ms = 0; uint64_t acc_steps = 0;
    } tuner;

    bool want_tiled(bool can_tile) const { return can_tile && tiled_ok && W <= GD_TILED_MAX_W; }      // open and periodic boxes alike
    // Steps of the next chunk of gd_run: shorter while the skin sweep measures candidates (four rebuild intervals), so that a sweep
    // costs a few thousand steps, not tens of thousands
    int64_t chunk_steps(int64_t left) const
    {
        const bool sweeping = tuner.enabled && !tuner.done && !tuner.cand.empty();
        return std::min<int64_t>(left, sweeping ? std::min<int64_t>(128, std::max<int64_t>(32, 4ll * K))
                                                : std::min<int64_t>(256, std::max<int64_t>(32, 12ll * K)));
    }
    // gd_set_tuning (validated by the caller); true when the caller's row width replaces W (the rows are to be reallocated)
    bool set_tuning(double t_skin, uint32_t rebuild_interval, uint32_t adapt_interval, uint32_t list_width, bool auto_skin)
    {
        if (t_skin > 0) { skin = t_skin; skin_fixed = true; }
        else if (t_skin < 0) { skin = 0.75; skin_fixed = false; skin_dense_from = 0; dense_by_tile = false; }      // back to the library's own choice
        skin_streak = 0; skin_hold = 0; skin_next = 0;
        if (rebuild_interval > 0) K = rebuild_interval;
        tuner = SkinTuner{}; tuner.enabled = auto_skin && adapt_interval != 0;          // (a fixed cadence: nothing to select for)
        a2_ema = 0; adapt = adapt_interval; tiled_ok = true; tiled_off = 0;
        if (list_width > 0 && list_width != W) { W = list_width; return true; }
        return false;
    }
    // Tile capacities (float4 entries) at which k_step still fits 3, 2, 1 blocks into the 160 KB of LDS of a CU (1.2 KB static LDS per
    // block on top of the tile; LDS is granted in 1280-byte granules: with 1184 B of static LDS 3264 entries fit 3 blocks, 3318 do not)
    unsigned pick_tile_cap(unsigned need) const
    {   // (> 8192: the need itself, the caller falls back to the generic path)
        for (unsigned c : tile_caps) if (need <= c) return c;
        return need;
    }
    // Interval the skin admits at the measured displacement rate (the adaptation formula of on_accepted)
    uint32_t interval_for_skin(double cut, double s) const
    {
        if (!(a2_ema > 0)) return K;
        const double lim = 0.5 * cut * s, k = 0.90 * lim * 0.90 * lim / a2_ema;
        return (uint32_t)std::max(1.0, std::min(200.0, std::floor(k)));
    }
    // Move to width `to` now: the interval follows the square of the skin (diffusive displacements) from the one adapted to at the old
    // width -- a tenth off on the way up -- and not beyond what the measured rate admits (the rate alone overshot after regime changes)
    void move_skin(double to, double cut)
    {
        const double ratio = skin > 0 ? to / skin : 1.0;
        const uint32_t k_scaled = (uint32_t)std::max(1.0, std::floor((double)K * ratio * ratio * (ratio > 1.0 ? 0.9 : 1.0)));
        skin = to;
        K = std::min(interval_for_skin(cut, skin), k_scaled); K_bad_ttl = 0;
    }
    // A pending width (class_skin, a dense state easing) takes over at a list build: interval and radius change together
    void take_pending_skin(double cut) { if (skin_next > 0) { const double to = skin_next; skin_next = 0; move_skin(to, cut); } }
    // Row width for a longest list of need_w entries: a quarter and 16 entries to spare, whole batches, at least 64
    static unsigned want_width(unsigned need_w) { return std::max(64u, (need_w + need_w / 4 + 16 + GD_UNROLL - 1) & ~(GD_UNROLL - 1)); }
    // What a build reported: widen the list, enlarge the LDS tile or fall back to the generic path, narrow the width of a dense state.
    // True when the build has to be redone (its chunk rolled back).
    bool on_report(const ListState &ls, const BuildReport &r)
    {
        if (r.need_t > 0 && r.need_t < (1u << 20)) last_need_t = r.need_t;
        if (r.need_w > 0) last_need_w = r.need_w;
        if (r.ncell > 0) ncell_seen = r.ncell;
        if (!r.tile_over && !r.over && ls.tiled && r.need_t > 0) {
            // size the LDS tile to what the builds need, at the largest capacity of its occupancy class (an overflow costs one
            // rolled-back chunk and keeps the larger class for a while, so the margin for the smaller class can be thin)
            unsigned want = pick_tile_cap(r.need_t + 24);
            if (want < tile_cap && tile_hold > 0) { tile_hold--; want = tile_cap; }
            // at the wider width class_skin selected the tiles are about to leave the three-block class: class_skin takes the
            // narrower list back at the next build, where they fit it -- no detour through the two-block class
            const bool wide = !skin_fixed && adapt && !tuner.enabled && !(skin_dense_from > 0) && !ls.droplet && skin >= 0.9 - 1e-9 && skin <= 0.9 + 1e-9;
            if (want > 3312u && tile_cap <= 3312u && wide) want = tile_cap;
            if (want != tile_cap && want <= 8192u && trace) fprintf(trace, "[gdyn] tile capacity %u -> %u (largest tile %u)\n", tile_cap, want, r.need_t);
            if (want <= 8192u) tile_cap = want;
        }
        if (r.tile_over) {
            const unsigned cap = pick_tile_cap(r.need_t + r.need_t / 32 + 32);
            const unsigned cap_max = 8192u;      // 128 KB dynamic + static LDS < 160 KB per CU (one block per CU: still ahead of the generic path)
            if (cap <= cap_max) { tile_cap = cap; tile_hold = 4; }
            else {
                // Too dense for one tile at this width (a globule).  A tile shrinks about with the square of the list radius: the width
                // is narrowed until the largest tile fits (skin >= 0.15 x cutoff; tiled lists stay 2-2.4 x cheaper per step), class_skin
                // eases it back.  Only when that is not enough, or the width is pinned, the generic path takes over (retried with back-off).
                bool narrowed = false;
                if (!skin_fixed && ls.cut > 0 && ls.rv > 0 && r.need_t < (1u << 20)) {
                    const double sc = ls.rv / ls.cut - skin;
                    const double ratio = std::min(0.97, std::max(0.5, std::sqrt(0.85 * (double)cap_max / (double)r.need_t)));
                    const double skin_new = std::max(0.15, ls.rv * ratio / ls.cut - sc);
                    if (skin_new < skin - 1e-9) {
                        narrow_for_dense(skin_new, true);
                        tile_cap = cap_max; tile_hold = 4; narrowed = true;
                        if (trace) fprintf(trace, "[gdyn] dense state (largest tile %u): skin %.3f\n", r.need_t, skin_new);
                    }
                }
                if (!narrowed) { tiled_ok = false; tiled_off = 1; }
            }
        }
        if (r.over) {
            // Tiled lists: the pool was full (pool_used is the need: the next build sizes the pool from it) or a build queued more waves
            // for repair than the repair launch has blocks.  Generic lists: the next build gets the longest list with 6 % to spare.
            if (ls.tiled && (r.bits & 4u) && (size_t)ls.pool_used <= ls.pool_kib) repair_wide = 16;      // (bit 4 with room in the pool: the repair queue)
            if (!ls.tiled) W = std::max(r.need_w + r.need_w / 16 + 8, W + 8);
            // a class beyond its field of the tiled record: single-class lists while that is the far class (a near class beyond 8 184
            // entries is beyond tiled rows)
            if (r.class_over && !all_near && r.need_w <= GD_TILED_MAX_NEAR) all_near = true;
            else if (r.class_over) W = std::max(W, GD_TILED_MAX_W + 8u);
            dense_guard(ls, r.need_w);
        }
        else if (!r.tile_over && r.need_w > 0) {
            if (ls.tiled && (size_t)ls.pool_used * 1024u > ((size_t)4 << 30)) dense_guard(ls, r.need_w);      // (rows of several GB: within the budget?)
            if (all_near && r.need_w <= GD_TILED_MAX_FAR) all_near = false;      // (no far class can overflow its field any more; from the next build)
            // the longest list is reported by every build: the row width is given back when a dense transient has passed.  Generic
            // lists: the uniform rows.  Tiled lists: the guess a build without history starts its ragged rows from, and sizes the row
            // pool by (plan_pool) -- a width left behind by a generic excursion or a caller's list_width is honoured once, then
            // replaced by what the lists were measured to need
            const unsigned want_w = want_width(r.need_w);
            if (2 * want_w <= W) W = want_w;       // (takes effect at the next build; the list in use keeps its width)
        }
        if ((r.over || r.tile_over) && trace)
            fprintf(trace, "[gdyn] overflow: list %d (bits %u, need %u -> W %u; rows %u KiB of a pool of %zu), tile %d (need %u -> cap %u, tiled_ok %d)\n", (int)r.over, r.bits,
                    r.need_w, W, ls.pool_used, ls.pool_kib, (int)r.tile_over, r.need_t, tile_cap, (int)tiled_ok);
        return r.over || r.tile_over;
    }
    // A chunk violated the skin (no overflow): a shorter interval, at K = 1 a wider skin.  False: the skin cannot cover one step.
    bool on_violation()
    {
        if (K == 1) { if (skin > 8) return false; skin *= 1.5; }
        else { K_bad = K; K_bad_ttl = 64; K = std::max(1u, K - std::max(1u, K / 4)); a2_ema = 0; }   // (a gentler cut, K/8 for 32 chunks, violates again sooner: measured 1% slower)
        return true;
    }
    // What the rollbacks of one chunk change of the width and the interval (on_violation), as they stood before the first of them.  A
    // chunk that is accepted in the end keeps what its retries arrived at; a chunk gd_run gives up (the skin cannot cover one step, too
    // many rollbacks) returns them: the handle stands at the last accepted chunk, and so does what its next list build looks like --
    // not a skin beyond 8 cutoffs and an interval of 1 that nothing would ever take back.
    struct Retries { bool held = false; double skin = 0; uint32_t K = 0, K_bad = 0, K_bad_ttl = 0; } retries;
    void hold_for_retries() { if (!retries.held) retries = Retries{true, skin, K, K_bad, K_bad_ttl}; }      // (every rollback: the first one of a chunk holds)
    void retries_over(bool given_up)
    {
        if (given_up && retries.held) {
            skin = std::min(skin, retries.skin);      // (a violation only widens; a width an overflow narrowed for a dense state meanwhile stays)
            K = retries.K; K_bad = retries.K_bad; K_bad_ttl = retries.K_bad_ttl;
        }
        retries.held = false;
    }
    // A chunk was rolled back: the candidate the sweep measures settles again
    void on_rollback(bool droplet)
    {
        if (tuner.enabled && !droplet && !(skin_dense_from > 0) && !(skin_next > 0)) { tuner.settle = std::max(tuner.settle, 1); tuner.acc_ms = 0; tuner.acc_steps = 0; tuner.measured = 0; }
    }
    // A chunk was accepted: tiled-path back-off, interval adaptation, skin selection, repair width.  scale_ahead(k): bead-scale factor of
    // the cutoff over the next k steps.  True when the list in use is to be dropped (the timing sweep moved the skin).
    template <class ScaleAhead>
    bool on_accepted(const ListState &ls, const Accepted &a, ScaleAhead &&scale_ahead)
    {
        const bool with_list = ls.cut > 0;
        if (ls.tiled) { tiled_backoff = 8; tiled_wait = 0; }
        else if (!tiled_ok && tiled_off == 1 && ++tiled_wait >= tiled_backoff) {
            // the tiled path was left for a tile that did not fit: try it again at the largest tile class (an overflow doubles the wait)
            tiled_ok = true; tiled_off = 0; tiled_wait = 0; tiled_backoff = std::min(2 * tiled_backoff, 1024u); tile_cap = 8192u;
        }
        if (adapt && with_list && a.full_interval && !a.on_search_list) {
            const double cut_now = ls.cut * a.scale_now;
            const double lim = 0.5 * (ls.rv - cut_now), d = std::sqrt((double)a.maxd2);
            if (lim > 0 && d > 0) {
                // displacement grows ~ sqrt(steps): aim at 90% of the skin at the end of an interval (the largest of a chunk's intervals,
                // averaged over chunks, is biased upwards already: no rollback in 40 000 steps of the benchmark state at 0.90, the first
                // ones at 0.92).  d^2 / K is averaged over the chunks, weight 0.4 for the newest, so that K does not jitter (12 ... 15).
                const double a2 = d * d / (double)K;
                a2_ema = a2_ema > 0 ? 0.6 * a2_ema + 0.4 * a2 : a2;
                const double knew = std::min(k_target * lim * k_target * lim / a2_ema, 2.0 * K + 1);
                K = (uint32_t)std::max(1.0, std::min(200.0, std::floor(knew)));
            } else if (d == 0) K = std::min(200u, K * 2);
            if (K_bad_ttl > 0) { K_bad_ttl--; if (K >= K_bad) K = std::max(1u, K_bad - 1); }
        }
        const bool drop = with_list && tune_skin(ls, a.ms, a.steps, a.full_interval);
        if (with_list && a.full_interval) class_skin(ls, scale_ahead(K));
        if (repair_wide > 0) repair_wide--;
        return drop;
    }

private:
    // the width of a dense state (memory of the rows or LDS tile): from here back by class_skin
    void narrow_for_dense(double skin_new, bool by_tile)
    {
        if (!(skin_dense_from > 0)) skin_dense_from = skin;
        skin = skin_new; skin_next = 0; a2_ema = 0;
        if (by_tile) dense_by_tile = true;
        if (adapt) K = std::max(1u, std::min(K, 4u));      // (a caller-fixed interval stays the caller's)
    }
    // A build that meets a dense state (the refined start of the pipeline: 1 500 neighbours per bead).  A safety net since tiled rows
    // are ragged: only when the rows exceed a sixteenth of the device memory is the width narrowed so that they fit (lists grow with the
    // cube of the radius; at least a skin of 0.15 x cutoff).  Not with a caller-chosen skin.
    void dense_guard(const ListState &ls, unsigned need_w)
    {
        if (skin_fixed || need_w <= 512u || !(ls.rv > 0) || !(ls.cut > 0) || mem_total == 0) return;
        // what the rows take: tiled lists the pool's use (the sum of what the waves need), generic lists the longest list per row
        const double cut = ls.cut, rows = ls.rows, budget_b = (double)(mem_total / 16);
        const double bytes = ls.tiled ? 1024.0 * (double)ls.pool_used : (double)need_w * 4.0 * rows;
        if (bytes <= budget_b) return;
        const double shrink = 0.9 * budget_b / bytes;                 // lists grow with the cube of the radius
        dense_budget = (uint32_t)std::max(64.0, (double)need_w * budget_b / bytes);
        const double sc = ls.rv / cut - skin;                         // bead-scale part of the radius the build used
        const double r_new = ls.rv * std::cbrt(shrink);
        const double skin_new = std::max(0.15, r_new / cut - sc);
        if (skin_new < skin - 1e-9) {
            narrow_for_dense(skin_new, false);
            if (!ls.tiled) W = std::max(64u, dense_budget & ~7u);      // (the narrowed list is predicted at 0.9 of the budget; a miss is one more exactly sized build)
            if (trace) fprintf(trace, "[gdyn] dense state (longest list %u, rows %.1f GB): skin %.3f\n", need_w, bytes / 1e9, skin_new);
        }
    }
    // One accepted chunk of `steps` steps took `ms` on the device.  Candidates: the width in use, 1.2 x it and 0.7 / 0.5 / 0.35 of it
    // (later rounds: 1.2, 0.85, 0.7), each one chunk to settle and three measured; the width the sweep started from is left only for a
    // gain of 6 % or more (chunk times scatter by a few per cent).  True when the skin moved.
    bool tune_skin(const ListState &ls, double ms, int64_t steps, bool full_interval)
    {
        auto &t = tuner;
        // (not during a dense transient at its narrow width: the selection starts once it has passed)
        if (!t.enabled || ls.droplet || skin_dense_from > 0 || skin_next > 0 || !full_interval || !(a2_ema > 0)) return false;
        if (t.done) {      // conditions drift (a relaxation, a growing bead scale): look again, around the width in use, once the rebuild
                           // interval has moved by a third since the last sweep, or the tiles have outgrown the class the width was selected in
            if (t.wait > 0) t.wait--;
            if (t.cap_ref == 0 && t.wait <= 45 && ls.tiled) t.cap_ref = std::max(ls.tile_cap, 3312u);
            const double k = (double)K, k0 = (double)std::max(t.K_ref, 1u);
            const bool outgrown = ls.tiled && t.cap_ref > 0 && ls.tile_cap > t.cap_ref;
            if (!(outgrown && t.wait <= 40) && (t.wait > 0 || (k < 1.33 * k0 && k0 < 1.33 * k))) return false;
            t.done = false; t.cand.clear();
        }
        if (t.cand.empty()) {
            if (t.wait > 0 && t.rounds == 0) { t.wait--; return false; }
            if (t.rounds == 0) t.cand = {skin, std::min(1.2 * skin, 1.0), 0.7 * skin, 0.5 * skin, 0.35 * skin};
            else t.cand = {skin, std::min(1.2 * skin, 1.0), 0.85 * skin, 0.7 * skin};      // (finer steps around the width in use)
            t.cost.assign(t.cand.size(), 0.0);
            t.idx = 0; t.settle = 0; t.measured = 0; t.acc_ms = 0; t.acc_steps = 0; t.rounds++;
        }
        if (t.settle > 0) { t.settle--; return false; }
        t.acc_ms += ms; t.acc_steps += (uint64_t)steps; t.measured++;
        if (t.measured < 3) return false;
        t.cost[t.idx] = t.acc_ms / (double)t.acc_steps;
        if (trace) fprintf(trace, "[gdyn] skin %.3f: %.4f ms per step (K %u, %s, W %u, tile %u)\n", t.cand[t.idx], t.cost[t.idx], K,
                           ls.tiled ? "tiled" : "generic", ls.W, ls.tile_cap);
        size_t next = t.idx + 1;
        while (next < t.cand.size() && (t.cand[next] == skin || interval_for_skin(ls.cut, t.cand[next]) < 2)) next++;
        if (next >= t.cand.size()) {      // sweep complete: the cheapest, but the width the sweep started from unless the gain is 6 % or more
            size_t best = 0;
            for (size_t k = 1; k < t.cand.size(); k++) if (t.cost[k] > 0 && t.cost[k] < 0.94 * t.cost[0] && t.cost[k] < t.cost[best]) best = k;
            next = best; t.done = true; t.wait = 50; t.K_ref = interval_for_skin(ls.cut, t.cand[best]);
            t.cap_ref = 0;      // (taken a few chunks on, once the selected width has found its class)
        }
        const bool moved = t.cand[next] != skin;
        if (moved) {
            // the tile class for the new width (tiles scale about with the square of the list radius), sized from the last build's
            // largest tile so that the candidate is not measured in a class it does not need
            if (last_need_t > 0 && ls.rv > 0) {
                const double cut = ls.cut, r0 = cut * (1.0 + skin), r1 = cut * (1.0 + t.cand[next]);
                const unsigned est = (unsigned)(1.08 * last_need_t * (r1 / r0) * (r1 / r0)) + 32u;
                tile_cap = std::min(pick_tile_cap(est), 8192u); tile_hold = 0;
            }
            move_skin(t.cand[next], ls.cut);
            if (ls.can_tile) { tiled_ok = true; tiled_off = 0; }      // smaller tiles may fit now
        }
        t.idx = next; t.settle = 1; t.measured = 0; t.acc_ms = 0; t.acc_steps = 0;
        return moved;
    }
    // List width by tile class (S-genome-30k: 2.5 % cheaper at 0.9 than at 0.75 while the largest tile fits the three-block LDS class of
    // 3 312 entries; one class up loses a third of the occupancy).  The handle moves from 0.75 to 0.9 once the largest tile, scaled to
    // the wider list, has fitted the class for three accepted chunks; back when a tile at 0.9 comes within 24 entries of the class,
    // then waits 64 chunks.  A rule on the state, never a clock; not with a caller-chosen skin or auto_skin.  sc: bead-scale factor over
    // the next interval.  A dense state's narrow width (dense_guard, on_report) returns here too.
    void class_skin(const ListState &ls, double sc)
    {
        if (skin_dense_from > 0 && !skin_fixed) {
            const unsigned need_w = last_need_w;
            const double cut = ls.cut, sc0 = ls.rv / cut - skin, ratio = (sc0 + skin_dense_from) / (sc0 + skin);
            // (for the rows: back when the longest list, scaled with the cube of the radius, fits the budget; for the LDS tile: back in
            // steps of at most x 1.35 while the largest tile, scaled with the square of the radius, fits 0.85 of the LDS)
            if (dense_by_tile) {
                if (ls.tiled && last_need_t > 0 && !(skin_next > 0)) {
                    const double target = std::min(skin_dense_from, skin * 1.35 + 0.02);
                    const double rt = (sc0 + target) / (sc0 + skin);
                    if ((double)last_need_t * rt * rt <= 0.85 * 8192.0) {      // (a decondensing globule: a miss costs one rolled-back chunk)
                        skin_next = target;
                        if (target >= skin_dense_from - 1e-9) { skin_dense_from = 0; dense_by_tile = false; }
                        if (trace) fprintf(trace, "[gdyn] dense state eases (largest tile %u): skin %.3f at the next build\n", last_need_t, skin_next);
                    }
                }
                return;
            }
            if (need_w > 0 && (double)need_w * ratio * ratio * ratio <= 0.8 * (double)dense_budget && !(skin_next > 0)) {
                skin_next = skin_dense_from; skin_dense_from = 0;
                { const bool on = tuner.enabled; tuner = SkinTuner{}; tuner.enabled = on; }      // (a fresh selection from the default width)
                if (trace) fprintf(trace, "[gdyn] dense state has passed (longest list %u): skin %.3f at the next build\n", need_w, skin_next);
            }
            return;
        }
        if (skin_fixed || !adapt || tuner.enabled || !ls.tiled || !last_need_t || ls.droplet || skin_next > 0) return;
        const double lo = 0.75, hi = 0.9;
        auto move_to = [&](double s) {      // takes effect at the next build (take_pending_skin): the list in use stays valid until then
            skin_next = s; skin_streak = 0;
            if (trace) fprintf(trace, "[gdyn] list width by tile class: skin %.2f at the next build (largest tile %u)\n", s, last_need_t);
        };
        if (skin < hi - 1e-9) {
            if (skin_hold > 0) { skin_hold--; return; }
            const double ratio = (sc + hi) / (sc + skin);
            // a tile = the block's own slots under three (dz) planes + the halo rows around them: only the halo grows with the cell
            // cross-section (measured on S-genome-30k: 2 930 entries at 0.75, 3 074 at 0.9)
            const double own = 3.0 * GD_BLOCK, est = own + std::max(0.0, (double)last_need_t - own) * ratio * ratio + 24.0;
            if (est <= 3312.0 - 24.0 && ls.tile_cap <= 3312u) { if (++skin_streak >= 3) move_to(hi); }
            else skin_streak = 0;
        } else if (skin <= hi + 1e-9 && (ls.tile_cap > 3312u || last_need_t + 24u > 3312u)) { move_to(lo); skin_hold = 64; }
    }
};

}  // namespace gd
