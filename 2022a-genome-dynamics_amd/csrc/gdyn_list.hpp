// gdyn_list.hpp -- the resident list of a handle: what the host knows about the neighbour list in use, and every event that changes it.
//
// One struct, one named transition per event (the table in DESIGN.md, "Resident list"), the questions the stepper asks of it as const
// queries.  Plain C++ (no HIP runtime, handle or environment): the handle's host files (gdyn_capi*.hip) call the transitions and never assign a member;
// tests/native/test_resident_list.cpp drives it alone.  Buffers, the position / order cursors and the counters of the handle
// (rebuilds, the per-replica entry counts) stay with the handle and are passed in where a query needs them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/gdyn.h"
#include "gdyn_policy.hpp"

namespace gd {

struct ResidentList {
    // the list in use
    bool valid = false;                 // it lists the current positions at the current model, cutoff, scales and tuning
    bool tiled = false;                 // path of the last build (stays when the list is dropped)
    uint32_t W = 0, tile_cap = 0;       // generic row width / tile capacity it was built with (the policy's may change for the next build)
    float rv = 0, rn = 0;               // list radius, near-class radius
    uint32_t steps_since_build = 0;
    bool search_list = false;           // built by a pair search at a radius beyond the force list's
    uint64_t verified_serial = 0;       // == the handle's state serial: the last run ended on an accepted chunk whose list covers the positions
                                        // and the cutoff an observation now sees (no bead beyond the skin margin): energies need no build
    // what a build leaves for the next one
    bool w_packed = false;              // pos.w of the current positions holds the packed (a,b) factors
    int bbox_cur = 0;                   // half of the box record the next build reads (it accumulates the other one)
    bool bbox_valid = false;            // open boxes: that half holds the bounding box of the positions the last build sorted
    bool need_valid = false;            // the row history describes the state about to be listed well enough to predict row widths from it
    float need_rv = 0; bool need_all_near = false;      // list radius / class mode the history was counted at
    bool order_valid = false;           // the thread-order key (len_prev) was left by a tiled build of this trajectory that no rollback or
                                        // retry has refused since: the next tiled build may order k_step's threads by it (else by slot)
    uint32_t pool_used = 0;             // KiB of the row pool the last build took (its cursor's final value: the need, when the pool was full)
    uint32_t repairs = 0;               // k_step waves the last build read back had to repair (diagnostics)

    // ---- transitions: one per event
    // the model, the cutoff, a scale or the tuning changed; a timing sweep moved the skin; a pair search met a bead beyond the margin
    void drop() { valid = false; }
    // positions from the caller: pos.w is plain, the box, what the beads needed before and the order key say nothing about them
    void positions_set() { valid = false; w_packed = false; bbox_valid = false; need_valid = false; order_valid = false; }
    // new topology: pos.w is repacked by the next build; the beads are where they were (box and history stay)
    void topology_changed() { valid = false; w_packed = false; }
    // a chunk was rolled back to its snapshot: pos.w is what it was before the chunk; the box the abandoned builds recorded may be that
    // of positions stepped on incomplete lists; the history and the pool's use stay (an overflow has counted the need into it).  The
    // order key does not: a build whose repairs were refused stored list lengths clamped to the rows of whichever waves the repair
    // queue or the pool happened to turn away, and the builds behind it listed positions stepped on those lists
    void rolled_back(bool w_packed_before) { valid = false; bbox_valid = false; w_packed = w_packed_before; order_valid = false; }
    // a build outside gd_run was refused and is run again on the same positions (build_now): its order key is as above
    void build_refused() { order_valid = false; }

    struct Build {
        float rv = 0, rn = 0;
        bool with_list = false, tiled = false;      // with_list false: the counting sort alone (no pair term)
        uint32_t W = 0, tile_cap = 0;               // the policy's, at the build
        bool packed_ab = false, all_near = false;
        bool predicted = false; uint32_t pool_guess = 0;      // tiled: rows predicted from the history / the pool's use expected without one
    };
    // a build is about to be launched (not yet in use: enter_use)
    void build_enqueued(const Build &b)
    {
        if (b.with_list) W = b.W;
        if (b.tiled) {
            if (!b.predicted) pool_used = b.pool_guess;      // (the guess stands in until a chunk's readback brings the real use)
            need_valid = true; need_rv = b.rv; need_all_near = b.all_near;
            order_valid = true;      // (this build writes the key of the next one; rolled_back / build_refused take it back)
        }
        bbox_cur ^= 1; bbox_valid = b.tiled;      // (the box of the positions this build sorted, reduced by k_tiles: the next build's grid)
        tiled = b.tiled; tile_cap = b.tile_cap;
        w_packed = b.packed_ab;
        rv = b.rv; rn = b.rn; steps_since_build = 0;
    }
    // the build's list enters use (by_search: at a radius beyond the force list's)
    void enter_use(bool by_search) { valid = true; search_list = by_search; }
    void stepped(uint32_t n) { steps_since_build += n; }
    // a chunk was read back; used: the pool's cursor, its largest value over the chunk's builds, the repaired waves
    void chunk_read(const unsigned used[3])
    {
        if (tiled && used[0] > 0) { pool_used = std::max(used[0], used[1]); repairs = used[2]; }
    }
    // A run ended on an accepted chunk.  settled: it stepped with lists, without the droplet term, and the scales did not move behind
    // its last step.  The positions that step WROTE are covered by the running bound of the tiled path only (dmax2, read back with the
    // chunk): the list serves an observation at the cutoff cut_obs if that bound is inside the margin too.
    void run_ended(bool settled, double cut_obs, float dmax2, uint64_t state_serial)
    {
        const double lim = 0.5 * ((double)rv - cut_obs);
        if (settled && valid && tiled && lim > 0 && (double)dmax2 <= lim * lim) verified_serial = state_serial;
    }

    // ---- queries
    // rows of a tiled build at radius rv_new are predicted from the history: same class mode, radius within 2 %
    bool predicts(float rv_new, bool all_near) const
    {
        return need_valid && need_all_near == all_near && need_rv > 0 && std::fabs(rv_new / need_rv - 1.f) <= 0.02f;
    }
    // a tiled build orders k_step's threads by the key in memory (false: the key is cleared first -- threads in slot order, as in a
    // handle's first build: what a handle computes from given positions and context does not depend on what it ran before)
    bool orders_by_history() const { return order_valid; }
    // an observation (energy, forces) needs no build: nothing has stepped on the list, or the last run verified it
    bool fresh(uint64_t state_serial) const { return valid && (steps_since_build == 0 || verified_serial == state_serial); }
    // a pair search at dcut is served from the list (W == 0: the handle has built without a list so far)
    bool serves_search(double dcut) const { return valid && (float)dcut <= rv && W != 0; }
    // the list in use and the handle, as the list policy sees them
    ListState state(double cut, size_t pool_kib, double rows, bool droplet, bool can_tile) const
    {
        return {cut, rv, tiled, tile_cap, W, pool_used, pool_kib, rows, droplet, can_tile};
    }
    // The list fields of gd_context.  rows: R x Np.  row_repairs and near_entries follow the path of the last build, not validity;
    // list_path is 0 only before the first build.
    void fill_context(gd_context *o, uint64_t rebuilds, uint64_t near_entries, uint32_t largest_tile, uint64_t rows) const
    {
        o->list_radius = rv;
        o->list_path = !valid && rebuilds == 0 ? 0u : (tiled ? 2u : 1u);
        o->tile_capacity = (valid && tiled) ? tile_cap : 0u;
        o->largest_tile = (valid && tiled) ? largest_tile : 0u;
        o->row_repairs = tiled ? repairs : 0u;
        o->near_entries = tiled ? near_entries : 0ull;
        o->list_bytes = !valid ? 0ull : tiled ? 1024ull * pool_used : (uint64_t)W * rows * 4ull;
    }
};

}  // namespace gd
