// gdyn_replica_pairs.hpp -- host side of the per-replica dynamic pair lists (include/gdyn_replica.h): what the caller set, and the
// table the device walks.  Plain C++: no HIP runtime, no handle, no environment (tests/native/test_replica_pairs.cpp drives it alone).
//
// One replica's pairs of all four slots become a compressed sparse row table over that replica's ACTIVE beads, the beads that appear
// in any pair of any slot:
//   row_bead[M]     the active bead ids, ascending
//   row_off[M + 1]  row offsets into ent, relative to the replica's first entry
//   ent[E]          one directed entry per pair end, E = 2 x pairs: partner id | slot << 30.  A row is ordered by (slot, position of the
//                   pair in the caller's list), so a bead's forces are summed in one fixed order whatever the other rows hold.
// The replicas are concatenated into ONE block of 32-bit words, so that one copy and one launch serve all R:
//   [R x 4]   per replica: M_r, first row (into row_bead), first offset (into row_off), first entry (into ent)
//   [32]      the four slots' parameter records, left to the caller (the device's record type is not known here)
//   [sum M_r] row_bead     [sum (M_r + 1)] row_off     [sum E_r] ent
#ifndef GDYN_REPLICA_PAIRS_HPP
#define GDYN_REPLICA_PAIRS_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gd {

constexpr uint32_t RP_SLOTS = 4;
constexpr uint32_t RP_SLOT_SHIFT = 30;                          // entry = partner | slot << 30 (bead ids stay below 2^26)
constexpr uint32_t RP_PARTNER_MASK = (1u << RP_SLOT_SHIFT) - 1u;
constexpr uint32_t RP_RECORD_WORDS = 32;                        // 4 records of 8 words

struct ReplicaTable {
    std::vector<uint32_t> row_bead, row_off, ent;
};

// The table of one replica.  pairs[s]: the slot's list as the caller gave it, (i, j) flat, i != j.
inline void flatten_replica(const std::vector<uint32_t> (&pairs)[RP_SLOTS], ReplicaTable &out)
{
    struct End { uint32_t bead, seq, ent; };
    size_t E = 0;
    for (auto &p : pairs) E += p.size();
    std::vector<End> ends;
    ends.reserve(E);
    uint32_t seq = 0;
    for (uint32_t s = 0; s < RP_SLOTS; s++)
        for (size_t k = 0; k + 1 < pairs[s].size(); k += 2, seq++) {
            const uint32_t i = pairs[s][k], j = pairs[s][k + 1];
            ends.push_back({i, seq, j | (s << RP_SLOT_SHIFT)});
            ends.push_back({j, seq, i | (s << RP_SLOT_SHIFT)});
        }
    std::sort(ends.begin(), ends.end(), [](const End &a, const End &b) { return a.bead != b.bead ? a.bead < b.bead : a.seq < b.seq; });
    out.row_bead.clear(); out.row_off.clear(); out.ent.clear();
    out.ent.reserve(ends.size());
    for (size_t k = 0; k < ends.size(); k++) {
        if (k == 0 || ends[k].bead != ends[k - 1].bead) { out.row_bead.push_back(ends[k].bead); out.row_off.push_back((uint32_t)k); }
        out.ent.push_back(ends[k].ent);
    }
    out.row_off.push_back((uint32_t)ends.size());
}

// Where the parts of the concatenated block start, in words
struct ReplicaLayout {
    size_t base = 0, rec = 0, row_bead = 0, row_off = 0, ent = 0, words = 0;
    uint32_t max_rows = 0;      // largest M_r: the launch's grid
};

// What the caller set for a handle of R replicas over N beads, and which replicas' tables are out of date
class ReplicaPairs {
public:
    void reset(uint32_t n_beads, uint32_t n_replicas)
    {
        N = n_beads; R = n_replicas;
        reps.assign(R, Rep{});
        for (auto &d : defined_) d = false;
        total = 0; dirty_ = false;
    }
    bool defined(uint32_t slot) const { return slot < RP_SLOTS && defined_[slot]; }
    // (a slot's parameters changed: the records travel with the block)
    void define(uint32_t slot) { defined_[slot] = true; dirty_ = true; }
    // 0, or the index (from 1) of the first bad pair: an id >= N, or i == j.  A bad list changes nothing.
    size_t set(uint32_t slot, uint32_t r, const uint32_t *pairs, uint32_t n)
    {
        for (uint32_t k = 0; k < n; k++)
            if (pairs[2 * k] >= N || pairs[2 * k + 1] >= N || pairs[2 * k] == pairs[2 * k + 1]) return (size_t)k + 1;
        Rep &rep = reps[r];
        total -= rep.pairs[slot].size() / 2;
        rep.pairs[slot].assign(pairs, pairs + 2 * (size_t)n);
        total += n;
        rep.dirty = true; dirty_ = true;
        return 0;
    }
    uint32_t count(uint32_t slot, uint32_t r) const { return (uint32_t)(reps[r].pairs[slot].size() / 2); }
    bool any() const { return total != 0; }             // some replica has a pair
    bool dirty() const { return dirty_; }
    // Flattens the replicas whose lists changed and lays the block out
    ReplicaLayout flatten()
    {
        ReplicaLayout l;
        size_t m = 0, e = 0;
        for (auto &rep : reps) {
            if (rep.dirty) { flatten_replica(rep.pairs, rep.tab); rep.dirty = false; }
            m += rep.tab.row_bead.size(); e += rep.tab.ent.size();
            l.max_rows = std::max(l.max_rows, (uint32_t)rep.tab.row_bead.size());
        }
        l.base = 0; l.rec = 4 * (size_t)R; l.row_bead = l.rec + RP_RECORD_WORDS; l.row_off = l.row_bead + m;
        l.ent = l.row_off + m + R; l.words = l.ent + e;
        return l;
    }
    // Writes the block of the layout flatten() returned (l.words words at dst; the records' words are left as they are)
    void pack(const ReplicaLayout &l, uint32_t *dst)
    {
        uint32_t row = 0, off = 0, ent = 0;
        for (uint32_t r = 0; r < R; r++) {
            const ReplicaTable &t = reps[r].tab;
            const uint32_t M = (uint32_t)t.row_bead.size();
            uint32_t *b = dst + l.base + 4 * (size_t)r;
            b[0] = M; b[1] = row; b[2] = off; b[3] = ent;
            std::copy(t.row_bead.begin(), t.row_bead.end(), dst + l.row_bead + row);
            if (t.row_off.empty()) dst[l.row_off + off] = 0;      // (never flattened: no rows)
            else std::copy(t.row_off.begin(), t.row_off.end(), dst + l.row_off + off);
            std::copy(t.ent.begin(), t.ent.end(), dst + l.ent + ent);
            row += M; off += M + 1; ent += (uint32_t)t.ent.size();
        }
        dirty_ = false;
    }

private:
    struct Rep {
        std::vector<uint32_t> pairs[RP_SLOTS];
        ReplicaTable tab;
        bool dirty = false;
    };
    uint32_t N = 0, R = 0;
    std::vector<Rep> reps;
    bool defined_[RP_SLOTS] = {false, false, false, false};
    size_t total = 0;
    bool dirty_ = false;
};

// Capacity for `need` elements of a buffer that holds `have`: grown geometrically, never shrunk
inline size_t grown_capacity(size_t have, size_t need) { return need <= have ? have : std::max(need, have + have / 2 + 64); }

}      // namespace gd

#endif
