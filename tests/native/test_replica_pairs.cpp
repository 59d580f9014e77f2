// The flattener of the per-replica dynamic pair lists (csrc/gdyn_replica_pairs.hpp) alone: one replica's table, then the block of all
// replicas, each checked against what the caller's lists say, pair by pair.  Driven by tests/test_replica_pairs.py (plain, and under
// AddressSanitizer + UBSan).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "gdyn_replica_pairs.hpp"

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using Lists = std::vector<uint32_t>[gd::RP_SLOTS];

// what a bead's row must hold: per bead, (partner | slot << 30) in (slot, position) order
static std::map<uint32_t, std::vector<uint32_t>> expected_rows(const std::vector<uint32_t> (&pairs)[gd::RP_SLOTS])
{
    std::map<uint32_t, std::vector<uint32_t>> rows;
    for (uint32_t s = 0; s < gd::RP_SLOTS; s++)
        for (size_t k = 0; k + 1 < pairs[s].size(); k += 2) {
            rows[pairs[s][k]].push_back(pairs[s][k + 1] | (s << 30));
            rows[pairs[s][k + 1]].push_back(pairs[s][k] | (s << 30));
        }
    return rows;
}

static void check_table(const std::vector<uint32_t> (&pairs)[gd::RP_SLOTS], const uint32_t *row_bead, const uint32_t *row_off, const uint32_t *ent,
                        uint32_t M)
{
    const auto rows = expected_rows(pairs);
    size_t E = 0;
    for (auto &p : pairs) E += p.size();
    CHECK(M == rows.size());
    if (M != rows.size()) return;
    CHECK(row_off[0] == 0 && row_off[M] == E);
    uint32_t t = 0;
    for (auto &kv : rows) {      // (std::map: ascending bead ids)
        CHECK(row_bead[t] == kv.first);
        CHECK(row_off[t + 1] - row_off[t] == kv.second.size());
        for (size_t k = 0; k < kv.second.size() && row_off[t] + k < E; k++) CHECK(ent[row_off[t] + k] == kv.second[k]);
        t++;
    }
}

static void check_replica(const std::vector<uint32_t> (&pairs)[gd::RP_SLOTS])
{
    gd::ReplicaTable tab;
    gd::flatten_replica(pairs, tab);
    CHECK(tab.row_off.size() == tab.row_bead.size() + 1);
    check_table(pairs, tab.row_bead.data(), tab.row_off.data(), tab.ent.data(), (uint32_t)tab.row_bead.size());
}

static void set_all(gd::ReplicaPairs &rp, uint32_t r, const std::vector<uint32_t> (&pairs)[gd::RP_SLOTS])
{
    for (uint32_t s = 0; s < gd::RP_SLOTS; s++) CHECK(rp.set(s, r, pairs[s].data(), (uint32_t)(pairs[s].size() / 2)) == 0);
}

static void check_block(gd::ReplicaPairs &rp, uint32_t R, const Lists *lists)
{
    const gd::ReplicaLayout l = rp.flatten();
    std::vector<uint32_t> blk(l.words, 0xdeadbeefu);      // exactly l.words: a write beyond it is the sanitizer's to find
    rp.pack(l, blk.data());
    CHECK(!rp.dirty());
    CHECK(l.rec == 4 * (size_t)R && l.row_bead == l.rec + gd::RP_RECORD_WORDS);
    for (size_t k = 0; k < gd::RP_RECORD_WORDS; k++) CHECK(blk[l.rec + k] == 0xdeadbeefu);      // the records are the caller's
    uint32_t row = 0, off = 0, ent = 0, max_rows = 0;
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t *b = blk.data() + l.base + 4 * (size_t)r;
        CHECK(b[1] == row && b[2] == off && b[3] == ent);
        CHECK(l.row_bead + b[1] + b[0] <= l.row_off && l.row_off + b[2] + b[0] + 1 <= l.ent);
        check_table(lists[r], blk.data() + l.row_bead + b[1], blk.data() + l.row_off + b[2], blk.data() + l.ent + b[3], b[0]);
        size_t E = 0;
        for (auto &p : lists[r]) E += p.size();
        CHECK(l.ent + b[3] + E <= l.words);
        row += b[0]; off += b[0] + 1; ent += (uint32_t)E;
        max_rows = std::max(max_rows, b[0]);
    }
    CHECK(l.words == l.ent + ent && l.max_rows == max_rows);
}

int main()
{
    const uint32_t N = 1000;
    {   // empty lists
        Lists e;
        check_replica(e);
        gd::ReplicaTable tab;
        gd::flatten_replica(e, tab);
        CHECK(tab.row_bead.empty() && tab.ent.empty() && tab.row_off.size() == 1 && tab.row_off[0] == 0);
    }
    Lists a;      // all four slots; a bead of degree 1 (bead 7) and one of degree 40 (bead 500); duplicates; ids 0 and N - 1
    a[0] = {7, 500, 0, N - 1, N - 1, 0, 3, 4, 3, 4};      // (0, N-1) and its mirror; (3, 4) twice
    for (uint32_t k = 0; k < 30; k++) { a[1].push_back(500); a[1].push_back(501 + 2 * k); }
    for (uint32_t k = 0; k < 9; k++) { a[2].push_back(400 + k); a[2].push_back(500); }
    a[3] = {4, 3, 999, 998};
    check_replica(a);
    {   // degrees and the entry order of the hub, spelled out
        gd::ReplicaTable tab;
        gd::flatten_replica(a, tab);
        size_t t7 = 0, t500 = 0;
        for (size_t t = 0; t < tab.row_bead.size(); t++) { if (tab.row_bead[t] == 7) t7 = t; if (tab.row_bead[t] == 500) t500 = t; }
        CHECK(tab.row_off[t7 + 1] - tab.row_off[t7] == 1);
        CHECK(tab.row_off[t500 + 1] - tab.row_off[t500] == 40);
        const uint32_t *row = tab.ent.data() + tab.row_off[t500];
        CHECK(row[0] == (7u | 0u << 30));                                    // slot 0 first
        for (uint32_t k = 0; k < 30; k++) CHECK(row[1 + k] == ((501 + 2 * k) | 1u << 30));      // then slot 1 in list order
        for (uint32_t k = 0; k < 9; k++) CHECK(row[31 + k] == ((400 + k) | 2u << 30));
        CHECK(tab.row_bead.front() == 0 && tab.row_bead.back() == N - 1);
        for (size_t t = 1; t < tab.row_bead.size(); t++) CHECK(tab.row_bead[t - 1] < tab.row_bead[t]);
        // bead 3: (3,4) twice in slot 0, then (4,3) of slot 3
        size_t t3 = 0;
        for (size_t t = 0; t < tab.row_bead.size(); t++) if (tab.row_bead[t] == 3) t3 = t;
        const uint32_t *r3 = tab.ent.data() + tab.row_off[t3];
        CHECK(tab.row_off[t3 + 1] - tab.row_off[t3] == 3 && r3[0] == 4u && r3[1] == 4u && r3[2] == (4u | 3u << 30));
    }
    {   // the order of a row follows the caller's list: the same pairs reversed give the reversed row
        Lists f, b;
        f[1] = {10, 20, 10, 30, 10, 40};
        b[1] = {10, 40, 10, 30, 10, 20};
        gd::ReplicaTable tf, tb;
        gd::flatten_replica(f, tf); gd::flatten_replica(b, tb);
        CHECK(tf.row_bead == tb.row_bead && tf.row_off == tb.row_off);
        CHECK(tf.ent[0] == (20u | 1u << 30) && tf.ent[2] == (40u | 1u << 30) && tb.ent[0] == (40u | 1u << 30) && tb.ent[2] == (20u | 1u << 30));
    }
    {   // three replicas, the middle one without pairs; then updates, an emptied replica and a rejected list
        gd::ReplicaPairs rp;
        rp.reset(N, 3);
        CHECK(!rp.any() && !rp.dirty() && !rp.defined(0) && !rp.defined(7));
        for (uint32_t s = 0; s < gd::RP_SLOTS; s++) rp.define(s);
        CHECK(rp.defined(3) && rp.dirty() && !rp.any());
        Lists lists[3];
        check_block(rp, 3, lists);      // defined, all empty
        for (uint32_t s = 0; s < gd::RP_SLOTS; s++) lists[0][s] = a[s];
        lists[2][1] = {0, 1, 1, 2, N - 2, N - 1};
        set_all(rp, 0, lists[0]); set_all(rp, 2, lists[2]);
        CHECK(rp.any() && rp.dirty() && rp.count(1, 0) == 30 && rp.count(1, 1) == 0 && rp.count(1, 2) == 3);
        check_block(rp, 3, lists);
        lists[1][3] = {5, 6};      // the middle replica gains a pair: the bases behind it move
        set_all(rp, 1, lists[1]);
        check_block(rp, 3, lists);
        const uint32_t bad_id[] = {1, 2, 3, N}, bad_self[] = {8, 8};
        CHECK(rp.set(1, 2, bad_id, 2) == 2 && rp.set(1, 2, bad_self, 1) == 1);
        CHECK(rp.count(1, 2) == 3 && !rp.dirty());      // a rejected list changes nothing
        check_block(rp, 3, lists);
        for (auto &p : lists[0]) p.clear();
        set_all(rp, 0, lists[0]);
        CHECK(rp.count(0, 0) == 0 && rp.any());
        check_block(rp, 3, lists);
        for (auto &p : lists[1]) p.clear();
        for (auto &p : lists[2]) p.clear();
        set_all(rp, 1, lists[1]); set_all(rp, 2, lists[2]);
        CHECK(!rp.any());
        check_block(rp, 3, lists);
    }
    // buffers grow geometrically and never shrink
    CHECK(gd::grown_capacity(0, 10) >= 10 && gd::grown_capacity(100, 50) == 100 && gd::grown_capacity(100, 101) >= 150 &&
          gd::grown_capacity(100, 1000) == 1000);
    if (failures) { std::printf("replica pairs: %d failure(s)\n", failures); return 1; }
    std::printf("replica pairs: ok\n");
    return 0;
}
