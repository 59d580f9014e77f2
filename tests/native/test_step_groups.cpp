// CPU unit test of the replica-group rule of the step launches (csrc/gdyn_policy.hpp: gd::step_group_split): the table of its
// decisions -- sizes and multiples of 8, each excluding condition, the size threshold, the three modes.  Built and run by
// tests/test_step_groups.py (plain g++, no HIP runtime).
#include <cstdio>

#include "gdyn_policy.hpp"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using gd::step_group_split;
enum { RULE = gd::STEP_GROUPS_RULE, ONE = gd::STEP_GROUPS_ONE, TWO = gd::STEP_GROUPS_TWO };

// a state in which nothing excludes two groups: tiled lists, nothing behind k_step, device noise, whole replicas per XCD, the
// specialised pair kernel
static gd::StepGroupState state(uint32_t R, uint32_t nblk)
{
    gd::StepGroupState st;
    st.R = R; st.nblk = nblk; st.tiled = true; st.post_step = false; st.device_noise = true; st.whole_replica_map = true; st.fast_pair = true;
    return st;
}

static void test_sizes()
{
    // mode 2 ignores the threshold: the sizes alone.  Both groups are multiples of 8 and not empty
    const uint32_t expect[][2] = {{1, 0}, {6, 0}, {8, 0}, {12, 0}, {15, 0}, {16, 8}, {17, 0}, {20, 0}, {24, 16}, {32, 16}, {40, 24},
                                  {64, 32}, {100, 0}, {128, 64}, {136, 72}, {256, 128}, {1000, 504}, {1024, 512}};
    for (auto &e : expect) {
        const uint32_t ra = step_group_split(TWO, state(e[0], 3));
        CHECK(ra == e[1]);
        if (ra) CHECK(ra % 8 == 0 && (e[0] - ra) % 8 == 0 && ra >= 8 && e[0] - ra >= 8 && ra >= e[0] - ra);
    }
    // every multiple of 8 from 16 on splits, into two multiples of 8 that differ by at most 8
    for (uint32_t R = 16; R <= 4096; R += 8) {
        const uint32_t ra = step_group_split(TWO, state(R, 1));
        CHECK(ra != 0 && ra % 8 == 0 && ra - (R - ra) <= 8);
    }
    // an unequal split (sixteenths of the replicas in group A), rounded to the nearest multiple of 8 and kept inside [8, R - 8]
    CHECK(step_group_split(TWO, state(128, 59), 0, 9) == 72);
    CHECK(step_group_split(TWO, state(128, 59), 0, 7) == 56);
    CHECK(step_group_split(TWO, state(16, 59), 0, 15) == 8);
    CHECK(step_group_split(TWO, state(16, 59), 0, 1) == 8);
    CHECK(step_group_split(TWO, state(64, 59), 0, 0) == 8);       // (clamped to one sixteenth, then to a group of 8)
    CHECK(step_group_split(TWO, state(64, 59), 0, 99) == 56);
    CHECK(step_group_split(TWO, state(128, 0)) == 0);             // no blocks: nothing to launch
    CHECK(step_group_split(TWO, state(0xfffffff8u, 1)) == 0x80000000u);      // (no 32-bit overflow in the share)
}

static void test_excluding_conditions()
{
    const gd::StepGroupState ok = state(128, 59);
    for (uint32_t mode : {(uint32_t)RULE, (uint32_t)TWO}) {
        CHECK(step_group_split(mode, ok) == 64);
        gd::StepGroupState st = ok; st.tiled = false;          CHECK(step_group_split(mode, st) == 0);      // generic lists
        st = ok; st.post_step = true;                          CHECK(step_group_split(mode, st) == 0);      // droplet term, per-replica pairs
        st = ok; st.device_noise = false;                      CHECK(step_group_split(mode, st) == 0);      // injected noise
        st = ok; st.whole_replica_map = false;                 CHECK(step_group_split(mode, st) == 0);      // slab map (cpb != 0)
        st = ok; st.fast_pair = false;                         CHECK(step_group_split(mode, st) == 0);      // runtime-power pair kernel
        st = ok; st.R = 6;                                     CHECK(step_group_split(mode, st) == 0);
        st = ok; st.R = 127;                                   CHECK(step_group_split(mode, st) == 0);
    }
}

static void test_threshold()
{
    const uint32_t M = gd::STEP_GROUPS_MIN_BLOCKS;
    CHECK(M > 0);
    // the smaller group's blocks against the threshold, exactly at it and one below
    CHECK(step_group_split(RULE, state(16, 10), 80) == 8);
    CHECK(step_group_split(RULE, state(16, 10), 81) == 0);
    CHECK(step_group_split(RULE, state(24, 10), 80) == 16);       // groups of 16 and 8: the smaller one counts
    CHECK(step_group_split(RULE, state(24, 10), 81) == 0);
    CHECK(step_group_split(RULE, state(128, 59), 64u * 59u) == 64);
    CHECK(step_group_split(RULE, state(128, 59), 64u * 59u + 1u) == 0);
    CHECK(step_group_split(RULE, state(128, 59), 56u * 59u, 9) == 72);
    CHECK(step_group_split(RULE, state(128, 59), 56u * 59u + 1u, 9) == 0);
    // the default: half a round of the device (256 CUs x 3 resident blocks = 768) per group, so that a launch that splits is more
    // than one round.  The headline (S-genome-30k x 128: 59 blocks per replica) and S-genome-30k x 16 run in two groups; S-genome-30k
    // x 1 and x 8, one-round grids (16 x 30 blocks, 16 x 47) and the suite's small models do not
    CHECK(M == 384u && 2u * M == 768u);
    CHECK(step_group_split(RULE, state(128, 59)) == 64);
    CHECK(step_group_split(RULE, state(16, 59)) == 8);
    CHECK(step_group_split(RULE, state(1, 59)) == 0);
    CHECK(step_group_split(RULE, state(8, 59)) == 0);
    CHECK(step_group_split(RULE, state(16, 48)) == 8);
    CHECK(step_group_split(RULE, state(16, 47)) == 0);
    CHECK(step_group_split(RULE, state(16, 30)) == 0);
    CHECK(step_group_split(RULE, state(16, 4)) == 0);
    CHECK(step_group_split(RULE, state(16, 3)) == 0);
    // mode 2 ignores the threshold and nothing else
    CHECK(step_group_split(TWO, state(16, 4)) == 8);
    CHECK(step_group_split(TWO, state(16, 4), 0xffffffffu) == 8);
}

static void test_modes()
{
    CHECK(step_group_split(ONE, state(128, 59)) == 0);
    CHECK(step_group_split(ONE, state(128, 59), 0) == 0);
    CHECK(step_group_split(RULE, state(128, 59)) == 64);
    CHECK(step_group_split(TWO, state(128, 59)) == 64);
    CHECK(step_group_split(3, state(128, 59)) == 0);              // (not a mode: gd_set_step_groups refuses it; one launch)
    CHECK(step_group_split(0xffffffffu, state(128, 59)) == 0);
    CHECK(RULE == 0 && ONE == 1 && TWO == 2);                     // the values of include/gdyn_groups.h
}

int main()
{
    test_sizes();
    test_excluding_conditions();
    test_threshold();
    test_modes();
    if (failures) { fprintf(stderr, "step groups: %d failure(s)\n", failures); return 1; }
    printf("step groups: ok\n");
    return 0;
}
