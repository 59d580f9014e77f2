// CPU unit test of the prepared-context rule of the grouped step launches (csrc/gdyn_policy.hpp: gd::ctx_prepared): the table of its
// decisions -- only in spans that run in two groups, the three group modes, the size threshold, the developer override.  Built and
// run by tests/test_ctx_prep.py (plain g++, no HIP runtime).
#include <cstdio>

#include "gdyn_policy.hpp"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using gd::ctx_prepared;
using gd::step_group_split;
enum { RULE = gd::STEP_GROUPS_RULE, ONE = gd::STEP_GROUPS_ONE, TWO = gd::STEP_GROUPS_TWO };
enum { NEVER = gd::CTX_PREP_NEVER, BY_RULE = gd::CTX_PREP_RULE, ALWAYS = gd::CTX_PREP_ALWAYS };

static gd::StepGroupState state(uint32_t R, uint32_t nblk)
{
    gd::StepGroupState st;
    st.R = R; st.nblk = nblk; st.tiled = true; st.post_step = false; st.device_noise = true; st.whole_replica_map = true; st.fast_pair = true;
    return st;
}
// the decision of a span as enqueue_chunk takes it: the split first, then the rule on its result
static bool span(uint32_t mode, const gd::StepGroupState &st, uint32_t prep = BY_RULE, uint32_t min_blocks = gd::CTX_PREP_MIN_BLOCKS)
{
    return ctx_prepared(mode, step_group_split(mode, st), st, prep, min_blocks);
}

static void test_only_in_grouped_spans()
{
    // one launch per step: never, whatever the mode and the override
    for (uint32_t mode : {(uint32_t)RULE, (uint32_t)ONE, (uint32_t)TWO, 3u})
        for (uint32_t prep : {(uint32_t)NEVER, (uint32_t)BY_RULE, (uint32_t)ALWAYS}) {
            CHECK(!ctx_prepared(mode, 0, state(128, 59), prep, 0));
            CHECK(!ctx_prepared(mode, 128, state(128, 59), prep, 0));      // (not a split: group B would be empty)
        }
    // every state step_group_split keeps on one launch stays on today's kernel
    const gd::StepGroupState ok = state(128, 59);
    for (uint32_t mode : {(uint32_t)RULE, (uint32_t)TWO})
        for (uint32_t prep : {(uint32_t)BY_RULE, (uint32_t)ALWAYS}) {
            CHECK(span(mode, ok, prep));
            gd::StepGroupState st = ok; st.tiled = false;          CHECK(!span(mode, st, prep));
            st = ok; st.post_step = true;                          CHECK(!span(mode, st, prep));
            st = ok; st.device_noise = false;                      CHECK(!span(mode, st, prep));
            st = ok; st.whole_replica_map = false;                 CHECK(!span(mode, st, prep));
            st = ok; st.fast_pair = false;                         CHECK(!span(mode, st, prep));
            st = ok; st.R = 6;                                     CHECK(!span(mode, st, prep));
            st = ok; st.R = 1;                                     CHECK(!span(mode, st, prep));
        }
}

static void test_modes()
{
    // mode 1 never; mode 2 in every grouped span, the suite's 1 500 x 16 included; mode 0 by size
    CHECK(!span(ONE, state(128, 59)));
    CHECK(!ctx_prepared(ONE, 64, state(128, 59)));                 // (even handed a split)
    CHECK(span(TWO, state(128, 59)));
    CHECK(span(TWO, state(16, 3)));
    CHECK(span(TWO, state(16, 3), BY_RULE, 0xffffffffu));          // mode 2 ignores the threshold
    CHECK(span(RULE, state(128, 59)));
    CHECK(!span(RULE, state(16, 3)));
    CHECK(!ctx_prepared(3, 64, state(128, 59)));                   // (not a mode)
}

static void test_threshold()
{
    // the smaller group's blocks against the threshold, exactly at it and one below (handed a split: the threshold alone)
    CHECK(ctx_prepared(RULE, 8, state(16, 10), BY_RULE, 80));
    CHECK(!ctx_prepared(RULE, 8, state(16, 10), BY_RULE, 81));
    CHECK(ctx_prepared(RULE, 16, state(24, 10), BY_RULE, 80));     // groups of 16 and 8: the smaller one counts
    CHECK(!ctx_prepared(RULE, 16, state(24, 10), BY_RULE, 81));
    CHECK(ctx_prepared(RULE, 72, state(128, 59), BY_RULE, 56u * 59u));
    CHECK(!ctx_prepared(RULE, 72, state(128, 59), BY_RULE, 56u * 59u + 1u));
    CHECK(ctx_prepared(RULE, 0x80000000u, state(0xfffffff8u, 0x10u), BY_RULE, 0xffffffffu));      // (64-bit product)
    // the default is not below the size at which mode 0 splits at all; the headline (30 000 beads x 128) runs prepared
    CHECK(gd::CTX_PREP_MIN_BLOCKS >= gd::STEP_GROUPS_MIN_BLOCKS);
    CHECK(span(RULE, state(128, 59)));
    CHECK(gd::CTX_PREP_MIN_BLOCKS == 1888u);                       // 30 000 beads x 64 replicas: the smallest size measured to win
    CHECK(span(RULE, state(64, 59)));
    CHECK(!span(RULE, state(56, 59)));                             // (groups of 32 + 24: the smaller one counts)
    CHECK(!span(RULE, state(32, 59)));                             // 944 blocks a group: two groups, contexts in the kernel
    CHECK(step_group_split(RULE, state(32, 59)) == 16);
    CHECK(!span(RULE, state(16, 59)));
    CHECK(!span(RULE, state(16, 30)));                             // (a one-round grid: one launch)
    CHECK(!span(RULE, state(1, 59)));
}

static void test_override()
{
    // the developer library's override: never / the rule / every grouped span
    CHECK(!span(TWO, state(128, 59), NEVER));
    CHECK(!span(RULE, state(128, 59), NEVER));
    CHECK(ctx_prepared(RULE, 8, state(16, 3), ALWAYS, 0xffffffffu));
    CHECK(!ctx_prepared(RULE, 8, state(16, 3), BY_RULE));
    CHECK(NEVER == 0 && BY_RULE == 1 && ALWAYS == 2);
}

int main()
{
    test_only_in_grouped_spans();
    test_modes();
    test_threshold();
    test_override();
    if (failures) { fprintf(stderr, "ctx prep: %d failure(s)\n", failures); return 1; }
    printf("ctx prep: ok\n");
    return 0;
}
