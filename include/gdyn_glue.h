/* gdyn_glue.h -- C-ABI of the glue kinetics on the device: the stochastic binding and unbinding of bead pairs ("glues") of every
 * replica of a stepper (gd_system, gdyn.h) in one call, from the positions and the pair search the device already holds.  The
 * bound pairs of a replica act through a per-replica pair slot of gdyn_replica.h.
 *
 * The rule.  Replica r holds a set B_r of pairs (i, j), i < j, unique, in ascending (i, j) order,
 *             |B_r| <= max_glues.  gd_glue_update(dt, epoch, seeds) computes, on the host in double,
 *                 p_off = -expm1(-unbinding_rate dt),  p_on = -expm1(-binding_rate dt),  thr = min(2^32, floor(p 2^32)),
 *             and draws for a pair (i, j) the four words w of philox4x32_10 with
 *                 counter (i, j, epoch & 0xffffffff, epoch >> 32),  key (seed_r & 0xffffffff, (seed_r >> 32) ^ 0x474C5545):
 *             w[0] < thr_off: the pair releases; w[1] < thr_on: the pair fires; sel = w[2] << 32 | w[3].  Then, per replica,
 *             1. a pair of B_r is removed if its minimum-image distance exceeds reach (fp32, from the positions the pair search
 *                reads, with the search's own test) or if it releases; the survivors are B';
 *             2. the candidates are all pairs i < j within reach that are not in B' (a pair released in 1 is a candidate again);
 *                those that fire are F;
 *             3. free = max_glues - |B'|; all of F binds if |F| <= free, else the `free` pairs of F with the smallest sel, ties
 *                by (i, j) ascending: a uniform sample without replacement;
 *             4. B_r becomes B' plus the newly bound pairs, sorted.
 *             The draws are counter-based: the result does not depend on the order in which the search emits pairs, and the
 *             same (positions, sets, dt, epoch, seeds) give the same sets on every run.
 * Slot.       gd_glue_define manages ONE per-replica slot of the handle, declared before with gd_replica_pairs_define (which
 *             gives the pairs' potential).  After every update, gd_glue_set and gd_glue_define the replicas' sets are installed
 *             in that slot as gd_replica_pairs_set would install them; gd_replica_pairs_set itself is refused on the managed
 *             slot (GD_ESTATE).  A handle that never calls gd_glue_define behaves exactly as without this header.
 * Traffic.    An update searches all replicas in one launch and leaves candidates and positions on the device; what crosses to
 *             the host is the new sets (at most max_glues pairs a replica), in one copy.
 * Errors.     GD_EINVAL: NULL argument, replica >= R, non-finite or negative rates, reach <= 0, dt <= 0 or non-finite,
 *             max_glues below a current set size, and for gd_glue_set: a bead id >= N, i == j, a pair listed twice, n > max_glues.
 *             GD_ESTATE: gd_glue_define on a slot that was never defined or while another slot is managed; any other function
 *             before gd_glue_define.  A failed call leaves the sets as they were.
 * The sets are outside the rollback snapshot of gd_run, like the lists they feed.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_GLUE_H
#define GDYN_GLUE_H

#include <stdint.h>

#include "gdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_GLUE_ABI_VERSION 1

typedef struct gd_glue_params {
    uint32_t max_glues;       /* capacity of a replica's set */
    double reach;             /* binding and holding distance */
    double binding_rate;      /* per unit time, of a candidate */
    double unbinding_rate;    /* per unit time, of a bound pair */
} gd_glue_params;

int gd_glue_abi_version(void);
/* manages per-replica slot `slot` (declared with gd_replica_pairs_define) with these parameters; every replica's set starts empty.
 * Calling it again (same slot) replaces the parameters and keeps the sets. */
int gd_glue_define(gd_system *sys, uint32_t slot, const gd_glue_params *p);
/* one update of every replica over the time dt; seeds: one per replica */
int gd_glue_update(gd_system *sys, double dt, uint64_t epoch, const uint64_t *seeds /* (R) */);
/* replaces one replica's set (a restart, a test): n pairs in any order and orientation */
int gd_glue_set(gd_system *sys, uint32_t replica, const uint32_t *pairs, uint32_t n);
/* the set of one replica, (i, j) ascending; count-then-fetch: *n is the set's size, at most cap pairs are written */
int gd_glue_fetch(gd_system *sys, uint32_t replica, uint32_t *pairs, uint32_t cap, uint32_t *n);
/* the sizes of all replicas' sets */
int gd_glue_counts(gd_system *sys, uint32_t *n /* (R) */);

#ifdef __cplusplus
}
#endif

#endif
