/* gdyn_replica.h -- C-ABI of the per-replica dynamic pair lists of a stepper (gd_system, gdyn.h): every replica of a handle gets
 * its own lists of bonded pairs that change during a run (the loops and glues of one trajectory of an ensemble), where
 * gd_set_dynamic_pairs gives all replicas the same.
 *
 * Slots.      Four per-replica slots, separate from the four shared slots of gd_set_dynamic_pairs.  Both kinds contribute to
 *             GD_TERM_DYNAMIC in gd_run, gd_compute_forces and gd_compute_energy.  A handle that never calls the functions below
 *             behaves exactly as without them.
 * Parameters. gd_bond_params means what it means for gd_set_dynamic_pairs: all four kinds, mix (the a / b factors of the two
 *             beads), scale_by_bond_scale (with the replica's own bond_scale) and minimum_image.  The argument rules are the same:
 *             a softcore set with mix or scale_by_bond_scale is GD_EINVAL, as are unsupported powers.  A pair listed twice acts
 *             twice, as on the shared path.
 * Errors.     GD_EINVAL: NULL argument, slot >= 4, replica >= R, a bead id >= N, i == j.  GD_ESTATE: gd_replica_pairs_set or
 *             gd_replica_pairs_count on a slot that was never defined.  A failed call leaves the previous lists in force.
 * No topology work.  A set does not mark the topology dirty, does not invalidate the resident neighbour list and does not touch
 *             the bond adjacency.  The lists are outside the rollback snapshot of gd_run: a chunk that is rolled back and re-run
 *             uses the same lists.  gd_set_positions, gd_begin_phase and gd_set_context leave them alone; gd_destroy frees them.
 * One upload for many sets.  gd_replica_pairs_set stores the pairs on the host and marks the replica; the next gd_run /
 *             gd_compute_forces / gd_compute_energy flattens the marked replicas and uploads all lists with one asynchronous copy
 *             on the handle's stream from a pinned buffer the handle owns.  The buffers grow geometrically and never shrink: no
 *             allocation and no blocking copy in the steady state.
 *
 * The term is evaluated by a kernel of its own behind the stepping kernel: one thread per bead that has a
 * pair, no floating-point atomics on positions or forces, so results are reproducible.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_REPLICA_H
#define GDYN_REPLICA_H

#include <stdint.h>

#include "gdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_REPLICA_ABI_VERSION 1

int gd_replica_abi_version(void);
/* declares per-replica slot `slot` (0..3) with these parameters; every replica's list of the slot starts empty.
 * Calling it again replaces the parameters and keeps the lists. */
int gd_replica_pairs_define(gd_system *sys, uint32_t slot, const gd_bond_params *p);
/* replaces the list of one replica of one defined slot: n pairs (i, j), i != j, both < N.  n == 0 empties it. */
int gd_replica_pairs_set(gd_system *sys, uint32_t slot, uint32_t replica, const uint32_t *pairs, uint32_t n);
/* pairs currently set (what the next evaluation uses) */
int gd_replica_pairs_count(gd_system *sys, uint32_t slot, uint32_t replica, uint32_t *n);

#ifdef __cplusplus
}
#endif

#endif
