/* gdyn_groups.h -- C-ABI of the replica groups of a stepper's step launches (gd_system, gdyn.h).
 *
 * What it is.  The replicas of a handle are independent trajectories.  Between two list builds gd_run may launch every step as TWO
 *             kernels -- replicas [0, A) on the handle's stream, replicas [A, R) on a second stream of the handle -- so that the blocks
 *             of one group fill the compute units the other leaves idle while its last blocks drain.  Builds, the per-chunk readback,
 *             rollbacks and everything a caller does on gd_get_stream's stream run on the one stream as before: the second stream is
 *             forked off it in front of a span of steps and joined to it behind.
 * Results.    Do not depend on the mode: every word a stepping launch reads or writes is addressed by the replica or by a bead of it,
 *             and both groups follow the one plan (list, rebuild interval, chunk) of the handle.  Trajectories, contexts, rollback and
 *             launch counts of mode 2 are bit for bit those of mode 1.
 * Modes.      0  the library's rule (the default): two groups where the list in use is tiled, no kernel runs behind the step kernel
 *                (droplet term, per-replica pairs), the noise is drawn on the device, R is a multiple of 8 and at least 16 (both groups
 *                then are multiples of 8 and keep the block placement they would have alone), and the smaller group has enough blocks
 *                for the overlap to pay;
 *             1  always one launch per step;
 *             2  two groups wherever the results allow it: the rule without its size threshold.
 * gd_timing.step_launches counts steps, whatever the mode.
 * Errors.     GD_EINVAL: NULL handle, mode > 2.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_GROUPS_H
#define GDYN_GROUPS_H

#include <stdint.h>

#include "gdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_GROUPS_ABI_VERSION 1

int gd_groups_abi_version(void);
int gd_set_step_groups(gd_system *sys, uint32_t mode);
/* mode: what was set; last_groups: 1 or 2, the groups the step launches of the last gd_run ran in (2: some span of it ran in two).
 * Either pointer may be NULL */
int gd_get_step_groups(gd_system *sys, uint32_t *mode, uint32_t *last_groups);

#ifdef __cplusplus
}
#endif

#endif
