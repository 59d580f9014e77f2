/* gdyn_prep.h -- C-ABI of the prepared contexts of a stepper's grouped step launches (gd_system, gdyn.h; gdyn_groups.h).
 *
 * What it is.  Every step applies the callback the step before left pending (step, time, scales, wall semiaxes from the summed wall
 *             reaction) and derives a handful of float constants from the replica's context.  In a span of steps that runs in two
 *             replica groups (gdyn_groups.h) the library may do that once per replica and step, in a small kernel in front of the
 *             group's step kernel on the group's own stream, instead of once in every block of the step kernel.
 * Results.    Do not depend on it: the same functions in the same order on the same values.  Trajectories, contexts, rollbacks and
 *             launch counts are bit for bit those of a handle that steps in one launch.
 * When.       Only in spans that run in two groups: under gd_set_step_groups mode 2 in every such span, under mode 0 where the smaller
 *             group is large enough for the other group's step kernel to cover the extra launch, under mode 1 never.
 * gd_timing.step_launches counts steps, whatever the library does.
 * Errors.     GD_EINVAL: NULL handle.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_PREP_H
#define GDYN_PREP_H

#include <stdint.h>

#include "gdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_PREP_ABI_VERSION 1

int gd_prep_abi_version(void);
/* launches: preparation launches of the last gd_run (one per group and step of the spans that ran on prepared contexts; rolled-back
 * chunks included; 0: every step of it computed its context in the step kernel).  May be NULL */
int gd_get_ctx_prepared(gd_system *sys, uint64_t *launches);

#ifdef __cplusplus
}
#endif

#endif
