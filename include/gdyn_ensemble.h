/* gdyn_ensemble.h -- C-ABI of the per-replica A/B tables of a stepper (gd_system, gdyn.h): every replica of a handle carries its own
 * per-bead (a, b) factors, where gd_set_bead_params gives all replicas the same.  A genome model and its randomised controls, or
 * several annotations of one genome -- the same beads, chains and bonds, other A/B factors -- run as the replicas of one handle.
 *
 * What a table enters.  The mixed pair potential, the wall's a / b factors, every bond set with `mix` (static, shared dynamic and
 *             per-replica dynamic pairs): all of them read replica r's own factors.  Mobilities, bending energies, the pair and bond
 *             parameters, the temperature and the topology stay per handle.
 * Unset.      A replica that was never set refers to the shared table of gd_set_bead_params.  A handle that never calls
 *             gd_ensemble_set_ab behaves exactly as without this header.
 * Homogeneous handles.  A handle on which every replica's table equals every other's is homogeneous, however that came about (never
 *             set, all set to one table, set and set back).  It takes the path of a handle that never made the call -- one table of N
 *             entries, bond records mixed per bond on the host -- and its results are bit for bit that handle's.
 * gd_set_bead_params with a non-NULL a (or b) replaces that column for EVERY replica: its meaning, "shared by all replicas", stays.
 * When.       A set may come at any time between evaluations.  It invalidates the factors the device positions carry and the resident
 *             neighbour list, and marks the topology dirty: the next evaluation decides again whether the bond records are mixed on
 *             the host.  Positions, contexts, contact tables, per-replica pair lists and a recorder's frames are untouched.  The
 *             tables are outside the rollback snapshot of gd_run: they cannot change inside a run.
 * Heterogeneous handles keep the bond records as given and mix them in the kernels from the two beads' factors (what a handle does
 *             today whose mixed records outnumber the parameter table), and hold R x N (a, b) pairs on the device, 8 R N bytes.
 * fp16.       The factors of every replica ride in the positions' fourth component only if EVERY value of EVERY replica is exact in
 *             fp16 (0, 0.5, 1, 5 ... are).  Otherwise the whole handle carries them in an array of their own and runs the generic
 *             lists (gd_context.list_path 1), as a shared table with such a value does.
 * Errors.     GD_EINVAL: NULL handle, replica >= R, a and b both NULL, a non-finite value.  A failed call leaves the tables as they
 *             were.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_ENSEMBLE_H
#define GDYN_ENSEMBLE_H

#include <stdint.h>

#include "gdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_ENSEMBLE_ABI_VERSION 1

int gd_ensemble_abi_version(void);
/* replaces the table of one replica.  a, b: N doubles each; either may be NULL (that column of the replica is kept) */
int gd_ensemble_set_ab(gd_system *sys, uint32_t replica, const double *a, const double *b);
/* what the next evaluation uses for that replica (the shared table if it was never set); either pointer may be NULL */
int gd_ensemble_get_ab(gd_system *sys, uint32_t replica, double *a, double *b);
/* class_of: R entries; replicas with identical tables share a class, classes numbered by first appearance.  Either pointer may be NULL */
int gd_ensemble_classes(gd_system *sys, uint32_t *class_of, uint32_t *n_classes);

#ifdef __cplusplus
}
#endif

#endif
