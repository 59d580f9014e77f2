/* gdyn_flow.h -- C-ABI of the flow analyses of libgdyn (device-side restatement of the reference's
 * 5-sim-genome/src/analyze_particle_flow and analyze_grid_flow).
 *
 * A gd_flow handle holds one trajectory history of F frames of N beads on one device:
 *   gd_flow_set_history   uploads the positions (float32 or float64, (F,N,3) row-major);
 *   gd_flow_velocities    optional Gaussian smoothing along time (utils.gaussian_smooth) and the windowed least-squares
 *                         velocity of every bead in every frame (estimate_velocity), both in fp64;
 *   gd_flow_particle      the mean velocity of the beads within r of each bead (compute_flow), (F,N,3) float32;
 *   gd_flow_grid          the same mean around given points and the number of beads within r, (F,G,3) float32 and (F,G) int32.
 * Pairs are "within r" when (dx*dx + dy*dy) + dz*dz <= r*r in fp64, coincident beads included (cKDTree's rule).
 * Results are deterministic: bit-identical from run to run and for every max_frames_per_launch.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not
 * part of gdyn.h's ABI. */
#ifndef GDYN_FLOW_H
#define GDYN_FLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_FLOW_ABI_VERSION 1

typedef struct gd_flow gd_flow;

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t max_frames_per_launch;  /* frames binned and gathered per launch; 0: automatic */
} gd_flow_desc;

int gd_flow_abi_version(void);
int gd_flow_create(const gd_flow_desc *desc, gd_flow **out);
int gd_flow_destroy(gd_flow *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise; forgets earlier velocities */
int gd_flow_set_history(gd_flow *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* smoothing: Gaussian window W (0 or 1: none); delay >= 0.  positions_out: the (smoothed) history, F*N*3 doubles;
 * velocities_out: F*N*3 doubles (NaN where the reference's window has one frame).  Either may be NULL. */
int gd_flow_velocities(gd_flow *h, uint32_t smoothing, uint32_t delay, double *positions_out, double *velocities_out);
/* after gd_flow_velocities: flows_out F*N*3 floats */
int gd_flow_particle(gd_flow *h, double radius, float *flows_out);
/* after gd_flow_velocities: points G*3 doubles; flows_out F*G*3 floats, coverage_out F*G int32 (either may be NULL) */
int gd_flow_grid(gd_flow *h, double radius, const double *points, uint32_t n_points, float *flows_out, int32_t *coverage_out);

#ifdef __cplusplus
}
#endif

#endif
