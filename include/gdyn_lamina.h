/* gdyn_lamina.h -- C-ABI of the lamina analysis of libgdyn (device-side restatement of the reference's
 * 5-sim-genome/src/analyze_lamina: geometry.py, Ellipsoid.distance_from_surface, and the contact rule of command.py,
 * analyze_contact_uniform).
 *
 * A gd_lamina handle is bound to one device:
 *   gd_lamina_distances  per (frame, bead), the second-order distance of the bead from the ellipsoid wall of its frame;
 *   gd_lamina_contacts   distance < contact_distance as bytes, added into an (F, N) float32 sum the handle keeps on the device;
 *   gd_lamina_average    that sum divided by the number of gd_lamina_contacts calls since the last reset;
 *   gd_lamina_reset      forgets the sum and its shape.
 *
 * The rules.  The distance, in fp64 on the (widened) coordinates x and the semiaxes s of the frame,
 * every operation rounded on its own (no contraction) and every three-term sum evaluated as (t0 + t1) + t2:
 *   inv = pow(s, -2)      s1 = inv * x     s2 = inv * s1     s3 = inv * s2        (per axis)
 *   a = s3 . x            b = s2 . x       c = s1 . x - 1
 *   u = (b - sqrt(b * b - a * c)) / (a + 1e-6)             v = sqrt(s1 . s1)
 *   distance = |u * v|
 * A bead at the centre gets 0; b * b - a * c < 0 (far outside the wall) gives NaN, as in the reference.
 * The contact: (double)distance < contact_distance (strict; NaN is never a contact).
 * The average: float32 sum / float32 number of calls.
 * Nothing is accumulated in an order that could vary: results are bit-identical from run to run and for every
 * max_frames_per_launch.
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not
 * part of gdyn.h's ABI. */
#ifndef GDYN_LAMINA_H
#define GDYN_LAMINA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_LAMINA_ABI_VERSION 1

typedef struct gd_lamina gd_lamina;

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t max_frames_per_launch;  /* frames uploaded, computed and downloaded at a time; 0: automatic */
} gd_lamina_desc;

int gd_lamina_abi_version(void);
int gd_lamina_create(const gd_lamina_desc *desc, gd_lamina **out);
int gd_lamina_destroy(gd_lamina *h);
/* xyz: frames * n_points * 3 values, float when is_f64 == 0, double otherwise; semiaxes: frames * 3 doubles, positive and
 * finite; out: frames * n_points doubles when out_is_f64 != 0, else floats (the fp64 result rounded once).
 * frames == 0 or n_points == 0: nothing is written. */
int gd_lamina_distances(gd_lamina *h, const void *xyz, int is_f64, uint32_t frames, uint32_t n_points, const double *semiaxes, void *out,
                        int out_is_f64);
/* distances: frames * n_points floats; contacts_out: as many bytes (0 / 1).  The first call after a reset fixes
 * (frames, n_points); a later call with another shape is GD_EINVAL.  contact_distance must not be NaN. */
int gd_lamina_contacts(gd_lamina *h, const float *distances, uint32_t frames, uint32_t n_points, double contact_distance,
                       uint8_t *contacts_out);
/* out: frames * n_points floats of the shape the contacts calls fixed; GD_ESTATE before the first of them */
int gd_lamina_average(gd_lamina *h, float *out);
int gd_lamina_reset(gd_lamina *h);

#ifdef __cplusplus
}
#endif

#endif
