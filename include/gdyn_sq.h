/* gdyn_sq.h -- C-ABI of the structure factors and scattering functions of libgdyn: the Fourier amplitudes of the bead density of
 * every label at chosen wave vectors, frame by frame, and from them the partial structure factors S_ab(q), the collective
 * intermediate scattering function F_ab(q, tau) and its self part F_s(q, tau), over the frames of a history.  It is what X-ray,
 * light-scattering and Fourier-imaging experiments report, and the standard measure of A/B phase separation (the low-q peak of
 * S_ab gives the domain size 2 pi / q*).  Nothing in the reference works in reciprocal space: this is a capability beyond it.
 * The work is a direct sum, beads x vectors x frames fp64 sine and cosine evaluations (csrc/gdyn_sq.hip).
 *
 * History.  A gd_sq handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the
 * precision it was given.  A history with a non-finite coordinate is refused (GD_EINVAL) and leaves the handle without one.
 *
 * Labels.  label[i] in [-1, K), K <= GD_SQ_MAX_LABELS; -1: the bead takes no part.  With no labels set there is one label of all
 * beads.  Labels belong to a history: they are set after it (GD_ESTATE before), kept by a new history of the same N and dropped by
 * one of another N (the rules of gd_dcorr_set_labels).  n_a is the number of beads of label a.
 *
 * Vectors.  Q vectors q[k] = (qx, qy, qz), finite doubles, the zero vector allowed, 1 <= Q <= GD_SQ_MAX_VECTORS.  They do not
 * depend on N and survive a new history.  GD_SQ_MAX_VECTORS = 2^20: a plane of one frame or one lag, K * K * Q values at most,
 * then has at most 2^26 elements and is indexed in 32 bits, every offset of a whole output is a 64-bit product of such an index
 * and a frame or lag, and the tiles of 64 vectors (2^14 at most) fit one grid dimension.
 *
 * Term.  fp64 on the widened coordinates (x, y, z), every operation rounded on its own (no contraction, no fast-math):
 *     phi = ((qx * x) + (qy * y)) + qz * z;      the term is (cos phi, sin phi), the device library's fp64 functions.
 *   Sign, stated once: rho_a(q, f) = sum over beads i of label a of exp(-i q . x_i(f)) = C - i S, with C = sum cos phi and
 *   S = sum sin phi.  The outputs are C and S.
 *
 * Summation order.  The beads of a label are taken in ascending bead index and cut, from the label's first bead, into chunks of
 * GD_SQ_CHUNK_BEADS.  A chunk's partial sum is ONE serial sum in ascending order, and the chunk partials are then added serially in
 * ascending order; both sums start from +0.0.  No floating-point atomic is used.  What follows:
 *   1. results are bit-identical from run to run, for every max_frames_per_pass, and between a host-fed and a live-fed float32
 *      history;
 *   2. a result does not depend on which other vectors, frames or lags a call lists: a subset of vectors gives the same columns,
 *      a window the same frames;
 *   3. the zero vector gives C = n_a and S = 0 exactly, an empty label +0.0;
 *   4. |C - exact|, |S - exact| <= n (T + GD_SQ_CHUNK_BEADS - 1 + ceil(n / GD_SQ_CHUNK_BEADS)) 2^-53 for a label of n beads, where
 *      exact is the sum of the true cos and sin of the rounded phi and T the ulp bound of the device library's fp64 sin and cos
 *      (tests/sq_restatement.py).
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_SQ_H
#define GDYN_SQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_SQ_ABI_VERSION 1
#define GD_SQ_MAX_LABELS 8
#define GD_SQ_MAX_VECTORS 1048576   /* 2^20: see above */
#define GD_SQ_CHUNK_BEADS 256       /* beads of one serial partial sum */

typedef struct gd_sq gd_sq;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                /* HIP device ordinal */
    uint32_t max_frames_per_pass;   /* frames (or origins) whose chunk partial sums are held at once; 0: automatic; no result depends on it */
} gd_sq_desc;

int gd_sq_abi_version(void);
int gd_sq_create(const gd_sq_desc *desc, gd_sq **out);
int gd_sq_destroy(gd_sq *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_sq_set_history(gd_sq *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_sq_set_history_live(gd_sq *h, gd_live_history *history, uint32_t replica);
/* label: N values in [-1, n_labels), 1 <= n_labels <= GD_SQ_MAX_LABELS; NULL with n_labels <= 1: one label of all beads.
 * GD_ESTATE without a history */
int gd_sq_set_labels(gd_sq *h, const int32_t *label, uint32_t n_labels);
/* q: (n_vectors, 3) finite doubles, 1 <= n_vectors <= GD_SQ_MAX_VECTORS */
int gd_sq_set_vectors(gd_sq *h, const double *q, uint32_t n_vectors);

/* The calls below work on the window of frames [first_frame, first_frame + n_frames).  GD_ESTATE: no history, or no vectors set.
 * GD_EINVAL: n_frames == 0 or a window past F, a lag >= n_frames, origin_stride == 0, a NULL output.  GD_ENOMEM: the outputs or
 * the partial sums of one frame do not fit on the device. */

/* cos_sum, sin_sum: (n_frames, K, Q) doubles, C and S of every frame of the window */
int gd_sq_amplitudes(gd_sq *h, uint32_t first_frame, uint32_t n_frames, double *cos_sum, double *sin_sum);
/* rho_a(t + tau) conj rho_b(t) summed over the origins t = first_frame + k * origin_stride, ascending, with t + tau inside the
 * window, for every lag tau and every ordered pair of labels (a, b):
 *     re = (C_a(t+tau) * C_b(t)) + (S_a(t+tau) * S_b(t));      im = (C_a(t+tau) * S_b(t)) - (S_a(t+tau) * C_b(t));
 * every operation rounded on its own, the terms added serially over ascending origins from +0.0.  The amplitudes are bit for bit
 * those of gd_sq_amplitudes over the same frames.  sum_re, sum_im: (n_lags, K, K, Q) doubles; count: (n_lags) uint64, the number
 * of origins, (n_frames - 1 - tau) / origin_stride + 1.  Lag 0 gives the static partial structure factors:
 * S_ab(q) = sum_re / (count * n), n the beads of the normalisation chosen; lags may repeat. */
int gd_sq_collective(gd_sq *h, uint32_t first_frame, uint32_t n_frames, const uint32_t *lags, uint32_t n_lags, uint32_t origin_stride,
                     double *sum_re, double *sum_im, uint64_t *count);
/* For every lag and origin (as above) the amplitudes of the displacement field d = double(X[t+tau, i]) - double(X[t, i]) per axis,
 * rounded once; unwrapped, no minimum image, as gdyn_msd.h takes displacements.  Term and order are those of the header with d in
 * place of x; the per-origin results are then added serially over ascending origins from +0.0.  cos_sum, sin_sum: (n_lags, K, Q)
 * doubles; count: (n_lags, K) uint64, origins * n_a.  F_s(q, tau) = cos_sum / count. */
int gd_sq_self(gd_sq *h, uint32_t first_frame, uint32_t n_frames, const uint32_t *lags, uint32_t n_lags, uint32_t origin_stride,
               double *cos_sum, double *sin_sum, uint64_t *count);

#ifdef __cplusplus
}
#endif

#endif
