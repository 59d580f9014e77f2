/* gdyn_gyr.h -- C-ABI of the gyration analyses of libgdyn: per frame, the centre and the gyration tensor of every segment of a
 * history (a chromosome territory: its radius, semi-axes, asphericity and orientation, and how they relax), and the compaction profile
 * along the chain, Rg^2 of a sliding window of w beads (what chromatin tracing reports).  Nothing in the reference computes either:
 * this is a capability beyond it (csrc/gdyn_gyr.hip).
 *
 * History.  A gd_gyr handle holds one history X[f, i, :] of F frames of N beads on one device, float32 or float64, in the precision
 * it was given.  A history with a non-finite coordinate is refused (GD_EINVAL) and leaves the handle without one.  Nothing is unwrapped
 * or reduced: periodic systems store unwrapped coordinates, as for gdyn_dcorr.h.
 *
 * Segments and chains.  Ranges [start, end) of beads, ascending and not overlapping, end <= N.  Segments (of the tensors) are
 * non-empty; beads in no segment take no part; with none set there is one segment [0, N).  Chains (of the profile) may be empty; with
 * none set there is one chain [0, N).  Both belong to a history: they are set after it (GD_ESTATE before), kept by a new history of
 * the same N and dropped by one of another N.
 *
 * Frames.  Every call selects the frames f_k = first + k stride, k < count; count == 0 takes all with f_k < F.  An explicit frame
 * with f_k >= F, stride 0 or a selection of no frame is GD_EINVAL.  K is the number of selected frames.
 *
 * Tensors (gd_gyr_tensors).  For every selected frame k and every segment s of n beads, all in fp64, every operation rounded on its
 * own (no contraction, no fast-math):
 *   centre_sum[k, s, a] = sum over the beads i of s of double(X[f_k, i, a])                               a = x, y, z
 *   centre[k, s, a]     = centre_sum[k, s, a] / double(n)
 *   moment[k, s, c]     = sum over the beads of d_a * d_b, d = double(X[f_k, i, :]) - centre[k, s, :]     c = xx, yy, zz, xy, xz, yz
 *   Order of both sums: the segment is cut into pieces of GD_GYR_PIECE_BEADS beads from its start; a piece is summed serially over
 *   its beads ascending, from +0; the pieces are added serially ascending, from +0.  The outputs are sums: the gyration tensor is
 *   moment / n and Rg^2 its trace, the caller's divisions.
 *
 * Compaction profile (gd_gyr_profile, gd_gyr_profile_frames).  A window is the beads [i, i + w), 2 <= w <= GD_GYR_MAX_WINDOW, indexed
 * by its first bead i; it is valid when it lies inside one chain.  For a frame f and a valid window, in fp64, every operation rounded on
 * its own:
 *   c[a]       = (serial sum of double(X[f, j, a]) over j = i .. i + w - 1 ascending, from +0) / double(w)
 *   v(f, i, w) = (serial sum over j ascending, from +0, of ((dx * dx + dy * dy) + dz * dz)) / double(w),  d = double(X[f, j, :]) - c
 *   gd_gyr_profile_frames returns v(f_k, i, w) as (K, N) doubles, +0 where the window is not valid.
 *   gd_gyr_profile, for up to GD_GYR_MAX_WINDOWS window sizes:  sum[m, i] = sum over k of v(f_k, i, w_m),  sum_sq[m, i] = sum of v * v.
 *   Order: the selected frames are cut into ranges of GD_GYR_FRAME_RANGE counted from k = 0; a range is summed serially over k
 *   ascending, from +0; the ranges are added serially ascending, from +0, by a second kernel.  Entries of windows that are not valid
 *   are +0.  count_out[m, i] = K where the window is valid and 0 elsewhere, a closed form computed on the host.
 *
 * No floating-point atomic is used.  What follows:
 *   1. the tensor outputs, sum, sum_sq and the per-frame values equal the numpy restatement of these orders byte for byte, for
 *      float32 and float64 histories (tests/gyr_restatement.py);
 *   2. results are bit-identical from run to run, for every beads_per_tile and frames_per_launch, whatever other windows or segments
 *      the call lists, and between a host-fed and a live-fed float32 history;
 *   3. adding the rows of gd_gyr_profile_frames in the range order above reproduces sum and sum_sq byte for byte;
 *   4. a frame selection knows only itself: selecting (first, stride, count) equals selecting all frames of the history cut to
 *      those frames by the caller;
 *   5. integer-valued coordinates with |x| < 2^10 and segments of 2^k <= 512 beads make every centre, every centred coordinate and
 *      every sum (< 512 * 2^22 = 2^31) exactly representable: centre_sum, centre and moment are then exact.  (With |x| < 2^20 the
 *      sums outgrow 53 bits.)
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error(); a failed call leaves the handle as it was, except that a history
 * with a non-finite coordinate leaves the handle without one.  This header has its own version: the symbols below are not part
 * of gdyn.h's ABI. */
#ifndef GDYN_GYR_H
#define GDYN_GYR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_GYR_ABI_VERSION 1
#define GD_GYR_PIECE_BEADS 32        /* beads of one piece of a segment */
#define GD_GYR_FRAME_RANGE 64        /* selected frames of one partial sum of the profile */
#define GD_GYR_MAX_WINDOWS 8         /* window sizes of one gd_gyr_profile */
#define GD_GYR_MAX_WINDOW 2048       /* beads of the longest window: a tile and its windows are staged in 64 KiB of LDS */

typedef struct gd_gyr gd_gyr;
typedef struct gd_live_history gd_live_history;      /* include/gdyn_live.h */

typedef struct {
    int32_t  device;                /* HIP device ordinal */
    uint32_t beads_per_tile;        /* window starts of one block of the profile, 1 to 512; 0: automatic (256); no result depends on it */
    uint32_t frames_per_launch;     /* selected frames of one kernel launch (the profile: whole ranges of GD_GYR_FRAME_RANGE, at least one);
                                       0: automatic; no result depends on it */
} gd_gyr_desc;

int gd_gyr_abi_version(void);
int gd_gyr_create(const gd_gyr_desc *desc, gd_gyr **out);
int gd_gyr_destroy(gd_gyr *h);
/* xyz: F*N*3 values, float when is_f64 == 0, double otherwise.  GD_EINVAL: non-finite coordinate, handle left without a history */
int gd_gyr_set_history(gd_gyr *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64);
/* the frames a recorder holds of one replica, float32 as recorded, without leaving the device (same device; GD_ESTATE without frames) */
int gd_gyr_set_history_live(gd_gyr *h, gd_live_history *history, uint32_t replica);
/* ranges: (S, 2) [start, end) pairs, ascending, non-empty, not overlapping, end <= N; NULL with n_segments == 0: one segment [0, N).
 * GD_ESTATE without a history */
int gd_gyr_set_segments(gd_gyr *h, const uint32_t *ranges, uint32_t n_segments);
/* ranges: (C, 2) [start, end) pairs, ascending, not overlapping, empty allowed, end <= N; NULL with n_chains == 0: one chain [0, N).
 * GD_ESTATE without a history */
int gd_gyr_set_chains(gd_gyr *h, const uint32_t *ranges, uint32_t n_chains);
/* centre_sum, centre: (K, S, 3) doubles; moment: (K, S, 6) doubles, xx yy zz xy xz yz.  Each of the three may be NULL.
 * GD_ESTATE without a history; GD_EINVAL: the frame selection (see Frames); GD_ENOMEM: the outputs do not fit on the device */
int gd_gyr_tensors(gd_gyr *h, uint32_t first, uint32_t stride, uint32_t count, double *centre_sum, double *centre, double *moment);
/* windows: n_windows sizes, 1 <= n_windows <= GD_GYR_MAX_WINDOWS, each 2 <= w <= GD_GYR_MAX_WINDOW (else GD_EINVAL).
 * sum, sum_sq (double), count_out (uint64): (n_windows, N).  Each of the three may be NULL.  GD_ESTATE without a history; GD_EINVAL:
 * the windows or the frame selection; GD_ENOMEM */
int gd_gyr_profile(gd_gyr *h, const uint32_t *windows, uint32_t n_windows, uint32_t first, uint32_t stride, uint32_t count, double *sum, double *sum_sq,
                   uint64_t *count_out);
/* out: (K, N) doubles, v(f_k, i, window).  Errors as gd_gyr_profile */
int gd_gyr_profile_frames(gd_gyr *h, uint32_t window, uint32_t first, uint32_t stride, uint32_t count, double *out);
/* Device times in milliseconds, between events on the handle's stream: of all kernels of the last successful gd_gyr_tensors, and of
 * the window kernel and of the merge kernel of the last successful gd_gyr_profile or gd_gyr_profile_frames (merge: 0 for the latter).
 * 0 before the first.  Each pointer may be NULL.  What tools/bench_gyr.py reports. */
int gd_gyr_last_times(const gd_gyr *h, double *tensors_ms, double *windows_ms, double *merge_ms);

#ifdef __cplusplus
}
#endif

#endif
