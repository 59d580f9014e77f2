/* gdyn_hic.h -- C-ABI of the Hi-C signal analyses of libgdyn: one pass over the pixel table of a cooler file
 * (resolutions/<binsize>/pixels/{bin1_id, bin2_id, count}) for the reference's stage-2 programs
 *   compute_interactions   extract_forward_bands, compute_local_decays, compute_insulation_ratios   -> a band target
 *   compute_local_alpha    load_contact_band, compute_W, estimate_slope                             -> a band target
 *   hic_power_law          collect_mean_contacts                                                    -> a distance profile target
 *
 * A gd_hic handle is bound to one device and to one bin table (the chromosome code of every bin).  It owns device-resident
 * accumulators ("targets", at most GD_HIC_MAX_TARGETS) and gd_hic_accumulate streams pixels through every one of them in one
 * pass.  With a pixel (b1, b2, c): i = min(b1, b2), j = max(b1, b2), d = j - i; it is cis when chrom_code[i] == chrom_code[j].
 * A pixel with a bin id that is negative, or at or beyond n_bins, is ignored.
 *   band(W)                            int64 (n_bins, W); a cis pixel with d < W adds c at [i, d].  Exact integer sums: the
 *                                      same bytes from run to run and for every max_pixels_per_launch.  A zero cell means
 *                                      unmappable and reads as NaN in the signals below.
 *   distance profile(mask, w, size)    length size; a cis pixel with neither bin masked and d < size adds v = c to sum[d]
 *                                      and 1 to n[d].  With weights, v = c / (w[i] * w[j]) in fp64 and a NaN v is dropped.
 *                                      Without weights the sums are int64 and exact.  With weights they are fp64 atomic sums:
 *                                      their last bits depend on the arrival order and may differ from run to run.
 * The signals of a band target are computed on the device in fp64 from the integer band.  A chromosome is a run of equal
 * codes; n is its number of bins and i counts from its first bin.
 *   gd_hic_decay_insulation   f(i, k) = band[i, k] / sqrt(band[i, 0] * band[i + k, 0]) for i < n - k;
 *                             D(i, k) = NaN-skipping mean of f(i, k) (i < n - k) and f(i - k, k) (i >= k); D(i, 0) = 1;
 *                             n <= 1: every D is NaN.  I(i, k) = D(i, k) / D(i, k + 1).
 *                             D: (n_bins, W - 1) holds D1 .. D(W-1); I: (n_bins, W - 2) holds I1 .. I(W-2).
 *   gd_hic_local_alpha        with width = W - 1: W(i, s) = NaN-skipping mean of band[i, s] / sqrt(band[i, 0] * band[i + s, 0])
 *                             (i < n - s) and band[i - s, s] / sqrt(band[i, 0] * band[i - s, 0]) (i >= s);
 *                             alpha(i) = -(mxy - mx * my) / (mxx - mx * mx) over s = 1 .. width with x = log s,
 *                             y = log W(i, s); mx and mxx are means over every s, my and mxy over the s with a finite y.
 *
 *
 * The compartment analysis of the reference's hic_analysis/cool.py (load_contact_matrices, compute_enrichment_matrices,
 * compute_contact_pca) is one more target kind and a solver behind it.  li, lj are bin indices inside a chromosome of n bins.
 *   dense(w)                           one float32 n x n matrix per chromosome.  A cis pixel gives v = c / (w[i] * w[j]) in
 *                                      fp64 (w = 1 without weights), rounded to float32 once, and v is added at [li, lj] and
 *                                      at [lj, li] with hardware float32 atomics: two adds, so a diagonal pixel counts twice.
 *                                      A NaN or infinite v is stored.  For the unique pixels of a valid cooler a cell receives
 *                                      at most two adds of one value: the matrices are the same bytes from run to run and for
 *                                      every max_pixels_per_launch.  With repeated pixels the last bits of a cell depend on
 *                                      the arrival order of its adds and may differ from run to run.
 *   gd_hic_dense_profile               contacts[d] = fp64 sum, counts[d] = number of the cells [i, i + d] (d = 0 .. n - 1) of
 *                                      every chromosome that is not excluded, cells equal to 0 and NaN cells skipped (infinite
 *                                      cells count); mean = contacts / counts, 0 / 0 = NaN.  Length: the largest n of any
 *                                      chromosome, excluded ones included.  A reduction of fixed shape without float atomics:
 *                                      the same input gives the same bytes.  (The reference sums every diagonal in float32
 *                                      first; the two agree bit for bit while a diagonal's sum is an integer below 2^24.)
 *   enrichment                         (double)C[i, j] / mean[|i - j|]: NaN wherever the mean is NaN
 *   gd_hic_dense_valid                 a bin is valid when its row of the contact matrix has a finite non-zero cell and no
 *                                      non-finite cell
 *   gd_hic_dense_pca, gd_hic_pca_matrix   compute_contact_pca for the leading k components.  Default mask: the row has a cell
 *                                      != 0 (a NaN counts).  X = the valid m x m submatrix, Xc = X - column means, fp64.  With
 *                                      the singular triplets (u_j, s_j, v_j) of Xc: variances[j] = s_j^2, axes[j] = v_j and
 *                                      pcs[:, j] = u_j sqrt(m - 1), scattered over the n bins with NaN at invalid ones.  Sign:
 *                                      the element of v_j of largest magnitude (lowest index on a tie) is positive and
 *                                      u_j = Xc v_j / s_j.  Method: block subspace iteration with Rayleigh-Ritz on Xc^T Xc,
 *                                      block min(m, k + 8), a fixed start block, until |Xc^T Xc v_j - l_j v_j| <= 1e-12 l_0
 *                                      for the k wanted.  GD_EINVAL: m < 2, k > m, a non-finite value in X.  GD_EUNSUPPORTED:
 *                                      no convergence in GD_HIC_PCA_MAX_ITERATIONS, or a wanted l_j <= 16 m 2^-52 l_0
 *                                      (degenerate or vanishing singular values; centring leaves rank <= m - 1, so k = m
 *                                      always asks for one).
 *
 * Errors return a gd_status of gdyn.h and set gd_last_error().  This header has its own version: the symbols below are not
 * part of gdyn.h's ABI. */
#ifndef GDYN_HIC_H
#define GDYN_HIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_HIC_ABI_VERSION 2
#define GD_HIC_MAX_TARGETS 8
/* distance-profile bins of a handle that are privatised in one LDS histogram per block (12 bytes each, 48 KiB); the bins of
 * profiles beyond this budget are updated with global atomics */
#define GD_HIC_LDS_BINS 4096
/* widest band */
#define GD_HIC_MAX_BAND 4096

/* most principal components of one call */
#define GD_HIC_MAX_PCS 8
#define GD_HIC_PCA_MAX_ITERATIONS 1000
/* `which` of gd_hic_fetch_dense and gd_hic_dense_pca */
#define GD_HIC_DENSE_CONTACT 0
#define GD_HIC_DENSE_ENRICHMENT 1

typedef struct gd_hic gd_hic;

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t max_pixels_per_launch;  /* pixels uploaded and accumulated at a time; 0: automatic */
} gd_hic_desc;

int gd_hic_abi_version(void);
/* chrom_code: the chromosome code of every bin (bins/chrom); copied.  1 <= n_bins < 2^31. */
int gd_hic_create(const gd_hic_desc *desc, const int32_t *chrom_code, uint32_t n_bins, gd_hic **out);
int gd_hic_destroy(gd_hic *h);
/* Each gd_hic_add_* creates a zeroed target and stores its index in *target.  The arrays are copied. */
int gd_hic_add_band(gd_hic *h, uint32_t W, int32_t *target);
/* excluded_bin_mask: n_bins bytes, non-zero for the bins of chromosomes that do not count, or NULL for none.
 * weights: n_bins doubles, or NULL for raw counts.  GD_EINVAL when two counted bins of one chromosome code lie size or more
 * apart. */
int gd_hic_add_distance_profile(gd_hic *h, const uint8_t *excluded_bin_mask, const double *weights, uint32_t size, int32_t *target);
/* one float32 n x n matrix for every chromosome of the bin table.  weights: n_bins doubles, or NULL for raw counts.  GD_EINVAL
 * when the bins of one chromosome code are not contiguous, GD_ENOMEM when the matrices do not fit the device. */
int gd_hic_add_dense(gd_hic *h, const double *weights, int32_t *target);
/* the columns of a cooler's pixel table as H5Dread returns them.  n == 0 is a no-op. */
int gd_hic_accumulate(gd_hic *h, const int64_t *bin1, const int64_t *bin2, const int32_t *count, uint64_t n);
/* a band target with W >= 2.  D: n_bins * (W - 1) doubles, I: n_bins * (W - 2) doubles; either may be NULL. */
int gd_hic_decay_insulation(gd_hic *h, int32_t band, double *D, double *I);
/* a band target with W >= 2.  alpha: n_bins doubles. */
int gd_hic_local_alpha(gd_hic *h, int32_t band, double *alpha);
/* out: n_bins * W int64 */
int gd_hic_fetch_band(gd_hic *h, int32_t band, int64_t *out);
/* a distance profile: sum[size] (the integer sums converted when the target has no weights), n[size] and mean[size] = sum / n
 * with 0 / 0 as NaN; any of the three may be NULL */
int gd_hic_fetch_profile(gd_hic *h, int32_t profile, double *sum, int64_t *n, double *mean);
/* the int64 sums of a distance profile without weights.  GD_EINVAL for a weighted one. */
int gd_hic_fetch_profile_raw(gd_hic *h, int32_t profile, int64_t *sum);
/* the mean contact per distance of a dense target over the chromosomes whose first bin is not masked (excluded_bin_mask as for a
 * distance profile).  contacts, counts, mean: max_size values each, the largest n of any chromosome; any may be NULL.  The mean
 * stays in the target for the enrichment. */
int gd_hic_dense_profile(gd_hic *h, int32_t dense, const uint8_t *excluded_bin_mask, double *contacts, int64_t *counts, double *mean);
/* the matrix of the chromosome with this code: n * n floats (GD_HIC_DENSE_CONTACT) or doubles (GD_HIC_DENSE_ENRICHMENT; GD_ESTATE
 * before gd_hic_dense_profile) */
int gd_hic_fetch_dense(gd_hic *h, int32_t dense, int32_t chrom_code, int32_t which, void *out);
/* mask: n_bins bytes, 1 for a valid bin */
int gd_hic_dense_valid(gd_hic *h, int32_t dense, uint8_t *mask);
/* the leading k components of a chromosome's matrix.  valid_mask: n bytes, or NULL for the default mask.  pcs: n * k doubles
 * (row-major, pcs[:, j]), variances: k, axes: k * n, iterations: the products Xc^T (Xc Q) taken; any output may be NULL. */
int gd_hic_dense_pca(gd_hic *h, int32_t dense, int32_t chrom_code, int32_t which, const uint8_t *valid_mask, uint32_t k, double *pcs, double *variances,
                     double *axes, int32_t *iterations);
/* the same for any row-major fp64 n x n matrix of the host; it need not be symmetric */
int gd_hic_pca_matrix(gd_hic *h, const double *matrix, uint32_t n, const uint8_t *valid_mask, uint32_t k, double *pcs, double *variances, double *axes,
                      int32_t *iterations);
/* zeroes every accumulator; the targets stay */
int gd_hic_reset(gd_hic *h);
/* removes every target */
int gd_hic_clear(gd_hic *h);

#ifdef __cplusplus
}
#endif

#endif
