// gdyn_hic.hip -- the Hi-C signal analyses (include/gdyn_hic.h): the pixel pass of the reference's compute_interactions,
// compute_local_alpha and hic_power_law over a cooler's (bin1_id, bin2_id, count) columns, and their per-bin signals.
//
//   k_hic_accumulate   one pass over a batch of pixels for every target of the handle.  A lane takes four consecutive pixels:
//                      the three columns lie on 16-byte aligned buffers padded to whole lanes, so its 80 bytes are five
//                      16-byte loads; pixels past the batch's end are masked by their index.  Per target kind:
//                        band     one 64-bit integer atomic add at [i, d] per cis pixel with d < W.  Pixels are sorted by
//                                 (bin1, bin2), so the lanes of a wave add to consecutive cells of a few rows.
//                        profile  a histogram in LDS per block (a 64-bit sum and a 32-bit count per bin, the handle's first
//                                 GD_HIC_LDS_BINS profile bins, 48 KiB), flushed with one global atomic pair per non-zero
//                                 bin; the bins beyond that budget use global atomics.  Sums are int64, or fp64 when the
//                                 target has weights.
//                        dense    two hardware float32 atomic adds per cis pixel, at [li, lj] and [lj, li] of its chromosome's
//                                 n x n matrix; a cell of a valid cooler receives at most two adds of one value
//                      Integer adds commute: no integer result depends on the batch size, the grid or the arrival order.
//   k_hic_decay, k_hic_insulation   D(i, k) and I(i, k) of a band target, one thread per (bin, k)
//   k_hic_alpha                     alpha(i) of a band target, one thread per bin
//   k_dense_profile, k_sum_parts    the mean contact per distance of a dense target: per block of 64 rows a lane owns a
//                                   distance and walks the rows (coalesced along a row), then the partial sums are added in a
//                                   fixed order: no float atomics
//   k_dense_f64, k_row_flags        the contact or enrichment matrix in fp64; per row: any cell != 0, any finite non-zero, any
//                                   non-finite
//   k_pca_*                         the leading principal components (block subspace iteration on Xc^T Xc, block kPB = 16
//                                   columns of which min(m, k + 8) are in use): compaction and centring, the two tall-skinny
//                                   products k_pca_xq (Y = Xc Q) and k_pca_xty (Z = Xc^T Y) that read the matrix once each, the
//                                   16 x 16 Gram matrices, the rotation of the block with its residuals.  The 16 x 16
//                                   eigen-problems are solved on the host (Jacobi).
// The signals are chains of fp64 operations in numpy's order (the object is built without fast-math and without contraction).
// Every index that addresses memory is checked against its array in the kernel: pixels are data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_hic.h"
#include "gdyn_analysis.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr int kPerLane = 4;                   // pixels per lane
constexpr unsigned kMaxBlocks = 2048;         // grid of k_hic_accumulate: blocks stride over the batch

enum kind : int { kBand = 0, kProfile = 1, kDense = 2 };

struct target_desc {
    int kind;
    int weighted;                     // profile: fp64 sums of c / (w[i] * w[j])
    unsigned width;                   // W of a band, size of a profile
    unsigned lds, lds_count;          // profile: its first LDS bin and how many of its first bins are privatised
    unsigned long long *sum;          // band cells; profile sums (int64, or the bits of a double); dense: the float32 matrices
    unsigned long long *cnt;          // profile counts
    const unsigned char *mask;        // profile: excluded bins, or NULL
    const double *w;                  // profile, dense: weights, or NULL
    const unsigned long long *row;    // dense: per bin, the float32 index of its row in its chromosome's matrix
};

struct launch_args {
    int n_targets;
    unsigned lds_bins;                // LDS bins in use
    unsigned n_bins;
    const int *chrom;
    const unsigned *run_beg;          // per bin: the first bin of its run of equal codes
    target_desc t[GD_HIC_MAX_TARGETS];
};

__global__ void __launch_bounds__(kBlock) k_hic_accumulate(const longlong2 *__restrict__ bin1, const longlong2 *__restrict__ bin2,
                                                          const int4 *__restrict__ count, unsigned n, unsigned groups, launch_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long hsum[];      // [lds_bins] sums, then [lds_bins] 32-bit counts
    unsigned *const hcnt = reinterpret_cast<unsigned *>(hsum + a.lds_bins);
    for (unsigned b = threadIdx.x; b < a.lds_bins; b += kBlock) {
        hsum[b] = 0;
        hcnt[b] = 0;
    }
    __syncthreads();
    unsigned const stride = gridDim.x * kBlock;
    for (unsigned g = blockIdx.x * kBlock + threadIdx.x; g < groups; g += stride) {
        longlong2 const p0 = bin1[2 * (size_t)g], p1 = bin1[2 * (size_t)g + 1], q0 = bin2[2 * (size_t)g], q1 = bin2[2 * (size_t)g + 1];
        int4 const c4 = count[g];
        long long const x[kPerLane] = {p0.x, p0.y, p1.x, p1.y}, y[kPerLane] = {q0.x, q0.y, q1.x, q1.y};
        int const c[kPerLane] = {c4.x, c4.y, c4.z, c4.w};
        unsigned lo[kPerLane], hi[kPerLane], d[kPerLane];
        bool cis[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; k++) {
            // a negative id is a huge unsigned one
            bool const live = g * kPerLane + k < n && (unsigned long long)x[k] < a.n_bins && (unsigned long long)y[k] < a.n_bins;
            unsigned const u = live ? (unsigned)x[k] : 0u, v = live ? (unsigned)y[k] : 0u;
            lo[k] = min(u, v);
            hi[k] = max(u, v);
            d[k] = hi[k] - lo[k];
            cis[k] = live && a.chrom[lo[k]] == a.chrom[hi[k]];
        }
        for (int ti = 0; ti < a.n_targets; ti++) {
            target_desc const &t = a.t[ti];
            if (t.kind == kBand) {
#pragma unroll
                for (int k = 0; k < kPerLane; k++)
                    if (cis[k] && d[k] < t.width) atomicAdd(t.sum + (size_t)lo[k] * t.width + d[k], (unsigned long long)(long long)c[k]);
            } else if (t.kind == kDense) {
                float *const cells = reinterpret_cast<float *>(t.sum);
#pragma unroll
                for (int k = 0; k < kPerLane; k++) {
                    if (!cis[k]) continue;
                    unsigned const beg = a.run_beg[lo[k]];
                    if (a.run_beg[hi[k]] != beg) continue;      // one matrix per run: hi - beg < n
                    float const v = (float)(t.w ? (double)c[k] / (t.w[lo[k]] * t.w[hi[k]]) : (double)c[k]);
                    unsafeAtomicAdd(cells + t.row[lo[k]] + (hi[k] - beg), v);
                    unsafeAtomicAdd(cells + t.row[hi[k]] + (lo[k] - beg), v);
                }
            } else {
#pragma unroll
                for (int k = 0; k < kPerLane; k++) {
                    if (!cis[k] || d[k] >= t.width) continue;      // d < size for every counted pair was checked when the target was added
                    if (t.mask && (t.mask[lo[k]] | t.mask[hi[k]])) continue;
                    bool const in_lds = d[k] < t.lds_count;
                    if (t.weighted) {
                        double const v = (double)c[k] / (t.w[lo[k]] * t.w[hi[k]]);
                        if (v != v) continue;
                        if (in_lds) {
                            unsafeAtomicAdd(reinterpret_cast<double *>(&hsum[t.lds + d[k]]), v);
                            atomicAdd(&hcnt[t.lds + d[k]], 1u);
                        } else {
                            unsafeAtomicAdd(reinterpret_cast<double *>(t.sum + d[k]), v);
                            atomicAdd(t.cnt + d[k], 1ull);
                        }
                    } else if (in_lds) {
                        atomicAdd(&hsum[t.lds + d[k]], (unsigned long long)(long long)c[k]);
                        atomicAdd(&hcnt[t.lds + d[k]], 1u);
                    } else {
                        atomicAdd(t.sum + d[k], (unsigned long long)(long long)c[k]);
                        atomicAdd(t.cnt + d[k], 1ull);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int ti = 0; ti < a.n_targets; ti++) {
        target_desc const &t = a.t[ti];
        if (t.kind != kProfile) continue;
        for (unsigned b = threadIdx.x; b < t.lds_count; b += kBlock) {
            unsigned const m = hcnt[t.lds + b];
            if (!m) continue;
            if (t.weighted) unsafeAtomicAdd(reinterpret_cast<double *>(t.sum + b), *reinterpret_cast<double *>(&hsum[t.lds + b]));
            else atomicAdd(t.sum + b, hsum[t.lds + b]);
            atomicAdd(t.cnt + b, (unsigned long long)m);
        }
    }
}

// a zero cell is unmappable
__device__ inline double cell(const long long *__restrict__ band, unsigned W, unsigned bin, unsigned k)
{
    long long const v = band[(size_t)bin * W + k];
    return v == 0 ? __builtin_nan("") : (double)v;
}

// np.nanmean of two values
__device__ inline double nanmean2(double a, double b)
{
    if (a != a) return b;
    if (b != b) return a;
    return (a + b) / 2;
}

// the symmetrised local decay of bin `bin` at separation k >= 1: run_beg <= bin < run_end is its chromosome
__device__ inline double local_decay(const long long *__restrict__ band, unsigned W, unsigned bin, unsigned k, unsigned beg, unsigned end)
{
    double forw = __builtin_nan(""), back = __builtin_nan("");
    if (k < end - bin) forw = cell(band, W, bin, k) / sqrt(cell(band, W, bin, 0) * cell(band, W, bin + k, 0));
    if (bin - beg >= k) back = cell(band, W, bin - k, k) / sqrt(cell(band, W, bin - k, 0) * cell(band, W, bin, 0));
    return nanmean2(forw, back);
}

// full: (n_bins, W) with column 0; out: (n_bins, W - 1), D1 .. D(W-1)
__global__ void __launch_bounds__(kBlock) k_hic_decay(const long long *__restrict__ band, unsigned W, unsigned n_bins, const unsigned *__restrict__ run_beg,
                                                     const unsigned *__restrict__ run_end, double *__restrict__ full, double *__restrict__ out)
{
    size_t const idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (size_t)n_bins * W) return;
    unsigned const bin = (unsigned)(idx / W), k = (unsigned)(idx % W);
    unsigned const beg = run_beg[bin], end = run_end[bin];
    double r;
    if (end - beg <= 1) r = __builtin_nan("");
    else if (k == 0) r = 1.0;
    else r = local_decay(band, W, bin, k, beg, end);
    full[idx] = r;
    if (k) out[(size_t)bin * (W - 1) + (k - 1)] = r;
}

// out: (n_bins, W - 2), I1 .. I(W-2)
__global__ void __launch_bounds__(kBlock) k_hic_insulation(const double *__restrict__ full, unsigned W, unsigned n_bins, double *__restrict__ out)
{
    size_t const idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (W < 3 || idx >= (size_t)n_bins * (W - 2)) return;
    unsigned const bin = (unsigned)(idx / (W - 2)), k = 1 + (unsigned)(idx % (W - 2));
    out[idx] = full[(size_t)bin * W + k] / full[(size_t)bin * W + k + 1];
}

__global__ void __launch_bounds__(kBlock) k_hic_alpha(const long long *__restrict__ band, unsigned W, unsigned n_bins, const unsigned *__restrict__ run_beg,
                                                     const unsigned *__restrict__ run_end, double *__restrict__ alpha)
{
    unsigned const bin = blockIdx.x * kBlock + threadIdx.x;
    if (bin >= n_bins) return;
    unsigned const beg = run_beg[bin], end = run_end[bin];
    double sx = 0, sxx = 0, sy = 0, sxy = 0;
    unsigned finite = 0;
    for (unsigned s = 1; s < W; s++) {
        double const x = log((double)s);
        sx += x;
        sxx += x * x;
        double const y = log(local_decay(band, W, bin, s, beg, end));
        if (y != y) continue;
        sy += y;
        sxy += x * y;
        finite++;
    }
    double const width = (double)(W - 1);
    double const mx = sx / width, mxx = sxx / width;
    double const my = finite ? sy / (double)finite : __builtin_nan(""), mxy = finite ? sxy / (double)finite : __builtin_nan("");
    alpha[bin] = -((mxy - mx * my) / (mxx - mx * mx));
}

// ---- dense targets: the mean contact per distance, fp64 views, row flags

constexpr unsigned kProfileRows = 64;      // rows of a matrix per block of k_dense_profile

// part_sum, part_cnt: [row block of this chromosome][size]; lane = distance d, rows r0 .. r0 + kProfileRows of one matrix
__global__ void __launch_bounds__(kBlock) k_dense_profile(const float *__restrict__ C, unsigned n, unsigned size, double *__restrict__ part_sum,
                                                         unsigned long long *__restrict__ part_cnt)
{
    unsigned const d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= size) return;
    unsigned const r0 = blockIdx.y * kProfileRows, r1 = min(r0 + kProfileRows, n);
    double s = 0;
    unsigned long long c = 0;
    for (unsigned i = r0; i < r1 && i + d < n; i++) {
        float const x = C[(size_t)i * n + i + d];
        if (x != 0.0f && x == x) {
            s += (double)x;
            c++;
        }
    }
    part_sum[(size_t)blockIdx.y * size + d] = s;
    part_cnt[(size_t)blockIdx.y * size + d] = c;
}

// contacts[d], counts[d] = the parts added in their order; mean = contacts / counts
__global__ void __launch_bounds__(kBlock) k_dense_profile_sum(const double *__restrict__ part_sum, const unsigned long long *__restrict__ part_cnt, unsigned parts,
                                                             unsigned size, double *__restrict__ contacts, unsigned long long *__restrict__ counts,
                                                             double *__restrict__ mean)
{
    unsigned const d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= size) return;
    double s = 0;
    unsigned long long c = 0;
    for (unsigned p = 0; p < parts; p++) {
        s += part_sum[(size_t)p * size + d];
        c += part_cnt[(size_t)p * size + d];
    }
    contacts[d] = s;
    counts[d] = c;
    mean[d] = s / (double)c;      // 0 / 0 = NaN
}

// out = (double)C, or (double)C / mean[|i - j|]
__global__ void __launch_bounds__(kBlock) k_dense_f64(const float *__restrict__ C, unsigned n, const double *__restrict__ mean, double *__restrict__ out)
{
    size_t const idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    unsigned const i = (unsigned)(idx / n), j = (unsigned)(idx % n);
    double const v = (double)C[idx];
    out[idx] = mean ? v / mean[i > j ? i - j : j - i] : v;
}

enum row_flag : unsigned char { kRowNonZero = 1, kRowFiniteNonZero = 2, kRowNonFinite = 4 };

// one block per row of an n x n matrix: flags[row] = the row_flag bits of its cells (a NaN is != 0)
template <typename T>
__global__ void __launch_bounds__(kBlock) k_row_flags(const T *__restrict__ M, unsigned n, unsigned char *__restrict__ flags)
{
    unsigned const row = blockIdx.x;
    int f = 0;
    for (unsigned j = threadIdx.x; j < n; j += kBlock) {
        T const x = M[(size_t)row * n + j];
        bool const finite = x - x == 0;
        if (x != 0) f |= kRowNonZero;
        if (x != 0 && finite) f |= kRowFiniteNonZero;
        if (!finite) f |= kRowNonFinite;
    }
    int const a = __syncthreads_or(f & kRowNonZero), b = __syncthreads_or(f & kRowFiniteNonZero), c = __syncthreads_or(f & kRowNonFinite);
    if (threadIdx.x == 0) flags[row] = (unsigned char)((a ? kRowNonZero : 0) | (b ? kRowFiniteNonZero : 0) | (c ? kRowNonFinite : 0));
}

// ---- principal components.  X: m rows of ld doubles (ld even, the pad column zero); Q, Y, Z, V: ld rows of kPB doubles, the rows
// from m on and the columns that are not in use zero.

constexpr int kPB = 16;                  // columns of a block: GD_HIC_MAX_PCS + 8
static_assert(kPB == GD_HIC_MAX_PCS + 8, "block = min(m, k + 8)");
constexpr int kXqRows = 4;               // rows of X per wave of k_pca_xq
constexpr int kWave = 64;
constexpr int kXtyCols = 64;             // columns of X per block of k_pca_xty
constexpr int kXtyUnroll = 4;            // rows of X a wave of k_pca_xty loads at a time

// X[a, b] = A[idx[a], idx[b]]; *bad is set when a value is not finite
__global__ void __launch_bounds__(kBlock) k_pca_compact(const double *__restrict__ A, unsigned n, const unsigned *__restrict__ idx, unsigned m, unsigned ld,
                                                       double *__restrict__ X, int *__restrict__ bad)
{
    size_t const t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (size_t)m * m) return;
    unsigned const a = (unsigned)(t / m), b = (unsigned)(t % m);
    unsigned const ia = idx[a], ib = idx[b];
    if (ia >= n || ib >= n) return;
    double const v = A[(size_t)ia * n + ib];
    X[(size_t)a * ld + b] = v;
    if (!(v - v == 0)) atomicOr(bad, 1);
}

// column j: X[:, j] -= sum(X[:, j]) / m, the rows added one after the other as np.mean(axis=0) adds them
__global__ void __launch_bounds__(kBlock) k_pca_center(double *__restrict__ X, unsigned m, unsigned ld)
{
    unsigned const j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    double s = 0;
    for (unsigned a = 0; a < m; a++) s += X[(size_t)a * ld + j];
    double const mean = s / (double)m;
    for (unsigned a = 0; a < m; a++) X[(size_t)a * ld + j] -= mean;
}

// the start block: a counter-based fill (a hash of the element's index), the same for every run
__global__ void __launch_bounds__(kBlock) k_pca_start(double *__restrict__ Q, unsigned m, unsigned b)
{
    unsigned const t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m * (unsigned)kPB) return;
    unsigned x = t * 2654435761u + 0x9e3779b9u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    Q[t] = t % kPB < b ? (double)x * (2.0 / 4294967296.0) - 1.0 : 0.0;
}

// Y = X Q.  A wave takes kXqRows rows; a lane takes two adjacent columns k, k + 1 of them at a time (one 16-byte load per row,
// 1 KiB per wave and row) with the rows k, k + 1 of Q (the four waves of a block walk k together, so Q comes from the CU's
// cache), then the 64 lanes' sums are added through LDS in lane order.
__global__ void __launch_bounds__(kBlock) k_pca_xq(const double *__restrict__ X, unsigned ld, unsigned m, const double *__restrict__ Q, double *__restrict__ Y)
{
    __shared__ double red[kBlock / kWave][kWave * (kPB + 1)];
    unsigned const wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    unsigned const r0 = (blockIdx.x * (kBlock / kWave) + wave) * kXqRows;
    double acc[kXqRows][kPB];
#pragma unroll
    for (int r = 0; r < kXqRows; r++)
#pragma unroll
        for (int c = 0; c < kPB; c++) acc[r][c] = 0;
    const double *rows[kXqRows];
#pragma unroll
    for (int r = 0; r < kXqRows; r++) rows[r] = X + (size_t)min(r0 + r, m - 1) * ld;      // rows past the end repeat the last one and are not stored
    if (r0 < m) {
        for (unsigned k = 2 * lane; k < ld; k += 2 * kWave) {
            double2 x[kXqRows];
#pragma unroll
            for (int r = 0; r < kXqRows; r++) x[r] = *reinterpret_cast<const double2 *>(rows[r] + k);
            const double2 *q = reinterpret_cast<const double2 *>(Q + (size_t)k * kPB);
#pragma unroll
            for (int c = 0; c < kPB / 2; c++) {
                double2 const q0 = q[c], q1 = q[kPB / 2 + c];
#pragma unroll
                for (int r = 0; r < kXqRows; r++) {
                    acc[r][2 * c] = __builtin_fma(x[r].x, q0.x, acc[r][2 * c]);      // fused by name: the object is built without contraction
                    acc[r][2 * c + 1] = __builtin_fma(x[r].x, q0.y, acc[r][2 * c + 1]);
                    acc[r][2 * c] = __builtin_fma(x[r].y, q1.x, acc[r][2 * c]);
                    acc[r][2 * c + 1] = __builtin_fma(x[r].y, q1.y, acc[r][2 * c + 1]);
                }
            }
        }
    }
    double *const mine = red[wave];
#pragma unroll
    for (int r = 0; r < kXqRows; r++) {
#pragma unroll
        for (int c = 0; c < kPB; c++) mine[lane * (kPB + 1) + c] = acc[r][c];
        __syncthreads();
        if (lane < kPB && r0 + r < m) {
            double s = 0;
            for (int l = 0; l < kWave; l++) s += mine[l * (kPB + 1) + lane];
            Y[(size_t)(r0 + r) * kPB + lane] = s;
        }
        __syncthreads();
    }
}

// part[split][j][c] = sum over the rows i of the split of X[i, j] Y[i, c].  A lane owns column j (a wave reads 512 contiguous
// bytes of a row), the row of Y is the same for the whole wave; the four waves of a block take every fourth group of four rows
// of the split and their sums are added through LDS in wave order.
__global__ void __launch_bounds__(kBlock) k_pca_xty(const double *__restrict__ X, unsigned ld, unsigned m, const double *__restrict__ Y, unsigned rows_per_split,
                                                   double *__restrict__ part)
{
    __shared__ double red[kBlock / kWave][kPB][kXtyCols];
    unsigned const wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    unsigned const j = blockIdx.x * kXtyCols + lane;
    unsigned const i0 = blockIdx.y * rows_per_split, i1 = min(i0 + rows_per_split, m);
    double acc[kPB];
#pragma unroll
    for (int c = 0; c < kPB; c++) acc[c] = 0;
    if (j < m) {
        // four rows at a time so that four loads are in flight; a row past the split's end counts as zero
        for (unsigned i = i0 + kXtyUnroll * wave; i < i1; i += kXtyUnroll * (kBlock / kWave)) {
            double x[kXtyUnroll];
#pragma unroll
            for (int u = 0; u < kXtyUnroll; u++) x[u] = i + u < i1 ? X[(size_t)(i + u) * ld + j] : 0.0;
#pragma unroll
            for (int u = 0; u < kXtyUnroll; u++) {
                const double *y = Y + (size_t)min(i + u, i1 - 1) * kPB;
#pragma unroll
                for (int c = 0; c < kPB; c++) acc[c] = __builtin_fma(x[u], y[c], acc[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kPB; c++) red[wave][c][lane] = acc[c];
    __syncthreads();
    // 1024 sums of four values for 256 threads: thread t takes (c, lane') = (t / 64 + 4 q, t % 64)
    if (j < m) {
#pragma unroll
        for (int q = 0; q < kPB / (kBlock / kWave); q++) {
            int const c = (int)wave + (kBlock / kWave) * q;
            double s = 0;
#pragma unroll
            for (int w = 0; w < kBlock / kWave; w++) s += red[w][c][lane];
            part[((size_t)blockIdx.y * m + j) * kPB + c] = s;
        }
    }
}

// out[e] = the `parts` arrays of `len` doubles added in their order
__global__ void __launch_bounds__(kBlock) k_sum_parts(const double *__restrict__ part, unsigned parts, size_t len, double *__restrict__ out)
{
    size_t const e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= len) return;
    double s = 0;
    for (unsigned p = 0; p < parts; p++) s += part[(size_t)p * len + e];
    out[e] = s;
}

constexpr unsigned kGramRows = 128;      // rows per block of k_pca_gram and k_pca_rotate

// part[block][0][a][c] = sum over the block's rows of P[i, a] R[i, c]; part[block][1][a][c] the same of R[i, a] R[i, c]
__global__ void __launch_bounds__(kBlock) k_pca_gram(const double *__restrict__ P, const double *__restrict__ R, unsigned m, double *__restrict__ part)
{
    __shared__ double sp[kGramRows][kPB], sr[kGramRows][kPB];
    unsigned const i0 = blockIdx.x * kGramRows;
    for (unsigned e = threadIdx.x; e < kGramRows * kPB; e += kBlock) {
        unsigned const i = i0 + e / kPB;
        sp[e / kPB][e % kPB] = i < m ? P[(size_t)i * kPB + e % kPB] : 0.0;
        sr[e / kPB][e % kPB] = i < m ? R[(size_t)i * kPB + e % kPB] : 0.0;
    }
    __syncthreads();
    unsigned const a = threadIdx.x / kPB, c = threadIdx.x % kPB;
    double pr = 0, rr = 0;
    for (unsigned i = 0; i < kGramRows; i++) {
        pr += sp[i][a] * sr[i][c];
        rr += sr[i][a] * sr[i][c];
    }
    part[((size_t)blockIdx.x * 2) * (kPB * kPB) + threadIdx.x] = pr;
    part[((size_t)blockIdx.x * 2 + 1) * (kPB * kPB) + threadIdx.x] = rr;
}

// per row, with the Ritz pairs (W, lam) of the block Q and Z = A Q: v = q W, p = z W, the squares of the residual p - lam v are
// added per column (rpart[block][c]); Qn = z T and V = v are stored
__global__ void __launch_bounds__(kGramRows) k_pca_rotate(const double *__restrict__ Q, const double *__restrict__ Z, unsigned m, const double *__restrict__ W,
                                                         const double *__restrict__ lam, const double *__restrict__ T, double *__restrict__ Qn,
                                                         double *__restrict__ V, double *__restrict__ rpart)
{
    __shared__ double sw[kPB][kPB], st[kPB][kPB], sl[kPB], r2[kGramRows][kPB + 1];
    for (unsigned e = threadIdx.x; e < kPB * kPB; e += kGramRows) {
        sw[e / kPB][e % kPB] = W[e];
        st[e / kPB][e % kPB] = T[e];
    }
    if (threadIdx.x < kPB) sl[threadIdx.x] = lam[threadIdx.x];
    __syncthreads();
    unsigned const i = blockIdx.x * kGramRows + threadIdx.x;
    double q[kPB], z[kPB];
#pragma unroll
    for (int c = 0; c < kPB; c++) {
        q[c] = i < m ? Q[(size_t)i * kPB + c] : 0.0;
        z[c] = i < m ? Z[(size_t)i * kPB + c] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < kPB; c++) {
        double v = 0, p = 0, o = 0;
#pragma unroll
        for (int a = 0; a < kPB; a++) {
            v += q[a] * sw[a][c];
            p += z[a] * sw[a][c];
            o += z[a] * st[a][c];
        }
        double const r = p - sl[c] * v;
        r2[threadIdx.x][c] = r * r;
        if (i < m) {
            Qn[(size_t)i * kPB + c] = o;
            V[(size_t)i * kPB + c] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < kPB) {
        double s = 0;
        for (unsigned t = 0; t < kGramRows; t++) s += r2[t][threadIdx.x];
        rpart[(size_t)blockIdx.x * kPB + threadIdx.x] = s;
    }
}

// out = in T, row by row
__global__ void __launch_bounds__(kGramRows) k_pca_mul(const double *__restrict__ in, unsigned m, const double *__restrict__ T, double *__restrict__ out)
{
    __shared__ double st[kPB][kPB];
    for (unsigned e = threadIdx.x; e < kPB * kPB; e += kGramRows) st[e / kPB][e % kPB] = T[e];
    __syncthreads();
    unsigned const i = blockIdx.x * kGramRows + threadIdx.x;
    if (i >= m) return;
    double q[kPB];
#pragma unroll
    for (int c = 0; c < kPB; c++) q[c] = in[(size_t)i * kPB + c];
#pragma unroll
    for (int c = 0; c < kPB; c++) {
        double o = 0;
#pragma unroll
        for (int a = 0; a < kPB; a++) o += q[a] * st[a][c];
        out[(size_t)i * kPB + c] = o;
    }
}

constexpr size_t kAutoPixels = (size_t)1 << 22;          // pixels per launch when max_pixels_per_launch is 0 (80 MiB)
constexpr size_t kMaxPixels = (size_t)1 << 28;           // pixel indices of a batch stay 32-bit
// blocks_for's cap of 2^30 blocks is never met here: a batch has at most kMaxPixels / kPerLane lanes, and the signals take one
// lane per cell of a band that gd_hic_add_band has allocated at 8 bytes a cell: 2^38 cells (2^30 blocks) would be 2 TiB
static_assert(kMaxPixels / kPerLane / kBlock < ((size_t)1 << 30), "a batch of pixels is one grid");

struct target_state {
    target_desc d{};           // what the kernels see: plain pointers into the buffers below
    size_t cells = 0;          // 64-bit values of `sum`
    dbuf<unsigned long long> sum, cnt;
    dbuf<unsigned char> mask;
    dbuf<double> w;
    dbuf<unsigned long long> row;      // dense: target_desc::row
    dbuf<double> mean;                 // dense: the mean contact per distance, once gd_hic_dense_profile has run
    bool has_mean = false;
};

struct chrom_run {      // a chromosome: a run of equal codes
    int32_t code;
    unsigned beg, n;
    size_t off;         // the first cell of its n x n matrix in a dense target
};

}  // namespace

struct gd_hic : gd::handle {
    unsigned max_pixels = 0;
    unsigned n_bins = 0;
    dbuf<int> chrom;                             // device copy of chrom_code
    dbuf<unsigned> run_beg, run_end;             // per bin: its run of equal codes
    std::vector<int32_t> host_chrom;
    dbuf<char> pixels;                           // one batch: bin1, bin2, count, each padded
    dbuf<double> signal;                         // scratch of the post-passes
    std::vector<target_state> targets;
    unsigned lds_bins = 0;
    std::vector<chrom_run> runs;
    bool contiguous = true;                      // every code is one run
    size_t dense_cells = 0;                      // float32 cells of a dense target
    unsigned max_size = 0;                       // the largest n of any run
    // the principal components: the n x n fp64 matrix, its valid m x ld submatrix, the blocks and the partial sums
    dbuf<double> pca_a, pca_x, pca_q, pca_q2, pca_y, pca_z, pca_v, pca_zpart, pca_part, pca_rpart, pca_small;
    dbuf<unsigned> pca_idx;
    dbuf<int> pca_bad;
    dbuf<unsigned char> flags;

    void drop_targets()
    {
        targets.clear();
        lds_bins = 0;
    }
};

namespace {

// zeroed accumulators and device copies of the target's arrays; nothing is left behind on failure
int new_target(gd_hic *h, const char *who, target_desc d, size_t cells, size_t counts, const uint8_t *mask, const double *w, int32_t *out)
{
    if (h->targets.size() >= GD_HIC_MAX_TARGETS) return fail(GD_EINVAL, "%s: a handle holds at most %d targets", who, GD_HIC_MAX_TARGETS);
    HIPCHK(hipSetDevice(h->device));
    target_state t;
    t.cells = cells;
    if (t.sum.ensure(cells) != hipSuccess || t.cnt.ensure(counts) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: no device memory for %zu accumulator cells", who, cells + counts);
    }
    if (mask) HIPCHK(t.mask.upload(mask, h->n_bins));
    if (w) HIPCHK(t.w.upload(w, h->n_bins));
    hipError_t e = t.sum.zero(h->stream);
    if (e == hipSuccess) e = t.cnt.zero(h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(GD_EHIP, "%s: hipMemset failed: %s", who, hipGetErrorString(e));
    d.sum = t.sum.p;
    d.cnt = t.cnt.p;
    d.mask = t.mask.p;
    d.w = t.w.p;
    d.lds = d.lds_count = 0;
    if (d.kind == kProfile) {
        d.lds = h->lds_bins;
        d.lds_count = std::min<unsigned>(d.width, GD_HIC_LDS_BINS - h->lds_bins);
        h->lds_bins += d.lds_count;
    }
    t.d = d;
    h->targets.push_back(std::move(t));
    *out = (int32_t)h->targets.size() - 1;
    return GD_OK;
}

int find(gd_hic *h, const char *who, int32_t target, int kind, target_state **out)
{
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (target < 0 || (size_t)target >= h->targets.size()) return fail(GD_EINVAL, "%s: target %d of %zu", who, target, h->targets.size());
    if (h->targets[(size_t)target].d.kind != kind) return fail(GD_EINVAL, "%s: target %d is not a %s", who, target, kind == kBand ? "band" : "distance profile");
    *out = &h->targets[(size_t)target];
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_hic_abi_version(void) { return GD_HIC_ABI_VERSION; }

int gd_hic_create(const gd_hic_desc *desc, const int32_t *chrom_code, uint32_t n_bins, gd_hic **out)
{
    if (!desc || !out || !chrom_code) return fail(GD_EINVAL, "gd_hic_create: NULL argument");
    *out = nullptr;
    if (n_bins == 0 || n_bins >= 0x80000000u) return fail(GD_EINVAL, "gd_hic_create: %u bins; 1 <= n_bins < 2^31", n_bins);
    if (int rc = gd::open("gd_hic_create", desc, out)) return rc;
    gd_hic *h = *out;
    h->max_pixels = desc->max_pixels_per_launch;
    h->n_bins = n_bins;
    h->host_chrom.assign(chrom_code, chrom_code + n_bins);
    std::vector<unsigned> beg(n_bins), end(n_bins);
    for (uint32_t b = 0, start = 0; b < n_bins; b++) {
        if (b && chrom_code[b] != chrom_code[b - 1]) start = b;
        beg[b] = start;
    }
    for (uint32_t b = n_bins, stop = n_bins; b-- > 0;) {
        if (b + 1 < n_bins && chrom_code[b] != chrom_code[b + 1]) stop = b + 1;
        end[b] = stop;
    }
    std::unordered_map<int32_t, int> seen;
    for (uint32_t b = 0; b < n_bins; b = end[b]) {
        h->contiguous = h->contiguous && seen.emplace(chrom_code[b], 0).second;
        unsigned const n = end[b] - b;
        h->runs.push_back(chrom_run{chrom_code[b], b, n, h->dense_cells});
        h->dense_cells += (size_t)n * n;
        h->max_size = std::max(h->max_size, n);
    }
    hipError_t e = h->chrom.upload(chrom_code, n_bins);
    if (e == hipSuccess) e = h->run_beg.upload(beg.data(), n_bins);
    if (e == hipSuccess) e = h->run_end.upload(end.data(), n_bins);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        gd::close(h);
        *out = nullptr;
        return fail(GD_EHIP, "gd_hic_create failed: %s", hipGetErrorString(e));
    }
    return GD_OK;
}

int gd_hic_destroy(gd_hic *h) { return gd::close(h); }

int gd_hic_add_band(gd_hic *h, uint32_t W, int32_t *target)
{
    if (!h || !target) return fail(GD_EINVAL, "gd_hic_add_band: NULL argument");
    if (W < 1 || W > GD_HIC_MAX_BAND) return fail(GD_EINVAL, "gd_hic_add_band: a band of %u columns; 1 <= W <= %d", W, GD_HIC_MAX_BAND);
    target_desc d{};
    d.kind = kBand;
    d.width = W;
    return new_target(h, "gd_hic_add_band", d, (size_t)h->n_bins * W, 0, nullptr, nullptr, target);
}

int gd_hic_add_distance_profile(gd_hic *h, const uint8_t *excluded_bin_mask, const double *weights, uint32_t size, int32_t *target)
{
    if (!h || !target) return fail(GD_EINVAL, "gd_hic_add_distance_profile: NULL argument");
    if (size == 0) return fail(GD_EINVAL, "gd_hic_add_distance_profile: a profile of 0 bins");
    std::unordered_map<int32_t, std::pair<uint32_t, uint32_t>> extent;      // first and last counted bin of every code
    for (uint32_t b = 0; b < h->n_bins; b++) {
        if (excluded_bin_mask && excluded_bin_mask[b]) continue;
        auto it = extent.find(h->host_chrom[b]);
        if (it == extent.end()) extent.emplace(h->host_chrom[b], std::make_pair(b, b));
        else it->second.second = b;
    }
    for (auto const &e : extent)
        if (e.second.second - e.second.first >= size)
            return fail(GD_EINVAL, "gd_hic_add_distance_profile: chromosome code %d spans bins %u to %u, a distance beyond the profile's %u bins", e.first,
                        e.second.first, e.second.second, size);
    target_desc d{};
    d.kind = kProfile;
    d.weighted = weights != nullptr;
    d.width = size;
    return new_target(h, "gd_hic_add_distance_profile", d, size, size, excluded_bin_mask, weights, target);
}

int gd_hic_accumulate(gd_hic *h, const int64_t *bin1, const int64_t *bin2, const int32_t *count, uint64_t n)
{
    if (!h) return fail(GD_EINVAL, "gd_hic_accumulate: NULL handle");
    if (n == 0) return GD_OK;
    if (!bin1 || !bin2 || !count) return fail(GD_EINVAL, "gd_hic_accumulate: NULL column");
    if (h->targets.empty()) return fail(GD_ESTATE, "gd_hic_accumulate: the handle has no target");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    size_t const B = (size_t)std::min<uint64_t>(std::min<size_t>(h->max_pixels ? h->max_pixels : kAutoPixels, kMaxPixels), n);
    size_t const capacity = (B + kPerLane - 1) / kPerLane * kPerLane;      // whole lanes: every column stays 16-byte aligned
    HIPCHK(h->pixels.ensure(capacity * 20));
    char *const d1 = h->pixels.p, *const d2 = d1 + capacity * 8, *const dc = d2 + capacity * 8;
    launch_args a{};
    a.n_targets = (int)h->targets.size();
    a.lds_bins = h->lds_bins;
    a.n_bins = h->n_bins;
    a.chrom = h->chrom.p;
    a.run_beg = h->run_beg.p;
    for (int k = 0; k < a.n_targets; k++) a.t[k] = h->targets[(size_t)k].d;
    for (uint64_t p0 = 0; p0 < n; p0 += B) {
        unsigned const b = (unsigned)std::min<uint64_t>(B, n - p0);
        unsigned const groups = (b + kPerLane - 1) / kPerLane;
        HIPCHK(hipMemcpyAsync(d1, bin1 + p0, (size_t)b * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d2, bin2 + p0, (size_t)b * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dc, count + p0, (size_t)b * 4, hipMemcpyHostToDevice, st));
        unsigned const blocks = std::min(blocks_for(groups, kBlock), kMaxBlocks);
        hipLaunchKernelGGL(k_hic_accumulate, dim3(blocks), dim3(kBlock), (size_t)h->lds_bins * 12, st, (const longlong2 *)d1, (const longlong2 *)d2,
                           (const int4 *)dc, b, groups, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    return GD_OK;
}

int gd_hic_decay_insulation(gd_hic *h, int32_t band, double *D, double *I)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_hic_decay_insulation", band, kBand, &t)) return rc;
    unsigned const W = t->d.width, n = h->n_bins;
    if (W < 2) return fail(GD_EINVAL, "gd_hic_decay_insulation: a band of %u columns has no D1", W);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    size_t const full = (size_t)n * W, nd = (size_t)n * (W - 1), ni = (size_t)n * (W - 2);
    HIPCHK(h->signal.ensure(full + nd + ni));
    double *const dfull = h->signal.p, *const dd = dfull + full, *const di = dd + nd;
    hipLaunchKernelGGL(k_hic_decay, dim3(blocks_for(full, kBlock)), dim3(kBlock), 0, st, (const long long *)t->d.sum, W, n, h->run_beg.p,
                       h->run_end.p, dfull, dd);
    HIPCHK(hipGetLastError());
    if (ni) {
        hipLaunchKernelGGL(k_hic_insulation, dim3(blocks_for(ni, kBlock)), dim3(kBlock), 0, st, dfull, W, n, di);
        HIPCHK(hipGetLastError());
    }
    if (D) HIPCHK(hipMemcpyAsync(D, dd, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (I && ni) HIPCHK(hipMemcpyAsync(I, di, ni * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GD_OK;
}

int gd_hic_local_alpha(gd_hic *h, int32_t band, double *alpha)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_hic_local_alpha", band, kBand, &t)) return rc;
    if (!alpha) return fail(GD_EINVAL, "gd_hic_local_alpha: NULL argument");
    if (t->d.width < 2) return fail(GD_EINVAL, "gd_hic_local_alpha: a band of %u columns has no separation to fit", t->d.width);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    HIPCHK(h->signal.ensure(h->n_bins));
    hipLaunchKernelGGL(k_hic_alpha, dim3(blocks_for(h->n_bins, kBlock)), dim3(kBlock), 0, st, (const long long *)t->d.sum, t->d.width, h->n_bins, h->run_beg.p,
                       h->run_end.p, h->signal.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(alpha, h->signal.p, (size_t)h->n_bins * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GD_OK;
}

int gd_hic_fetch_band(gd_hic *h, int32_t band, int64_t *out)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_hic_fetch_band", band, kBand, &t)) return rc;
    if (!out) return fail(GD_EINVAL, "gd_hic_fetch_band: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out, t->d.sum, t->cells * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_hic_fetch_profile(gd_hic *h, int32_t profile, double *sum, int64_t *n, double *mean)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_hic_fetch_profile", profile, kProfile, &t)) return rc;
    HIPCHK(hipSetDevice(h->device));
    size_t const size = t->cells;
    std::vector<unsigned long long> s(size), c(size);
    HIPCHK(hipMemcpyAsync(s.data(), t->d.sum, size * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(c.data(), t->d.cnt, size * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < size; k++) {
        double v;
        if (t->d.weighted) memcpy(&v, &s[k], sizeof v);
        else v = (double)(long long)s[k];
        if (sum) sum[k] = v;
        if (n) n[k] = (int64_t)c[k];
        if (mean) mean[k] = c[k] ? v / (double)c[k] : std::nan("");
    }
    return GD_OK;
}

int gd_hic_fetch_profile_raw(gd_hic *h, int32_t profile, int64_t *sum)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_hic_fetch_profile_raw", profile, kProfile, &t)) return rc;
    if (!sum) return fail(GD_EINVAL, "gd_hic_fetch_profile_raw: NULL argument");
    if (t->d.weighted) return fail(GD_EINVAL, "gd_hic_fetch_profile_raw: target %d has weights; its sums are fp64", profile);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(sum, t->d.sum, t->cells * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_hic_reset(gd_hic *h)
{
    if (!h) return fail(GD_EINVAL, "gd_hic_reset: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    for (auto &t : h->targets) {
        HIPCHK(t.sum.zero(h->stream));
        HIPCHK(t.cnt.zero(h->stream));
        t.has_mean = false;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_hic_clear(gd_hic *h)
{
    if (!h) return fail(GD_EINVAL, "gd_hic_clear: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->drop_targets();
    return GD_OK;
}

}  // extern "C"

// ---- dense targets and the principal components

namespace {

int find_dense(gd_hic *h, const char *who, int32_t target, target_state **out)
{
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (target < 0 || (size_t)target >= h->targets.size()) return fail(GD_EINVAL, "%s: target %d of %zu", who, target, h->targets.size());
    if (h->targets[(size_t)target].d.kind != kDense) return fail(GD_EINVAL, "%s: target %d is not a dense target", who, target);
    *out = &h->targets[(size_t)target];
    return GD_OK;
}

int find_run(gd_hic *h, const char *who, int32_t code, const chrom_run **out)
{
    for (auto const &r : h->runs)
        if (r.code == code) {
            *out = &r;
            return GD_OK;
        }
    return fail(GD_EINVAL, "%s: the bin table has no chromosome code %d", who, code);
}

// the eigenvalues (descending) and eigenvectors (the columns of V) of a symmetric n x n matrix, n <= kPB: cyclic Jacobi
void jacobi(int n, double A[kPB][kPB], double lam[kPB], double V[kPB][kPB])
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i][j] = i == j;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) (i == j ? diag : off) += A[i][j] * A[i][j];
        if (off <= 1e-34 * diag || off == 0) break;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                if (A[p][q] == 0) continue;
                double const theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                double const t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
                double const c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < n; k++) {
                    double const akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    double const apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    double const vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int order[kPB];
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order, order + n, [&](int a, int b) { return A[a][a] > A[b][b]; });
    double l[kPB], U[kPB][kPB];
    for (int j = 0; j < n; j++) {
        l[j] = A[order[j]][order[j]];
        for (int i = 0; i < n; i++) U[i][j] = V[i][order[j]];
    }
    for (int j = 0; j < n; j++) {
        lam[j] = l[j];
        for (int i = 0; i < n; i++) V[i][j] = U[i][j];
    }
}

// T (kPB x kPB, zero outside b x b) with (P T)^T (P T) = 1 on the columns it keeps, from G = P^T P: the columns of P are scaled
// to unit length, the scaled Gram matrix is diagonalised and its eigen-directions are normalised.  A column whose length is at
// most `drop` times the longest one carries no direction (the block has met the matrix's rank) and is left out: its column of T
// is zero.  *cond receives the smallest eigenvalue of the scaled Gram matrix over the largest.
void orth_transform(int b, const double G[kPB][kPB], double drop, double T[kPB][kPB], double *cond)
{
    double len[kPB], longest = 0;
    for (int j = 0; j < b; j++) {
        len[j] = std::sqrt(std::max(G[j][j], 0.0));
        longest = std::max(longest, len[j]);
    }
    int keep[kPB], nk = 0;
    for (int j = 0; j < b; j++)
        if (len[j] > drop * longest && len[j] > 0) keep[nk++] = j;
    double S[kPB][kPB], s[kPB], U[kPB][kPB];
    for (int a = 0; a < nk; a++)
        for (int c = 0; c < nk; c++) S[a][c] = a == c ? 1.0 : 0.5 * (G[keep[a]][keep[c]] + G[keep[c]][keep[a]]) / (len[keep[a]] * len[keep[c]]);
    jacobi(nk, S, s, U);
    for (int a = 0; a < kPB; a++)
        for (int c = 0; c < kPB; c++) T[a][c] = 0;
    *cond = nk ? s[nk - 1] / s[0] : 1.0;
    for (int c = 0; c < nk; c++) {
        double const scale = 1 / std::sqrt(std::max(s[c], 1e-28 * s[0]));
        for (int a = 0; a < nk; a++) T[keep[a]][c] = U[a][c] * scale / len[keep[a]];
    }
}

struct pca_out {
    double *pcs, *variances, *axes;
    int32_t *iterations;
};

// P^T R and R^T R of two blocks
int gram(gd_hic *h, const double *P, const double *R, unsigned m, double PR[kPB][kPB], double RR[kPB][kPB])
{
    unsigned const blocks = (m + kGramRows - 1) / kGramRows;
    HIPCHK(h->pca_part.ensure((size_t)blocks * 2 * kPB * kPB));
    HIPCHK(h->pca_small.ensure(4 * kPB * kPB));
    hipLaunchKernelGGL(k_pca_gram, dim3(blocks), dim3(kBlock), 0, h->stream, P, R, m, h->pca_part.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sum_parts, dim3(blocks_for(2 * kPB * kPB, kBlock)), dim3(kBlock), 0, h->stream, h->pca_part.p, blocks, (size_t)2 * kPB * kPB, h->pca_small.p);
    HIPCHK(hipGetLastError());
    double both[2][kPB][kPB];
    HIPCHK(hipMemcpyAsync(both, h->pca_small.p, sizeof both, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(PR, both[0], sizeof both[0]);
    memcpy(RR, both[1], sizeof both[1]);
    return GD_OK;
}

int upload_small(gd_hic *h, size_t at, const void *src, size_t doubles)
{
    HIPCHK(hipMemcpyAsync(h->pca_small.p + at, src, doubles * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return GD_OK;
}

// out = in T with T from the Gram matrix of `in`: an orthonormal block.  *kept: its columns that are not zero.
int orthonormalize(gd_hic *h, const double *in, double *out, unsigned m, int b, double drop, double *cond)
{
    double G[kPB][kPB], unused[kPB][kPB], T[kPB][kPB];
    if (int rc = gram(h, in, in, m, unused, G)) return rc;
    orth_transform(b, G, drop, T, cond);
    if (int rc = upload_small(h, 2 * kPB * kPB, T, kPB * kPB)) return rc;
    hipLaunchKernelGGL(k_pca_mul, dim3((m + kGramRows - 1) / kGramRows), dim3(kGramRows), 0, h->stream, in, m, h->pca_small.p + 2 * kPB * kPB, out);
    HIPCHK(hipGetLastError());
    return GD_OK;
}

int product(gd_hic *h, unsigned m, unsigned ld, const double *Q, double *Y)
{
    unsigned const rows_per_block = (kBlock / kWave) * kXqRows;
    hipLaunchKernelGGL(k_pca_xq, dim3((m + rows_per_block - 1) / rows_per_block), dim3(kBlock), 0, h->stream, h->pca_x.p, ld, m, Q, Y);
    HIPCHK(hipGetLastError());
    return GD_OK;
}

// the leading k components of the n x n fp64 matrix in h->pca_a
int pca_run(gd_hic *h, const char *who, unsigned n, const uint8_t *valid_mask, uint32_t k, pca_out const &o)
{
    hipStream_t st = h->stream;
    std::vector<unsigned char> mask(n);
    if (valid_mask) {
        for (unsigned i = 0; i < n; i++) mask[i] = valid_mask[i] != 0;
    } else {
        HIPCHK(h->flags.ensure(n));
        hipLaunchKernelGGL(k_row_flags<double>, dim3(n), dim3(kBlock), 0, st, (const double *)h->pca_a.p, n, h->flags.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(mask.data(), h->flags.p, n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (auto &f : mask) f = (f & kRowNonZero) != 0;
    }
    std::vector<unsigned> idx;
    for (unsigned i = 0; i < n; i++)
        if (mask[i]) idx.push_back(i);
    unsigned const m = (unsigned)idx.size();
    if (m < 2) return fail(GD_EINVAL, "%s: %u valid bins; the principal components need at least 2", who, m);
    if (k > m) return fail(GD_EINVAL, "%s: %u components of %u valid bins", who, k, m);
    int const b = (int)std::min<unsigned>(m, k + 8);
    unsigned const ld = (m + 1) / 2 * 2;

    // compaction and centring
    HIPCHK(h->pca_idx.upload(idx.data(), m));
    HIPCHK(h->pca_x.ensure((size_t)m * ld));
    HIPCHK(h->pca_bad.ensure(1));
    for (auto *buf : {&h->pca_q, &h->pca_q2, &h->pca_y, &h->pca_z, &h->pca_v}) {
        HIPCHK(buf->ensure((size_t)ld * kPB));
        HIPCHK(buf->zero(st));
    }
    HIPCHK(h->pca_x.zero(st));
    HIPCHK(h->pca_bad.zero(st));
    hipLaunchKernelGGL(k_pca_compact, dim3(blocks_for((size_t)m * m, kBlock)), dim3(kBlock), 0, st, (const double *)h->pca_a.p, n, (const unsigned *)h->pca_idx.p, m,
                       ld, h->pca_x.p, h->pca_bad.p);
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, h->pca_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad) return fail(GD_EINVAL, "%s: the valid submatrix holds a value that is not finite (numpy.linalg.svd raises LinAlgError there); pass a mask of bins", who);
    hipLaunchKernelGGL(k_pca_center, dim3(blocks_for(m, kBlock)), dim3(kBlock), 0, st, h->pca_x.p, m, ld);
    HIPCHK(hipGetLastError());

    // the split of Z = X^T Y over the rows: enough blocks to fill the device, at most 32 partial blocks to add
    unsigned const xblocks = (m + kXtyCols - 1) / kXtyCols;
    unsigned const splits = std::max(1u, std::min({32u, (1024 + xblocks - 1) / xblocks, (m + 15) / 16}));
    unsigned const rows_per_split = (m + splits - 1) / splits;
    HIPCHK(h->pca_zpart.ensure((size_t)splits * m * kPB));
    unsigned const rblocks = (m + kGramRows - 1) / kGramRows;
    HIPCHK(h->pca_rpart.ensure((size_t)rblocks * kPB));
    std::vector<double> rpart((size_t)rblocks * kPB);

    double const drop = 16.0 * m * 0x1p-52, rho = 1e-12;
    double cond = 1;
    hipLaunchKernelGGL(k_pca_start, dim3(blocks_for((size_t)m * kPB, kBlock)), dim3(kBlock), 0, st, h->pca_q2.p, m, (unsigned)b);
    HIPCHK(hipGetLastError());
    if (int rc = orthonormalize(h, h->pca_q2.p, h->pca_q.p, m, b, 0.0, &cond)) return rc;
    double *Q = h->pca_q.p, *Qn = h->pca_q2.p;
    double lam[kPB] = {0}, W[kPB][kPB];
    int iterations = 0;
    bool converged = false;
    while (iterations < GD_HIC_PCA_MAX_ITERATIONS && !converged) {
        iterations++;
        if (int rc = product(h, m, ld, Q, h->pca_y.p)) return rc;
        hipLaunchKernelGGL(k_pca_xty, dim3(xblocks, splits), dim3(kBlock), 0, st, (const double *)h->pca_x.p, ld, m, (const double *)h->pca_y.p, rows_per_split,
                           h->pca_zpart.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_sum_parts, dim3(blocks_for((size_t)m * kPB, kBlock)), dim3(kBlock), 0, st, (const double *)h->pca_zpart.p, splits, (size_t)m * kPB,
                           h->pca_z.p);
        HIPCHK(hipGetLastError());
        // Rayleigh-Ritz: H = Q^T Z = W diag(lam) W^T
        double H[kPB][kPB], G[kPB][kPB];
        if (int rc = gram(h, Q, h->pca_z.p, m, H, G)) return rc;
        for (int a = 0; a < kPB; a++)
            for (int c = a + 1; c < kPB; c++) H[a][c] = H[c][a] = 0.5 * (H[a][c] + H[c][a]);
        for (int a = 0; a < kPB; a++)
            for (int c = 0; c < kPB; c++) W[a][c] = 0;
        double Hb[kPB][kPB], Wb[kPB][kPB];
        memcpy(Hb, H, sizeof H);
        jacobi(b, Hb, lam, Wb);
        for (int a = 0; a < b; a++)
            for (int c = 0; c < b; c++) W[a][c] = Wb[a][c];
        for (int c = b; c < kPB; c++) lam[c] = 0;
        // the next block: the columns of Z W made orthonormal; its Gram matrix is W^T (Z^T Z) W
        double GW[kPB][kPB], Gp[kPB][kPB], T1[kPB][kPB], T[kPB][kPB];
        for (int a = 0; a < kPB; a++)
            for (int c = 0; c < kPB; c++) {
                double s = 0;
                for (int e = 0; e < kPB; e++) s += G[a][e] * W[e][c];
                GW[a][c] = s;
            }
        for (int a = 0; a < kPB; a++)
            for (int c = 0; c < kPB; c++) {
                double s = 0;
                for (int e = 0; e < kPB; e++) s += W[e][a] * GW[e][c];
                Gp[a][c] = s;
            }
        orth_transform(b, Gp, drop, T1, &cond);
        for (int a = 0; a < kPB; a++)
            for (int c = 0; c < kPB; c++) {
                double s = 0;
                for (int e = 0; e < kPB; e++) s += W[a][e] * T1[e][c];
                T[a][c] = s;
            }
        if (int rc = upload_small(h, 0, W, kPB * kPB)) return rc;
        if (int rc = upload_small(h, kPB * kPB, T, kPB * kPB)) return rc;
        if (int rc = upload_small(h, 3 * kPB * kPB, lam, kPB)) return rc;
        hipLaunchKernelGGL(k_pca_rotate, dim3(rblocks), dim3(kGramRows), 0, st, (const double *)Q, (const double *)h->pca_z.p, m, (const double *)h->pca_small.p,
                           (const double *)(h->pca_small.p + 3 * kPB * kPB), (const double *)(h->pca_small.p + kPB * kPB), Qn, h->pca_v.p, h->pca_rpart.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rpart.data(), h->pca_rpart.p, rpart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        converged = lam[0] > 0;
        for (uint32_t j = 0; j < k && converged; j++) {
            double r2 = 0;
            for (unsigned blk = 0; blk < rblocks; blk++) r2 += rpart[(size_t)blk * kPB + j];
            converged = std::sqrt(r2) <= rho * lam[0];      // false for a NaN
        }
        if (!converged) {
            if (!(lam[0] > 0)) break;                       // a zero matrix: nothing to iterate on
            std::swap(Q, Qn);
            if (cond < 1e-6) {                              // far from orthonormal after one pass: a second one
                if (int rc = orthonormalize(h, Q, Qn, m, b, 0.0, &cond)) return rc;
                std::swap(Q, Qn);
            }
        }
    }
    if (o.iterations) *o.iterations = iterations;
    if (!converged)
        return fail(GD_EUNSUPPORTED, "%s: the block iteration did not meet its residual of 1e-12 in %d iterations: degenerate or vanishing singular values", who,
                    iterations);
    for (uint32_t j = 0; j < k; j++)
        if (!(lam[j] > drop * lam[0]))
            return fail(GD_EUNSUPPORTED, "%s: component %u has a vanishing singular value (%g of the largest squared); the centred matrix has rank below %u", who,
                        j + 1, lam[j] / lam[0], k);

    // u_j s_j = Xc v_j
    if (int rc = product(h, m, ld, h->pca_v.p, h->pca_y.p)) return rc;
    std::vector<double> V((size_t)m * kPB), Y((size_t)m * kPB);
    HIPCHK(hipMemcpyAsync(V.data(), h->pca_v.p, V.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(Y.data(), h->pca_y.p, Y.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double const nan = std::nan(""), root = std::sqrt((double)m - 1);
    if (o.pcs) std::fill(o.pcs, o.pcs + (size_t)n * k, nan);
    if (o.axes) std::fill(o.axes, o.axes + (size_t)n * k, nan);
    for (uint32_t j = 0; j < k; j++) {
        double vv = 0, yy = 0, big = -1;
        unsigned at = 0;
        for (unsigned a = 0; a < m; a++) {
            double const v = V[(size_t)a * kPB + j], y = Y[(size_t)a * kPB + j];
            vv += v * v;
            yy += y * y;
            if (std::fabs(v) > big) {
                big = std::fabs(v);
                at = a;
            }
        }
        double const sign = V[(size_t)at * kPB + j] < 0 ? -1.0 : 1.0;
        double const nv = std::sqrt(vv), s = std::sqrt(yy) / nv;
        if (!(s > 0) || !std::isfinite(s)) return fail(GD_EUNSUPPORTED, "%s: component %u has a vanishing singular value", who, j + 1);
        if (o.variances) o.variances[j] = s * s;
        for (unsigned a = 0; a < m; a++) {
            if (o.axes) o.axes[(size_t)j * n + idx[a]] = sign * V[(size_t)a * kPB + j] / nv;
            if (o.pcs) o.pcs[(size_t)idx[a] * k + j] = sign * Y[(size_t)a * kPB + j] / (nv * s) * root;
        }
    }
    return GD_OK;
}

int check_k(const char *who, uint32_t k)
{
    if (k < 1 || k > GD_HIC_MAX_PCS) return fail(GD_EINVAL, "%s: %u components; 1 <= k <= %d", who, k, GD_HIC_MAX_PCS);
    return GD_OK;
}

// the fp64 matrix of a chromosome (contact or enrichment) into h->pca_a
int dense_f64(gd_hic *h, const char *who, target_state *t, const chrom_run *r, int32_t which)
{
    if (which != GD_HIC_DENSE_CONTACT && which != GD_HIC_DENSE_ENRICHMENT) return fail(GD_EINVAL, "%s: which = %d is neither the contact nor the enrichment matrix", who, which);
    if (which == GD_HIC_DENSE_ENRICHMENT && !t->has_mean) return fail(GD_ESTATE, "%s: the enrichment needs the mean contact profile; call gd_hic_dense_profile first", who);
    size_t const cells = (size_t)r->n * r->n;
    HIPCHK(h->pca_a.ensure(cells));
    hipLaunchKernelGGL(k_dense_f64, dim3(blocks_for(cells, kBlock)), dim3(kBlock), 0, h->stream, reinterpret_cast<const float *>(t->d.sum) + r->off, r->n,
                       which == GD_HIC_DENSE_ENRICHMENT ? (const double *)t->mean.p : nullptr, h->pca_a.p);
    HIPCHK(hipGetLastError());
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_hic_add_dense(gd_hic *h, const double *weights, int32_t *target)
{
    if (!h || !target) return fail(GD_EINVAL, "gd_hic_add_dense: NULL argument");
    if (!h->contiguous) return fail(GD_EINVAL, "gd_hic_add_dense: the bins of a chromosome code are not contiguous");
    std::vector<unsigned long long> row(h->n_bins);
    for (auto const &r : h->runs)
        for (unsigned i = 0; i < r.n; i++) row[r.beg + i] = r.off + (unsigned long long)i * r.n;
    target_desc d{};
    d.kind = kDense;
    d.weighted = weights != nullptr;
    if (int rc = new_target(h, "gd_hic_add_dense", d, (h->dense_cells + 1) / 2, 0, nullptr, weights, target)) return rc;
    target_state &t = h->targets.back();
    hipError_t const e = t.row.upload(row.data(), h->n_bins);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->targets.pop_back();
        *target = -1;
        return fail(e == hipErrorOutOfMemory ? GD_ENOMEM : GD_EHIP, "gd_hic_add_dense: %s", hipGetErrorString(e));
    }
    t.d.row = t.row.p;
    return GD_OK;
}

int gd_hic_dense_profile(gd_hic *h, int32_t dense, const uint8_t *excluded_bin_mask, double *contacts, int64_t *counts, double *mean)
{
    target_state *t = nullptr;
    if (int rc = find_dense(h, "gd_hic_dense_profile", dense, &t)) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    unsigned const size = h->max_size;
    unsigned parts = 0;
    for (auto const &r : h->runs)
        if (!(excluded_bin_mask && excluded_bin_mask[r.beg])) parts += (r.n + kProfileRows - 1) / kProfileRows;
    dbuf<double> part_sum, sums;
    dbuf<unsigned long long> part_cnt, cnts;
    HIPCHK(part_sum.ensure((size_t)parts * size));
    HIPCHK(part_cnt.ensure((size_t)parts * size));
    HIPCHK(sums.ensure(size));
    HIPCHK(cnts.ensure(size));
    HIPCHK(t->mean.ensure(size));
    unsigned at = 0;
    for (auto const &r : h->runs) {
        if (excluded_bin_mask && excluded_bin_mask[r.beg]) continue;
        unsigned const blocks = (r.n + kProfileRows - 1) / kProfileRows;
        hipLaunchKernelGGL(k_dense_profile, dim3(blocks_for(size, kBlock), blocks), dim3(kBlock), 0, st, reinterpret_cast<const float *>(t->d.sum) + r.off, r.n, size,
                           part_sum.p + (size_t)at * size, part_cnt.p + (size_t)at * size);
        HIPCHK(hipGetLastError());
        at += blocks;
    }
    hipLaunchKernelGGL(k_dense_profile_sum, dim3(blocks_for(size, kBlock)), dim3(kBlock), 0, st, (const double *)part_sum.p, (const unsigned long long *)part_cnt.p,
                       parts, size, sums.p, cnts.p, t->mean.p);
    HIPCHK(hipGetLastError());
    if (contacts) HIPCHK(hipMemcpyAsync(contacts, sums.p, (size_t)size * 8, hipMemcpyDeviceToHost, st));
    if (counts) HIPCHK(hipMemcpyAsync(counts, cnts.p, (size_t)size * 8, hipMemcpyDeviceToHost, st));
    if (mean) HIPCHK(hipMemcpyAsync(mean, t->mean.p, (size_t)size * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    t->has_mean = true;
    return GD_OK;
}

int gd_hic_fetch_dense(gd_hic *h, int32_t dense, int32_t chrom_code, int32_t which, void *out)
{
    target_state *t = nullptr;
    const chrom_run *r = nullptr;
    if (int rc = find_dense(h, "gd_hic_fetch_dense", dense, &t)) return rc;
    if (!out) return fail(GD_EINVAL, "gd_hic_fetch_dense: NULL argument");
    if (int rc = find_run(h, "gd_hic_fetch_dense", chrom_code, &r)) return rc;
    HIPCHK(hipSetDevice(h->device));
    size_t const cells = (size_t)r->n * r->n;
    if (which == GD_HIC_DENSE_CONTACT) {
        HIPCHK(hipMemcpyAsync(out, reinterpret_cast<const float *>(t->d.sum) + r->off, cells * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    } else {
        if (int rc = dense_f64(h, "gd_hic_fetch_dense", t, r, which)) return rc;
        HIPCHK(hipMemcpyAsync(out, h->pca_a.p, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_hic_dense_valid(gd_hic *h, int32_t dense, uint8_t *mask)
{
    target_state *t = nullptr;
    if (int rc = find_dense(h, "gd_hic_dense_valid", dense, &t)) return rc;
    if (!mask) return fail(GD_EINVAL, "gd_hic_dense_valid: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(h->flags.ensure(h->n_bins));
    for (auto const &r : h->runs) {
        hipLaunchKernelGGL(k_row_flags<float>, dim3(r.n), dim3(kBlock), 0, h->stream, reinterpret_cast<const float *>(t->d.sum) + r.off, r.n, h->flags.p + r.beg);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(mask, h->flags.p, h->n_bins, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (unsigned b = 0; b < h->n_bins; b++) mask[b] = (mask[b] & kRowFiniteNonZero) && !(mask[b] & kRowNonFinite);
    return GD_OK;
}

int gd_hic_dense_pca(gd_hic *h, int32_t dense, int32_t chrom_code, int32_t which, const uint8_t *valid_mask, uint32_t k, double *pcs, double *variances,
                     double *axes, int32_t *iterations)
{
    target_state *t = nullptr;
    const chrom_run *r = nullptr;
    if (int rc = find_dense(h, "gd_hic_dense_pca", dense, &t)) return rc;
    if (int rc = check_k("gd_hic_dense_pca", k)) return rc;
    if (int rc = find_run(h, "gd_hic_dense_pca", chrom_code, &r)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = dense_f64(h, "gd_hic_dense_pca", t, r, which)) return rc;
    return pca_run(h, "gd_hic_dense_pca", r->n, valid_mask, k, pca_out{pcs, variances, axes, iterations});
}

int gd_hic_pca_matrix(gd_hic *h, const double *matrix, uint32_t n, const uint8_t *valid_mask, uint32_t k, double *pcs, double *variances, double *axes,
                      int32_t *iterations)
{
    if (!h || !matrix) return fail(GD_EINVAL, "gd_hic_pca_matrix: NULL argument");
    if (int rc = check_k("gd_hic_pca_matrix", k)) return rc;
    if (n < 2 || n > 65535) return fail(GD_EINVAL, "gd_hic_pca_matrix: a matrix of %u rows; 2 <= n <= 65535", n);
    HIPCHK(hipSetDevice(h->device));
    if (h->pca_a.ensure((size_t)n * n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "gd_hic_pca_matrix: no device memory for a matrix of %u rows", n);
    }
    HIPCHK(hipMemcpyAsync(h->pca_a.p, matrix, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return pca_run(h, "gd_hic_pca_matrix", n, valid_mask, k, pca_out{pcs, variances, axes, iterations});
}

}  // extern "C"
