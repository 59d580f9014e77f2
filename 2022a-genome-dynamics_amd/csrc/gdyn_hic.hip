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
//                      Integer adds commute: no integer result depends on the batch size, the grid or the arrival order.
//   k_hic_decay, k_hic_insulation   D(i, k) and I(i, k) of a band target, one thread per (bin, k)
//   k_hic_alpha                     alpha(i) of a band target, one thread per bin
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

enum kind : int { kBand = 0, kProfile = 1 };

struct target_desc {
    int kind;
    int weighted;                     // profile: fp64 sums of c / (w[i] * w[j])
    unsigned width;                   // W of a band, size of a profile
    unsigned lds, lds_count;          // profile: its first LDS bin and how many of its first bins are privatised
    unsigned long long *sum;          // band cells; profile sums (int64, or the bits of a double)
    unsigned long long *cnt;          // profile counts
    const unsigned char *mask;        // profile: excluded bins, or NULL
    const double *w;                  // profile: weights, or NULL
};

struct launch_args {
    int n_targets;
    unsigned lds_bins;                // LDS bins in use
    unsigned n_bins;
    const int *chrom;
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
