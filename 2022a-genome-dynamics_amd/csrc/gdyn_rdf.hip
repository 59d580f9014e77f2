// gdyn_rdf.hip -- the pair counts of the radial distribution analyses (include/gdyn_rdf.h), restating the pair search of
// 4-sim-ab/box/src/rdf_analysis/distance_histogram.cc:40-59 (unique pairs of one selection) and
// rdf_analysis_hetero/distance_histogram.cc:40-65 (one query per centre over the targets) on the device.
//
// Per batch of frames:
//   k_rdf_keys    gathers the selected beads of each frame (fp64), bins them into periodic cells of side >= max_distance
//                 (at most a cap of cells per frame) and keys them (type, frame, cell): in cross mode the centres of all
//                 frames sort ahead of all targets, so each kind is one contiguous run per frame
//   gd_sort_contacts  rocPRIM's radix sort (gdyn_sort.hip) orders the beads by key
//   k_rdf_sorted  sorted fp64 copies of the positions
//   k_rdf_starts  first sorted index of every partner cell (binary search); the cells of one x-row form one span
//   k_rdf_count   one lane per centre.  Per axis the lane walks the cells that [q - r, q + r] touches (r = max_distance, widened
//                 by kScanSlack against the rounding of the cell assignment; the pair test is not widened), each cell once
//                 even when the range wraps onto itself (fewer than 3 cells per axis).  In self mode only partners later in
//                 sorted order count, so every unordered pair is seen once.  The pair test is the project's rule (DESIGN.md
//                 section 7b) in fp64 without contraction; the bin is the reference's size_t(d * (1 / bin_width)).
//                 Counts go to a per-block uint32 histogram in LDS (one copy per wave when it fits) and its non-zero bins to
//                 the uint64 counts with one integer atomic each; above GD_RDF_LDS_BINS bins every pair goes to global
//                 memory directly.  Integer sums: results do not depend on the batch size or on the order of arrival.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_rdf.h"
#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"
#include "gdyn_pair_rules.hpp"
#include "gdyn_types.h"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr double kScanSlack = 1e-9;     // widening of the walked cell ranges (never of the pair test), relative to max_distance + box

struct RdfGrid {
    double box[3];
    double inv_side[3];      // cells per unit length along each axis
    int n[3];                // cells per axis (>= 1)
    unsigned cells;
};

__global__ void __launch_bounds__(kBlock) k_rdf_keys(const void *__restrict__ xyz, int is_f64, unsigned n_points, const unsigned *__restrict__ sel,
                                                     unsigned n_sel, unsigned n_center, unsigned B, RdfGrid g, unsigned long long *__restrict__ keys,
                                                     unsigned *__restrict__ vals, double4 *__restrict__ gpos)
{
    size_t const idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * n_sel) return;
    unsigned const f = (unsigned)(idx / n_sel), k = (unsigned)(idx % n_sel);
    size_t const src = ((size_t)f * n_points + sel[k]) * 3;
    double p[3];
    for (int a = 0; a < 3; a++)
        p[a] = is_f64 ? static_cast<const double *>(xyz)[src + a] : (double)static_cast<const float *>(xyz)[src + a];
    int c[3];
    for (int a = 0; a < 3; a++) c[a] = cell_of(wrap(p[a], g.box[a]), g.inv_side[a], g.n[a]);
    unsigned const cell = ((unsigned)c[2] * (unsigned)g.n[1] + (unsigned)c[1]) * (unsigned)g.n[0] + (unsigned)c[0];
    unsigned long long const kind = k >= n_center ? (unsigned long long)B * g.cells : 0ull;
    keys[idx] = kind + (unsigned long long)f * g.cells + cell;
    vals[idx] = (unsigned)idx;
    gpos[idx] = make_double4(p[0], p[1], p[2], 0.0);
}

__global__ void __launch_bounds__(kBlock) k_rdf_sorted(const double4 *__restrict__ gpos, const unsigned *__restrict__ vals, size_t n,
                                                       double4 *__restrict__ spos)
{
    size_t const s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    spos[s] = gpos[vals[s]];
}

// starts[t] = first sorted index whose key >= base + t, t in [0, B * cells]
__global__ void __launch_bounds__(kBlock) k_rdf_starts(const unsigned long long *__restrict__ keys, size_t n, unsigned long long base,
                                                       size_t count, unsigned *__restrict__ starts)
{
    size_t const t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    unsigned long long const key = base + t;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        size_t const mid = (lo + hi) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    starts[t] = (unsigned)lo;
}

// the distinct cells of one axis that [q - r_scan, q + r_scan] touches: first (in [0, n)) and count (every cell when it wraps)
__device__ inline void axis_cells(double qw, double inv_side, int n, double r_scan, int &first, int &count)
{
    double const lo = floor((qw - r_scan) * inv_side), hi = floor((qw + r_scan) * inv_side);
    if (!(hi - lo + 1.0 < (double)n)) {
        first = 0;
        count = n;
        return;
    }
    int const a = (int)lo;
    first = ((a % n) + n) % n;
    count = (int)(hi - lo) + 1;
}

template <bool kSelf, bool kLds>
__global__ void __launch_bounds__(kBlock) k_rdf_count(const double4 *__restrict__ spos, const unsigned *__restrict__ starts, unsigned n_center,
                                                      RdfGrid g, double md2, double r_scan, double inv_bw, unsigned n_bins, int copies,
                                                      unsigned long long *__restrict__ counts)
{
#pragma clang fp contract(off)
    extern __shared__ unsigned hist[];
    unsigned const f = blockIdx.y;
    unsigned const i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long *out = counts + (size_t)f * n_bins;
    if (kLds) {
        for (unsigned b = threadIdx.x; b < n_bins * (unsigned)copies; b += blockDim.x) hist[b] = 0u;
        __syncthreads();
    }
    unsigned *h = kLds ? hist + (copies > 1 ? (threadIdx.x / 64) * n_bins : 0u) : nullptr;
    size_t const s = (size_t)f * n_center + i;
    double4 const q = i < n_center ? spos[s] : make_double4(NAN, NAN, NAN, 0.0);
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {
        int x0, nx, y0, ny, z0, nz;
        axis_cells(wrap(q.x, g.box[0]), g.inv_side[0], g.n[0], r_scan, x0, nx);
        axis_cells(wrap(q.y, g.box[1]), g.inv_side[1], g.n[1], r_scan, y0, ny);
        axis_cells(wrap(q.z, g.box[2]), g.inv_side[2], g.n[2], r_scan, z0, nz);
        const unsigned *st = starts + (size_t)f * g.cells;
        // x spans of a row: [x0, x0 + nx) split where it wraps past the last cell
        int const xa1 = std::min(x0 + nx, g.n[0]), xb1 = x0 + nx - xa1;
        for (int iz = 0; iz < nz; iz++) {
            int const cz = (z0 + iz) % g.n[2];
            for (int iy = 0; iy < ny; iy++) {
                int const cy = (y0 + iy) % g.n[1];
                unsigned const row = ((unsigned)cz * (unsigned)g.n[1] + (unsigned)cy) * (unsigned)g.n[0];
                for (int span = 0; span < 2; span++) {
                    unsigned a = span ? st[row] : st[row + x0];
                    unsigned const b = span ? st[row + xb1] : st[row + xa1];
                    if (kSelf) a = std::max(a, (unsigned)s + 1u);      // partners later in sorted order only
                    for (unsigned j = a; j < b; j++) {
                        double4 const p = spos[j];
                        double const dx = min_image(q.x - p.x, g.box[0]);
                        double const dy = min_image(q.y - p.y, g.box[1]);
                        double const dz = min_image(q.z - p.z, g.box[2]);
                        double const r2 = (dx * dx + dy * dy) + dz * dz;
                        if (r2 < md2) {
                            unsigned long long const bin = (unsigned long long)(sqrt(r2) * inv_bw);
                            if (bin < n_bins) {
                                if (kLds) atomicAdd(&h[bin], 1u);
                                else atomicAdd(&out[bin], 1ull);
                            }
                        }
                    }
                }
            }
        }
    }
    if (kLds) {
        __syncthreads();
        for (unsigned b = threadIdx.x; b < n_bins; b += blockDim.x) {
            unsigned long long v = 0;
            for (int c = 0; c < copies; c++) v += hist[(unsigned)c * n_bins + b];
            if (v) atomicAdd(&out[b], v);
        }
    }
}

}  // namespace

struct gd_rdf : gd::handle {
    unsigned max_frames = 0;
    bool have_selection = false, self = true;
    unsigned n_points = 0, n_center = 0, n_target = 0;
    dbuf<unsigned> sel;                  // centres, then targets
    // per batch
    dbuf<char> in;
    dbuf<double4> gpos, spos;
    dbuf<unsigned long long> keys[2];
    dbuf<unsigned> vals[2], starts;
    dbuf<char> sort_tmp;
    dbuf<unsigned long long> counts;
};

namespace {

// cells of side >= max_distance per axis, coarsened until a frame has at most cap cells
RdfGrid make_grid(const double box[3], double md, unsigned cap)
{
    RdfGrid g;
    double n[3];
    for (int a = 0; a < 3; a++) n[a] = std::min(std::max(1.0, std::floor(box[a] / md)), 1048576.0);
    while (n[0] * n[1] * n[2] > (double)cap) {
        int const a = (n[0] >= n[1] && n[0] >= n[2]) ? 0 : (n[1] >= n[2] ? 1 : 2);
        n[a] = std::max(1.0, std::floor(n[a] * 0.9));
    }
    g.cells = 1;
    for (int a = 0; a < 3; a++) {
        g.box[a] = box[a];
        g.n[a] = (int)n[a];
        g.inv_side[a] = n[a] / box[a];
        g.cells *= (unsigned)g.n[a];
    }
    return g;
}

// xyz: the B frames of the batch, in host memory (on_device false: they are uploaded into h->in first) or on the handle's device,
// where k_rdf_keys reads them in place
int count_batch(gd_rdf *h, const void *xyz, bool on_device, int is_f64, unsigned B, const RdfGrid &g, double bin_width, double md, unsigned n_bins,
                uint64_t *counts_out)
{
    hipStream_t st = h->stream;
    unsigned const n_sel = h->n_center + (h->self ? 0u : h->n_target);
    unsigned const n_part = h->self ? h->n_center : h->n_target;
    size_t const nb = (size_t)B * n_sel, n_in = (size_t)B * h->n_points * 3 * (is_f64 ? 8 : 4);
    size_t const n_starts = (size_t)B * g.cells + 1;
    if (!on_device) HIPCHK(h->in.ensure(n_in));
    HIPCHK(h->gpos.ensure(nb));
    HIPCHK(h->spos.ensure(nb));
    HIPCHK(h->keys[0].ensure(nb));
    HIPCHK(h->keys[1].ensure(nb));
    HIPCHK(h->vals[0].ensure(nb));
    HIPCHK(h->vals[1].ensure(nb));
    HIPCHK(h->starts.ensure(n_starts));
    HIPCHK(h->counts.ensure((size_t)B * n_bins));
    if (!on_device) HIPCHK(hipMemcpyAsync(h->in.p, xyz, n_in, hipMemcpyHostToDevice, st));
    const void *frames = on_device ? xyz : h->in.p;
    hipLaunchKernelGGL(k_rdf_keys, dim3(blocks_for(nb, kBlock)), dim3(kBlock), 0, st, frames, is_f64, h->n_points, h->sel.p, n_sel, h->n_center, B, g,
                       h->keys[0].p, h->vals[0].p, h->gpos.p);
    unsigned long long const key_end = (unsigned long long)(h->self ? 1 : 2) * B * g.cells;
    unsigned bits = 1;
    while (bits < 64 && (key_end >> bits)) bits++;
    size_t tmp_bytes = 0;
    HIPCHK(gd_sort_contacts(nullptr, &tmp_bytes, h->keys[0].p, h->keys[1].p, h->vals[0].p, h->vals[1].p, nb, bits, st));
    HIPCHK(h->sort_tmp.ensure(tmp_bytes));
    HIPCHK(gd_sort_contacts(h->sort_tmp.p, &tmp_bytes, h->keys[0].p, h->keys[1].p, h->vals[0].p, h->vals[1].p, nb, bits, st));
    hipLaunchKernelGGL(k_rdf_sorted, dim3(blocks_for(nb, kBlock)), dim3(kBlock), 0, st, h->gpos.p, h->vals[1].p, nb, h->spos.p);
    unsigned long long const base = h->self ? 0ull : (unsigned long long)B * g.cells;
    hipLaunchKernelGGL(k_rdf_starts, dim3(blocks_for(n_starts, kBlock)), dim3(kBlock), 0, st, h->keys[1].p, nb, base, n_starts, h->starts.p);
    HIPCHK(hipMemsetAsync(h->counts.p, 0, (size_t)B * n_bins * sizeof(unsigned long long), st));
    // a block adds at most kBlock * n_part to one uint32 counter
    bool const lds = n_bins <= GD_RDF_LDS_BINS && n_part < (1u << 24);
    int const copies = lds && (size_t)n_bins * kWaves <= GD_RDF_LDS_BINS ? kWaves : 1;
    size_t const shmem = lds ? (size_t)n_bins * copies * sizeof(unsigned) : 0;
    double const r_scan = md + kScanSlack * (md + std::max(std::max(g.box[0], g.box[1]), g.box[2]));
    dim3 const grid((h->n_center + kBlock - 1) / kBlock, B);
    double const md2 = md * md, inv_bw = 1 / bin_width;
    if (h->self && lds)
        hipLaunchKernelGGL((k_rdf_count<true, true>), grid, dim3(kBlock), shmem, st, h->spos.p, h->starts.p, h->n_center, g, md2, r_scan, inv_bw,
                           n_bins, copies, h->counts.p);
    else if (h->self)
        hipLaunchKernelGGL((k_rdf_count<true, false>), grid, dim3(kBlock), 0, st, h->spos.p, h->starts.p, h->n_center, g, md2, r_scan, inv_bw,
                           n_bins, 1, h->counts.p);
    else if (lds)
        hipLaunchKernelGGL((k_rdf_count<false, true>), grid, dim3(kBlock), shmem, st, h->spos.p, h->starts.p, h->n_center, g, md2, r_scan,
                           inv_bw, n_bins, copies, h->counts.p);
    else
        hipLaunchKernelGGL((k_rdf_count<false, false>), grid, dim3(kBlock), 0, st, h->spos.p, h->starts.p, h->n_center, g, md2, r_scan, inv_bw,
                           n_bins, 1, h->counts.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counts_out, h->counts.p, (size_t)B * n_bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GD_OK;
}

// gd_rdf_counts (`who`) of frames in host memory or on the handle's device
int counts(gd_rdf *h, const char *who, const void *xyz, bool on_device, int is_f64, uint32_t frames, const double box[3], double bin_width,
           double max_distance, uint64_t *counts_out)
{
    if (!h || !box || (!counts_out && frames)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->have_selection) return fail(GD_ESTATE, "%s: call gd_rdf_set_selection first", who);
    for (int a = 0; a < 3; a++)
        if (!(box[a] > 0.0) || !std::isfinite(box[a])) return fail(GD_EINVAL, "%s: box[%d] = %g is not positive and finite", who, a, box[a]);
    unsigned const n_bins = gd_rdf_bins(bin_width, max_distance);
    if (!n_bins)
        return fail(GD_EINVAL, "%s: bin width %g and max distance %g must be positive and finite, with at most %u bins", who, bin_width,
                    max_distance, GD_RDF_MAX_BINS);
    if (frames == 0) return GD_OK;
    if (!xyz && h->n_points) return fail(GD_EINVAL, "%s: NULL coordinates", who);
    unsigned const n_sel = h->n_center + (h->self ? 0u : h->n_target);
    unsigned const n_part = h->self ? h->n_center : h->n_target;
    if (h->n_center == 0 || n_part == 0) {      // nothing to pair
        std::memset(counts_out, 0, (size_t)frames * n_bins * sizeof(uint64_t));
        return GD_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    RdfGrid const g = make_grid(box, max_distance, std::max(4096u, n_sel));
    size_t const want = h->max_frames ? h->max_frames : ((size_t)1 << 20) / h->n_center + 1;      // ~1M centre lanes per launch
    // sorted indices stay 32-bit, frames fit gridDim.y, the cell starts of a batch stay below 2^26 entries
    size_t const limit = std::min<size_t>(std::min<size_t>(65535, ((size_t)1 << 26) / g.cells),
                                          ((size_t)1 << 30) / std::max(n_sel, h->n_points));
    unsigned const B = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(want, limit), frames));
    size_t const frame_bytes = (size_t)h->n_points * 3 * (is_f64 ? 8 : 4);
    for (unsigned f0 = 0; f0 < frames; f0 += B) {
        unsigned const b = std::min(B, frames - f0);
        if (int rc = count_batch(h, static_cast<const char *>(xyz) + f0 * frame_bytes, on_device, is_f64, b, g, bin_width, max_distance, n_bins,
                                 counts_out + (size_t)f0 * n_bins))
            return rc;
    }
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_rdf_abi_version(void) { return GD_RDF_ABI_VERSION; }

uint32_t gd_rdf_bins(double bin_width, double max_distance)
{
    if (!(bin_width > 0.0) || !(max_distance > 0.0) || !std::isfinite(bin_width) || !std::isfinite(max_distance)) return 0;
    double const n = std::ceil(max_distance / bin_width);      // distance_histogram.cc:25
    return n >= 1.0 && n <= (double)GD_RDF_MAX_BINS ? (uint32_t)n : 0u;
}

int gd_rdf_create(const gd_rdf_desc *desc, gd_rdf **out)
{
    if (int rc = gd::open("gd_rdf_create", desc, out)) return rc;
    (*out)->max_frames = desc->max_frames_per_launch;
    return GD_OK;
}

int gd_rdf_destroy(gd_rdf *h) { return gd::close(h); }

int gd_rdf_set_selection(gd_rdf *h, uint32_t n_points, const uint32_t *center_idx, uint32_t n_center, const uint32_t *target_idx,
                         uint32_t n_target)
{
    if (!h || (!center_idx && n_center)) return fail(GD_EINVAL, "gd_rdf_set_selection: NULL argument");
    bool const self = target_idx == nullptr;
    if (self) n_target = 0;
    if (n_points > (1u << 28) || (uint64_t)n_center + n_target > (1u << 28))
        return fail(GD_EINVAL, "gd_rdf_set_selection: %u points, %u centres, %u targets exceed 2^28", n_points, n_center, n_target);
    std::vector<unsigned> all(center_idx, center_idx + n_center);
    if (!self) all.insert(all.end(), target_idx, target_idx + n_target);
    std::vector<char> role(self ? 0 : n_points, 0);
    for (size_t k = 0; k < all.size(); k++) {
        if (all[k] >= n_points) return fail(GD_EINVAL, "gd_rdf_set_selection: index %u of %u points", all[k], n_points);
        if (self) continue;
        char const r = k < n_center ? 1 : 2;
        if (role[all[k]] && role[all[k]] != r) return fail(GD_EINVAL, "gd_rdf_set_selection: bead %u is both a centre and a target", all[k]);
        role[all[k]] = r;
    }
    HIPCHK(hipSetDevice(h->device));
    h->have_selection = false;
    HIPCHK(h->sel.ensure(all.size()));
    if (!all.empty()) HIPCHK(hipMemcpy(h->sel.p, all.data(), all.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    h->self = self;
    h->n_points = n_points;
    h->n_center = n_center;
    h->n_target = n_target;
    h->have_selection = true;
    return GD_OK;
}

int gd_rdf_counts(gd_rdf *h, const void *xyz, int is_f64, uint32_t frames, const double box[3], double bin_width, double max_distance,
                  uint64_t *counts_out)
{
    return counts(h, "gd_rdf_counts", xyz, false, is_f64, frames, box, bin_width, max_distance, counts_out);
}

}  // extern "C"

// ---- the live seam (gdyn_live.hpp)

int gd_rdf_device(const gd_rdf *h) { return h->device; }

int gd_rdf_counts_dev(gd_rdf *h, const char *who, const float *xyz_dev, uint32_t frames, uint32_t n_points, const double box[3], double bin_width,
                      double max_distance, uint64_t *counts_out)
{
    if (h->have_selection && h->n_points != n_points)
        return fail(GD_EINVAL, "%s: the selection is over %u points, the system has %u beads", who, h->n_points, n_points);
    return counts(h, who, xyz_dev, true, 0, frames, box, bin_width, max_distance, counts_out);
}
