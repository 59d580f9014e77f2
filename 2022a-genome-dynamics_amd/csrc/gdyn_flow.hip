// gdyn_flow.hip -- the flow analyses of a trajectory history (include/gdyn_flow.h), restating
// 5-sim-genome/src/analyze_particle_flow and analyze_grid_flow of the reference on the device.
//
//   k_flow_smooth     utils.gaussian_smooth: direct FIR over numpy's "reflect" padding of the time axis, fp64
//   k_flow_velocity   estimate_velocity: least-squares slope over a window of delay + 1 frames clipped at both ends, fp64;
//                     a one-frame window gives 0 * (1/0) = NaN as in numpy (so no fast-math anywhere in this file)
//   per batch of frames (the cell list of the stepper is not reused: it lives in fp32 and in the stepper's set-up):
//     k_flow_bounds      bounding box of each frame (block reduction) and its cell grid: side h = r/2, grown until the cell
//                        count fits the cap, so one far-away bead cannot blow the grid up
//     k_flow_keys        key (frame * cap + cell, bead); rocPRIM's radix sort (stable, gdyn_sort.hip) orders beads by cell
//     k_flow_sorted      sorted fp64 copies of positions and velocities
//     k_flow_cell_starts first sorted index of every cell (binary search), so the cells of one x-row form one span
//     k_flow_particle    one lane per sorted bead; k_flow_grid: one lane per grid point.  Both walk the x-contiguous spans of
//                        their (y, z) rows, test (dx*dx + dy*dy) + dz*dz <= r*r in fp64 without contraction (cKDTree's
//                        inclusive test; coincident beads count), and sum velocities in fp64 in sorted order: no atomics,
//                        so results do not depend on the batch size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_flow.h"
#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"
#include "gdyn_types.h"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr double kScanSlack = 1e-7;     // relative widening of the cell ranges (never of the pair test) against rounding

struct FrameGrid {
    double lo[3];
    double inv_h;
    int dims[3];
    unsigned cells;
};

__device__ inline size_t reflect_index(long long i, long long F)     // numpy.pad(mode="reflect"), repeated reflection included
{
    if (F == 1) return 0;
    long long const P = 2 * (F - 1);
    long long j = i % P;
    if (j < 0) j += P;
    return (size_t)(j < F ? j : P - j);
}

__global__ void __launch_bounds__(kBlock) k_flow_smooth(const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ w,
                                                        int W, int lpad, unsigned F, size_t M)
{
    size_t const total = (size_t)F * M;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        long long const t = (long long)(idx / M);
        size_t const e = idx % M;
        double acc = 0.0;
        for (int k = 0; k < W; k++) acc += w[W - 1 - k] * x[reflect_index(t + k - lpad, F) * M + e];      // "valid" convolution
        y[idx] = acc;
    }
}

__global__ void __launch_bounds__(kBlock) k_flow_velocity(const double *__restrict__ p, double *__restrict__ v, unsigned F, size_t M, int delay)
{
    size_t const total = (size_t)F * M;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        long long const t = (long long)(idx / M);
        size_t const e = idx % M;
        long long const window = (long long)delay + 1;
        long long back = window / 2, forw = window - back;
        if (t - back < 0) back = t;
        if (t + forw > (long long)F) forw = (long long)F - t;
        long long const w = back + forw;
        double const tmean = (double)(w * (w - 1) / 2) / (double)w;
        double ssq = 0.0, pmean = 0.0;
        for (long long k = 0; k < w; k++) {
            double const c = (double)k - tmean;
            ssq += c * c;
            pmean += p[(size_t)(t - back + k) * M + e];
        }
        pmean /= (double)w;
        double num = 0.0;
        for (long long k = 0; k < w; k++) num += ((double)k - tmean) * (p[(size_t)(t - back + k) * M + e] - pmean);
        v[idx] = num * (1.0 / ssq);      // w == 1: 0 * inf = NaN, as the reference computes it
    }
}

__device__ inline double dist2(double dx, double dy, double dz)
{
#pragma clang fp contract(off)
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline int cell_of(double x, double lo, double inv_h, int n)
{
    return (int)fmin(fmax(floor((x - lo) * inv_h), 0.0), (double)(n - 1));      // (NaN -> 0)
}

__global__ void __launch_bounds__(kBlock) k_flow_bounds(const double *__restrict__ pos, unsigned N, double r, unsigned cap, FrameGrid *grids)
{
    __shared__ double red[6][kBlock];
    const double *p = pos + (size_t)blockIdx.x * N * 3;
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (unsigned i = threadIdx.x; i < N; i += kBlock)
        for (int a = 0; a < 3; a++) {
            double const x = p[3 * (size_t)i + a];
            m[a] = fmin(m[a], x);
            m[3 + a] = fmax(m[3 + a], x);
        }
    for (int a = 0; a < 6; a++) red[a][threadIdx.x] = m[a];
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; a++) {
                red[a][threadIdx.x] = fmin(red[a][threadIdx.x], red[a][threadIdx.x + s]);
                red[3 + a][threadIdx.x] = fmax(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    FrameGrid g;
    double ext[3];
    for (int a = 0; a < 3; a++) {
        double const lo = red[a][0], hi = red[3 + a][0];
        bool const ok = lo <= hi;          // false only when every coordinate is NaN
        g.lo[a] = ok ? lo : 0.0;
        ext[a] = ok ? hi - lo : 0.0;
    }
    double h = 0.5 * r;
    bool fits = false;
    for (int it = 0; it < 64 && !fits; it++, h *= 1.25) {
        g.inv_h = 1.0 / h;
        double cells = 1.0;
        for (int a = 0; a < 3; a++) cells *= floor(ext[a] * g.inv_h) + 1.0;
        fits = cells <= (double)cap;
    }
    if (!fits) {      // (extents beyond 1e6 radii) at most cbrt(cap) cells per axis
        double const side = floor(cbrt((double)cap)) - 1.0;
        g.inv_h = side / fmax(fmax(ext[0], ext[1]), ext[2]);
    }
    g.cells = 1;
    for (int a = 0; a < 3; a++) {
        g.dims[a] = (int)(floor(ext[a] * g.inv_h) + 1.0);
        g.cells *= (unsigned)g.dims[a];
    }
    grids[blockIdx.x] = g;
}

__global__ void __launch_bounds__(kBlock) k_flow_keys(const double *__restrict__ pos, unsigned N, unsigned B, unsigned cap,
                                                      const FrameGrid *__restrict__ grids, unsigned long long *keys, unsigned *vals)
{
    size_t const idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * N) return;
    unsigned const f = (unsigned)(idx / N), b = (unsigned)(idx % N);
    FrameGrid const g = grids[f];
    const double *x = pos + idx * 3;
    int const cx = cell_of(x[0], g.lo[0], g.inv_h, g.dims[0]);
    int const cy = cell_of(x[1], g.lo[1], g.inv_h, g.dims[1]);
    int const cz = cell_of(x[2], g.lo[2], g.inv_h, g.dims[2]);
    keys[idx] = (unsigned long long)f * cap + ((unsigned)cz * g.dims[1] + cy) * (unsigned)g.dims[0] + cx;
    vals[idx] = b;
}

__global__ void __launch_bounds__(kBlock) k_flow_sorted(const double *__restrict__ pos, const double *__restrict__ vel, unsigned N, unsigned B,
                                                        const unsigned *__restrict__ vals, double4 *spos, double4 *svel)
{
    size_t const s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (size_t)B * N) return;
    size_t const src = ((s / N) * N + vals[s]) * 3;
    spos[s] = make_double4(pos[src], pos[src + 1], pos[src + 2], 0.0);
    svel[s] = make_double4(vel[src], vel[src + 1], vel[src + 2], 0.0);
}

__global__ void __launch_bounds__(kBlock) k_flow_cell_starts(const unsigned long long *__restrict__ keys, unsigned N, unsigned B, unsigned cap,
                                                             const FrameGrid *__restrict__ grids, unsigned *starts)
{
    size_t const idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * (cap + 1)) return;
    unsigned const f = (unsigned)(idx / (cap + 1)), c = (unsigned)(idx % (cap + 1));
    if (c > grids[f].cells) return;
    unsigned long long const key = (unsigned long long)f * cap + c;
    size_t lo = (size_t)f * N, hi = lo + N;      // first sorted index of frame f with a key >= key
    while (lo < hi) {
        size_t const mid = (lo + hi) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    starts[idx] = (unsigned)lo;
}

// the candidate cells of a point: per axis, the (clamped) cells of [q - r, q + r] widened by kScanSlack; false when empty
__device__ inline bool cell_range(const FrameGrid &g, double q, int a, double r_scan, int &c0, int &c1)
{
    double const u0 = floor(((q - g.lo[a]) - r_scan) * g.inv_h), u1 = floor(((q - g.lo[a]) + r_scan) * g.inv_h);
    if (!(u1 >= 0.0) || !(u0 <= (double)(g.dims[a] - 1))) return false;
    c0 = (int)fmax(u0, 0.0);
    c1 = (int)fmin(u1, (double)(g.dims[a] - 1));
    return true;
}

struct Gathered {
    double sx, sy, sz;
    int n;
};

__device__ inline Gathered gather(const FrameGrid &g, const unsigned *__restrict__ starts, const double4 *__restrict__ spos,
                                  const double4 *__restrict__ svel, double qx, double qy, double qz, double r, double r2)
{
    Gathered o{0.0, 0.0, 0.0, 0};
    double const r_scan = r * (1.0 + kScanSlack) + kScanSlack;
    int x0, x1, y0, y1, z0, z1;
    if (!cell_range(g, qx, 0, r_scan, x0, x1) || !cell_range(g, qy, 1, r_scan, y0, y1) || !cell_range(g, qz, 2, r_scan, z0, z1)) return o;
    for (int cz = z0; cz <= z1; cz++)
        for (int cy = y0; cy <= y1; cy++) {
            unsigned const row = ((unsigned)cz * g.dims[1] + cy) * (unsigned)g.dims[0];
            unsigned const a = starts[row + x0], b = starts[row + x1 + 1];
            for (unsigned j = a; j < b; j++) {
                double4 const p = spos[j];
                if (dist2(p.x - qx, p.y - qy, p.z - qz) <= r2) {
                    double4 const v = svel[j];
                    o.sx += v.x;
                    o.sy += v.y;
                    o.sz += v.z;
                    o.n++;
                }
            }
        }
    return o;
}

__global__ void __launch_bounds__(kBlock) k_flow_particle(const double4 *__restrict__ spos, const double4 *__restrict__ svel,
                                                          const unsigned *__restrict__ vals, const unsigned *__restrict__ starts,
                                                          const FrameGrid *__restrict__ grids, unsigned N, unsigned B, unsigned cap,
                                                          double r, double r2, float *__restrict__ out)
{
    size_t const s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (size_t)B * N) return;
    unsigned const f = (unsigned)(s / N);
    double4 const q = spos[s];
    Gathered const o = gather(grids[f], starts + (size_t)f * (cap + 1), spos, svel, q.x, q.y, q.z, r, r2);
    double const n = (double)o.n;      // >= 1: the bead itself (distance 0)
    float *dst = out + ((size_t)f * N + vals[s]) * 3;
    dst[0] = (float)(o.sx / n);
    dst[1] = (float)(o.sy / n);
    dst[2] = (float)(o.sz / n);
}

__global__ void __launch_bounds__(kBlock) k_flow_grid(const double4 *__restrict__ spos, const double4 *__restrict__ svel,
                                                      const unsigned *__restrict__ starts, const FrameGrid *__restrict__ grids,
                                                      const double *__restrict__ points, unsigned G, unsigned B, unsigned cap,
                                                      double r, double r2, float *__restrict__ flows, int *__restrict__ coverage)
{
    size_t const idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * G) return;
    unsigned const f = (unsigned)(idx / G), k = (unsigned)(idx % G);
    Gathered const o = gather(grids[f], starts + (size_t)f * (cap + 1), spos, svel, points[3 * (size_t)k], points[3 * (size_t)k + 1],
                              points[3 * (size_t)k + 2], r, r2);
    double const n = (double)(o.n > 1 ? o.n : 1);
    flows[3 * idx] = (float)(o.sx / n);
    flows[3 * idx + 1] = (float)(o.sy / n);
    flows[3 * idx + 2] = (float)(o.sz / n);
    coverage[idx] = o.n;
}

unsigned stream_blocks(size_t n) { return (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 256 * 64); }

}  // namespace

struct gd_flow : gd::handle {
    unsigned max_frames = 0;
    unsigned F = 0, N = 0;
    bool have_velocities = false;
    dbuf<double> x, smoothed, vel, weights, points;
    const double *pos = nullptr;       // x or smoothed
    // per batch
    dbuf<unsigned long long> keys[2];
    dbuf<unsigned> vals[2], starts;
    dbuf<double4> spos, svel;
    dbuf<FrameGrid> grids;
    dbuf<char> sort_tmp;
    dbuf<float> out_f;
    dbuf<int> out_i;
};

namespace {

unsigned cell_cap(unsigned N) { return std::max(4u * N, 4096u); }

unsigned frames_per_launch(const gd_flow *h, size_t lanes_per_frame)
{
    size_t const limit = std::max<size_t>(1, ((size_t)1 << 30) / h->N);      // sorted indices stay 32-bit
    size_t const want = h->max_frames ? h->max_frames : ((size_t)1 << 20) / std::max<size_t>(lanes_per_frame, 1) + 1;      // ~1M lanes
    return (unsigned)std::min<size_t>(std::min(want, limit), h->F);
}

// bins frames [f0, f0 + B) into the sorted arrays, the cell grids and the cell starts
int bin_frames(gd_flow *h, unsigned f0, unsigned B, double r)
{
    size_t const nb = (size_t)B * h->N;
    unsigned const cap = cell_cap(h->N);
    hipStream_t st = h->stream;
    HIPCHK(h->grids.ensure(B));
    HIPCHK(h->keys[0].ensure(nb));
    HIPCHK(h->keys[1].ensure(nb));
    HIPCHK(h->vals[0].ensure(nb));
    HIPCHK(h->vals[1].ensure(nb));
    HIPCHK(h->spos.ensure(nb));
    HIPCHK(h->svel.ensure(nb));
    HIPCHK(h->starts.ensure((size_t)B * (cap + 1)));
    const double *pos = h->pos + (size_t)f0 * h->N * 3;
    const double *vel = h->vel.p + (size_t)f0 * h->N * 3;
    hipLaunchKernelGGL(k_flow_bounds, dim3(B), dim3(kBlock), 0, st, pos, h->N, r, cap, h->grids.p);
    hipLaunchKernelGGL(k_flow_keys, dim3(blocks_for(nb, kBlock)), dim3(kBlock), 0, st, pos, h->N, B, cap, h->grids.p, h->keys[0].p, h->vals[0].p);
    unsigned bits = 1;
    while (bits < 64 && ((unsigned long long)B * cap) >> bits) bits++;
    size_t tmp_bytes = 0;
    HIPCHK(gd_sort_contacts(nullptr, &tmp_bytes, h->keys[0].p, h->keys[1].p, h->vals[0].p, h->vals[1].p, nb, bits, st));
    HIPCHK(h->sort_tmp.ensure(tmp_bytes));
    HIPCHK(gd_sort_contacts(h->sort_tmp.p, &tmp_bytes, h->keys[0].p, h->keys[1].p, h->vals[0].p, h->vals[1].p, nb, bits, st));
    hipLaunchKernelGGL(k_flow_sorted, dim3(blocks_for(nb, kBlock)), dim3(kBlock), 0, st, pos, vel, h->N, B, h->vals[1].p, h->spos.p, h->svel.p);
    hipLaunchKernelGGL(k_flow_cell_starts, dim3(blocks_for((size_t)B * (cap + 1), kBlock)), dim3(kBlock), 0, st, h->keys[1].p, h->N, B, cap,
                       h->grids.p, h->starts.p);
    HIPCHK(hipGetLastError());
    return GD_OK;
}

int check_radius(double r, const char *who)
{
    if (!(r > 0.0) || !std::isfinite(r)) return fail(GD_EINVAL, "%s: the scan radius must be positive and finite (got %g)", who, r);
    return GD_OK;
}

}  // namespace

// ---- the seams of the live bridge (gdyn_live.hpp)
int gd_flow_device(const gd_flow *h) { return h->device; }

int gd_flow_history_begin(gd_flow *h, const char *who, uint32_t frames, uint32_t n_beads, double **x, hipStream_t *stream)
{
    if (frames == 0 || n_beads == 0) return fail(GD_EINVAL, "%s: empty history (%u frames of %u beads)", who, frames, n_beads);
    if (n_beads > (1u << 28)) return fail(GD_EINVAL, "%s: %u beads exceed 2^28", who, n_beads);
    HIPCHK(hipSetDevice(h->device));
    h->have_velocities = false;
    h->F = 0;      // x is about to be overwritten: no history until gd_flow_history_end
    HIPCHK(h->x.ensure((size_t)frames * n_beads * 3));
    *x = h->x.p;
    *stream = h->stream;
    return GD_OK;
}

void gd_flow_history_end(gd_flow *h, uint32_t frames, uint32_t n_beads, bool ok)
{
    h->F = ok ? frames : 0;
    h->N = ok ? n_beads : 0;
    h->pos = h->x.p;
}

extern "C" {

int gd_flow_abi_version(void) { return GD_FLOW_ABI_VERSION; }

int gd_flow_create(const gd_flow_desc *desc, gd_flow **out)
{
    if (int rc = gd::open("gd_flow_create", desc, out)) return rc;
    (*out)->max_frames = desc->max_frames_per_launch;
    return GD_OK;
}

int gd_flow_destroy(gd_flow *h) { return gd::close(h); }

int gd_flow_set_history(gd_flow *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    if (!h || !xyz) return fail(GD_EINVAL, "gd_flow_set_history: NULL argument");
    if (frames == 0 || n_beads == 0) return fail(GD_EINVAL, "gd_flow_set_history: empty history (%u frames of %u beads)", frames, n_beads);
    if (n_beads > (1u << 28)) return fail(GD_EINVAL, "gd_flow_set_history: %u beads exceed 2^28", n_beads);
    size_t const n = (size_t)frames * n_beads * 3;
    std::vector<double> host(n);
    for (size_t i = 0; i < n; i++) {
        host[i] = is_f64 ? static_cast<const double *>(xyz)[i] : (double)static_cast<const float *>(xyz)[i];
        if (!std::isfinite(host[i])) return fail(GD_EINVAL, "gd_flow_set_history: non-finite coordinate at %zu", i);
    }
    HIPCHK(hipSetDevice(h->device));
    h->have_velocities = false;
    HIPCHK(h->x.ensure(n));
    HIPCHK(hipMemcpy(h->x.p, host.data(), n * sizeof(double), hipMemcpyHostToDevice));
    h->F = frames;
    h->N = n_beads;
    h->pos = h->x.p;
    return GD_OK;
}

int gd_flow_velocities(gd_flow *h, uint32_t smoothing, uint32_t delay, double *positions_out, double *velocities_out)
{
    if (!h) return fail(GD_EINVAL, "gd_flow_velocities: NULL handle");
    if (!h->F) return fail(GD_ESTATE, "gd_flow_velocities: no history set");
    if (delay > (1u << 30) || smoothing > (1u << 30)) return fail(GD_EINVAL, "gd_flow_velocities: delay %u / smoothing %u too large", delay, smoothing);
    HIPCHK(hipSetDevice(h->device));
    h->have_velocities = false;
    size_t const M = (size_t)h->N * 3, n = (size_t)h->F * M;
    h->pos = h->x.p;
    if (smoothing > 0) {      // utils.gaussian_smooth (the reference skips it when --smoothing is 0 or absent; W = 1 is the identity)
        int const W = (int)smoothing;
        std::vector<double> w(W);
        double const step = W > 1 ? 6.0 / (W - 1) : 0.0;      // numpy.linspace(-3, 3, W): start + i * step, the last one exactly 3
        for (int i = 0; i < W; i++) {
            double const t = (W > 1 && i == W - 1) ? 3.0 : -3.0 + i * step;
            w[i] = std::exp(-(t * t) / 2);
        }
        double sum = 0.0;
        for (double v : w) sum += v;
        for (double &v : w) v /= sum;
        HIPCHK(h->weights.ensure(W));
        HIPCHK(hipMemcpy(h->weights.p, w.data(), W * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(h->smoothed.ensure(n));
        hipLaunchKernelGGL(k_flow_smooth, dim3(stream_blocks(n)), dim3(kBlock), 0, h->stream, h->x.p, h->smoothed.p, h->weights.p, W, W / 2,
                           h->F, M);
        h->pos = h->smoothed.p;
    }
    HIPCHK(h->vel.ensure(n));
    hipLaunchKernelGGL(k_flow_velocity, dim3(stream_blocks(n)), dim3(kBlock), 0, h->stream, h->pos, h->vel.p, h->F, M, (int)delay);
    HIPCHK(hipGetLastError());
    if (positions_out) HIPCHK(hipMemcpyAsync(positions_out, h->pos, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (velocities_out) HIPCHK(hipMemcpyAsync(velocities_out, h->vel.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_velocities = true;
    return GD_OK;
}

int gd_flow_particle(gd_flow *h, double radius, float *flows_out)
{
    if (!h || !flows_out) return fail(GD_EINVAL, "gd_flow_particle: NULL argument");
    if (!h->have_velocities) return fail(GD_ESTATE, "gd_flow_particle: call gd_flow_velocities first");
    if (int rc = check_radius(radius, "gd_flow_particle")) return rc;
    HIPCHK(hipSetDevice(h->device));
    unsigned const B = frames_per_launch(h, h->N), cap = cell_cap(h->N);
    HIPCHK(h->out_f.ensure((size_t)B * h->N * 3));
    for (unsigned f0 = 0; f0 < h->F; f0 += B) {
        unsigned const b = std::min(B, h->F - f0);
        if (int rc = bin_frames(h, f0, b, radius)) return rc;
        size_t const nb = (size_t)b * h->N;
        hipLaunchKernelGGL(k_flow_particle, dim3(blocks_for(nb, kBlock)), dim3(kBlock), 0, h->stream, h->spos.p, h->svel.p, h->vals[1].p, h->starts.p,
                           h->grids.p, h->N, b, cap, radius, radius * radius, h->out_f.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(flows_out + (size_t)f0 * h->N * 3, h->out_f.p, nb * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GD_OK;
}

int gd_flow_grid(gd_flow *h, double radius, const double *points, uint32_t n_points, float *flows_out, int32_t *coverage_out)
{
    if (!h || (!points && n_points)) return fail(GD_EINVAL, "gd_flow_grid: NULL argument");
    if (!h->have_velocities) return fail(GD_ESTATE, "gd_flow_grid: call gd_flow_velocities first");
    if (int rc = check_radius(radius, "gd_flow_grid")) return rc;
    if (n_points > (1u << 28)) return fail(GD_EINVAL, "gd_flow_grid: %u points exceed 2^28", n_points);
    if (n_points == 0) return GD_OK;
    for (size_t i = 0; i < 3 * (size_t)n_points; i++)
        if (!std::isfinite(points[i])) return fail(GD_EINVAL, "gd_flow_grid: non-finite point coordinate at %zu", i);
    HIPCHK(hipSetDevice(h->device));
    unsigned const G = n_points, cap = cell_cap(h->N);
    unsigned const B = std::min(frames_per_launch(h, std::max(h->N, G)), std::max(1u, (1u << 30) / G));
    HIPCHK(h->points.ensure((size_t)G * 3));
    HIPCHK(hipMemcpy(h->points.p, points, (size_t)G * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h->out_f.ensure((size_t)B * G * 3));
    HIPCHK(h->out_i.ensure((size_t)B * G));
    for (unsigned f0 = 0; f0 < h->F; f0 += B) {
        unsigned const b = std::min(B, h->F - f0);
        if (int rc = bin_frames(h, f0, b, radius)) return rc;
        size_t const ng = (size_t)b * G;
        hipLaunchKernelGGL(k_flow_grid, dim3(blocks_for(ng, kBlock)), dim3(kBlock), 0, h->stream, h->spos.p, h->svel.p, h->starts.p, h->grids.p,
                           h->points.p, G, b, cap, radius, radius * radius, h->out_f.p, h->out_i.p);
        HIPCHK(hipGetLastError());
        if (flows_out)
            HIPCHK(hipMemcpyAsync(flows_out + (size_t)f0 * G * 3, h->out_f.p, ng * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (coverage_out)
            HIPCHK(hipMemcpyAsync(coverage_out + (size_t)f0 * G, h->out_i.p, ng * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GD_OK;
}

}  // extern "C"
