// gdyn_lamina.hip -- the lamina analysis (include/gdyn_lamina.h), restating 5-sim-genome/src/analyze_lamina on the device:
// geometry.py:13-28 (the second-order distance of a point from an ellipsoid surface, EPSILON included) and the contact and
// average lines of command.py:99-133.
//
//   k_lamina_distance  four consecutive bead-frames per lane.  A batch of frames is one flat array of beads on a 16-byte
//                      aligned buffer, so a lane's twelve coordinates are three 16-byte loads (six for fp64 input) and its
//                      results one 16-byte (fp32) or 32-byte (fp64) store, whatever the number of beads per frame.  The
//                      inverse squared semiaxes of a frame (pow(s, -2), computed on the host) are read again only where a
//                      lane's beads cross into the next frame.  fp64 without contraction in numpy's operation order: the
//                      results do not depend on how frames are batched.
//   k_lamina_contact   four distances per lane: (double)d < D as bytes, and the same 0 / 1 added to the handle's float32
//                      sum (each element belongs to one lane: no atomics)
//   k_lamina_average   sum / calls in float32
// The buffers are padded to whole lanes, so only the grid is bounds-checked; the pad is never copied back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_lamina.h"
#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr int kPerLane = 4;                 // bead-frames (or distances) per lane
constexpr double kEpsilon = 1e-6;           // geometry.py:4

__device__ inline void load12(const float *p, double x[12])
{
    const float4 *q = reinterpret_cast<const float4 *>(p);
    float4 const a = q[0], b = q[1], c = q[2];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
}

__device__ inline void load12(const double *p, double x[12])
{
    const double2 *q = reinterpret_cast<const double2 *>(p);
    for (int k = 0; k < 6; k++) {
        double2 const a = q[k];
        x[2 * k] = a.x;
        x[2 * k + 1] = a.y;
    }
}

__device__ inline void store4(float *p, const double d[4])
{
    *reinterpret_cast<float4 *>(p) = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
}

__device__ inline void store4(double *p, const double d[4])
{
    reinterpret_cast<double2 *>(p)[0] = make_double2(d[0], d[1]);
    reinterpret_cast<double2 *>(p)[1] = make_double2(d[2], d[3]);
}

// geometry.py:18-28 for one point; i0..i2 = semiaxes ** -2
__device__ inline double surface_distance(double x0, double x1, double x2, double i0, double i1, double i2)
{
#pragma clang fp contract(off)
    double const p0 = i0 * x0, p1 = i1 * x1, p2 = i2 * x2;          // s1
    double const q0 = i0 * p0, q1 = i1 * p1, q2 = i2 * p2;          // s2
    double const r0 = i0 * q0, r1 = i1 * q1, r2 = i2 * q2;          // s3
    double const a = (r0 * x0 + r1 * x1) + r2 * x2;
    double const b = (q0 * x0 + q1 * x1) + q2 * x2;
    double const c = ((p0 * x0 + p1 * x1) + p2 * x2) - 1.0;
    double const u = (b - sqrt(b * b - a * c)) / (a + kEpsilon);
    double const v = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
    return fabs(u * v);
}

// groups: lanes with work, each with kPerLane flat bead indices 4 g .. 4 g + 3 of the batch (beads past the batch's end read
// the buffer's pad and write the output's pad); inv: (frames, 3)
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kBlock) k_lamina_distance(const Tin *__restrict__ xyz, unsigned n_points, unsigned frames, unsigned groups,
                                                            const double *__restrict__ inv, Tout *__restrict__ out)
{
    unsigned const g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    unsigned const first = g * kPerLane;
    double x[12];
    load12(xyz + (size_t)first * 3, x);
    unsigned f = std::min(first / n_points, frames - 1u);
    unsigned r = first - f * n_points;                   // bead within its frame
    double i0 = inv[3 * f], i1 = inv[3 * f + 1], i2 = inv[3 * f + 2];
    double d[kPerLane];
    for (int j = 0; j < kPerLane; j++) {
        if (r >= n_points && f + 1 < frames) {           // into the next frame (past the last one: the pad)
            r -= n_points;
            f++;
            i0 = inv[3 * f];
            i1 = inv[3 * f + 1];
            i2 = inv[3 * f + 2];
        }
        d[j] = surface_distance(x[3 * j], x[3 * j + 1], x[3 * j + 2], i0, i1, i2);
        r++;
    }
    store4(out + first, d);
}

// sum + offset need not be 16-byte aligned (a batch starts at any frame): kVec says that it is
template <bool kVec>
__global__ void __launch_bounds__(kBlock) k_lamina_contact(const float *__restrict__ dist, unsigned groups, unsigned count, double threshold,
                                                           uchar4 *__restrict__ contacts, float *__restrict__ sum)
{
    unsigned const g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    float4 const d = reinterpret_cast<const float4 *>(dist)[g];
    unsigned char const c0 = (double)d.x < threshold, c1 = (double)d.y < threshold, c2 = (double)d.z < threshold, c3 = (double)d.w < threshold;
    contacts[g] = make_uchar4(c0, c1, c2, c3);
    unsigned const first = g * kPerLane;
    if (kVec) {                                          // the sum is padded like the other buffers
        float4 s = *reinterpret_cast<float4 *>(sum + first);
        s.x += (float)c0; s.y += (float)c1; s.z += (float)c2; s.w += (float)c3;
        *reinterpret_cast<float4 *>(sum + first) = s;
    } else {
        unsigned char const c[kPerLane] = {c0, c1, c2, c3};
        for (int j = 0; j < kPerLane; j++)
            if (first + j < count) sum[first + j] += (float)c[j];
    }
}

__global__ void __launch_bounds__(kBlock) k_lamina_average(const float4 *__restrict__ sum, unsigned groups, float calls, float4 *__restrict__ out)
{
    unsigned const g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    float4 const s = sum[g];
    out[g] = make_float4(s.x / calls, s.y / calls, s.z / calls, s.w / calls);
}

constexpr size_t kAutoElements = (size_t)1 << 22;      // bead-frames per launch when max_frames_per_launch is 0
constexpr size_t kMaxElements = (size_t)1 << 30;       // flat indices of a batch stay 32-bit
static_assert(kMaxElements / kPerLane / kBlock < ((size_t)1 << 30), "the lanes of a batch are one grid, far below blocks_for's cap");

size_t padded(size_t count) { return (count + kPerLane - 1) / kPerLane * kPerLane; }

}  // namespace

struct gd_lamina : gd::handle {
    unsigned max_frames = 0;
    dbuf<char> in, out;                  // one batch
    dbuf<char> flags;                    // the contacts of a batch whose distances were computed on the device (in h->out)
    dbuf<double> inv;
    dbuf<float> sum;                     // (frames, n_points) of the contacts calls, padded
    bool have_shape = false;
    unsigned frames = 0, n_points = 0, calls = 0;

    unsigned batch_frames(unsigned total_frames, unsigned n) const
    {
        size_t want = max_frames ? max_frames : std::max<size_t>(1, kAutoElements / n);
        if (!max_frames && want >= kPerLane) want -= want % kPerLane;      // whole lanes per batch: every batch of the sum starts aligned
        return (unsigned)std::min<size_t>(std::min(want, std::max<size_t>(1, kMaxElements / n)), total_frames);
    }
};

namespace {

// pow(s, -2) of every semiaxis (numpy's semiaxes ** -2), after the check of gd_lamina_distances
int inverse_squares(const char *who, const double *semiaxes, uint32_t frames, std::vector<double> &inv)
{
    if (frames && !semiaxes) return fail(GD_EINVAL, "%s: NULL semiaxes", who);
    inv.resize((size_t)frames * 3);
    for (size_t k = 0; k < inv.size(); k++) {
        if (!(semiaxes[k] > 0.0) || !std::isfinite(semiaxes[k]))
            return fail(GD_EINVAL, "%s: semiaxis %zu of frame %zu = %g is not positive and finite", who, k % 3, k / 3, semiaxes[k]);
        inv[k] = std::pow(semiaxes[k], -2.0);
    }
    return GD_OK;
}

// One batch of distances, enqueued: b frames at src (host memory, or the handle's device: kind) are copied into h->in, whose
// pad and alignment the kernel relies on, their inverse squared semiaxes into h->inv, and the distances are left in h->out.
int distance_batch(gd_lamina *h, const void *src, hipMemcpyKind kind, int is_f64, unsigned n_points, unsigned b, const double *inv, int out_is_f64)
{
    hipStream_t st = h->stream;
    size_t const count = (size_t)b * n_points, in_elem = is_f64 ? 8 : 4;
    unsigned const groups = (unsigned)(padded(count) / kPerLane);
    HIPCHK(hipMemcpyAsync(h->in.p, src, count * 3 * in_elem, kind, st));
    HIPCHK(hipMemcpyAsync(h->inv.p, inv, (size_t)b * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    dim3 const grid(blocks_for(groups, kBlock)), block(kBlock);
    if (is_f64 && out_is_f64)
        hipLaunchKernelGGL((k_lamina_distance<double, double>), grid, block, 0, st, (const double *)h->in.p, n_points, b, groups, h->inv.p,
                           (double *)h->out.p);
    else if (is_f64)
        hipLaunchKernelGGL((k_lamina_distance<double, float>), grid, block, 0, st, (const double *)h->in.p, n_points, b, groups, h->inv.p,
                           (float *)h->out.p);
    else if (out_is_f64)
        hipLaunchKernelGGL((k_lamina_distance<float, double>), grid, block, 0, st, (const float *)h->in.p, n_points, b, groups, h->inv.p,
                           (double *)h->out.p);
    else
        hipLaunchKernelGGL((k_lamina_distance<float, float>), grid, block, 0, st, (const float *)h->in.p, n_points, b, groups, h->inv.p,
                           (float *)h->out.p);
    HIPCHK(hipGetLastError());
    return GD_OK;
}

// gd_lamina_distances (`who`) of frames in host memory or on the handle's device (kind); out_optional: out may be NULL, and
// then nothing is copied back
int distances(gd_lamina *h, const char *who, const void *xyz, hipMemcpyKind kind, int is_f64, uint32_t frames, uint32_t n_points,
              const double *semiaxes, void *out, int out_is_f64, bool out_optional)
{
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (frames && !semiaxes) return fail(GD_EINVAL, "%s: NULL semiaxes", who);
    if (n_points > (1u << 28)) return fail(GD_EINVAL, "%s: %u points exceed 2^28", who, n_points);
    std::vector<double> inv;
    if (int rc = inverse_squares(who, semiaxes, frames, inv)) return rc;
    if (frames == 0 || n_points == 0) return GD_OK;
    if (!xyz || (!out && !out_optional)) return fail(GD_EINVAL, "%s: NULL argument", who);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    unsigned const B = h->batch_frames(frames, n_points);
    size_t const in_elem = is_f64 ? 8 : 4, out_elem = out_is_f64 ? 8 : 4;
    HIPCHK(h->in.ensure(padded((size_t)B * n_points) * 3 * in_elem));
    HIPCHK(h->out.ensure(padded((size_t)B * n_points) * out_elem));
    HIPCHK(h->inv.ensure((size_t)B * 3));
    for (unsigned f0 = 0; f0 < frames; f0 += B) {
        unsigned const b = std::min(B, frames - f0);
        size_t const count = (size_t)b * n_points;
        if (int rc = distance_batch(h, static_cast<const char *>(xyz) + (size_t)f0 * n_points * 3 * in_elem, kind, is_f64, n_points, b,
                                    inv.data() + (size_t)f0 * 3, out_is_f64))
            return rc;
        if (out) HIPCHK(hipMemcpyAsync(static_cast<char *>(out) + (size_t)f0 * n_points * out_elem, h->out.p, count * out_elem, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return GD_OK;
}

// gd_lamina_contacts (`who`).  The float32 distances of a batch come from host memory (distances), or are computed on the
// device from float32 frames that lie there (xyz_dev, semiaxes) and never leave it.  out_optional: contacts_out may be NULL.
int contacts(gd_lamina *h, const char *who, const float *distances, const float *xyz_dev, const double *semiaxes, uint32_t frames,
             uint32_t n_points, double contact_distance, uint8_t *contacts_out, bool out_optional)
{
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    std::vector<double> inv;
    if (xyz_dev) {      // the checks of the distances call that the host-fed sequence makes first
        if (n_points > (1u << 28)) return fail(GD_EINVAL, "%s: %u points exceed 2^28", who, n_points);
        if (int rc = inverse_squares(who, semiaxes, frames, inv)) return rc;
    }
    if (std::isnan(contact_distance)) return fail(GD_EINVAL, "%s: the contact distance is NaN", who);
    if (n_points > (1u << 28)) return fail(GD_EINVAL, "%s: %u points exceed 2^28", who, n_points);
    if (h->have_shape && (frames != h->frames || n_points != h->n_points))
        return fail(GD_EINVAL, "%s: a (%u, %u) history after (%u, %u) ones; call gd_lamina_reset between shapes", who, frames, n_points,
                    h->frames, h->n_points);
    size_t const total = (size_t)frames * n_points;
    if (total && ((!distances && !xyz_dev) || (!contacts_out && !out_optional))) return fail(GD_EINVAL, "%s: NULL argument", who);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (!h->have_shape) {
        HIPCHK(h->sum.ensure(padded(total) + kPerLane));
        HIPCHK(hipMemsetAsync(h->sum.p, 0, (padded(total) + kPerLane) * sizeof(float), st));
        HIPCHK(hipStreamSynchronize(st));
        h->frames = frames;
        h->n_points = n_points;
        h->calls = 0;
        h->have_shape = true;
    }
    if (total) {
        unsigned const B = h->batch_frames(frames, n_points);
        size_t const lanes = padded((size_t)B * n_points);
        HIPCHK(h->in.ensure(lanes * (xyz_dev ? 3 : 1) * sizeof(float)));
        HIPCHK(h->out.ensure(lanes * (xyz_dev ? sizeof(float) : 1)));
        if (xyz_dev) {
            HIPCHK(h->inv.ensure((size_t)B * 3));
            HIPCHK(h->flags.ensure(lanes));
        }
        for (unsigned f0 = 0; f0 < frames; f0 += B) {
            unsigned const b = std::min(B, frames - f0);
            size_t const count = (size_t)b * n_points, offset = (size_t)f0 * n_points;
            unsigned const groups = (unsigned)(padded(count) / kPerLane);
            const float *dist = (const float *)h->in.p;
            uchar4 *flags = (uchar4 *)h->out.p;
            if (xyz_dev) {      // h->in: the frames, h->out: their distances, h->flags: the contacts
                if (int rc = distance_batch(h, xyz_dev + offset * 3, hipMemcpyDeviceToDevice, 0, n_points, b, inv.data() + (size_t)f0 * 3, 0)) return rc;
                dist = (const float *)h->out.p;
                flags = (uchar4 *)h->flags.p;
            } else
                HIPCHK(hipMemcpyAsync(h->in.p, distances + offset, count * sizeof(float), hipMemcpyHostToDevice, st));
            dim3 const grid(blocks_for(groups, kBlock)), block(kBlock);
            // the vector form may touch the sum's pad behind the last batch only: an earlier batch that is not a whole number
            // of lanes would add its pad lanes into the next batch's elements
            if (offset % kPerLane == 0 && (count % kPerLane == 0 || f0 + b == frames))
                hipLaunchKernelGGL((k_lamina_contact<true>), grid, block, 0, st, dist, groups, (unsigned)count, contact_distance, flags,
                                   h->sum.p + offset);
            else
                hipLaunchKernelGGL((k_lamina_contact<false>), grid, block, 0, st, dist, groups, (unsigned)count, contact_distance, flags,
                                   h->sum.p + offset);
            HIPCHK(hipGetLastError());
            if (contacts_out) HIPCHK(hipMemcpyAsync(contacts_out + offset, flags, count, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    h->calls++;
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_lamina_abi_version(void) { return GD_LAMINA_ABI_VERSION; }

int gd_lamina_create(const gd_lamina_desc *desc, gd_lamina **out)
{
    if (int rc = gd::open("gd_lamina_create", desc, out)) return rc;
    (*out)->max_frames = desc->max_frames_per_launch;
    return GD_OK;
}

int gd_lamina_destroy(gd_lamina *h) { return gd::close(h); }

int gd_lamina_distances(gd_lamina *h, const void *xyz, int is_f64, uint32_t frames, uint32_t n_points, const double *semiaxes, void *out,
                        int out_is_f64)
{
    return distances(h, "gd_lamina_distances", xyz, hipMemcpyHostToDevice, is_f64, frames, n_points, semiaxes, out, out_is_f64, false);
}

int gd_lamina_contacts(gd_lamina *h, const float *distances, uint32_t frames, uint32_t n_points, double contact_distance,
                       uint8_t *contacts_out)
{
    return contacts(h, "gd_lamina_contacts", distances, nullptr, nullptr, frames, n_points, contact_distance, contacts_out, false);
}

int gd_lamina_average(gd_lamina *h, float *out)
{
    if (!h) return fail(GD_EINVAL, "gd_lamina_average: NULL handle");
    if (!h->have_shape || h->calls == 0) return fail(GD_ESTATE, "gd_lamina_average: call gd_lamina_contacts first");
    size_t const total = (size_t)h->frames * h->n_points;
    if (total == 0) return GD_OK;
    if (!out) return fail(GD_EINVAL, "gd_lamina_average: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    size_t const step = kAutoElements;                   // a multiple of kPerLane: every piece of the sum starts aligned
    HIPCHK(h->out.ensure(step * sizeof(float)));
    for (size_t e0 = 0; e0 < total; e0 += step) {
        size_t const count = std::min(step, total - e0);
        unsigned const groups = (unsigned)(padded(count) / kPerLane);
        hipLaunchKernelGGL(k_lamina_average, dim3(blocks_for(groups, kBlock)), dim3(kBlock), 0, st, (const float4 *)(h->sum.p + e0), groups, (float)h->calls,
                           (float4 *)h->out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + e0, h->out.p, count * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return GD_OK;
}

int gd_lamina_reset(gd_lamina *h)
{
    if (!h) return fail(GD_EINVAL, "gd_lamina_reset: NULL handle");
    h->have_shape = false;
    h->frames = h->n_points = h->calls = 0;
    return GD_OK;
}

}  // extern "C"

// ---- the live seam (gdyn_live.hpp)

int gd_lamina_device(const gd_lamina *h) { return h->device; }

int gd_lamina_distances_dev(gd_lamina *h, const char *who, const float *xyz_dev, uint32_t frames, uint32_t n_points, const double *semiaxes,
                            void *out, int out_is_f64)
{
    return distances(h, who, xyz_dev, hipMemcpyDeviceToDevice, 0, frames, n_points, semiaxes, out, out_is_f64, true);
}

int gd_lamina_contacts_dev(gd_lamina *h, const char *who, const float *xyz_dev, uint32_t frames, uint32_t n_points, const double *semiaxes,
                           double contact_distance, uint8_t *contacts_out)
{
    return contacts(h, who, nullptr, xyz_dev, semiaxes, frames, n_points, contact_distance, contacts_out, true);
}
