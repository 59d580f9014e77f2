// gdyn_sq.hip -- structure factors and scattering functions of a trajectory history (include/gdyn_sq.h): the Fourier amplitudes
// C = sum cos(q . x), S = sum sin(q . x) of every label at every wave vector, frame by frame, by the direct sum, and from them the
// collective and self intermediate scattering functions.  Beyond the reference, and the first kernel of this code base that is
// bound by fp64 transcendentals: beads x vectors x frames evaluations of sin and cos.
//
// The beads that take part are sorted by (label, bead index) once per (history, labels) on the host, and every label is cut into
// chunks of GD_SQ_CHUNK_BEADS beads from its first bead: a chunk belongs to one label, so no lane ever chooses an accumulator.
//
//   k_sq_chunks<T, SELF>  block = 4 waves = 4 chunks x 64 vectors: wave w takes chunk 4 blockIdx.x + w of frame (or origin)
//                    blockIdx.z, lane l the vector 64 blockIdx.y + l, its three components in registers.  The wave stages its chunk in
//                    LDS as three doubles per bead (6 KiB a wave), widened from T; with SELF the loader stores the difference of two
//                    frames instead.  Every lane then walks the chunk serially, all lanes reading one address (an LDS broadcast),
//                    and leaves the chunk's (C, S) in partial[z][chunk][C|S][vector].  The grid is (chunks / 4, vector tiles,
//                    frames): 64 vectors over 62 178 beads and one frame are already 61 blocks, so a small Q fills the device
//                    through chunks and frames, not through vectors.
//   k_sq_reduce      one lane per (frame, label, vector): adds the label's chunk partials in ascending order from +0.0.
//   k_sq_add         self part: one lane per (label, vector) adds the per-origin amplitudes of a pass, ascending, to the lag's sums.
//   k_sq_collective  one lane per (lag, a, b, vector): rho_a(t + tau) conj rho_b(t) over ascending origins.
// Frames (origins) are walked in passes of max_frames_per_pass, which bounds the partial sums held at once; a pass only decides which
// launch computes a frame, so no bit depends on it.  The history itself (upload, non-finite check) is gd::History's.
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics.  sin and cos come from one sincos:
// it is inlined, its out-pointers stay in registers (no scratch memory: profiles/sq_kernel_resources.txt) and the argument is
// reduced once, where separate calls of sin and cos reduce it twice (117 against 68 vector instructions a term on the path of small
// arguments, 219 against 124 on the Payne-Hanek path of large ones).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_sq.h"
#include "gdyn_analysis.hpp"
#include "gdyn_history.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr unsigned kWave = 64;                       // vectors of a tile: one per lane of a wave
constexpr unsigned kWaves = kBlock / kWave;          // chunks of a block
constexpr unsigned kChunk = GD_SQ_CHUNK_BEADS;
constexpr unsigned kMaxK = GD_SQ_MAX_LABELS;
constexpr size_t kPartialBytes = (size_t)256 << 20;  // automatic pass: the chunk partials of its frames fit this
constexpr unsigned kMaxPass = 65535;                 // frames of a pass: a grid dimension
constexpr unsigned kLagBatch = 32768;                // lags of one launch of k_sq_collective: a grid dimension

struct ChunkArgs {
    const void *x;                  // the history, (F, N, 3) of T
    const unsigned *order;          // the beads that take part, sorted by (label, bead)
    const uint2 *chunks;            // (first place in order, beads) of every chunk, label by label
    const double *q;                // (Q, 3)
    double *partial;                // (frames of the pass, n_chunks, 2, Q)
    unsigned N, Q, n_chunks;
    unsigned f0, stride, lag;       // block z works on frame f0 + z * stride, with SELF on the displacement from there to lag frames on
};

template <typename T, bool SELF>
__global__ void __launch_bounds__(kBlock) k_sq_chunks(ChunkArgs p)
{
    __shared__ double s_x[kWaves][kChunk * 3];
    unsigned const wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    unsigned const chunk = blockIdx.x * kWaves + wave;
    uint2 const ck = chunk < p.n_chunks ? p.chunks[chunk] : make_uint2(0u, 0u);
    size_t const f = (size_t)p.f0 + (size_t)blockIdx.z * p.stride;
    const T *xa = static_cast<const T *>(p.x) + f * p.N * 3;
    const T *xb = xa + (size_t)p.lag * p.N * 3;
    double *mine = s_x[wave];
    for (unsigned j = lane; j < ck.y; j += kWave) {
        size_t const bead = p.order[ck.x + j];
#pragma unroll
        for (unsigned k = 0; k < 3; k++) mine[3 * j + k] = SELF ? (double)xb[3 * bead + k] - (double)xa[3 * bead + k] : (double)xa[3 * bead + k];
    }
    __syncthreads();
    unsigned const qi = blockIdx.y * kWave + lane;
    bool const live = qi < p.Q;
    const double *qv = p.q + 3 * (size_t)(live ? qi : 0);
    double const qx = qv[0], qy = qv[1], qz = qv[2];
    double c = 0.0, s = 0.0;
    for (unsigned j = 0; j < ck.y; j++) {
        double const phi = ((qx * mine[3 * j]) + (qy * mine[3 * j + 1])) + qz * mine[3 * j + 2];
        double sv, cv;
        sincos(phi, &sv, &cv);
        c += cv;
        s += sv;
    }
    if (live && chunk < p.n_chunks) {
        double *out = p.partial + ((size_t)blockIdx.z * p.n_chunks + chunk) * 2 * p.Q + qi;
        out[0] = c;
        out[p.Q] = s;
    }
}

struct ReduceArgs {
    const double *partial;          // (frames, n_chunks, 2, Q)
    double *out_c, *out_s;          // (frames, K, Q) each
    unsigned frames, K, Q, n_chunks;
    unsigned chunk_first[kMaxK + 1];      // label a owns the chunks [chunk_first[a], chunk_first[a + 1])
};

__global__ void __launch_bounds__(kBlock) k_sq_reduce(ReduceArgs p)
{
    size_t const i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    size_t const plane = (size_t)p.K * p.Q;
    if (i >= plane * p.frames) return;
    unsigned const z = (unsigned)(i / plane), a = (unsigned)(i % plane / p.Q), qi = (unsigned)(i % p.Q);
    const double *mine = p.partial + (size_t)z * p.n_chunks * 2 * p.Q + qi;
    double c = 0.0, s = 0.0;
    for (unsigned ch = p.chunk_first[a]; ch < p.chunk_first[a + 1]; ch++) {
        c = c + mine[(size_t)ch * 2 * p.Q];
        s = s + mine[(size_t)ch * 2 * p.Q + p.Q];
    }
    p.out_c[i] = c;
    p.out_s[i] = s;
}

// acc[i] += amp[z, i] over the origins z of a pass, ascending
__global__ void __launch_bounds__(kBlock) k_sq_add(double *acc_c, double *acc_s, const double *amp_c, const double *amp_s, unsigned origins, unsigned plane)
{
    unsigned const i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= plane) return;
    double c = acc_c[i], s = acc_s[i];
    for (unsigned z = 0; z < origins; z++) {
        c = c + amp_c[(size_t)z * plane + i];
        s = s + amp_s[(size_t)z * plane + i];
    }
    acc_c[i] = c;
    acc_s[i] = s;
}

struct CollectiveArgs {
    const double *amp_c, *amp_s;    // (n_frames, K, Q)
    const unsigned *lags;           // the lags of this launch
    double *out_re, *out_im;        // (lags of this launch, K, K, Q)
    unsigned n_frames, stride, K, Q;
};

__global__ void __launch_bounds__(kBlock) k_sq_collective(CollectiveArgs p)
{
    unsigned const i = blockIdx.x * kBlock + threadIdx.x, cells = p.K * p.K * p.Q, plane = p.K * p.Q;
    if (i >= cells) return;
    unsigned const a = i / plane, b = i % plane / p.Q, qi = i % p.Q, lag = p.lags[blockIdx.y];
    const double *ca = p.amp_c + (size_t)lag * plane + a * p.Q + qi, *sa = p.amp_s + (size_t)lag * plane + a * p.Q + qi;
    const double *cb = p.amp_c + b * p.Q + qi, *sb = p.amp_s + b * p.Q + qi;
    double re = 0.0, im = 0.0;
    for (unsigned t = 0; t + lag < p.n_frames; t += p.stride) {
        size_t const at = (size_t)t * plane;
        double const Ca = ca[at], Sa = sa[at], Cb = cb[at], Sb = sb[at];
        re = re + ((Ca * Cb) + (Sa * Sb));
        im = im + ((Ca * Sb) - (Sa * Cb));
        if (p.n_frames - lag - t <= p.stride) break;      // t + stride would pass the window (and could wrap)
    }
    p.out_re[(size_t)blockIdx.y * cells + i] = re;
    p.out_im[(size_t)blockIdx.y * cells + i] = im;
}

}  // namespace

struct gd_sq : gd::handle {
    unsigned knob = 0;
    History hist;
    // the labels, which belong to hist.beads(), as the sorted index of the kernel
    bool have_labels = false;
    unsigned K = 1, n_chunks = 0;
    std::vector<uint64_t> members;         // beads per label
    unsigned chunk_first[kMaxK + 1] = {};
    dbuf<unsigned> order_dev;
    dbuf<uint2> chunks_dev;
    unsigned Q = 0;
    dbuf<double> q_dev;
    // per call
    dbuf<double> partial, amp, out;
    dbuf<unsigned> lags_dev;
};

namespace {

// the sorted index of `label` (NULL: one label of all beads) over N beads becomes the handle's; the handle changes only when all
// of it is on the device
int install_labels(gd_sq *h, const int32_t *label, unsigned K, unsigned N)
{
    std::vector<uint64_t> members(K, 0);
    for (unsigned i = 0; i < N; i++)
        if (!label || label[i] >= 0) members[label ? label[i] : 0]++;
    std::vector<unsigned> start(K + 1, 0), first(K + 1, 0);
    for (unsigned a = 0; a < K; a++) {
        start[a + 1] = start[a] + (unsigned)members[a];
        first[a + 1] = first[a] + (unsigned)((members[a] + kChunk - 1) / kChunk);
    }
    std::vector<unsigned> order(start[K]), at(start.begin(), start.end() - 1);
    for (unsigned i = 0; i < N; i++)
        if (!label || label[i] >= 0) order[at[label ? label[i] : 0]++] = i;
    std::vector<uint2> chunks(first[K]);
    for (unsigned a = 0; a < K; a++)
        for (unsigned c = first[a]; c < first[a + 1]; c++) {
            unsigned const begin = start[a] + (c - first[a]) * kChunk;
            chunks[c] = make_uint2(begin, std::min(kChunk, start[a + 1] - begin));
        }
    dbuf<unsigned> order_dev;
    dbuf<uint2> chunks_dev;
    HIPCHK(order_dev.upload(order.data(), order.size()));
    HIPCHK(chunks_dev.upload(chunks.data(), chunks.size()));
    h->order_dev = std::move(order_dev);
    h->chunks_dev = std::move(chunks_dev);
    h->members = std::move(members);
    h->K = K;
    h->n_chunks = first[K];
    std::copy(first.begin(), first.end(), h->chunk_first);
    h->have_labels = label != nullptr;
    return GD_OK;
}

History::Rebind rebind(gd_sq *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads() || h->members.empty()) GDCHK(install_labels(h, nullptr, 1, n_beads));      // labels belonged to another N
        return GD_OK;
    };
}

// what the three calls refuse alike
int check_window(const gd_sq *h, const char *who, uint32_t first_frame, uint32_t n_frames)
{
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (!h->Q) return fail(GD_ESTATE, "%s: no vectors set", who);
    if (n_frames == 0 || (uint64_t)first_frame + n_frames > h->hist.frames())
        return fail(GD_EINVAL, "%s: frames %u to %llu of %u", who, first_frame, (unsigned long long)first_frame + n_frames, h->hist.frames());
    return GD_OK;
}

int check_lags(const char *who, const uint32_t *lags, uint32_t n_lags, uint32_t n_frames, uint32_t origin_stride)
{
    if (!lags || !n_lags) return fail(GD_EINVAL, "%s: no lags", who);
    if (!origin_stride) return fail(GD_EINVAL, "%s: origin_stride is 0", who);
    for (unsigned k = 0; k < n_lags; k++)
        if (lags[k] >= n_frames) return fail(GD_EINVAL, "%s: lag %u of a window of %u frames", who, lags[k], n_frames);
    return GD_OK;
}

uint64_t origins_of(uint32_t n_frames, uint32_t lag, uint32_t stride) { return (uint64_t)(n_frames - 1 - lag) / stride + 1; }

// frames of a pass, and room for their chunk partials (GD_ENOMEM when not even those of one frame fit)
int plan_passes(gd_sq *h, const char *who, unsigned items, unsigned &pass)
{
    size_t const per_frame = std::max<size_t>((size_t)h->n_chunks * 2 * h->Q, 1);
    pass = h->knob ? h->knob : (unsigned)std::max<size_t>(kPartialBytes / 8 / per_frame, 1);
    pass = std::min(std::min(pass, kMaxPass), items);
    if (h->partial.ensure(per_frame * pass) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: the partial sums of %u chunks and %u vectors do not fit on the device", who, h->n_chunks, h->Q);
    }
    return GD_OK;
}

int ensure(dbuf<double> &b, size_t count, const char *who, const char *what)
{
    if (b.ensure(count) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: %s (%zu doubles) do not fit on the device", who, what, count);
    }
    return GD_OK;
}

// The amplitudes of `items` frames f0 + k * stride (self: of the displacements from there to `lag` frames on), in passes.
// add == false: out_c, out_s are (items, K, Q).  add == true: they are (K, Q) sums, to which the amplitudes are added in ascending k
// through h->amp, which holds 2 * pass planes.
int amplitudes_of(gd_sq *h, bool self, unsigned lag, unsigned f0, unsigned items, unsigned stride, unsigned pass, bool add, double *out_c, double *out_s)
{
    unsigned const plane = h->K * h->Q;
    ChunkArgs a{h->hist.x(), h->order_dev.p, h->chunks_dev.p, h->q_dev.p, h->partial.p, h->hist.beads(), h->Q, h->n_chunks, 0, stride, lag};
    ReduceArgs r{};
    r.partial = h->partial.p;
    r.K = h->K;
    r.Q = h->Q;
    r.n_chunks = h->n_chunks;
    std::copy(h->chunk_first, h->chunk_first + kMaxK + 1, r.chunk_first);
    for (unsigned z0 = 0; z0 < items; z0 += pass) {
        unsigned const m = std::min(pass, items - z0);
        a.f0 = f0 + z0 * stride;
        if (h->n_chunks) {
            dim3 const grid((h->n_chunks + kWaves - 1) / kWaves, (h->Q + kWave - 1) / kWave, m);
            bool const f64 = h->hist.is_f64;
            if (self && f64) hipLaunchKernelGGL((k_sq_chunks<double, true>), grid, dim3(kBlock), 0, h->stream, a);
            else if (self) hipLaunchKernelGGL((k_sq_chunks<float, true>), grid, dim3(kBlock), 0, h->stream, a);
            else if (f64) hipLaunchKernelGGL((k_sq_chunks<double, false>), grid, dim3(kBlock), 0, h->stream, a);
            else hipLaunchKernelGGL((k_sq_chunks<float, false>), grid, dim3(kBlock), 0, h->stream, a);
            HIPCHK(hipGetLastError());
        }
        r.frames = m;
        r.out_c = add ? h->amp.p : out_c + (size_t)z0 * plane;
        r.out_s = add ? h->amp.p + (size_t)pass * plane : out_s + (size_t)z0 * plane;
        hipLaunchKernelGGL(k_sq_reduce, dim3(blocks_for((size_t)m * plane, kBlock)), dim3(kBlock), 0, h->stream, r);
        HIPCHK(hipGetLastError());
        if (add) {
            hipLaunchKernelGGL(k_sq_add, dim3(blocks_for(plane, kBlock)), dim3(kBlock), 0, h->stream, out_c, out_s, r.out_c, r.out_s, m, plane);
            HIPCHK(hipGetLastError());
        }
    }
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_sq_abi_version(void) { return GD_SQ_ABI_VERSION; }

int gd_sq_create(const gd_sq_desc *desc, gd_sq **out)
{
    if (int rc = gd::open("gd_sq_create", desc, out)) return rc;
    (*out)->knob = desc->max_frames_per_pass;
    return GD_OK;
}

int gd_sq_destroy(gd_sq *h) { return gd::close(h); }

int gd_sq_set_history(gd_sq *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_sq_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_sq_set_history_live(gd_sq *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_sq_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_sq_set_labels(gd_sq *h, const int32_t *label, uint32_t n_labels)
{
    const char *who = "gd_sq_set_labels";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the labels are N values of its beads)", who);
    if (!label) {
        GDCHK(check_labels(who, "label", nullptr, h->hist.beads(), n_labels));
        HIPCHK(hipSetDevice(h->device));
        return install_labels(h, nullptr, 1, h->hist.beads());
    }
    if (n_labels == 0 || n_labels > kMaxK) return fail(GD_EINVAL, "%s: %u labels (1 to %u)", who, n_labels, kMaxK);
    GDCHK(check_labels(who, "label", label, h->hist.beads(), n_labels));
    HIPCHK(hipSetDevice(h->device));
    return install_labels(h, label, n_labels, h->hist.beads());
}

int gd_sq_set_vectors(gd_sq *h, const double *q, uint32_t n_vectors)
{
    const char *who = "gd_sq_set_vectors";
    if (!h || !q) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (n_vectors == 0 || n_vectors > GD_SQ_MAX_VECTORS) return fail(GD_EINVAL, "%s: %u vectors (1 to %d)", who, n_vectors, GD_SQ_MAX_VECTORS);
    for (size_t k = 0; k < 3 * (size_t)n_vectors; k++)
        if (!std::isfinite(q[k])) return fail(GD_EINVAL, "%s: component %zu of vector %zu is %g", who, k % 3, k / 3, q[k]);
    HIPCHK(hipSetDevice(h->device));
    dbuf<double> dev;
    HIPCHK(dev.upload(q, 3 * (size_t)n_vectors));
    h->q_dev = std::move(dev);
    h->Q = n_vectors;
    return GD_OK;
}

int gd_sq_amplitudes(gd_sq *h, uint32_t first_frame, uint32_t n_frames, double *cos_sum, double *sin_sum)
{
    const char *who = "gd_sq_amplitudes";
    GDCHK(check_window(h, who, first_frame, n_frames));
    if (!cos_sum || !sin_sum) return fail(GD_EINVAL, "%s: NULL argument", who);
    HIPCHK(hipSetDevice(h->device));
    size_t const total = (size_t)n_frames * h->K * h->Q;
    unsigned pass = 0;
    GDCHK(ensure(h->amp, 2 * total, who, "the outputs"));
    GDCHK(plan_passes(h, who, n_frames, pass));
    GDCHK(amplitudes_of(h, false, 0, first_frame, n_frames, 1, pass, false, h->amp.p, h->amp.p + total));
    HIPCHK(hipMemcpyAsync(cos_sum, h->amp.p, total * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(sin_sum, h->amp.p + total, total * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_sq_collective(gd_sq *h, uint32_t first_frame, uint32_t n_frames, const uint32_t *lags, uint32_t n_lags, uint32_t origin_stride, double *sum_re,
                     double *sum_im, uint64_t *count)
{
    const char *who = "gd_sq_collective";
    GDCHK(check_window(h, who, first_frame, n_frames));
    GDCHK(check_lags(who, lags, n_lags, n_frames, origin_stride));
    if (!sum_re || !sum_im || !count) return fail(GD_EINVAL, "%s: NULL argument", who);
    HIPCHK(hipSetDevice(h->device));
    size_t const total = (size_t)n_frames * h->K * h->Q, cells = (size_t)h->K * h->K * h->Q;
    unsigned pass = 0;
    GDCHK(ensure(h->amp, 2 * total, who, "the amplitudes of the window"));
    GDCHK(ensure(h->out, 2 * cells * n_lags, who, "the outputs"));
    GDCHK(plan_passes(h, who, n_frames, pass));
    HIPCHK(h->lags_dev.upload(lags, n_lags));
    GDCHK(amplitudes_of(h, false, 0, first_frame, n_frames, 1, pass, false, h->amp.p, h->amp.p + total));
    double *re = h->out.p, *im = h->out.p + cells * n_lags;
    for (unsigned l0 = 0; l0 < n_lags; l0 += kLagBatch) {
        unsigned const n = std::min(kLagBatch, n_lags - l0);
        CollectiveArgs c{h->amp.p, h->amp.p + total, h->lags_dev.p + l0, re + cells * l0, im + cells * l0, n_frames, origin_stride, h->K, h->Q};
        hipLaunchKernelGGL(k_sq_collective, dim3(blocks_for(cells, kBlock), n), dim3(kBlock), 0, h->stream, c);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(sum_re, re, cells * n_lags * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(sum_im, im, cells * n_lags * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (unsigned k = 0; k < n_lags; k++) count[k] = origins_of(n_frames, lags[k], origin_stride);
    return GD_OK;
}

int gd_sq_self(gd_sq *h, uint32_t first_frame, uint32_t n_frames, const uint32_t *lags, uint32_t n_lags, uint32_t origin_stride, double *cos_sum,
               double *sin_sum, uint64_t *count)
{
    const char *who = "gd_sq_self";
    GDCHK(check_window(h, who, first_frame, n_frames));
    GDCHK(check_lags(who, lags, n_lags, n_frames, origin_stride));
    if (!cos_sum || !sin_sum || !count) return fail(GD_EINVAL, "%s: NULL argument", who);
    HIPCHK(hipSetDevice(h->device));
    size_t const plane = (size_t)h->K * h->Q;
    unsigned pass = 0;
    GDCHK(plan_passes(h, who, n_frames, pass));
    GDCHK(ensure(h->amp, 2 * plane * pass, who, "the amplitudes of a pass"));
    GDCHK(ensure(h->out, 2 * plane * n_lags, who, "the outputs"));
    HIPCHK(hipMemsetAsync(h->out.p, 0, 2 * plane * n_lags * 8, h->stream));      // +0.0
    double *c = h->out.p, *s = h->out.p + plane * n_lags;
    for (unsigned k = 0; k < n_lags; k++) {
        uint64_t const origins = origins_of(n_frames, lags[k], origin_stride);
        GDCHK(amplitudes_of(h, true, lags[k], first_frame, (unsigned)origins, origin_stride, pass, true, c + plane * k, s + plane * k));
        for (unsigned a = 0; a < h->K; a++) count[(size_t)k * h->K + a] = origins * h->members[a];
    }
    HIPCHK(hipMemcpyAsync(cos_sum, c, plane * n_lags * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(sin_sum, s, plane * n_lags * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

}  // extern "C"
