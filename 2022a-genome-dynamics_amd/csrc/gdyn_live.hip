// gdyn_live.hip -- the bridge of include/gdyn_live.h: the device analyses fed from a running stepper's device-resident state.
// It checks that the two handles of a call fit each other and joins the seams of gdyn_live.hpp: the stepper hands out its contact
// tables or its positions in bead order with its stream idle, and the analysis runs its own kernels on them on its own
// stream (k_cmap_accumulate_tab in gdyn_cmap.hip; the distance, contact and pair-count kernels of gdyn_lamina.hip and
// gdyn_rdf.hip, which take the frames from device memory).  Every call returns with the analysis stream idle too, so the
// next gd_run finds the buffers unread.
//
// The flow analyses need a history, which gd_live_history records here.  Both of its kernels are pure
// streaming, one coalesced pass each, 128-bit accesses when the 3 N floats of a frame are a multiple of four (every frame of
// every slot then starts on 16 bytes), plain 32-bit ones otherwise:
//   k_history_record   the frames of the selected replicas from the stepper's (R, N, 3) float32 buffer into their slots of a block
//   k_history_widen    the frames of one slot from a block into the (F, N, 3) fp64 copy of a gd_flow handle; the lowest index of
//                      a non-finite coordinate goes to one flag (atomicMin, reached by no lane of a finite history)
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/gdyn_live.h"
#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"

using namespace gd;

namespace {

int same_device(const char *who, const gd_live_shape &v, int device)
{
    if (v.device != device) return fail(GD_EINVAL, "%s: the system is on device %d, the analysis handle on device %d", who, v.device, device);
    return GD_OK;
}

// the semiaxes gd_get_context reports, replica by replica
int wall_semiaxes(gd_system *sys, const gd_live_shape &v, std::vector<double> &semiaxes)
{
    semiaxes.resize((size_t)v.R * 3);
    for (uint32_t r = 0; r < v.R; r++) {
        gd_context c;
        if (int rc = gd_get_context(sys, r, &c)) return rc;
        for (int k = 0; k < 3; k++) semiaxes[3 * (size_t)r + k] = c.semiaxes[k];
    }
    return GD_OK;
}

int lamina_frames(const char *who, gd_system *sys, gd_lamina *lam, int quantize, gd_live_shape *v, std::vector<double> &semiaxes, const float **xyz)
{
    if (!sys || !lam) return fail(GD_EINVAL, "%s: NULL handle", who);
    *v = gd_live_shape_of(sys);
    if (int rc = same_device(who, *v, gd_lamina_device(lam))) return rc;
    if (!v->has_wall) return fail(GD_EINVAL, "%s: the system has no ellipsoid wall", who);
    if (int rc = wall_semiaxes(sys, *v, semiaxes)) return rc;
    return gd_live_positions(sys, quantize, xyz);
}

constexpr int kBlock = 256;
constexpr unsigned long long kNoBadIndex = ~0ull;

// slot s of dst <- replica ids[s] of src (ids == NULL: replica s), m elements of T each
template <typename T>
__global__ void __launch_bounds__(kBlock) k_history_record(const T *__restrict__ src, const uint32_t *__restrict__ ids, T *__restrict__ dst,
                                                           size_t m, unsigned slots)
{
    for (unsigned s = blockIdx.y; s < slots; s += gridDim.y) {
        const T *from = src + (size_t)(ids ? ids[s] : s) * m;
        T *to = dst + (size_t)s * m;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) to[i] = from[i];
    }
}

__device__ inline bool finite4(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }

// frame f of dst (M doubles each) <- src + f * stride, widened; base: the index of dst[0] in the whole history.  VEC: M, stride and
// the offsets of src and dst are multiples of four elements.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_history_widen(const float *__restrict__ src, size_t stride, unsigned frames, double *__restrict__ dst,
                                                          size_t M, unsigned long long base, unsigned long long *first_bad)
{
    unsigned long long bad = kNoBadIndex;
    for (unsigned f = blockIdx.y; f < frames; f += gridDim.y) {
        const float *from = src + (size_t)f * stride;
        double *to = dst + (size_t)f * M;
        size_t const i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
        if (VEC) {
            for (size_t q = i0; q < M / 4; q += step) {
                float4 const v = reinterpret_cast<const float4 *>(from)[q];
                reinterpret_cast<double2 *>(to)[2 * q] = make_double2((double)v.x, (double)v.y);
                reinterpret_cast<double2 *>(to)[2 * q + 1] = make_double2((double)v.z, (double)v.w);
                if (!finite4(v)) {
                    unsigned long long const at = base + (unsigned long long)f * M + 4 * q;
                    unsigned long long const k = !isfinite(v.x) ? 0 : !isfinite(v.y) ? 1 : !isfinite(v.z) ? 2 : 3;
                    bad = min(bad, at + k);
                }
            }
        } else {
            for (size_t i = i0; i < M; i += step) {
                float const v = from[i];
                to[i] = (double)v;
                if (!isfinite(v)) bad = min(bad, base + (unsigned long long)f * M + i);
            }
        }
    }
    if (bad != kNoBadIndex) atomicMin(first_bad, bad);
}

unsigned stream_blocks(size_t n) { return (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 4096); }

struct device_of {
    int device;
};

}  // namespace

struct gd_live_history : gd::handle {
    uint32_t N = 0, R = 0;
    uint32_t slots = 0;                  // recorded replicas
    std::vector<uint32_t> ids;           // their ids, slot by slot; empty: all R, slot r = replica r
    dbuf<uint32_t> ids_dev;
    uint32_t frames_per_block = 0, frames = 0;
    std::vector<dbuf<float>> blocks;     // (frames_per_block, slots, N, 3) each; a block is never reallocated
    dbuf<unsigned long long> first_bad;

    size_t frame_floats() const { return (size_t)N * 3; }
    bool vec() const { return frame_floats() % 4 == 0; }
    const float *frame(uint32_t f, uint32_t slot) const
    {
        return blocks[f / frames_per_block].p + ((size_t)(f % frames_per_block) * slots + slot) * frame_floats();
    }
    int slot_of(const char *who, uint32_t replica, uint32_t *slot) const
    {
        if (ids.empty() && replica < R) {
            *slot = replica;
            return GD_OK;
        }
        for (uint32_t s = 0; s < ids.size(); s++)
            if (ids[s] == replica) {
                *slot = s;
                return GD_OK;
            }
        return fail(GD_EINVAL, "%s: replica %u is not recorded", who, replica);
    }
};

// ---- the seams of an analysis that reads the blocks itself (gdyn_live.hpp)
gd_live_history_shape gd_live_history_shape_of(const gd_live_history *h)
{
    return {h->device, h->N, h->frames, h->frames_per_block, (size_t)h->slots * h->frame_floats()};
}

int gd_live_history_slot(const gd_live_history *h, const char *who, uint32_t replica, uint32_t *slot) { return h->slot_of(who, replica, slot); }

const float *gd_live_history_frame(const gd_live_history *h, uint32_t f, uint32_t slot) { return h->frame(f, slot); }

extern "C" {

int gd_live_abi_version(void) { return GD_LIVE_ABI_VERSION; }

int gd_live_contacts(gd_system *sys, uint32_t replica, gd_cmap *cm)
{
    if (!sys || !cm) return fail(GD_EINVAL, "gd_live_contacts: NULL handle");
    gd_live_shape const v = gd_live_shape_of(sys);
    if (replica != GD_ALL_REPLICAS && replica >= v.R) return fail(GD_EINVAL, "gd_live_contacts: replica %u of %u", replica, v.R);
    if (int rc = same_device("gd_live_contacts", v, gd_cmap_device(cm))) return rc;
    ContactTab tab;
    const unsigned *occupancy = nullptr;
    if (int rc = gd_live_contact_tab(sys, &tab, &occupancy)) return rc;
    if (tab.cap == 0) return GD_OK;                          // never updated
    uint32_t const r0 = replica == GD_ALL_REPLICAS ? 0 : replica, nr = replica == GD_ALL_REPLICAS ? v.R : 1;
    uint64_t rows = 0;
    for (uint32_t r = r0; r < r0 + nr; r++) rows += occupancy[r];
    return gd_cmap_accumulate_tab(cm, "gd_live_contacts", tab, r0, nr, rows);
}

int gd_live_lamina_distances(gd_system *sys, gd_lamina *lam, int quantize, void *out, int out_is_f64)
{
    gd_live_shape v;
    std::vector<double> semiaxes;
    const float *xyz = nullptr;
    if (int rc = lamina_frames("gd_live_lamina_distances", sys, lam, quantize, &v, semiaxes, &xyz)) return rc;
    return gd_lamina_distances_dev(lam, "gd_live_lamina_distances", xyz, v.R, v.N, semiaxes.data(), out, out_is_f64);
}

int gd_live_lamina_contacts(gd_system *sys, gd_lamina *lam, int quantize, double contact_distance, uint8_t *contacts_out)
{
    gd_live_shape v;
    std::vector<double> semiaxes;
    const float *xyz = nullptr;
    if (int rc = lamina_frames("gd_live_lamina_contacts", sys, lam, quantize, &v, semiaxes, &xyz)) return rc;
    return gd_lamina_contacts_dev(lam, "gd_live_lamina_contacts", xyz, v.R, v.N, semiaxes.data(), contact_distance, contacts_out);
}

int gd_live_rdf_counts(gd_system *sys, gd_rdf *rdf, int quantize, double bin_width, double max_distance, uint64_t *counts_out)
{
    if (!sys || !rdf) return fail(GD_EINVAL, "gd_live_rdf_counts: NULL handle");
    gd_live_shape const v = gd_live_shape_of(sys);
    if (int rc = same_device("gd_live_rdf_counts", v, gd_rdf_device(rdf))) return rc;
    if (!v.periodic) return fail(GD_EINVAL, "gd_live_rdf_counts: the system's box is open");
    const float *xyz = nullptr;
    if (int rc = gd_live_positions(sys, quantize, &xyz)) return rc;
    return gd_rdf_counts_dev(rdf, "gd_live_rdf_counts", xyz, v.R, v.N, v.box, bin_width, max_distance, counts_out);
}

int gd_live_history_create(gd_system *sys, const uint32_t *replicas, uint32_t n_replicas, uint32_t frames_per_block, gd_live_history **out)
{
    if (!sys || !out || (n_replicas && !replicas)) return fail(GD_EINVAL, "gd_live_history_create: NULL argument");
    *out = nullptr;
    gd_live_shape const v = gd_live_shape_of(sys);
    std::vector<bool> seen(v.R, false);
    for (uint32_t k = 0; k < n_replicas; k++) {
        if (replicas[k] >= v.R) return fail(GD_EINVAL, "gd_live_history_create: replica %u of %u", replicas[k], v.R);
        if (seen[replicas[k]]) return fail(GD_EINVAL, "gd_live_history_create: replica %u is listed twice", replicas[k]);
        seen[replicas[k]] = true;
    }
    device_of const desc{v.device};
    gd_live_history *h = nullptr;
    if (int rc = gd::open("gd_live_history_create", &desc, &h)) return rc;
    h->N = v.N;
    h->R = v.R;
    h->slots = n_replicas ? n_replicas : v.R;
    h->ids.assign(replicas, replicas + n_replicas);
    size_t const frame_bytes = (size_t)h->slots * h->frame_floats() * sizeof(float);
    h->frames_per_block = frames_per_block ? frames_per_block : (uint32_t)std::min<size_t>(std::max<size_t>(((size_t)256 << 20) / frame_bytes, 1), 1u << 30);
    hipError_t e = n_replicas ? h->ids_dev.upload(replicas, n_replicas) : hipSuccess;
    if (e == hipSuccess) e = h->first_bad.ensure(1);
    if (e != hipSuccess) {
        gd::close(h);
        return fail(GD_EHIP, "gd_live_history_create: %s", hipGetErrorString(e));
    }
    *out = h;
    return GD_OK;
}

int gd_live_history_destroy(gd_live_history *h) { return gd::close(h); }

int gd_live_history_record(gd_live_history *h, gd_system *sys, int quantize)
{
    if (!h || !sys) return fail(GD_EINVAL, "gd_live_history_record: NULL handle");
    gd_live_shape const v = gd_live_shape_of(sys);
    if (v.device != h->device) return fail(GD_EINVAL, "gd_live_history_record: the system is on device %d, the recorder on device %d", v.device, h->device);
    if (v.N != h->N || v.R != h->R)
        return fail(GD_EINVAL, "gd_live_history_record: a system of %u replicas of %u beads, the recorder was created for %u of %u", v.R, v.N, h->R, h->N);
    if (h->frames == UINT32_MAX) return fail(GD_EINVAL, "gd_live_history_record: the recorder is full");
    HIPCHK(hipSetDevice(h->device));
    size_t const b = h->frames / h->frames_per_block, block_floats = (size_t)h->frames_per_block * h->slots * h->frame_floats();
    if (b == h->blocks.size()) {      // a new block; the earlier ones stay where they are
        dbuf<float> block;
        hipError_t const e = block.ensure(block_floats);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e == hipErrorOutOfMemory)
            return fail(GD_ENOMEM, "gd_live_history_record: no device memory for block %zu of %zu bytes (%u frames are recorded)", b,
                        block_floats * sizeof(float), h->frames);
        HIPCHK(e);
        h->blocks.push_back(std::move(block));
    }
    const float *xyz = nullptr;
    if (int rc = gd_live_positions(sys, quantize, &xyz)) return rc;
    float *dst = const_cast<float *>(h->frame(h->frames, 0));
    // all replicas: the (R, N, 3) buffer is one slot; a selection: one slot per replica
    bool const all = h->ids.empty();
    size_t const m = all ? (size_t)h->R * h->frame_floats() : h->frame_floats();
    unsigned const slots = all ? 1 : h->slots;
    const uint32_t *ids = all ? nullptr : h->ids_dev.p;
    if (h->vec())
        hipLaunchKernelGGL(k_history_record<float4>, dim3(stream_blocks(m / 4), std::min(slots, 65535u)), dim3(kBlock), 0, h->stream,
                           reinterpret_cast<const float4 *>(xyz), ids, reinterpret_cast<float4 *>(dst), m / 4, slots);
    else
        hipLaunchKernelGGL(k_history_record<float>, dim3(stream_blocks(m), std::min(slots, 65535u)), dim3(kBlock), 0, h->stream, xyz, ids, dst, m, slots);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->frames++;
    return GD_OK;
}

int gd_live_history_frames(const gd_live_history *h, uint32_t *frames)
{
    if (!h || !frames) return fail(GD_EINVAL, "gd_live_history_frames: NULL argument");
    *frames = h->frames;
    return GD_OK;
}

int gd_live_history_fetch(gd_live_history *h, uint32_t replica, uint32_t first, uint32_t count, float *out)
{
    if (!h || (!out && count)) return fail(GD_EINVAL, "gd_live_history_fetch: NULL argument");
    uint32_t slot = 0;
    if (int rc = h->slot_of("gd_live_history_fetch", replica, &slot)) return rc;
    if ((uint64_t)first + count > h->frames)
        return fail(GD_EINVAL, "gd_live_history_fetch: frames %u to %llu of %u recorded", first, (unsigned long long)first + count, h->frames);
    HIPCHK(hipSetDevice(h->device));
    for (uint32_t k = 0; k < count; k++)
        HIPCHK(hipMemcpyAsync(out + (size_t)k * h->frame_floats(), h->frame(first + k, slot), h->frame_floats() * sizeof(float), hipMemcpyDeviceToHost,
                              h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_live_history_clear(gd_live_history *h)
{
    if (!h) return fail(GD_EINVAL, "gd_live_history_clear: NULL handle");
    h->frames = 0;
    return GD_OK;
}

int gd_live_flow_set_history(gd_live_history *h, uint32_t replica, gd_flow *flow)
{
    const char *who = "gd_live_flow_set_history";
    if (!h || !flow) return fail(GD_EINVAL, "%s: NULL handle", who);
    uint32_t slot = 0;
    if (int rc = h->slot_of(who, replica, &slot)) return rc;
    if (gd_flow_device(flow) != h->device)
        return fail(GD_EINVAL, "%s: the recorder is on device %d, the analysis handle on device %d", who, h->device, gd_flow_device(flow));
    if (!h->frames) return fail(GD_ESTATE, "%s: no frame recorded", who);
    double *x = nullptr;
    hipStream_t st = nullptr;
    if (int rc = gd_flow_history_begin(flow, who, h->frames, h->N, &x, &st)) return rc;
    size_t const M = h->frame_floats(), stride = (size_t)h->slots * M;
    HIPCHK(hipMemsetAsync(h->first_bad.p, 0xff, sizeof(unsigned long long), st));
    for (uint32_t f0 = 0; f0 < h->frames; f0 += h->frames_per_block) {      // one launch per block
        unsigned const nf = std::min(h->frames_per_block, h->frames - f0);
        dim3 const grid(stream_blocks(h->vec() ? M / 4 : M), std::min(nf, 65535u));
        if (h->vec())
            hipLaunchKernelGGL(k_history_widen<true>, grid, dim3(kBlock), 0, st, h->frame(f0, slot), stride, nf, x + (size_t)f0 * M, M,
                               (unsigned long long)f0 * M, h->first_bad.p);
        else
            hipLaunchKernelGGL(k_history_widen<false>, grid, dim3(kBlock), 0, st, h->frame(f0, slot), stride, nf, x + (size_t)f0 * M, M,
                               (unsigned long long)f0 * M, h->first_bad.p);
    }
    HIPCHK(hipGetLastError());
    unsigned long long bad = kNoBadIndex;
    HIPCHK(hipMemcpyAsync(&bad, h->first_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    gd_flow_history_end(flow, h->frames, h->N, bad == kNoBadIndex);
    if (bad != kNoBadIndex) return fail(GD_EINVAL, "%s: non-finite coordinate at %llu", who, bad);
    return GD_OK;
}

}  // extern "C"
