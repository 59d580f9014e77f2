// gdyn_msd.hip -- the lag statistics of a trajectory history (include/gdyn_msd.h): MSD(tau) along the frame axis and R2(s) along
// the chains, one kernel family for both.  Beyond the reference, which has neither.
//
// A *sequence* is a run of items (3 coordinates each) a fixed stride apart: along time one bead's trajectory (item stride 3 N
// elements, neighbouring beads 3 elements apart), along the chain one chain in one frame (item stride 3, the same chain in the
// next frame 3 N elements on).  A *tile* is kSeqs = 16 sequences that lie side by side: 16 consecutive beads, or one chain in 16
// consecutive frames of the window.  The walk over the windows of a tile is gdyn_lagwalk.hpp's, which van Hove's self part shares.
//
//   k_msd_lag<T>     one block per (tile, origin range of kRange = 4096 origins): the lag walk with the body LagSums.  Lane =
//                    (sequence, lag), 16 x 64 per block, so the 16 lanes of a lag read items 3 elements apart (conflict-free) and run
//                    the same trip count.  Every (sequence, lag, range) sum is ONE lane's serial sum over ascending origins, carried
//                    from window pair to window pair in its slot of `partial` (always the same lane's): no bit depends on W.
//   k_msd_reduce1/2  the sums of a group: per fixed chunk of 256 sequences, serially over ascending sequences (each the serial sum
//                    of its ranges), then serially over the chunks.  The order depends on the shapes alone.
//   k_msd_per_seq    gd_msd_time_per_bead: the serial sum of a sequence's ranges.
// The history itself (upload, non-finite check) is gd::History's (gdyn_history.hpp).
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_msd.h"
#include "gdyn_analysis.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"
#include "gdyn_lagwalk.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr unsigned kChunk = 256;             // sequences of one serial group sum: fixed, like kRange, so that the order of summation is
constexpr size_t kPartialBytes = (size_t)1 << 30;      // lags are evaluated in batches whose partial sums fit this

struct LagArgs {
    const void *x;                  // the history, (F, N, 3) of T
    const uint32_t *chains;         // (C, 2) on the device: along the chain; NULL: along time
    const uint32_t *lags;           // ascending
    double2 *partial;               // (ranges, sequences, lags): (sum of t2, sum of t4)
    unsigned N, F, C;
    unsigned f0, nf, ftiles;        // along the chain: the frame window and its tiles of kSeqs frames
    unsigned n_lags, W, windows;    // W items per window; windows: 1 (the longest sequence fits in one) or 2
    size_t n_seqs;
};

// The body of the lag walk: lane = (sequence, lag slot).  Lag k is always the same lane's, and its sum over the origins of a window pair
// goes on serially from where the last pair left it in `mine`.
template <typename T>
struct LagSums {
    const uint32_t *lags;
    double2 *mine;      // this lane's sequence's row of `partial` in this range
    unsigned s, slot, valid;

    __device__ bool wants(long long, long long) const { return true; }
    __device__ void operator()(const LagPair &w, const T *A, const T *Bw) const
    {
        if (s < valid)
            for (unsigned k = w.lo / kSlots * kSlots + slot; k < w.hi; k += kSlots) {      // lag k is always this lane's
                if (k < w.lo) continue;
                long long const shift = (long long)lags[k] - w.d * w.W;      // partner's place in B = origin's place in A + shift
                long long const r0 = max(0ll, -shift), r1 = min(w.nO, w.nB - shift);
                if (r1 <= r0) continue;
                const T *pa = A + r0 * kRow + 3 * s, *pb = Bw + (r0 + shift) * kRow + 3 * s;
                double2 acc = mine[k];
#pragma unroll 4
                for (long long r = r0; r < r1; r++, pa += kRow, pb += kRow) {
                    double const dx = (double)pb[0] - (double)pa[0], dy = (double)pb[1] - (double)pa[1], dz = (double)pb[2] - (double)pa[2];
                    double const t2 = (dx * dx + dy * dy) + dz * dz;
                    acc.x += t2;
                    acc.y += t2 * t2;
                }
                mine[k] = acc;
            }
    }
};

template <typename T>
__global__ void __launch_bounds__(kLagBlock) k_msd_lag(LagArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *A = reinterpret_cast<T *>(smem);
    T *B = A + (size_t)(p.windows - 1) * p.W * kRow;      // one window: partners lie in A

    // the tile: where its sequences lie, how long they are, and which rows of `partial` are theirs
    LagTile t;
    size_t q0, q_stride;
    if (p.chains) {
        unsigned const c = blockIdx.x / p.ftiles, ft = blockIdx.x % p.ftiles;
        unsigned const start = p.chains[2 * c];
        t.L = p.chains[2 * c + 1] - start;
        t.base = ((size_t)p.f0 + (size_t)ft * kSeqs) * p.N * 3 + (size_t)start * 3;
        t.seq_stride = (size_t)p.N * 3;
        t.item_stride = 3;
        t.valid = min(kSeqs, p.nf - ft * kSeqs);
        q0 = (size_t)ft * kSeqs * p.C + c;
        q_stride = p.C;
    } else {
        t.L = p.F;
        t.base = (size_t)blockIdx.x * kSeqs * 3;
        t.seq_stride = 3;
        t.item_stride = (size_t)p.N * 3;
        t.valid = min(kSeqs, p.N - blockIdx.x * kSeqs);
        q0 = (size_t)blockIdx.x * kSeqs;
        q_stride = 1;
    }
    unsigned const s = threadIdx.x % kSeqs, slot = threadIdx.x / kSeqs;
    if (t.L < 2) return;
    unsigned const ranges = (t.L - 1 + kRange - 1) / kRange;      // origins 0 .. L-2
    for (unsigned g = blockIdx.y; g < ranges; g += gridDim.y) {
        long long const O0 = (long long)g * kRange, O1 = min(O0 + (long long)kRange, (long long)t.L - 1);
        LagSums<T> body{p.lags, p.partial + ((size_t)g * p.n_seqs + q0 + (size_t)s * q_stride) * p.n_lags, s, slot, t.valid};
        lag_walk(static_cast<const T *>(p.x), t, p.lags, p.n_lags, (long long)p.W, O0, O1, A, B, body);
    }
}

// how a sequence's group is found: gmod > 0: q % gmod; else group[q] (NULL: group 0)
struct GroupMap {
    const int32_t *group;
    unsigned gmod;
};

__device__ inline double2 sum_ranges(const double2 *__restrict__ partial, unsigned ranges, size_t n_seqs, unsigned n_lags, size_t q, unsigned k)
{
    double2 r = partial[q * n_lags + k];
    for (unsigned g = 1; g < ranges; g++) {
        double2 const v = partial[((size_t)g * n_seqs + q) * n_lags + k];
        r.x += v.x;
        r.y += v.y;
    }
    return r;
}

// tmp[chunk][group][lag]: the sums of the chunk's sequences of a group, in ascending order
__global__ void __launch_bounds__(kBlock) k_msd_reduce1(const double2 *__restrict__ partial, unsigned ranges, size_t n_seqs, unsigned n_lags,
                                                        GroupMap m, unsigned G, double2 *__restrict__ tmp)
{
    size_t const q0 = (size_t)blockIdx.x * kChunk, q1 = min(q0 + kChunk, n_seqs);
    size_t const tasks = (size_t)G * n_lags;
    for (size_t e = threadIdx.x; e < tasks; e += kBlock) {
        unsigned const grp = (unsigned)(e / n_lags), k = (unsigned)(e % n_lags);
        double2 acc = make_double2(0.0, 0.0);
        if (m.gmod) {
            size_t q = q0 + (grp + m.gmod - q0 % m.gmod) % m.gmod;
            for (; q < q1; q += m.gmod) {
                double2 const v = sum_ranges(partial, ranges, n_seqs, n_lags, q, k);
                acc.x += v.x;
                acc.y += v.y;
            }
        } else {
            for (size_t q = q0; q < q1; q++) {
                if ((m.group ? m.group[q] : 0) != (int)grp) continue;
                double2 const v = sum_ranges(partial, ranges, n_seqs, n_lags, q, k);
                acc.x += v.x;
                acc.y += v.y;
            }
        }
        tmp[(size_t)blockIdx.x * tasks + e] = acc;
    }
}

__global__ void __launch_bounds__(kBlock) k_msd_reduce2(const double2 *__restrict__ tmp, unsigned chunks, size_t tasks, double2 *__restrict__ out)
{
    size_t const e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= tasks) return;
    double2 acc = tmp[e];
    for (unsigned c = 1; c < chunks; c++) {
        double2 const v = tmp[(size_t)c * tasks + e];
        acc.x += v.x;
        acc.y += v.y;
    }
    out[e] = acc;
}

__global__ void __launch_bounds__(kBlock) k_msd_per_seq(const double2 *__restrict__ partial, unsigned ranges, size_t n_seqs, double2 *__restrict__ out)
{
    size_t const q = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (q < n_seqs) out[q] = sum_ranges(partial, ranges, n_seqs, 1, q, 0);
}

// the dynamic LDS a block of k_msd_lag may ask for (gd::lds_opt_in).  A refusal only makes the windows smaller.
int lds_budget(int device)
{
    static DeviceOnce<> once;
    return lds_opt_in(once, device, {reinterpret_cast<const void *>(&k_msd_lag<float>), reinterpret_cast<const void *>(&k_msd_lag<double>)});
}

}  // namespace

struct gd_msd : gd::handle {
    unsigned knob = 0;
    int lds_bytes = 64 * 1024;
    History hist;
    // groups and chains, which belong to hist.beads()
    unsigned G = 1;
    bool have_groups = false;      // false: one group of all beads
    std::vector<int32_t> group;
    dbuf<int32_t> group_dev;
    std::vector<uint32_t> chains;  // (C, 2)
    dbuf<uint32_t> chains_dev;
    // per call
    dbuf<uint32_t> lags_dev;
    dbuf<double2> partial, tmp, out;
};

namespace {

History::Rebind rebind(gd_msd *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads()) {      // groups and chains belonged to another N
            h->have_groups = false;
            h->G = 1;
            h->group.clear();
            h->chains.clear();
        }
        return GD_OK;
    };
}

// lags: distinct and >= 1; order: their indices by ascending lag
int check_lags(const char *who, const char *what, const uint32_t *lags, uint32_t n, std::vector<uint32_t> &order)
{
    LagOrder lo = sort_lags(lags, n);
    if (lo.least == 0) return fail(GD_EINVAL, "%s: %s 0", who, what);
    if (lo.twice) return fail(GD_EINVAL, "%s: %s %u is listed twice", who, what, lo.repeated);
    order = std::move(lo.order);
    return GD_OK;
}

struct Plan {      // one axis of one call
    bool along_chain;
    unsigned f0, nf, ftiles;
    size_t n_seqs, tiles;
    unsigned longest;      // items of the longest sequence
    unsigned ranges;
};

// evaluates the sorted lags [k0, k0 + nl) into h->partial ((ranges, n_seqs, nl), zero where nothing is summed)
int run_lags(gd_msd *h, const Plan &pl, const uint32_t *sorted_lags_dev, unsigned nl)
{
    size_t const row = (size_t)kRow * h->hist.elem();
    LagWindows const lw = lag_windows((size_t)h->lds_bytes, 0, row, pl.longest, h->knob);
    size_t const cells = (size_t)pl.ranges * pl.n_seqs * nl;
    HIPCHK(h->partial.ensure(cells));
    HIPCHK(hipMemsetAsync(h->partial.p, 0, cells * sizeof(double2), h->stream));
    LagArgs a;
    a.x = h->hist.x();
    a.chains = pl.along_chain ? h->chains_dev.p : nullptr;
    a.lags = sorted_lags_dev;
    a.partial = h->partial.p;
    a.N = h->hist.beads();
    a.F = h->hist.frames();
    a.C = (unsigned)(h->chains.size() / 2);
    a.f0 = pl.f0;
    a.nf = pl.nf;
    a.ftiles = pl.ftiles;
    a.n_lags = nl;
    a.W = lw.W;
    a.windows = lw.windows;
    a.n_seqs = pl.n_seqs;
    dim3 const grid((unsigned)pl.tiles, std::min(pl.ranges, 65535u));
    size_t const lds = (size_t)lw.windows * lw.W * row;
    if (h->hist.is_f64) hipLaunchKernelGGL(k_msd_lag<double>, grid, dim3(kLagBlock), lds, h->stream, a);
    else hipLaunchKernelGGL(k_msd_lag<float>, grid, dim3(kLagBlock), lds, h->stream, a);
    HIPCHK(hipGetLastError());
    return GD_OK;
}

// the group sums of every lag of `lags` (in the caller's order) along one axis: sum2 / sum4 (G, n) on the host
int group_sums(gd_msd *h, const Plan &pl, const uint32_t *lags, const std::vector<uint32_t> &order, GroupMap m, unsigned G, double *sum2, double *sum4)
{
    unsigned const n = (unsigned)order.size();
    std::vector<uint32_t> sorted(n);
    for (unsigned k = 0; k < n; k++) sorted[k] = lags[order[k]];
    HIPCHK(h->lags_dev.upload(sorted.data(), n));
    size_t const per_lag = (size_t)pl.ranges * pl.n_seqs * sizeof(double2);
    unsigned const batch = (unsigned)std::min<size_t>(std::max<size_t>(kPartialBytes / std::max<size_t>(per_lag, 1), 1), n);
    unsigned const chunks = (unsigned)((pl.n_seqs + kChunk - 1) / kChunk);
    std::vector<double2> host;
    for (unsigned k0 = 0; k0 < n; k0 += batch) {
        unsigned const nl = std::min(batch, n - k0);
        if (int rc = run_lags(h, pl, h->lags_dev.p + k0, nl)) return rc;
        size_t const tasks = (size_t)G * nl;
        HIPCHK(h->tmp.ensure((size_t)chunks * tasks));
        HIPCHK(h->out.ensure(tasks));
        hipLaunchKernelGGL(k_msd_reduce1, dim3(chunks), dim3(kBlock), 0, h->stream, h->partial.p, pl.ranges, pl.n_seqs, nl, m, G, h->tmp.p);
        hipLaunchKernelGGL(k_msd_reduce2, dim3(blocks_for(tasks, kBlock)), dim3(kBlock), 0, h->stream, h->tmp.p, chunks, tasks, h->out.p);
        HIPCHK(hipGetLastError());
        host.resize(tasks);
        HIPCHK(hipMemcpyAsync(host.data(), h->out.p, tasks * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (unsigned g = 0; g < G; g++)
            for (unsigned k = 0; k < nl; k++) {
                size_t const at = (size_t)g * n + order[k0 + k];
                sum2[at] = host[(size_t)g * nl + k].x;
                if (sum4) sum4[at] = host[(size_t)g * nl + k].y;
            }
    }
    return GD_OK;
}

Plan time_plan(const gd_msd *h)
{
    Plan pl{};
    pl.along_chain = false;
    pl.n_seqs = h->hist.beads();
    pl.tiles = (h->hist.beads() + kSeqs - 1) / kSeqs;
    pl.longest = h->hist.frames();
    pl.ranges = h->hist.frames() > 1 ? (h->hist.frames() - 1 + kRange - 1) / kRange : 1;
    return pl;
}

}  // namespace

extern "C" {

int gd_msd_abi_version(void) { return GD_MSD_ABI_VERSION; }

int gd_msd_create(const gd_msd_desc *desc, gd_msd **out)
{
    if (int rc = gd::open("gd_msd_create", desc, out)) return rc;
    (*out)->knob = desc->max_items_per_tile;
    (*out)->lds_bytes = lds_budget(desc->device);
    return GD_OK;
}

int gd_msd_destroy(gd_msd *h) { return gd::close(h); }

int gd_msd_set_history(gd_msd *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_msd_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_msd_set_history_live(gd_msd *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_msd_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_msd_set_groups(gd_msd *h, const int32_t *group, uint32_t n_groups)
{
    const char *who = "gd_msd_set_groups";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the groups are N values of its beads)", who);
    if (!group) {
        GDCHK(check_labels(who, "group", nullptr, h->hist.beads(), n_groups));
        h->have_groups = false;
        h->G = 1;
        h->group.clear();
        return GD_OK;
    }
    if (n_groups == 0 || n_groups > (1u << 20)) return fail(GD_EINVAL, "%s: %u groups (1 to 2^20)", who, n_groups);
    GDCHK(check_labels(who, "group", group, h->hist.beads(), n_groups));
    HIPCHK(hipSetDevice(h->device));
    dbuf<int32_t> dev;
    HIPCHK(dev.upload(group, h->hist.beads()));
    h->group_dev = std::move(dev);
    h->group.assign(group, group + h->hist.beads());
    h->G = n_groups;
    h->have_groups = true;
    return GD_OK;
}

int gd_msd_set_chains(gd_msd *h, const uint32_t *ranges, uint32_t n_chains)
{
    const char *who = "gd_msd_set_chains";
    if (!h || (!ranges && n_chains)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the chains are ranges of its beads)", who);
    if (n_chains > (1u << 24)) return fail(GD_EINVAL, "%s: %u chains exceed 2^24", who, n_chains);
    if (int rc = check_ranges(who, "chain", true, ranges, n_chains, h->hist.beads())) return rc;
    HIPCHK(hipSetDevice(h->device));
    dbuf<uint32_t> dev;
    HIPCHK(dev.upload(ranges, 2 * (size_t)n_chains));
    h->chains_dev = std::move(dev);
    h->chains.assign(ranges, ranges + 2 * (size_t)n_chains);
    return GD_OK;
}

int gd_msd_time(gd_msd *h, const uint32_t *lags, uint32_t n_lags, double *sum2, double *sum4, uint64_t *count)
{
    const char *who = "gd_msd_time";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (n_lags && (!lags || !sum2 || !count)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (n_lags > (1u << 28)) return fail(GD_EINVAL, "%s: %u lags exceed 2^28", who, n_lags);
    std::vector<uint32_t> order;
    if (int rc = check_lags(who, "lag", lags, n_lags, order)) return rc;
    if (h->have_groups)
        if (int rc = check_labels(who, "group", h->group.data(), h->hist.beads(), h->G)) return rc;
    if (n_lags == 0) return GD_OK;
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> s2((size_t)h->G * n_lags), s4((size_t)h->G * n_lags);
    GroupMap const m{h->have_groups ? h->group_dev.p : nullptr, 0};
    if (int rc = group_sums(h, time_plan(h), lags, order, m, h->G, s2.data(), s4.data())) return rc;
    std::vector<uint64_t> members(h->G, h->have_groups ? 0 : h->hist.beads());
    if (h->have_groups)
        for (int32_t g : h->group)
            if (g >= 0) members[g]++;
    for (unsigned g = 0; g < h->G; g++)
        for (unsigned l = 0; l < n_lags; l++) count[(size_t)g * n_lags + l] = members[g] * (lags[l] < h->hist.frames() ? h->hist.frames() - lags[l] : 0);
    std::memcpy(sum2, s2.data(), s2.size() * sizeof(double));
    if (sum4) std::memcpy(sum4, s4.data(), s4.size() * sizeof(double));
    return GD_OK;
}

int gd_msd_time_per_bead(gd_msd *h, uint32_t lag, double *m2, double *m4)
{
    const char *who = "gd_msd_time_per_bead";
    if (!h || !m2) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (lag == 0 || lag >= h->hist.frames()) return fail(GD_EINVAL, "%s: lag %u of %u frames (1 to F - 1)", who, lag, h->hist.frames());
    HIPCHK(hipSetDevice(h->device));
    Plan const pl = time_plan(h);
    HIPCHK(h->lags_dev.upload(&lag, 1));
    if (int rc = run_lags(h, pl, h->lags_dev.p, 1)) return rc;
    HIPCHK(h->out.ensure(h->hist.beads()));
    hipLaunchKernelGGL(k_msd_per_seq, dim3(blocks_for(h->hist.beads(), kBlock)), dim3(kBlock), 0, h->stream, h->partial.p, pl.ranges, pl.n_seqs, h->out.p);
    HIPCHK(hipGetLastError());
    std::vector<double2> host(h->hist.beads());
    HIPCHK(hipMemcpyAsync(host.data(), h->out.p, host.size() * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (unsigned i = 0; i < h->hist.beads(); i++) {
        m2[i] = host[i].x;
        if (m4) m4[i] = host[i].y;
    }
    return GD_OK;
}

int gd_msd_chain(gd_msd *h, const uint32_t *seps, uint32_t n_seps, uint32_t first_frame, uint32_t n_frames, double *sum2, double *sum4,
                 uint64_t *count)
{
    const char *who = "gd_msd_chain";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    unsigned const C = (unsigned)(h->chains.size() / 2);
    if (n_seps && C && (!seps || !sum2 || !count)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (n_seps > (1u << 28)) return fail(GD_EINVAL, "%s: %u separations exceed 2^28", who, n_seps);
    if ((uint64_t)first_frame + n_frames > h->hist.frames())
        return fail(GD_EINVAL, "%s: frames %u to %llu of %u", who, first_frame, (unsigned long long)first_frame + n_frames, h->hist.frames());
    std::vector<uint32_t> order;
    if (int rc = check_lags(who, "separation", seps, n_seps, order)) return rc;
    if (int rc = check_ranges(who, "chain", true, h->chains.data(), C, h->hist.beads())) return rc;
    if (n_seps == 0 || C == 0) return GD_OK;
    size_t const cells = (size_t)C * n_seps;
    unsigned longest = 0;
    for (unsigned c = 0; c < C; c++) longest = std::max(longest, h->chains[2 * c + 1] - h->chains[2 * c]);
    for (unsigned c = 0; c < C; c++)
        for (unsigned l = 0; l < n_seps; l++) {
            uint64_t const len = h->chains[2 * c + 1] - h->chains[2 * c];
            count[(size_t)c * n_seps + l] = (uint64_t)n_frames * (seps[l] < len ? len - seps[l] : 0);
        }
    if (n_frames == 0 || longest < 2) {
        std::fill(sum2, sum2 + cells, 0.0);
        if (sum4) std::fill(sum4, sum4 + cells, 0.0);
        return GD_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    Plan pl{};
    pl.along_chain = true;
    pl.f0 = first_frame;
    pl.nf = n_frames;
    pl.ftiles = (n_frames + kSeqs - 1) / kSeqs;
    pl.n_seqs = (size_t)n_frames * C;
    pl.tiles = (size_t)C * pl.ftiles;
    pl.longest = longest;
    pl.ranges = (longest - 1 + kRange - 1) / kRange;
    if (pl.tiles > 0x7fffffffu) return fail(GD_EINVAL, "%s: %zu tiles of %u chains in %u frames exceed 2^31", who, pl.tiles, C, n_frames);
    std::vector<double> s2(cells), s4(cells);
    GroupMap const m{nullptr, C};
    if (int rc = group_sums(h, pl, seps, order, m, C, s2.data(), s4.data())) return rc;
    std::memcpy(sum2, s2.data(), cells * sizeof(double));
    if (sum4) std::memcpy(sum4, s4.data(), cells * sizeof(double));
    return GD_OK;
}

}  // extern "C"
