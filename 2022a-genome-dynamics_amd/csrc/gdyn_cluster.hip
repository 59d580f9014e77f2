// gdyn_cluster.hip -- the connected clusters of a history (include/gdyn_cluster.h): per frame, the connected components of the
// graph whose edges are the pairs of selected beads closer than a distance, as the smallest bead index of every bead's component,
// with the number of clusters, the largest, the sum of squared sizes and the histogram of sizes.  Beyond the reference, which has
// no such analysis.  The pair rules, the cell grid and the walk over it are gdyn_cells.hpp's, which gdyn_dcorr.hip shares, the
// history is gd::History's (gdyn_history.hpp).  Unlike every other analysis here the result is not a sum of independent terms but a fixed point: a
// concurrent union-find over the pair graph.
//
// Per batch of frames (max_frames_per_launch; no result depends on it):
//   gd::CellIndex    (gdyn_cells.hpp) as in gdyn_dcorr.hip: cells of side >= distance (1 + kCellSlack), coarsened until a frame has
//                    at most `cap` = n / 16 of them, so that a cell holds 16 beads or so and a block's lanes have centres to serve;
//                    the records in (frame, cell) order, the cell starts, one work item per kCellChunk centres of a non-empty cell
//   PositionFill     (gdyn_cells.hpp) between its steps: the selected beads of each frame as 32-byte records (position, bead, label)
//   k_cluster_init   parent[b, i] = i: every bead is the root of its own tree (uint32, bead-index space, one array per frame)
//   k_cluster_link   the hot path: the tile walk of gdyn_cells.hpp in tiles of kTile records in static LDS (x y z and bead|label as
//                    four arrays of 8-byte words); only partners later in sorted order count, so every unordered pair is seen once.
//                    The body: a pair inside the cutoff whose class may link is an edge, and the lane calls unite() on its frame's
//                    parent array, unless both ends already report the same parent.
//   k_cluster_flatten   a launch of its own, so that every write of the link kernel is visible to it: root[b, i] = the root of
//                    bead i's tree (-1 for a bead that is not selected).  parent is read-only here and root is another array.
//   k_cluster_sizes  members per root (uint32 integer atomics; the lanes of a wave that count for one root add once, for the root of
//                    the wave's first lane and then of the first lane left: a frame's largest cluster may hold most of its beads)
//   k_cluster_summary   per frame: selected beads, roots, the largest (atomicMax), the sum of s*s and the histogram of sizes:
//                    uint64 integer atomics, pre-aggregated per block in LDS (the first kLdsBins bins of the histogram too)
//
// unite(u, v) walks whichever of the two is larger towards its root and hangs a root only under a smaller index, so a bead's parent
// never increases.  At the fixed point every tree's root is the smallest index of its component and no relabelling pass is needed.
//
// The memory-model rules of k_cluster_link.  Blocks of one launch run on different CUs and XCDs; per-XCD L2s are not coherent with
// each other and a CU's L1 is never refreshed by another CU's stores.
//   1. Every write to parent while other blocks may touch it is an agent-scope atomic: a compare-and-swap for the hook, an
//      atomic minimum for path halving.  There is no plain store to parent in the link kernel.
//   2. Correctness rests only on (a) a bead's parent never increases and never leaves the bead's component, and (b) the value an
//      atomic returns.  A load of parent may return any earlier value of the word.  A stale parent is an older ancestor: it is
//      smaller than the bead and in its component, so the walk goes on from a legal place.  A stale "I am a root" is settled by
//      the compare-and-swap, which fails and returns the current parent.  Two ends that report the same parent, or a walk in
//      which both ends meet in one index, are in one tree whatever the age of the values read.
//   3. No fence inside a loop, no flag, no waiting of one block for another: the kernel has no spin.  Its one loop is a retry in
//      which every trip makes progress: the larger of the two indices is replaced by a strictly smaller one, or the call returns.
//   4. That loop still carries a trip bound derived from N (u + v falls with every trip: at most 2 N trips), and so does the walk
//      of k_cluster_flatten (N).  A lane that exceeds its bound sets an error word and returns; the host turns the word into GD_EHIP
//      with a message.  A bug ends the call; it cannot hang the device.
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics: every output is an integer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_cluster.h"
#include "gdyn_analysis.hpp"
#include "gdyn_cells.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"
#include "gdyn_types.h"

using namespace gd;

namespace {

constexpr int kBlock = kCellBlock;
constexpr unsigned kTile = 512;              // records of a partner tile
constexpr unsigned kTileWords = 4;           // x y z bead|label
constexpr unsigned kUnroll = 4;              // partners of a lane whose positions are read together
constexpr unsigned kLdsBins = 2048;          // size bins a block of k_cluster_summary counts in LDS

enum : unsigned { kErrLink = 1u, kErrFlatten = 2u };      // bits of the error word

struct Rec {      // one selected bead of one frame
    double p[3];
    unsigned bead;
    int label;
};
static_assert(sizeof(Rec) == 32, "a record is 32 bytes");

// ---- the union-find

__global__ void __launch_bounds__(kBlock) k_cluster_init(unsigned *__restrict__ parent, unsigned N, size_t n)
{
    size_t const idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx < n) parent[idx] = (unsigned)(idx % N);
}

// any earlier value of the word will do (rule 2); the agent scope only keeps the read out of this CU's L1, where it would never change
__device__ inline unsigned peek(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Joins the trees of u and v, two beads of one frame (parent: that frame's array).  The larger of the two indices is walked: while it
// has a parent it moves up (and its parent word is lowered to its grandparent, path halving); once it looks like a root it is hung
// under the smaller index by a compare-and-swap, which either succeeds or returns the parent it has acquired meanwhile.  Every trip
// ends the call or replaces the larger index by a strictly smaller one, so u + v bounds the trips.  false: the bound was exceeded.
__device__ inline bool unite(unsigned *parent, unsigned u, unsigned v, unsigned bound)
{
    for (unsigned trip = 0; trip < bound; trip++) {
        if (u == v) return true;
        if (u < v) {
            unsigned const t = u;
            u = v;
            v = t;
        }
        unsigned const pu = peek(parent + u);
        if (pu != u) {      // pu < u: an ancestor of u, perhaps an old one
            unsigned const g = peek(parent + pu);
            if (g != pu) (void)__hip_atomic_fetch_min(parent + u, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            u = g;
            continue;
        }
        unsigned expected = u;
        if (__hip_atomic_compare_exchange_strong(parent + u, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
        u = expected;      // no root any more: its current parent, smaller than u
    }
    return false;
}

struct LinkArgs {
    double d2;
    unsigned long long mask;
    unsigned K, N, cap, bound;
    unsigned *parent;      // (B, N)
    unsigned *err;
};

template <bool kPeriodic>
__global__ void __launch_bounds__(kBlock) k_cluster_link(const Rec *__restrict__ srec, const unsigned *__restrict__ starts, const uint2 *__restrict__ work,
                                                         const Grid *__restrict__ grids, LinkArgs a)
{
    constexpr unsigned stride = kTile + kCellTilePad;
    __shared__ __attribute__((aligned(16))) unsigned long long smem[kTileWords * stride];
    double *tx = reinterpret_cast<double *>(smem);      // [3][stride]
    unsigned long long *tmeta = smem + 3 * stride;

    CellWork const cw = cell_work(work[blockIdx.x], starts, a.cap);
    Grid const g = grids[cw.o];
    unsigned const s = cw.s_begin + cw.ci, gs = cw.gs;
    Rec q;
    if (cw.active) q = srec[s];
    unsigned *parent = a.parent + (size_t)cw.o * a.N;
    bool failed = false;

    // partners later in sorted order only
    cell_tile_walk<kPeriodic, kTileWords, kTileWords>(g, cw.cell, starts + (size_t)cw.o * a.cap, cw.s_begin + 1u, srec, smem, std::integral_constant<unsigned, kTile>{}, cw.active, [&](unsigned j0, unsigned nt) {
        for (unsigned k0 = cw.sl; k0 < nt; k0 += kUnroll * gs) {
            // the positions of kUnroll partners first, so that their LDS reads are in flight together
            double r2[kUnroll];
#pragma unroll
            for (unsigned u = 0; u < kUnroll; u++) {
                unsigned const k = k0 + u * gs, kc = min(k, nt - 1u);
                double dx = q.p[0] - tx[kc], dy = q.p[1] - tx[stride + kc], dz = q.p[2] - tx[2 * stride + kc];
                if (kPeriodic) {
                    dx = min_image(dx, g.box[0]);
                    dy = min_image(dy, g.box[1]);
                    dz = min_image(dz, g.box[2]);
                }
                r2[u] = k < nt && j0 + k > s ? (dx * dx + dy * dy) + dz * dz : INFINITY;
            }
#pragma unroll
            for (unsigned u = 0; u < kUnroll; u++) {
                if (!(r2[u] < a.d2)) continue;
                unsigned long long const meta = tmeta[k0 + u * gs];
                unsigned const bj = (unsigned)(meta & 0xffffffffu), lj = (unsigned)(meta >> 32);
                if (!((a.mask >> pair_class((unsigned)q.label, lj, a.K)) & 1ull)) continue;
                unsigned const pi = peek(parent + q.bead), pj = peek(parent + bj);
                if (pi == pj) continue;      // one tree already
                if (!unite(parent, pi, pj, a.bound)) failed = true;
            }
        }
    });
    if (failed) atomicOr(a.err, kErrLink);
}

// root[b, i] of every bead of the batch; parent is read-only here, so plain loads see all of it
__global__ void __launch_bounds__(kBlock) k_cluster_flatten(const unsigned *__restrict__ parent, const int *__restrict__ label, unsigned N, size_t n,
                                                            int *__restrict__ root, unsigned *__restrict__ err)
{
    size_t const idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n) return;
    unsigned const i = (unsigned)(idx % N);
    if (label && label[i] < 0) {
        root[idx] = -1;
        return;
    }
    const unsigned *par = parent + (idx - i);
    unsigned r = i, trips = 0;
    for (unsigned p = par[r]; p != r && trips <= N; p = par[r], trips++) r = p;
    if (trips > N) atomicOr(err, kErrFlatten);
    root[idx] = (int)r;
}

__global__ void __launch_bounds__(kBlock) k_cluster_sizes(const int *__restrict__ root, unsigned N, size_t n, unsigned *__restrict__ members)
{
    size_t const idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    int const r = idx < n ? root[idx] : -1;
    bool todo = r >= 0;
    size_t const target = todo ? idx - idx % N + (unsigned)r : ~(size_t)0;
    // a frame's largest cluster may hold most of its beads: the lanes of a wave that count for the same root as its first lane
    // still to count add once, twice over; whoever is left adds for itself
    unsigned long long left = __ballot(todo);
    for (int round = 0; round < 2 && left; round++) {
        size_t const first = (size_t)__shfl((unsigned long long)target, __ffsll(left) - 1);
        bool const mine = todo && target == first;
        unsigned long long const same = __ballot(mine);
        if (mine && (threadIdx.x % 64) == (unsigned)(__ffsll(same) - 1)) atomicAdd(&members[first], (unsigned)__popcll(same));
        todo = todo && !mine;
        left &= ~same;
    }
    if (todo) atomicAdd(&members[target], 1u);
}

// summary[b, 0..3] and hist[b, :] (or NULL); grid (blocks over the beads, B)
__global__ void __launch_bounds__(kBlock) k_cluster_summary(const int *__restrict__ root, const unsigned *__restrict__ members, unsigned N, unsigned n_bins,
                                                            unsigned long long *__restrict__ summary, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned lh[kLdsBins];
    __shared__ unsigned long long acc[4];      // selected, clusters, largest, sum of s*s
    unsigned const lds_bins = hist ? min(n_bins, kLdsBins) : 0u;
    for (unsigned e = threadIdx.x; e < lds_bins; e += kBlock) lh[e] = 0u;
    if (threadIdx.x < 4) acc[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned const b = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
    int const r = i < N ? root[(size_t)b * N + i] : -1;
    bool const selected = r >= 0, is_root = selected && (unsigned)r == i;
    unsigned const n_selected = (unsigned)__popcll(__ballot(selected)), n_roots = (unsigned)__popcll(__ballot(is_root));
    if (threadIdx.x % 64 == 0) {
        if (n_selected) atomicAdd(&acc[0], (unsigned long long)n_selected);
        if (n_roots) atomicAdd(&acc[1], (unsigned long long)n_roots);
    }
    if (is_root) {
        unsigned long long const s = members[(size_t)b * N + i];
        atomicMax(&acc[2], s);
        atomicAdd(&acc[3], s * s);
        if (hist) {
            unsigned const bin = (unsigned)min(s, (unsigned long long)n_bins) - 1u;
            if (bin < lds_bins) atomicAdd(&lh[bin], 1u);
            else atomicAdd(&hist[(size_t)b * n_bins + bin], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && acc[threadIdx.x]) {
        if (threadIdx.x == 2) atomicMax(&summary[4 * (size_t)b + 2], acc[2]);
        else atomicAdd(&summary[4 * (size_t)b + threadIdx.x], acc[threadIdx.x]);
    }
    for (unsigned e = threadIdx.x; e < lds_bins; e += kBlock)
        if (lh[e]) atomicAdd(&hist[(size_t)b * n_bins + e], (unsigned long long)lh[e]);
}

}  // namespace

struct gd_cluster : gd::handle {
    unsigned max_frames = 0;
    History hist;
    // selection: labels and link mask, which belong to hist.beads()
    LabelSelection ls;
    uint64_t mask = 1;
    // per batch
    CellIndex<Rec> cells;
    dbuf<unsigned> err, parent, members;
    dbuf<int> root;
    dbuf<unsigned long long> summary, sizes;

    unsigned P() const { return ls.K * (ls.K + 1) / 2; }
};

namespace {

uint64_t all_classes(unsigned K) { return (1ull << (K * (K + 1) / 2)) - 1; }      // P <= 36

History::Rebind rebind(gd_cluster *h, const char *who)
{
    return [h, who](unsigned n_beads) -> int {
        if (n_beads >= (1u << 31)) return fail(GD_EINVAL, "%s: %u beads (fewer than 2^31)", who, n_beads);
        if (n_beads != h->hist.beads() || !h->ls.sel.p) {      // labels and mask belonged to another N
            GDCHK(h->ls.select_all(n_beads));
            h->mask = all_classes(1);
        }
        return GD_OK;
    };
}

uint32_t frames_of(const gd_cluster *h, uint32_t first, uint32_t count, uint32_t stride)
{
    if (!h || !h->hist.frames() || !stride) return 0;
    return (uint32_t)frames_served(frames_fit(h->hist.frames(), first, stride), count);
}

struct Call {      // what a batch needs of its call
    FrameSel fr;
    Space sp;
    double distance;
    unsigned n_bins, cap;
};

int run_batch(gd_cluster *h, const Call &c, unsigned o0, unsigned B, int32_t *root_out, uint64_t *summary_out, uint64_t *hist_out)
{
    hipStream_t st = h->stream;
    CellIndex<Rec> &ci = h->cells;
    unsigned const n = h->ls.n_sel, N = h->hist.beads();
    size_t const nb = (size_t)B * n, nB = (size_t)B * N, slots = (size_t)B * c.cap;
    GDCHK(ci.room(B, n, c.cap));
    HIPCHK(h->err.ensure(1));
    HIPCHK(h->parent.ensure(nB));
    HIPCHK(h->members.ensure(nB));
    HIPCHK(h->root.ensure(nB));
    HIPCHK(h->summary.ensure(4 * (size_t)B));
    if (hist_out) HIPCHK(h->sizes.ensure((size_t)B * c.n_bins));
    const int *label = h->ls.labels();
    int const is64 = h->hist.is_f64;
    BatchFrames const fr{c.fr, o0};
    GDCHK(ci.make_grids(st, h->hist.x(), is64, N, h->ls.sel.p, n, fr, B, c.sp, c.cap));
    GDCHK(ci.make_keys(st, PositionFill<BatchFrames>{h->hist.x(), is64, N, label, fr, 0}, h->ls.sel.p, n, B, ci.grids.p, c.sp.periodic, c.cap));
    GDCHK(ci.sort(st, nb, slots));
    hipLaunchKernelGGL(k_cluster_init, dim3(blocks_for(nB, kBlock)), dim3(kBlock), 0, st, h->parent.p, N, nB);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(h->err.p, 0, sizeof(unsigned), st));
    HIPCHK(hipMemsetAsync(h->members.p, 0, nB * sizeof(unsigned), st));
    HIPCHK(hipMemsetAsync(h->summary.p, 0, 4 * (size_t)B * sizeof(unsigned long long), st));
    if (hist_out) HIPCHK(hipMemsetAsync(h->sizes.p, 0, (size_t)B * c.n_bins * sizeof(unsigned long long), st));
    unsigned n_work = 0;
    GDCHK(ci.work_items("gd_cluster_components", st, &n_work));
    if (n_work) {
        LinkArgs a;
        a.d2 = c.distance * c.distance;
        a.mask = h->mask;
        a.K = h->ls.K;
        a.N = N;
        a.cap = c.cap;
        a.bound = (unsigned)std::min<uint64_t>(2 * (uint64_t)N + 2, 0xffffffffu);
        a.parent = h->parent.p;
        a.err = h->err.p;
        dim3 const grid(n_work), block(kBlock);
        if (c.sp.periodic) hipLaunchKernelGGL(k_cluster_link<true>, grid, block, 0, st, ci.srec.p, ci.starts.p, ci.work.p, ci.grids.p, a);
        else hipLaunchKernelGGL(k_cluster_link<false>, grid, block, 0, st, ci.srec.p, ci.starts.p, ci.work.p, ci.grids.p, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cluster_flatten, dim3(blocks_for(nB, kBlock)), dim3(kBlock), 0, st, h->parent.p, label, N, nB, h->root.p, h->err.p);
    hipLaunchKernelGGL(k_cluster_sizes, dim3(blocks_for(nB, kBlock)), dim3(kBlock), 0, st, h->root.p, N, nB, h->members.p);
    hipLaunchKernelGGL(k_cluster_summary, dim3(blocks_for(N, kBlock), B), dim3(kBlock), 0, st, h->root.p, h->members.p, N, c.n_bins, h->summary.p,
                       hist_out ? h->sizes.p : nullptr);
    HIPCHK(hipGetLastError());
    unsigned err = 0;
    HIPCHK(hipMemcpyAsync(&err, h->err.p, sizeof err, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (err)
        return fail(GD_EHIP, "gd_cluster_components: %s exceeded its trip bound for %u beads: the parent array is not a forest", err & kErrLink ? "unite" : "the walk to a root", N);
    if (root_out) HIPCHK(hipMemcpyAsync(root_out, h->root.p, nB * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(summary_out, h->summary.p, 4 * (size_t)B * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (hist_out) HIPCHK(hipMemcpyAsync(hist_out, h->sizes.p, (size_t)B * c.n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_cluster_abi_version(void) { return GD_CLUSTER_ABI_VERSION; }

int gd_cluster_create(const gd_cluster_desc *desc, gd_cluster **out)
{
    if (int rc = gd::open("gd_cluster_create", desc, out)) return rc;
    (*out)->max_frames = desc->max_frames_per_launch;
    return GD_OK;
}

int gd_cluster_destroy(gd_cluster *h) { return gd::close(h); }

int gd_cluster_set_history(gd_cluster *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_cluster_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (n_beads >= (1u << 31)) return fail(GD_EINVAL, "%s: %u beads (fewer than 2^31)", who, n_beads);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h, who));
}

int gd_cluster_set_history_live(gd_cluster *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_cluster_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h, who));
}

int gd_cluster_set_labels(gd_cluster *h, const int32_t *label, uint32_t n_labels)
{
    const char *who = "gd_cluster_set_labels";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the labels are N values of its beads)", who);
    GDCHK(h->ls.set(who, h->device, label, n_labels, GD_CLUSTER_MAX_LABELS, h->hist.beads()));
    h->mask = all_classes(h->ls.K);
    return GD_OK;
}

int gd_cluster_set_links(gd_cluster *h, uint64_t link_mask)
{
    const char *who = "gd_cluster_set_links";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the classes are those of its beads' labels)", who);
    if (!link_mask) return fail(GD_EINVAL, "%s: an empty mask links nothing", who);
    if (link_mask & ~all_classes(h->ls.K))
        return fail(GD_EINVAL, "%s: mask 0x%llx has a bit at or past the %u classes of %u labels", who, (unsigned long long)link_mask, h->P(), h->ls.K);
    h->mask = link_mask;
    return GD_OK;
}

uint32_t gd_cluster_classes(const gd_cluster *h) { return h ? h->P() : 0u; }

uint32_t gd_cluster_frames(const gd_cluster *h, uint32_t first_frame, uint32_t n_frames, uint32_t frame_stride)
{
    return frames_of(h, first_frame, n_frames, frame_stride);
}

int gd_cluster_components(gd_cluster *h, uint32_t first_frame, uint32_t n_frames, uint32_t frame_stride, const double *box, double distance,
                          uint32_t n_size_bins, int32_t *root_out, uint64_t *summary_out, uint64_t *hist_out)
{
    const char *who = "gd_cluster_components";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (frame_stride == 0) return fail(GD_EINVAL, "%s: frame stride 0", who);
    if (n_frames && (uint64_t)first_frame + (uint64_t)(n_frames - 1) * frame_stride >= h->hist.frames())
        return fail(GD_EINVAL, "%s: frame %llu lies beyond the %u frames", who, (unsigned long long)first_frame + (unsigned long long)(n_frames - 1) * frame_stride,
                    h->hist.frames());
    if (box)
        for (int a = 0; a < 3; a++)
            if (!(box[a] > 0.0) || !std::isfinite(box[a])) return fail(GD_EINVAL, "%s: box[%d] = %g is not positive and finite", who, a, box[a]);
    if (!(distance > 0.0) || !std::isfinite(distance)) return fail(GD_EINVAL, "%s: distance %g is not positive and finite", who, distance);
    if (n_size_bins == 0 || n_size_bins > GD_CLUSTER_MAX_SIZE_BINS)
        return fail(GD_EINVAL, "%s: %u size bins (1 to %u)", who, n_size_bins, GD_CLUSTER_MAX_SIZE_BINS);
    FrameSel const fr{first_frame, frame_stride, frames_of(h, first_frame, n_frames, frame_stride)};
    if (!fr.count) return GD_OK;
    if (!summary_out) return fail(GD_EINVAL, "%s: NULL summary output", who);
    unsigned const n = h->ls.n_sel, N = h->hist.beads();
    if (n == 0) {      // nobody takes part
        if (root_out) std::fill(root_out, root_out + (size_t)fr.count * N, -1);
        std::memset(summary_out, 0, (size_t)fr.count * 4 * sizeof(uint64_t));
        if (hist_out) std::memset(hist_out, 0, (size_t)fr.count * n_size_bins * sizeof(uint64_t));
        return GD_OK;
    }
    HIPCHK(hipSetDevice(h->device));

    Call c;
    c.fr = fr;
    c.sp.periodic = box != nullptr;
    for (int a = 0; a < 3; a++) c.sp.box[a] = box ? box[a] : 0.0;
    c.sp.cell_side = distance * (1.0 + kCellSlack);
    c.distance = distance;
    c.n_bins = n_size_bins;
    // about 16 beads a cell: with cells of side `distance` and a bead or fewer in each (a melt at a contact distance) a block of 256 lanes
    // would serve one or two centres.  Measured on 62 178 beads x 701 frames: n cells 181 ms, n / 4 cells 98 ms, n / 16 cells 80 ms a call
    c.cap = std::max(64u, n / 16);
    size_t const want = h->max_frames ? h->max_frames : ((size_t)1 << 20) / N + 1;      // ~1M beads per launch
    // sorted indices stay 32-bit, frames fit gridDim.y, the cell starts and the histograms of a batch stay below 2^26 and 2^24 entries
    size_t const limit = std::min<size_t>(std::min<size_t>(std::min<size_t>(65535, ((size_t)1 << 26) / c.cap), ((size_t)1 << 30) / N),
                                          hist_out ? ((size_t)1 << 24) / n_size_bins : 65535);
    unsigned const B = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(want, limit), fr.count));
    for (unsigned o0 = 0; o0 < fr.count; o0 += B) {
        unsigned const b = std::min(B, fr.count - o0);
        if (int rc = run_batch(h, c, o0, b, root_out ? root_out + (size_t)o0 * N : nullptr, summary_out + (size_t)o0 * 4,
                               hist_out ? hist_out + (size_t)o0 * n_size_bins : nullptr))
            return rc;
    }
    return GD_OK;
}

}  // extern "C"
