// gdyn_vanhove.hip -- the van Hove functions of a trajectory history (include/gdyn_vanhove.h): the histogram of single-bead
// displacements per lag and label (self part) and the histogram of the distances from where a bead was to where the OTHER beads are a
// lag later, per ordered label pair (distinct part).  Beyond the reference, which has neither.  Every output is an integer count.
//
//   k_vh_self<T, LDS>      the lag walk of gdyn_lagwalk.hpp, which gdyn_msd.hip shares, with the body SelfCount; an origin window that
//                          holds no selected origin is not staged.  Lane = (bead, slot); the kSlots = 64 slots share out the (lag,
//                          origin) pairs of a window pair, whose order does not matter: every count is an integer.  A lane finds its
//                          cell by bisection over the squared edges (fp64, squared on the host) in LDS; cell 0 of a (lag, label) row
//                          is `below`, cells 1 .. B the bins, cell B + 1 `above`.  LDS: counts go to a block histogram of uint32 (a
//                          block adds at most kSeqs * kRange = 2^16 to a cell before it is flushed, once per range around the walk,
//                          with one 64-bit atomic per non-zero cell); else (more than GD_VANHOVE_LDS_CELLS cells) straight to the
//                          global table.  per_origin is added to directly in global memory: a tile's 16 beads of one origin are all
//                          that ever meet in one of its cells (lag, origin, label, bin).
//   PairFrames             distinct part, for gdyn_cells.hpp's kernels and its PositionFill: both frames of an (origin, lag) pair for the bounding box,
//                          and the records (position, label, bead) of the centres (frame f) and of the partners (frame f + tau)
//   k_vh_pairs<PERIODIC, LDS>   the tile walk of gdyn_cells.hpp with two sets of records: the centres are those of a cell of the centres'
//                          index, the cells around it those of the PARTNERS' index on the one grid of the pair, from their first
//                          record on: every ordered pair of different beads is seen once.  The body bins a partner by bisection.
//                          Block histogram in LDS (class, bin) or, above GD_VANHOVE_LDS_CELLS cells, global atomics.
// Only integer atomics.  fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math.  The history is gd::History's, the labels
// gd::LabelSelection's (gdyn_history.hpp), the grid, the sort, the tile walk and the pair rules gdyn_cells.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_vanhove.h"
#include "gdyn_analysis.hpp"
#include "gdyn_cells.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"
#include "gdyn_lagwalk.hpp"
#include "gdyn_types.h"

using namespace gd;

namespace {

typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "the outputs are uint64");

constexpr int kSelfBlock = kLagBlock;        // the lag walk's: a tile is kSeqs beads, and kSeqs * kRange < 2^32 bounds a uint32 cell
constexpr unsigned kMaxLags = GD_VANHOVE_MAX_LAGS, kMaxBins = GD_VANHOVE_MAX_BINS, kLdsCells = GD_VANHOVE_LDS_CELLS;
constexpr int kBlock = kCellBlock;
constexpr unsigned kTileWords = 4;           // x y z label|bead

// the number of edges2[0 .. B] that are <= r2: 0 below, B + 1 above, else 1 + bin
__device__ inline unsigned cell_of_r2(const double *e2, unsigned B, double r2)
{
    unsigned lo = 0, hi = B + 1;
    while (lo < hi) {
        unsigned const mid = (lo + hi) / 2;
        if (e2[mid] <= r2) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// hist[cell] += 1 for the lanes with `valid`; every lane of the wave calls
__device__ inline void lds_count(unsigned *hist, unsigned cell, bool valid)
{
#ifdef GD_VANHOVE_WAVE_COUNT
    // up to four rounds in which the lanes of one cell are counted by ballot and added once; what is left adds lane by lane
    u64 todo = __ballot(valid);
    unsigned const lane = threadIdx.x & 63u;
    for (int round = 0; round < 4 && todo; round++) {
        int const lead = __ffsll((long long)todo) - 1;
        unsigned const c = __shfl(cell, lead);
        u64 const same = __ballot(valid && cell == c);
        if ((int)lane == lead) atomicAdd(&hist[c], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&hist[cell], 1u);
#else
    if (valid) atomicAdd(&hist[cell], 1u);
#endif
}

struct SelfArgs {
    const void *x;              // the history, (F, N, 3) of T
    const int *label;           // (N) or nullptr: label 0
    const uint32_t *lags;       // (n_lags) ascending, all < F
    const double *edges2;       // (B + 1)
    unsigned N, F, n_lags, B, K, W, windows;
    unsigned first, stride, O;  // the origins first + k stride, k < O
    unsigned axes, cells;       // cells = n_lags K (B + 2)
    u64 *table;                 // (n_lags, K, B + 2)
    u64 *per_origin;            // (n_lags, O, K, B) or nullptr
};

// The body of the lag walk: lane = (bead, slot).  The slots share out the (lag, origin) pairs of a window pair and count each
// displacement in its cell of the histogram.
template <typename T, bool LDS>
struct SelfCount {
    const SelfArgs &p;
    const double *e2;
    unsigned *hist;
    unsigned s, slot;
    int lab;
    long long k_lo;      // the selected origins of the window: k_lo + [0, nk)
    unsigned nk;

    __device__ bool wants(long long A0, long long nO)
    {
        // the origins k with A0 <= first + k stride < A0 + nO
        k_lo = A0 <= (long long)p.first ? 0 : (A0 - p.first + p.stride - 1) / p.stride;
        long long const k_hi = A0 + nO <= (long long)p.first ? 0 : min((long long)p.O, (A0 + nO - p.first + p.stride - 1) / p.stride);
        nk = (unsigned)(k_hi - k_lo);
        return k_lo < k_hi;
    }
    __device__ void operator()(const LagPair &w, const T *A, const T *Bw) const
    {
        unsigned const B = p.B;
        bool const ax = p.axes & 1u, ay = p.axes & 2u, az = p.axes & 4u;
        unsigned const total = (w.hi - w.lo) * nk;      // <= 32 * 4096
        for (unsigned i0 = 0; i0 < total; i0 += kSlots) {      // the same trip count for every lane of the block
            unsigned const idx = i0 + slot;
            bool ok = lab >= 0 && idx < total;
            unsigned cell = 0, li = 0, k = 0;
            if (ok) {
                li = w.lo + idx / nk;
                k = (unsigned)k_lo + idx % nk;
                long long const r = (long long)p.first + (long long)k * p.stride - w.A0;      // in [0, nO)
                long long const rb = r + (long long)p.lags[li] - w.d * w.W;
                ok = rb >= 0 && rb < w.nB;
                if (ok) {
                    const T *pa = A + r * kRow + 3 * s, *pb = Bw + rb * kRow + 3 * s;
                    double const dx = (double)pb[0] - (double)pa[0], dy = (double)pb[1] - (double)pa[1], dz = (double)pb[2] - (double)pa[2];
                    double const tx = ax ? dx * dx : 0.0, ty = ay ? dy * dy : 0.0, tz = az ? dz * dz : 0.0;
                    cell = cell_of_r2(e2, B, (tx + ty) + tz);
                }
            }
            unsigned const at = (li * p.K + (unsigned)lab) * (B + 2) + cell;
            if (LDS) lds_count(hist, at, ok);
            else if (ok) atomicAdd(&p.table[at], 1ull);
            if (ok && p.per_origin && cell >= 1 && cell <= B)
                atomicAdd(&p.per_origin[(((size_t)li * p.O + k) * p.K + (unsigned)lab) * B + (cell - 1)], 1ull);
        }
    }
};

template <typename T, bool LDS>
__global__ void __launch_bounds__(kSelfBlock) k_vh_self(SelfArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *e2 = reinterpret_cast<double *>(smem);
    unsigned *hist = reinterpret_cast<unsigned *>(e2 + p.B + 1);
    T *A = reinterpret_cast<T *>(hist + (LDS ? (p.cells + 1u) / 2u * 2u : 0u));
    T *Bw0 = A + (size_t)(p.windows - 1) * p.W * kRow;      // one window: partners lie in A
    __builtin_assume(p.N >= 1);      // item_stride >= seq_stride: only the along-time half of stage() is this kernel's
    LagTile const t{(size_t)blockIdx.x * kSeqs * 3, 3, (size_t)p.N * 3, min(kSeqs, p.N - blockIdx.x * kSeqs), p.F};
    unsigned const s = threadIdx.x % kSeqs, slot = threadIdx.x / kSeqs;
    int const lab = s < t.valid ? (p.label ? p.label[blockIdx.x * kSeqs + s] : 0) : -1;
    SelfCount<T, LDS> body{p, e2, hist, s, slot, lab, 0, 0};
    for (unsigned e = threadIdx.x; e <= p.B; e += kSelfBlock) e2[e] = p.edges2[e];
    unsigned const ranges = (p.F + kRange - 1) / kRange;
    for (unsigned g = blockIdx.y; g < ranges; g += gridDim.y) {
        long long const O0 = (long long)g * kRange, O1 = min(O0 + (long long)kRange, (long long)p.F);
        if (LDS) {
            __syncthreads();      // the last range has been flushed
            for (unsigned c = threadIdx.x; c < p.cells; c += kSelfBlock) hist[c] = 0u;
        }
        lag_walk(static_cast<const T *>(p.x), t, p.lags, p.n_lags, (long long)p.W, O0, O1, A, Bw0, body);
        if (LDS) {
            __syncthreads();
            for (unsigned c = threadIdx.x; c < p.cells; c += kSelfBlock) {
                unsigned const v = hist[c];
                if (v) atomicAdd(&p.table[c], (u64)v);
            }
        }
    }
}

// the dynamic LDS a block of k_vh_self may ask for (gd::lds_opt_in).  A refusal only makes the windows smaller.
int lds_budget(int device)
{
    static DeviceOnce<> once;
    return lds_opt_in(once, device, {reinterpret_cast<const void *>(&k_vh_self<float, false>), reinterpret_cast<const void *>(&k_vh_self<float, true>),
                                     reinterpret_cast<const void *>(&k_vh_self<double, false>), reinterpret_cast<const void *>(&k_vh_self<double, true>)});
}

// ---- distinct part

struct Rec {      // one selected bead of one frame
    double p[3];
    int label;
    unsigned bead;
};
static_assert(sizeof(Rec) == 32, "a record is 32 bytes");

struct Item {      // one (origin, lag) frame pair: the centres' frame, the partners' frame, the lag's row of the output
    unsigned fo, fp, l;
};

struct PairFrames {      // k_cells_bbox: both frames of item o of the batch
    const Item *items;
    static constexpr int kFrames = 2;
    __device__ unsigned frame(unsigned o, int which) const { return which ? items[o].fp : items[o].fo; }
};

struct PairArgs {
    const double *edges2;      // (B + 1)
    const Item *items;         // of the batch
    unsigned B, K, cells;      // cells = K K B
    unsigned tile, cap;
    u64 *table;                // (L, K K, B)
};

template <bool kPeriodic, bool kLds>
__global__ void __launch_bounds__(kBlock) k_vh_pairs(const Rec *__restrict__ crec, const unsigned *__restrict__ cstarts, const uint2 *__restrict__ work,
                                                     const Rec *__restrict__ prec, const unsigned *__restrict__ pstarts, const Grid *__restrict__ grids, PairArgs a)
{
    extern __shared__ __attribute__((aligned(16))) u64 smem2[];
    unsigned const stride = a.tile + kCellTilePad, B = a.B;
    double *tx = reinterpret_cast<double *>(smem2);      // [kTileWords][stride]
    u64 *tmeta = smem2 + 3 * (size_t)stride;
    double *e2 = reinterpret_cast<double *>(smem2 + kTileWords * (size_t)stride);
    unsigned *hist = reinterpret_cast<unsigned *>(e2 + B + 1);

    CellWork const cw = cell_work(work[blockIdx.x], cstarts, a.cap);
    Grid const g = grids[cw.o];
    Rec q;
    if (cw.active) q = crec[cw.s_begin + cw.ci];
    for (unsigned e = threadIdx.x; e <= B; e += kBlock) e2[e] = a.edges2[e];
    if (kLds)
        for (unsigned e = threadIdx.x; e < a.cells; e += kBlock) hist[e] = 0u;
    u64 *gtable = a.table + (size_t)a.items[cw.o].l * a.cells;

    // every partner of the cells around: the index is another, so no pair is seen twice
    cell_tile_walk<kPeriodic, kTileWords, kTileWords>(g, cw.cell, pstarts + (size_t)cw.o * a.cap, 0u, prec, smem2, a.tile, cw.active, [&](unsigned, unsigned nt) {
        for (unsigned k = cw.sl; k < nt; k += cw.gs) {
            double dx = tx[k] - q.p[0], dy = tx[stride + k] - q.p[1], dz = tx[2 * stride + k] - q.p[2];
            if (kPeriodic) {
                dx = min_image(dx, g.box[0]);
                dy = min_image(dy, g.box[1]);
                dz = min_image(dz, g.box[2]);
            }
            double const r2 = (dx * dx + dy * dy) + dz * dz;
            if (!(r2 < e2[B]) || r2 < e2[0]) continue;
            u64 const meta = tmeta[k];
            if ((unsigned)(meta >> 32) == q.bead) continue;      // the bead itself is the self part's
            unsigned const bin = cell_of_r2(e2, B, r2) - 1u;    // in [0, B)
            unsigned const e = ((unsigned)q.label * a.K + (unsigned)(meta & 0xffffffffu)) * B + bin;
            if (kLds) atomicAdd(&hist[e], 1u);
            else atomicAdd(&gtable[e], 1ull);
        }
    });
    if (kLds) {
        __syncthreads();
        for (unsigned e = threadIdx.x; e < a.cells; e += kBlock) {
            unsigned const c = hist[e];
            if (c) atomicAdd(&gtable[e], (u64)c);
        }
    }
}

size_t tile_bytes(unsigned tile) { return (size_t)kTileWords * (tile + kCellTilePad) * 8; }

}  // namespace

struct gd_vanhove : gd::handle {
    unsigned frames_per_tile = 0, frames_per_launch = 0;
    int lds_bytes = 64 * 1024;
    History hist;
    LabelSelection ls;
    // per call
    dbuf<uint32_t> lags_dev;
    dbuf<double> edges_dev;
    dbuf<u64> table, per_origin;
    dbuf<Item> items_dev;
    CellIndex<Rec> centres, partners;
    StageTimer timer;      // gd_vanhove_last_times: the count, the index, the rest
};

namespace {

History::Rebind rebind(gd_vanhove *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads() || !h->ls.sel.p) GDCHK(h->ls.select_all(n_beads));      // the labels belonged to another N
        return GD_OK;
    };
}

uint32_t origins_of(unsigned F, uint32_t first, uint32_t stride, uint32_t count)
{
    uint64_t const fit = frames_fit(F, first, stride);
    if (fit == 0 || count > fit) return 0;
    return (uint32_t)frames_served(fit, count);
}

struct Plan {      // what a call's spec comes to
    unsigned O = 0, B = 0;
    std::vector<uint32_t> order;         // the indices of the call's lags by ascending lag
    std::vector<uint64_t> origins;       // (L) the origins that take part in a lag, in the caller's order
    std::vector<double> edges2;          // (B + 1)
};

int check_spec(const char *who, const gd_vanhove *h, const gd_vanhove_spec *s, uint32_t least_lag, Plan &pl)
{
    if (!s) return fail(GD_EINVAL, "%s: NULL spec", who);
    unsigned const F = h->hist.frames();
    if (!s->lags || !s->edges) return fail(GD_EINVAL, "%s: NULL lags or edges", who);
    if (s->n_lags < 1 || s->n_lags > kMaxLags) return fail(GD_EINVAL, "%s: %u lags, 1 to %u are served at once", who, s->n_lags, kMaxLags);
    if (s->n_bins < 1 || s->n_bins > kMaxBins) return fail(GD_EINVAL, "%s: %u bins, 1 to %u are served at once", who, s->n_bins, kMaxBins);
    for (uint32_t b = 0; b <= s->n_bins; b++) {
        double const e = s->edges[b];
        if (!std::isfinite(e) || e < 0.0 || (b && !(e > s->edges[b - 1]))) return fail(GD_EINVAL, "%s: edge %u is %g (0 <= e_0 < e_1 < ..., finite)", who, b, e);
        if (!std::isfinite(e * e)) return fail(GD_EINVAL, "%s: the square of edge %u (%g) is not finite", who, b, e);
    }
    if (s->stride == 0) return fail(GD_EINVAL, "%s: origin stride 0", who);
    pl.O = origins_of(F, s->first, s->stride, s->count);
    if (!pl.O)
        return fail(GD_EINVAL, "%s: %u origins from frame %u with stride %u: %llu fit in %u frames", who, s->count, s->first, s->stride,
                    (unsigned long long)frames_fit(F, s->first, s->stride), F);
    LagOrder lo = sort_lags(s->lags, s->n_lags);
    if (lo.least < least_lag) return fail(GD_EINVAL, "%s: lag %u (at least %u)", who, lo.least, least_lag);
    if (lo.twice) return fail(GD_EINVAL, "%s: lag %u is listed twice", who, lo.repeated);
    pl.order = std::move(lo.order);
    pl.B = s->n_bins;
    pl.origins.resize(s->n_lags);
    for (uint32_t l = 0; l < s->n_lags; l++) pl.origins[l] = std::min<uint64_t>(pl.O, frames_fit(F, s->first, s->stride, s->lags[l]));
    pl.edges2.resize(pl.B + 1);
    for (uint32_t b = 0; b <= pl.B; b++) pl.edges2[b] = s->edges[b] * s->edges[b];
    return GD_OK;
}

template <typename T>
void launch_self(const gd_vanhove *h, dim3 grid, size_t shmem, bool lds, const SelfArgs &a)
{
    if (lds) hipLaunchKernelGGL((k_vh_self<T, true>), grid, dim3(kSelfBlock), shmem, h->stream, a);
    else hipLaunchKernelGGL((k_vh_self<T, false>), grid, dim3(kSelfBlock), shmem, h->stream, a);
}

}  // namespace

extern "C" {

int gd_vanhove_abi_version(void) { return GD_VANHOVE_ABI_VERSION; }

int gd_vanhove_create(const gd_vanhove_desc *desc, gd_vanhove **out)
{
    const char *who = "gd_vanhove_create";
    if (int rc = gd::open(who, desc, out)) return rc;
    (*out)->frames_per_tile = desc->max_frames_per_tile;
    (*out)->frames_per_launch = desc->max_frames_per_launch;
    (*out)->lds_bytes = lds_budget(desc->device);
    hipError_t const rc = (*out)->timer.create();
    if (rc != hipSuccess) {
        gd::close(*out);
        *out = nullptr;
        return fail(GD_EHIP, "%s: hipEventCreate failed: %s", who, hipGetErrorString(rc));
    }
    return GD_OK;
}

int gd_vanhove_destroy(gd_vanhove *h) { return gd::close(h); }

int gd_vanhove_set_history(gd_vanhove *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_vanhove_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_vanhove_set_history_live(gd_vanhove *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_vanhove_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_vanhove_set_labels(gd_vanhove *h, const int32_t *label, uint32_t n_labels)
{
    const char *who = "gd_vanhove_set_labels";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the labels are N values of its beads)", who);
    return h->ls.set(who, h->device, label, n_labels, GD_VANHOVE_MAX_LABELS, h->hist.beads());
}

uint32_t gd_vanhove_origins(const gd_vanhove *h, uint32_t first, uint32_t stride, uint32_t count)
{
    return h && h->hist.frames() ? origins_of(h->hist.frames(), first, stride, count) : 0u;
}

int gd_vanhove_self(gd_vanhove *h, const gd_vanhove_spec *spec, uint32_t axes, const gd_vanhove_self_out *out)
{
    const char *who = "gd_vanhove_self";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames(), N = h->hist.beads();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    if (!out) return fail(GD_EINVAL, "%s: NULL outputs", who);
    if (axes == 0 || axes > 7) return fail(GD_EINVAL, "%s: axes mask %u (1 to 7: x = 1, y = 2, z = 4)", who, axes);
    Plan pl;
    GDCHK(check_spec(who, h, spec, 1, pl));
    unsigned const L = spec->n_lags, B = pl.B, K = h->ls.K, O = pl.O;
    // the lags that have a partner frame at all, ascending, and their rows of the device tables
    std::vector<uint32_t> sorted;
    std::vector<int> row_of(L, -1);
    for (uint32_t k : pl.order)
        if (spec->lags[k] < F) {
            row_of[k] = (int)sorted.size();
            sorted.push_back(spec->lags[k]);
        }
    unsigned const nl = (unsigned)sorted.size();
    size_t const row_cells = (size_t)K * (B + 2), cells = nl * row_cells, po_row = (size_t)O * K * B;
    std::vector<u64> table(cells, 0);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    double ms[3] = {0.0, 0.0, 0.0};
    if (nl) {
        if (h->table.ensure(cells) != hipSuccess || (out->per_origin && h->per_origin.ensure(nl * po_row) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(GD_ENOMEM, "%s: the tables of %u lags x %u origins x %u labels x %u bins do not fit on the device", who, nl, O, K, B);
        }
        HIPCHK(h->lags_dev.upload(sorted.data(), nl));
        HIPCHK(h->edges_dev.upload(pl.edges2.data(), B + 1));
        bool const lds = cells <= kLdsCells;
        size_t const fixed = (size_t)(B + 1) * 8 + (lds ? (cells + 1) / 2 * 8 : 0), row = (size_t)kRow * h->hist.elem();
        LagWindows const lw = lag_windows((size_t)h->lds_bytes, fixed, row, F, h->frames_per_tile);
        SelfArgs a{};
        a.x = h->hist.x();
        a.label = h->ls.labels();
        a.lags = h->lags_dev.p;
        a.edges2 = h->edges_dev.p;
        a.N = N;
        a.F = F;
        a.n_lags = nl;
        a.B = B;
        a.K = K;
        a.W = lw.W;
        a.windows = lw.windows;
        a.first = spec->first;
        a.stride = spec->stride;
        a.O = O;
        a.axes = axes;
        a.cells = (unsigned)cells;
        a.table = h->table.p;
        a.per_origin = out->per_origin ? h->per_origin.p : nullptr;
        HIPCHK(h->timer.mark(0, st));
        HIPCHK(hipMemsetAsync(h->table.p, 0, cells * sizeof(u64), st));
        if (out->per_origin) HIPCHK(hipMemsetAsync(h->per_origin.p, 0, nl * po_row * sizeof(u64), st));
        HIPCHK(h->timer.mark(1, st));
        dim3 const grid((N + kSeqs - 1) / kSeqs, std::min((F + kRange - 1) / kRange, 65535u));
        size_t const shmem = fixed + (size_t)lw.windows * lw.W * row;
        if (h->hist.is_f64) launch_self<double>(h, grid, shmem, lds, a);
        else launch_self<float>(h, grid, shmem, lds, a);
        HIPCHK(hipGetLastError());
        HIPCHK(h->timer.mark(2, st));
        HIPCHK(hipMemcpyAsync(table.data(), h->table.p, cells * sizeof(u64), hipMemcpyDeviceToHost, st));
        if (out->per_origin)
            for (uint32_t l = 0; l < L; l++)
                if (row_of[l] >= 0)
                    HIPCHK(hipMemcpyAsync(out->per_origin + l * po_row, h->per_origin.p + (size_t)row_of[l] * po_row, po_row * sizeof(u64), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(h->timer.between(1, 2, &ms[0]));
        HIPCHK(h->timer.between(0, 1, &ms[2]));
    }
    for (uint32_t l = 0; l < L; l++) {
        if (out->origins) out->origins[l] = pl.origins[l];
        if (out->per_origin && row_of[l] < 0) std::memset(out->per_origin + l * po_row, 0, po_row * sizeof(u64));
        for (unsigned k = 0; k < K; k++) {
            const u64 *src = row_of[l] >= 0 ? table.data() + (size_t)row_of[l] * row_cells + (size_t)k * (B + 2) : nullptr;
            if (out->below) out->below[(size_t)l * K + k] = src ? src[0] : 0;
            if (out->above) out->above[(size_t)l * K + k] = src ? src[B + 1] : 0;
            if (out->counts)
                for (unsigned b = 0; b < B; b++) out->counts[((size_t)l * K + k) * B + b] = src ? src[1 + b] : 0;
        }
    }
    std::copy(ms, ms + 3, h->timer.ms);
    return GD_OK;
}

int gd_vanhove_distinct(gd_vanhove *h, const gd_vanhove_spec *spec, const double *box, uint64_t *counts, uint64_t *origins)
{
    const char *who = "gd_vanhove_distinct";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames(), N = h->hist.beads();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    if (!counts) return fail(GD_EINVAL, "%s: NULL counts", who);
    if (box)
        for (int a = 0; a < 3; a++)
            if (!(box[a] > 0.0) || !std::isfinite(box[a])) return fail(GD_EINVAL, "%s: box[%d] = %g is not positive and finite", who, a, box[a]);
    Plan pl;
    GDCHK(check_spec(who, h, spec, 0, pl));
    unsigned const L = spec->n_lags, B = pl.B, K = h->ls.K, n = h->ls.n_sel;
    size_t const cells = (size_t)K * K * B;
    std::vector<Item> items;
    for (uint32_t l = 0; l < L; l++)
        for (uint64_t k = 0; k < pl.origins[l]; k++) {
            unsigned const f = spec->first + (unsigned)k * spec->stride;
            items.push_back(Item{f, f + spec->lags[l], l});
        }
    double ms[3] = {0.0, 0.0, 0.0};
    if (n >= 2 && !items.empty()) {
        HIPCHK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        if (h->table.ensure(L * cells) != hipSuccess) {
            (void)hipGetLastError();
            return fail(GD_ENOMEM, "%s: the table of %u lags x %u classes x %u bins does not fit on the device", who, L, K * K, B);
        }
        HIPCHK(h->edges_dev.upload(pl.edges2.data(), B + 1));
        HIPCHK(h->items_dev.upload(items.data(), items.size()));
        HIPCHK(hipMemsetAsync(h->table.p, 0, L * cells * sizeof(u64), st));
        Space sp;
        sp.periodic = box != nullptr;
        for (int a = 0; a < 3; a++) sp.box[a] = box ? box[a] : 0.0;
        sp.cell_side = spec->edges[B] * (1.0 + kCellSlack);
        unsigned const cap = std::max(4096u, n);
        // the histogram in LDS: a block adds at most kCellChunk * n to one uint32 counter
        bool const lds = cells <= kLdsCells && n < (1u << 24);
        unsigned const tile = 256;
        size_t const shmem = tile_bytes(tile) + (size_t)(B + 1) * 8 + (lds ? cells * 4 : 0);      // < 64 KiB
        size_t const want = h->frames_per_launch ? h->frames_per_launch : ((size_t)1 << 20) / n + 1;      // ~1M beads per launch
        // sorted indices stay 32-bit, items fit gridDim.y, the cell starts of a batch stay below 2^26 entries
        size_t const limit = std::min<size_t>(std::min<size_t>(65535, ((size_t)1 << 26) / cap), ((size_t)1 << 30) / n);
        unsigned const per_batch = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(want, limit), items.size()));
        CellIndex<Rec> &cc = h->centres, &pp = h->partners;
        int const is64 = h->hist.is_f64;
        for (size_t i0 = 0; i0 < items.size(); i0 += per_batch) {
            unsigned const nb_items = (unsigned)std::min<size_t>(per_batch, items.size() - i0);
            size_t const nb = (size_t)nb_items * n, slots = (size_t)nb_items * cap;
            const Item *batch = h->items_dev.p + i0;
            GDCHK(cc.room(nb_items, n, cap));
            GDCHK(pp.room(nb_items, n, cap));
            HIPCHK(h->timer.mark(0, st));
            PairFrames const fr{batch};
            GDCHK(pp.make_grids(st, h->hist.x(), is64, N, h->ls.sel.p, n, fr, nb_items, sp, cap));      // one grid for both frames of an item
            for (int partner = 0; partner < 2; partner++) {
                CellIndex<Rec> &ci = partner ? pp : cc;
                GDCHK(ci.make_keys(st, PositionFill<PairFrames>{h->hist.x(), is64, N, h->ls.labels(), fr, partner}, h->ls.sel.p, n, nb_items, pp.grids.p, sp.periodic, cap));
                GDCHK(ci.sort(st, nb, slots));
                HIPCHK(hipGetLastError());
            }
            unsigned n_work = 0;
            GDCHK(cc.work_items(who, st, &n_work));
            HIPCHK(h->timer.mark(1, st));
            if (n_work) {
                PairArgs a;
                a.edges2 = h->edges_dev.p;
                a.items = batch;
                a.B = B;
                a.K = K;
                a.cells = (unsigned)cells;
                a.tile = tile;
                a.cap = cap;
                a.table = h->table.p;
                dim3 const grid(n_work), block(kBlock);
                if (sp.periodic && lds)
                    hipLaunchKernelGGL((k_vh_pairs<true, true>), grid, block, shmem, st, cc.srec.p, cc.starts.p, cc.work.p, pp.srec.p, pp.starts.p, pp.grids.p, a);
                else if (sp.periodic)
                    hipLaunchKernelGGL((k_vh_pairs<true, false>), grid, block, shmem, st, cc.srec.p, cc.starts.p, cc.work.p, pp.srec.p, pp.starts.p, pp.grids.p, a);
                else if (lds)
                    hipLaunchKernelGGL((k_vh_pairs<false, true>), grid, block, shmem, st, cc.srec.p, cc.starts.p, cc.work.p, pp.srec.p, pp.starts.p, pp.grids.p, a);
                else
                    hipLaunchKernelGGL((k_vh_pairs<false, false>), grid, block, shmem, st, cc.srec.p, cc.starts.p, cc.work.p, pp.srec.p, pp.starts.p, pp.grids.p, a);
                HIPCHK(hipGetLastError());
            }
            HIPCHK(h->timer.mark(2, st));
            HIPCHK(hipStreamSynchronize(st));      // the events are marked again by the next batch
            double index = 0.0, count = 0.0;
            HIPCHK(h->timer.between(0, 1, &index));
            HIPCHK(h->timer.between(1, 2, &count));
            ms[0] += count;
            ms[1] += index;
        }
        HIPCHK(hipMemcpyAsync(counts, h->table.p, L * cells * sizeof(u64), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        std::memset(counts, 0, L * cells * sizeof(uint64_t));
    }
    if (origins) std::copy(pl.origins.begin(), pl.origins.end(), origins);
    std::copy(ms, ms + 3, h->timer.ms);
    return GD_OK;
}

int gd_vanhove_last_times(const gd_vanhove *h, double *count_ms, double *index_ms, double *other_ms)
{
    if (!h) return fail(GD_EINVAL, "gd_vanhove_last_times: NULL handle");
    h->timer.report(count_ms, index_ms, other_ms);
    return GD_OK;
}

}  // extern "C"
