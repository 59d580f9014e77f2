// gdyn_dcorr.hip -- the spatial correlation of bead displacements (include/gdyn_dcorr.h): per origin frame, pair class and
// distance bin, the number of pairs and the fixed-point sum of D_i . D_j.  Beyond the reference, which has no such analysis.
// The pair rules, the cell grid and the walk over it are gdyn_cells.hpp's, the history is gd::History's (gdyn_history.hpp).
//
// Per call:
//   k_dcorr_tmax   the largest squared displacement t2 of the selected beads over all origins of the call (integer atomicMax on the
//                  bit pattern of the non-negative double).  The host turns it into the scale S and refuses an illegal one before
//                  any pair is walked.
//   k_dcorr_self   per origin and label, the sum of llrint(t2 * 2^S) (LDS integer atomics per block, one global one per label).
// Per batch of origins (max_frames_per_launch; no result depends on it):
//   gd::CellIndex  (gdyn_cells.hpp) the cells of each origin, of side >= max_distance (1 + kCellSlack) and at most `cap` a frame, the
//                  beads in (origin, cell) order as 64-byte records (position, D, label, chain), the first sorted index of every cell
//                  and one work item per kCellChunk centres of a non-empty cell (their order is arbitrary: the sums are integers)
//   Fill           between its steps, for k_cells_keys: gathers the selected beads of each origin and computes D in fp64
//   k_dcorr_pairs  the hot path: the tile walk of gdyn_cells.hpp over seven of a record's eight words (x y z Dx Dy Dz and label|chain),
//                  from the sorted index after the block's first centre on: only partners later in sorted order count, so every
//                  unordered pair is seen once.  The body reads the positions of four partners first and D and the labels only for
//                  the ~15 % of partners inside the cutoff.  Pairs go to a block histogram in LDS (uint32 counts, 64-bit sums) whose
//                  non-zero cells are flushed with one 64-bit integer global atomic each (a signed sum added as two's complement
//                  through the unsigned atomic is exact); above GD_DCORR_LDS_BINS cells every pair goes to global memory directly.
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics: every table is an integer sum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_dcorr.h"
#include "gdyn_analysis.hpp"
#include "gdyn_cells.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"
#include "gdyn_types.h"

using namespace gd;

namespace {

constexpr int kBlock = kCellBlock;
constexpr unsigned kTileWords = 7;           // words of a record that are staged: x y z Dx Dy Dz label|chain
constexpr unsigned kUnroll = 4;              // partners of a lane whose positions are read together

struct Rec {      // one selected bead of one origin
    double p[3];
    double d[3];
    int label;
    unsigned chain;
    unsigned pad[2];
};
static_assert(sizeof(Rec) == 64, "a record is 64 bytes");

// t2 of selected bead k at origin o (and D)
__device__ inline double disp_of(const void *__restrict__ xyz, int is_f64, unsigned N, unsigned bead, unsigned f, unsigned lag, double p[3], double d[3])
{
    double q[3];
    load3(xyz, is_f64, ((size_t)f * N + bead) * 3, p);
    load3(xyz, is_f64, ((size_t)(f + lag) * N + bead) * 3, q);
    for (int a = 0; a < 3; a++) d[a] = q[a] - p[a];
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

__global__ void __launch_bounds__(kBlock) k_dcorr_tmax(const void *__restrict__ xyz, int is_f64, unsigned N, const unsigned *__restrict__ sel,
                                                       unsigned n_sel, unsigned lag, FrameSel og, unsigned long long *__restrict__ tmax)
{
    __shared__ double sh[kBlock / 64];
    double t2 = 0.0;
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < (size_t)og.count * n_sel; idx += (size_t)gridDim.x * kBlock) {
        unsigned const o = (unsigned)(idx / n_sel), k = (unsigned)(idx % n_sel);
        double p[3], d[3];
        t2 = fmax(t2, disp_of(xyz, is_f64, N, sel[k], og.first + o * og.stride, lag, p, d));
    }
    t2 = block_max(t2, sh);      // (finite coordinates: never NaN; an overflow is +inf, the largest pattern)
    if (threadIdx.x == 0 && t2 > 0.0) atomicMax(tmax, (unsigned long long)__double_as_longlong(t2));
}

// self_sum[o, label] += llrint(t2 * scale); grid (blocks over the selection, origins of this launch)
__global__ void __launch_bounds__(kBlock) k_dcorr_self(const void *__restrict__ xyz, int is_f64, unsigned N, const unsigned *__restrict__ sel,
                                                       const int *__restrict__ label, unsigned n_sel, unsigned lag, FrameSel og, unsigned o0,
                                                       double scale, unsigned K, unsigned long long *__restrict__ self_sum)
{
    __shared__ unsigned long long acc[GD_DCORR_MAX_LABELS];
    if (threadIdx.x < GD_DCORR_MAX_LABELS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned const o = o0 + blockIdx.y, k = blockIdx.x * kBlock + threadIdx.x;
    if (k < n_sel) {
        unsigned const bead = sel[k];
        double p[3], d[3];
        double const t2 = disp_of(xyz, is_f64, N, bead, og.first + o * og.stride, lag, p, d);
        atomicAdd(&acc[label ? label[bead] : 0], (unsigned long long)llrint(t2 * scale));
    }
    __syncthreads();
    if (threadIdx.x < K && acc[threadIdx.x]) atomicAdd(&self_sum[(size_t)o * K + threadIdx.x], acc[threadIdx.x]);
}

struct Fill {      // k_cells_keys: the record of a bead at origin o0 + o of the batch
    const void *xyz;
    int is_f64;
    unsigned N;
    const int *label;
    const unsigned *chain;
    unsigned lag;
    BatchFrames fr;
    __device__ void operator()(unsigned o, unsigned bead, Rec &r) const
    {
        (void)disp_of(xyz, is_f64, N, bead, fr.frame(o, 0), lag, r.p, r.d);
        r.label = label ? label[bead] : 0;
        r.chain = chain ? chain[bead] : 0u;
        r.pad[0] = r.pad[1] = 0u;
    }
};

struct PairArgs {
    double md2, inv_bw, scale;
    unsigned n_bins, K, split, cells;      // cells = P * n_bins
    unsigned tile, cap;
    unsigned long long *counts, *sums;     // (B, P, n_bins)
};

template <bool kPeriodic, bool kLds>
__global__ void __launch_bounds__(kBlock) k_dcorr_pairs(const Rec *__restrict__ srec, const unsigned *__restrict__ starts, const uint2 *__restrict__ work,
                                                        const Grid *__restrict__ grids, PairArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    unsigned const stride = a.tile + kCellTilePad;
    double *tx = reinterpret_cast<double *>(smem);      // [kTileWords][stride]
    unsigned long long *tmeta = smem + 6 * (size_t)stride;
    unsigned long long *hsum = smem + kTileWords * (size_t)stride;
    unsigned *hcount = reinterpret_cast<unsigned *>(hsum + (kLds ? a.cells : 0));

    CellWork const cw = cell_work(work[blockIdx.x], starts, a.cap);
    Grid const g = grids[cw.o];
    unsigned const s = cw.s_begin + cw.ci, gs = cw.gs;
    Rec q;
    if (cw.active) q = srec[s];
    if (kLds) {
        for (unsigned e = threadIdx.x; e < a.cells; e += kBlock) {
            hsum[e] = 0ull;
            hcount[e] = 0u;
        }
    }
    unsigned long long *gcount = a.counts + (size_t)cw.o * a.cells, *gsum = a.sums + (size_t)cw.o * a.cells;

    // partners later in sorted order only
    cell_tile_walk<kPeriodic, kTileWords, 8>(g, cw.cell, starts + (size_t)cw.o * a.cap, cw.s_begin + 1u, srec, smem, a.tile, cw.active, [&](unsigned j0, unsigned nt) {
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
                if (!(r2[u] < a.md2)) continue;
                unsigned const k = k0 + u * gs;
                unsigned long long const bin = (unsigned long long)(sqrt(r2[u]) * a.inv_bw);
                if (bin >= a.n_bins) continue;
                double const dot = (q.d[0] * tx[3 * stride + k] + q.d[1] * tx[4 * stride + k]) + q.d[2] * tx[5 * stride + k];
                unsigned long long const term = (unsigned long long)llrint(dot * a.scale);
                unsigned long long const meta = tmeta[k];
                unsigned const lj = (unsigned)(meta & 0xffffffffu), chj = (unsigned)(meta >> 32);
                unsigned p = pair_class((unsigned)q.label, lj, a.K);
                if (a.split) p = 2u * p + (q.chain != chj ? 1u : 0u);
                unsigned const e = p * a.n_bins + (unsigned)bin;
                if (kLds) {
                    atomicAdd(&hcount[e], 1u);
                    atomicAdd(&hsum[e], term);
                } else {
                    atomicAdd(&gcount[e], 1ull);
                    atomicAdd(&gsum[e], term);
                }
            }
        }
    });
    if (kLds) {
        __syncthreads();
        for (unsigned e = threadIdx.x; e < a.cells; e += kBlock) {
            unsigned const c = hcount[e];
            if (c) {
                atomicAdd(&gcount[e], (unsigned long long)c);
                if (hsum[e]) atomicAdd(&gsum[e], hsum[e]);
            }
        }
    }
}

// the dynamic LDS a block of k_dcorr_pairs may ask for (gd::lds_opt_in).  A refusal only makes the tiles and the LDS histogram smaller.
int lds_budget(int device)
{
    static DeviceOnce<> once;
    return lds_opt_in(once, device, {reinterpret_cast<const void *>(&k_dcorr_pairs<false, false>), reinterpret_cast<const void *>(&k_dcorr_pairs<false, true>),
                                     reinterpret_cast<const void *>(&k_dcorr_pairs<true, false>), reinterpret_cast<const void *>(&k_dcorr_pairs<true, true>)});
}

size_t tile_bytes(unsigned tile) { return (size_t)kTileWords * (tile + kCellTilePad) * 8; }

// max(n (n - 1) / 2, 1) * (M * 2^S + 1) < 2^62, exactly (M = m * 2^e with a 53-bit integer m)
bool scale_legal(uint64_t n, double M, int S)
{
    if (!(M >= 0.0) || !std::isfinite(M)) return false;
    typedef unsigned __int128 u128;
    u128 const lim = (u128)1 << 62, pairs = std::max<u128>((u128)n * (n ? n - 1 : 0) / 2, 1);
    if (M == 0.0) return pairs < lim;
    int e = 0;
    uint64_t const m = (uint64_t)std::ldexp(std::frexp(M, &e), 53);
    int const sh = e - 53 + S;
    if (sh >= 0) {
        if (sh >= 62) return false;
        u128 const v = (u128)m << sh;
        return v < lim && pairs * (v + 1) < lim;
    }
    int const k = -sh;
    if (k >= 64) return pairs * 2 < lim;      // M * 2^S < 2^-11
    return pairs * ((u128)m + ((u128)1 << k)) < (lim << k);
}

}  // namespace

struct gd_dcorr : gd::handle {
    unsigned max_frames = 0;
    int lds_bytes = 64 * 1024;
    History hist;
    // selection: labels and chains, which belong to hist.beads()
    LabelSelection ls;
    bool have_chains = false;
    dbuf<unsigned> chain_dev;
    // per call
    dbuf<unsigned long long> tmax, self_sum;
    // per batch
    CellIndex<Rec> cells;
    dbuf<unsigned long long> counts, sums;

    unsigned P() const { return ls.K * (ls.K + 1) / 2 * (have_chains ? 2u : 1u); }
};

namespace {

History::Rebind rebind(gd_dcorr *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads() || !h->ls.sel.p) {      // labels and chains belonged to another N
            GDCHK(h->ls.select_all(n_beads));
            h->have_chains = false;
        }
        return GD_OK;
    };
}

uint32_t origins_of(const gd_dcorr *h, uint32_t lag, uint32_t first, uint32_t n_origins, uint32_t stride)
{
    if (!h || !h->hist.frames() || !stride || !lag) return 0;
    return (uint32_t)frames_served(frames_fit(h->hist.frames(), first, stride, lag), n_origins);
}

struct Call {      // what a batch needs of its call
    unsigned lag;
    FrameSel og;
    Space sp;
    double bin_width, md, scale;
    unsigned n_bins, cap;
    bool lds;
    unsigned tile;
};

int run_batch(gd_dcorr *h, const Call &c, unsigned o0, unsigned B, uint64_t *count_out, int64_t *sum_out)
{
    hipStream_t st = h->stream;
    CellIndex<Rec> &ci = h->cells;
    unsigned const n = h->ls.n_sel;
    size_t const nb = (size_t)B * n, slots = (size_t)B * c.cap, cells = (size_t)h->P() * c.n_bins;
    GDCHK(ci.room(B, n, c.cap));
    HIPCHK(h->counts.ensure((size_t)B * cells));
    HIPCHK(h->sums.ensure((size_t)B * cells));
    const unsigned *chain = h->have_chains ? h->chain_dev.p : nullptr;
    int const is64 = h->hist.is_f64;
    BatchFrames const fr{c.og, o0};
    GDCHK(ci.make_grids(st, h->hist.x(), is64, h->hist.beads(), h->ls.sel.p, n, fr, B, c.sp, c.cap));
    GDCHK(ci.make_keys(st, Fill{h->hist.x(), is64, h->hist.beads(), h->ls.labels(), chain, c.lag, fr}, h->ls.sel.p, n, B, ci.grids.p, c.sp.periodic, c.cap));
    GDCHK(ci.sort(st, nb, slots));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(h->counts.p, 0, (size_t)B * cells * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(h->sums.p, 0, (size_t)B * cells * sizeof(unsigned long long), st));
    unsigned n_work = 0;
    GDCHK(ci.work_items("gd_dcorr_pairs", st, &n_work));
    if (n_work) {
        PairArgs a;
        a.md2 = c.md * c.md;
        a.inv_bw = 1 / c.bin_width;
        a.scale = c.scale;
        a.n_bins = c.n_bins;
        a.K = h->ls.K;
        a.split = h->have_chains;
        a.cells = (unsigned)cells;
        a.tile = c.tile;
        a.cap = c.cap;
        a.counts = h->counts.p;
        a.sums = h->sums.p;
        size_t const shmem = tile_bytes(c.tile) + (c.lds ? cells * 12 : 0);
        dim3 const grid(n_work), block(kBlock);
        if (c.sp.periodic && c.lds)
            hipLaunchKernelGGL((k_dcorr_pairs<true, true>), grid, block, shmem, st, ci.srec.p, ci.starts.p, ci.work.p, ci.grids.p, a);
        else if (c.sp.periodic)
            hipLaunchKernelGGL((k_dcorr_pairs<true, false>), grid, block, shmem, st, ci.srec.p, ci.starts.p, ci.work.p, ci.grids.p, a);
        else if (c.lds)
            hipLaunchKernelGGL((k_dcorr_pairs<false, true>), grid, block, shmem, st, ci.srec.p, ci.starts.p, ci.work.p, ci.grids.p, a);
        else
            hipLaunchKernelGGL((k_dcorr_pairs<false, false>), grid, block, shmem, st, ci.srec.p, ci.starts.p, ci.work.p, ci.grids.p, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(count_out, h->counts.p, (size_t)B * cells * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(sum_out, h->sums.p, (size_t)B * cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_dcorr_abi_version(void) { return GD_DCORR_ABI_VERSION; }

uint32_t gd_dcorr_bins(double bin_width, double max_distance)
{
    if (!(bin_width > 0.0) || !(max_distance > 0.0) || !std::isfinite(bin_width) || !std::isfinite(max_distance)) return 0;
    double const n = std::ceil(max_distance / bin_width);
    return n >= 1.0 && n <= (double)GD_DCORR_MAX_BINS ? (uint32_t)n : 0u;
}

int gd_dcorr_create(const gd_dcorr_desc *desc, gd_dcorr **out)
{
    if (int rc = gd::open("gd_dcorr_create", desc, out)) return rc;
    (*out)->max_frames = desc->max_frames_per_launch;
    (*out)->lds_bytes = lds_budget(desc->device);
    return GD_OK;
}

int gd_dcorr_destroy(gd_dcorr *h) { return gd::close(h); }

int gd_dcorr_set_history(gd_dcorr *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_dcorr_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_dcorr_set_history_live(gd_dcorr *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_dcorr_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_dcorr_set_labels(gd_dcorr *h, const int32_t *label, uint32_t n_labels)
{
    const char *who = "gd_dcorr_set_labels";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the labels are N values of its beads)", who);
    return h->ls.set(who, h->device, label, n_labels, GD_DCORR_MAX_LABELS, h->hist.beads());
}

int gd_dcorr_set_chains(gd_dcorr *h, const uint32_t *chain_id)
{
    const char *who = "gd_dcorr_set_chains";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the chains are N values of its beads)", who);
    if (!chain_id) {
        h->have_chains = false;
        return GD_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    dbuf<unsigned> dev;
    HIPCHK(dev.upload(chain_id, h->hist.beads()));
    h->chain_dev = std::move(dev);
    h->have_chains = true;
    return GD_OK;
}

uint32_t gd_dcorr_classes(const gd_dcorr *h) { return h ? h->P() : 0u; }

uint32_t gd_dcorr_origins(const gd_dcorr *h, uint32_t lag, uint32_t first_origin, uint32_t n_origins, uint32_t origin_stride)
{
    return origins_of(h, lag, first_origin, n_origins, origin_stride);
}

int gd_dcorr_pairs(gd_dcorr *h, uint32_t lag, uint32_t first_origin, uint32_t n_origins, uint32_t origin_stride, const double *box, double bin_width,
                   double max_distance, int32_t scale_bits, int32_t *scale_used, uint64_t *count_out, int64_t *sum_out, uint64_t *self_count_out,
                   int64_t *self_sum_out)
{
    const char *who = "gd_dcorr_pairs";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (lag == 0) return fail(GD_EINVAL, "%s: lag 0", who);
    if (origin_stride == 0) return fail(GD_EINVAL, "%s: origin stride 0", who);
    if (n_origins && (uint64_t)first_origin + (uint64_t)(n_origins - 1) * origin_stride + lag >= h->hist.frames())
        return fail(GD_EINVAL, "%s: origin %llu with lag %u lies beyond the %u frames", who,
                    (unsigned long long)first_origin + (unsigned long long)(n_origins - 1) * origin_stride, lag, h->hist.frames());
    if (box)
        for (int a = 0; a < 3; a++)
            if (!(box[a] > 0.0) || !std::isfinite(box[a])) return fail(GD_EINVAL, "%s: box[%d] = %g is not positive and finite", who, a, box[a]);
    unsigned const n_bins = gd_dcorr_bins(bin_width, max_distance);
    if (!n_bins)
        return fail(GD_EINVAL, "%s: bin width %g and max distance %g must be positive and finite, with at most %u bins", who, bin_width, max_distance,
                    GD_DCORR_MAX_BINS);
    if (scale_bits != 0 && scale_bits != GD_DCORR_SCALE_UNIT && (scale_bits < 0 || scale_bits > GD_DCORR_MAX_SCALE_BITS))
        return fail(GD_EINVAL, "%s: scale_bits %d (0: automatic, 1 to %d, or GD_DCORR_SCALE_UNIT)", who, scale_bits, GD_DCORR_MAX_SCALE_BITS);
    size_t const cells = (size_t)h->P() * n_bins;
    if (cells > (1u << 30)) return fail(GD_EINVAL, "%s: %u classes of %u bins exceed 2^30 cells", who, h->P(), n_bins);
    FrameSel const og{first_origin, origin_stride, origins_of(h, lag, first_origin, n_origins, origin_stride)};
    if (og.count && (!count_out || !sum_out)) return fail(GD_EINVAL, "%s: NULL output", who);
    if ((self_count_out == nullptr) != (self_sum_out == nullptr)) return fail(GD_EINVAL, "%s: one self output without the other", who);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    unsigned const n = h->ls.n_sel, K = h->ls.K;
    const int *label = h->ls.labels();

    // the largest t2 of the call, then the scale
    double M = 0.0;
    if (og.count && n) {
        HIPCHK(h->tmax.ensure(1));
        HIPCHK(hipMemsetAsync(h->tmax.p, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_dcorr_tmax, dim3(std::min(blocks_for((size_t)og.count * n, kBlock), 2048u)), dim3(kBlock), 0, st, h->hist.x(), (int)h->hist.is_f64, h->hist.beads(), h->ls.sel.p, n, lag,
                           og, h->tmax.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&M, h->tmax.p, sizeof M, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    int S = scale_bits == GD_DCORR_SCALE_UNIT ? 0 : scale_bits;
    if (scale_bits == 0) {
        S = GD_DCORR_MAX_SCALE_BITS;
        while (S >= 0 && !scale_legal(n, M, S)) S--;
        if (S < 0) return fail(GD_EINVAL, "%s: the largest squared displacement %g of %u beads overflows the sums at every scale", who, M, n);
    } else if (!scale_legal(n, M, S)) {
        return fail(GD_EINVAL, "%s: scale 2^%d overflows the sums of %u beads whose largest squared displacement is %g", who, S, n, M);
    }
    if (scale_used) *scale_used = S;
    if (!og.count) return GD_OK;
    double const scale = std::ldexp(1.0, S);

    if (self_sum_out) {
        for (unsigned o = 0; o < og.count; o++)
            for (unsigned l = 0; l < K; l++) self_count_out[(size_t)o * K + l] = h->ls.members[l];
        std::memset(self_sum_out, 0, (size_t)og.count * K * sizeof(int64_t));
        if (n) {
            HIPCHK(h->self_sum.ensure((size_t)og.count * K));
            HIPCHK(hipMemsetAsync(h->self_sum.p, 0, (size_t)og.count * K * sizeof(unsigned long long), st));
            for (unsigned o0 = 0; o0 < og.count; o0 += 65535u)
                hipLaunchKernelGGL(k_dcorr_self, dim3(blocks_for(n, kBlock), std::min(65535u, og.count - o0)), dim3(kBlock), 0, st, h->hist.x(), (int)h->hist.is_f64,
                                   h->hist.beads(), h->ls.sel.p, label, n, lag, og, o0, scale, K, h->self_sum.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(self_sum_out, h->self_sum.p, (size_t)og.count * K * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    if (n < 2) {      // nothing to pair
        std::memset(count_out, 0, (size_t)og.count * cells * sizeof(uint64_t));
        std::memset(sum_out, 0, (size_t)og.count * cells * sizeof(int64_t));
        return GD_OK;
    }

    Call c;
    c.lag = lag;
    c.og = og;
    c.sp.periodic = box != nullptr;
    for (int a = 0; a < 3; a++) c.sp.box[a] = box ? box[a] : 0.0;
    c.sp.cell_side = max_distance * (1.0 + kCellSlack);
    c.bin_width = bin_width;
    c.md = max_distance;
    c.scale = scale;
    c.n_bins = n_bins;
    c.cap = std::max(4096u, n);
    // the histogram in LDS: a block adds at most kCellChunk * n to one uint32 counter; the tile takes what the table leaves, 64 to 256 records
    c.tile = 256;
    c.lds = cells <= GD_DCORR_LDS_BINS && n < (1u << 24) && cells * 12 + tile_bytes(64) <= (size_t)h->lds_bytes;
    while (c.tile > 64 && tile_bytes(c.tile) + (c.lds ? cells * 12 : 0) > (size_t)h->lds_bytes) c.tile /= 2;
    size_t const want = h->max_frames ? h->max_frames : ((size_t)1 << 20) / n + 1;      // ~1M beads per launch
    // sorted indices stay 32-bit, origins fit gridDim.y, the cell starts of a batch stay below 2^26 entries
    size_t const limit = std::min<size_t>(std::min<size_t>(65535, ((size_t)1 << 26) / c.cap), ((size_t)1 << 30) / n);
    unsigned const B = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(want, limit), og.count));
    for (unsigned o0 = 0; o0 < og.count; o0 += B) {
        unsigned const b = std::min(B, og.count - o0);
        if (int rc = run_batch(h, c, o0, b, count_out + (size_t)o0 * cells, sum_out + (size_t)o0 * cells)) return rc;
    }
    return GD_OK;
}

}  // extern "C"
