// gdyn_dmap.hip -- distance and contact-frequency maps of a trajectory history (include/gdyn_dmap.h): for every pair of bins the sums
// of r and r2 over the bead pairs and the frames, and the number of pairs closer than each threshold.  Beyond the reference, and
// the first dense all-pairs kernel of this code base: every other pair kernel walks cells.
//
// The bins are tiled in a grid that is fixed by the bins alone: tile t holds the bins [16 t, 16 t + 16).  A call lists the *canonical*
// tiles (ta <= tb) that its rectangle touches, each once; a tile below the diagonal is the transpose of one above it.
//
//   k_dmap_tile<T, BOX, SQRT>   one block per (canonical tile, frame range of GD_DMAP_FRAME_RANGE frames), one lane per cell (a of
//                    tile ta, b of tile tb; on a diagonal tile lane (p, q) takes a = min, b = max, so both lanes of a mirrored
//                    pair run the same instructions on the same data).  The lane keeps sum1, sum2 and the hit counters in registers
//                    and walks its cell serially: pieces u of a, pieces v of b, frames, beads i of the piece of a, beads j of the
//                    piece of b (the order the header states).  For each (u, v) the block stages piece u of its 16 a-bins and piece v
//                    of its 16 b-bins through LDS, `chunk` frames at a time (max_frames_per_stage); the accumulators live across the
//                    chunks, so no bit depends on the chunk.  LDS holds a structure of arrays in the stored type,
//                    [frame][side][axis][bin slot][bead of the piece], with an odd number of elements per bin slot: the 16 bin slots
//                    that the lanes of a half wave read in one instruction lie on different banks (8-byte and 4-byte reads alike), and
//                    lanes of one slot read one address (a broadcast).  The terms of kAhead = 4 partners j are computed side by
//                    side, so that their reads and square roots overlap, and added one by one in ascending j.
//   k_dmap_reduce    adds a cell's partial sums over the frame ranges in ascending order and writes the cell where the rectangle
//                    holds it, and its mirror image where the rectangle holds that.
// The history itself (upload, non-finite check) is gd::History's (gdyn_history.hpp).
// Hit counters are 32-bit while one (u, v) pair of pieces is walked over one frame range: at most GD_DMAP_FRAME_RANGE *
// GD_DMAP_PIECE_BEADS^2 = 2^16 terms, far below 2^32; they are added to 64-bit counters after each pair of pieces.
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_dmap.h"
#include "gdyn_analysis.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr unsigned kTB = 16;                         // bins of a tile side; kTB * kTB == kBlock
constexpr unsigned kRange = GD_DMAP_FRAME_RANGE;
constexpr unsigned kPiece = GD_DMAP_PIECE_BEADS;
constexpr unsigned kMaxT = GD_DMAP_MAX_THRESHOLDS;
constexpr unsigned kWords = 2 + kMaxT;               // 8-byte words a lane leaves per frame range: sum1, sum2, hits[4]
constexpr size_t kPartialBytes = (size_t)1 << 30;    // tiles are walked in batches whose partial sums fit this
constexpr size_t kAutoStageBytes = 40 * 1024;        // automatic chunk: four blocks per CU keep 16 waves resident
constexpr size_t kStaticLds = 2 * kTB * 2 * sizeof(unsigned);      // the tile's bin table, next to the staged frames
static_assert(kTB * kTB == kBlock, "one lane per cell");
static_assert((unsigned long long)kRange * kPiece * kPiece < (1ull << 32), "32-bit hit counters of a pair of pieces");

struct MapArgs {
    const void *x;                  // the history, (F, N, 3) of T
    const uint32_t *bins;           // (B, 2)
    const uint2 *tiles;             // canonical tiles (ta <= tb) of this launch
    unsigned long long *partial;    // (ranges, tiles, kWords, kBlock) words; doubles as their bit patterns
    unsigned N, B;
    unsigned f0, f1;                // the frame window [f0, f1)
    unsigned g0;                    // the first frame range of the window
    unsigned chunk;                 // frames staged at once
    unsigned L, S;                  // beads of a staged piece (the longest bin, at most kPiece) and elements per bin slot (odd)
    double box[3];
    double thr2[kMaxT];             // thr * thr; -1 for a threshold that is not asked for (no r2 lies below it)
};

constexpr unsigned kAhead = 4;      // partners whose terms are computed side by side

// the pair term of the header: r2 of a bead at (ax, ay, az) and one at (bx, by, bz)
template <bool BOX>
__device__ inline double pair_r2(double ax, double ay, double az, double bx, double by, double bz, const double (&box)[3])
{
    double dx = ax - bx, dy = ay - by, dz = az - bz;
    if (BOX) {
        dx -= box[0] * nearbyint(dx / box[0]);
        dy -= box[1] * nearbyint(dy / box[1]);
        dz -= box[2] * nearbyint(dz / box[2]);
    }
    return (dx * dx + dy * dy) + dz * dz;
}

template <typename T, bool BOX, bool SQRT>
__global__ void __launch_bounds__(kBlock) k_dmap_tile(MapArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned s_bin[2][kTB][2];
    T *lds = reinterpret_cast<T *>(smem);
    const T *x = static_cast<const T *>(p.x);
    uint2 const tile = p.tiles[blockIdx.x];
    unsigned const tid = threadIdx.x;
    if (tid < 2 * kTB) {
        unsigned const side = tid / kTB, s = tid % kTB, bin = (side ? tile.y : tile.x) * kTB + s;
        s_bin[side][s][0] = bin < p.B ? p.bins[2 * bin] : 0;
        s_bin[side][s][1] = bin < p.B ? p.bins[2 * bin + 1] : 0;
    }
    __syncthreads();
    unsigned nU = 0, nV = 0;      // pieces of the longest bin of either side
    for (unsigned s = 0; s < kTB; s++) {
        nU = max(nU, (s_bin[0][s][1] - s_bin[0][s][0] + kPiece - 1) / kPiece);
        nV = max(nV, (s_bin[1][s][1] - s_bin[1][s][0] + kPiece - 1) / kPiece);
    }
    unsigned const P = tid / kTB, Q = tid % kTB;
    bool const diag = tile.x == tile.y;
    unsigned const a = diag ? min(P, Q) : P, b = diag ? max(P, Q) : Q;
    unsigned const aS = s_bin[0][a][0], aE = s_bin[0][a][1], bS = s_bin[1][b][0], bE = s_bin[1][b][1];
    // staging: eight lanes per (side, bin slot)
    unsigned const st_side = tid / (8 * kTB), st_slot = tid / 8 % kTB, st_lane = tid % 8;
    unsigned const st_start = s_bin[st_side][st_slot][0], st_end = s_bin[st_side][st_slot][1];

    unsigned const g = p.g0 + blockIdx.y;
    unsigned const F0 = max(p.f0, g * kRange), F1 = min(p.f1, (g + 1) * kRange);
    unsigned const S = p.S, side_stride = 3 * kTB * S, frame_stride = 2 * side_stride, axis_stride = kTB * S;

    double sum1 = 0.0, sum2 = 0.0;
    unsigned long long hits[kMaxT] = {0, 0, 0, 0};
    for (unsigned u = 0; u < nU; u++)
        for (unsigned v = 0; v < nV; v++) {
            unsigned const a0 = aS + u * kPiece, b0 = bS + v * kPiece;
            unsigned const la = a0 < aE ? min(kPiece, aE - a0) : 0, lb = b0 < bE ? min(kPiece, bE - b0) : 0;
            unsigned const st0 = st_start + (st_side ? v : u) * kPiece;
            unsigned const st_n = st0 < st_end ? 3 * min(kPiece, st_end - st0) : 0;
            unsigned hl[kMaxT] = {0, 0, 0, 0};
            for (unsigned fc = F0; fc < F1; fc += p.chunk) {
                unsigned const nf = min(p.chunk, F1 - fc);
                __syncthreads();      // the last chunk has been read
                for (unsigned f = 0; f < nf; f++) {
                    const T *src = x + ((size_t)(fc + f) * p.N + st0) * 3;
                    T *dst = lds + f * frame_stride + st_side * side_stride + st_slot * S;
                    for (unsigned e = st_lane; e < st_n; e += 8) dst[e % 3 * axis_stride + e / 3] = src[e];
                }
                __syncthreads();
                if (la == 0 || lb == 0) continue;
                for (unsigned f = 0; f < nf; f++) {
                    const T *A = lds + f * frame_stride + a * S, *Bp = lds + f * frame_stride + side_stride + b * S;
                    for (unsigned i = 0; i < la; i++) {
                        double const ax = (double)A[i], ay = (double)A[axis_stride + i], az = (double)A[2 * axis_stride + i];
                        unsigned const self = a0 + i - b0;      // the place of bead a0 + i in the piece of b, if it is there
                        unsigned j = 0;
                        // four partners at a time: their reads, differences and square roots are independent and overlap; the sums
                        // are still added one by one in ascending j.  The bead itself adds +0, which changes no bit of a sum >= +0
                        for (; j + kAhead <= lb; j += kAhead) {
                            double r2[kAhead];
#pragma unroll
                            for (unsigned k = 0; k < kAhead; k++)
                                r2[k] = pair_r2<BOX>(ax, ay, az, (double)Bp[j + k], (double)Bp[axis_stride + j + k], (double)Bp[2 * axis_stride + j + k], p.box);
#pragma unroll
                            for (unsigned k = 0; k < kAhead; k++) {
                                bool const other = j + k != self;
                                double const v = other ? r2[k] : 0.0;
                                sum2 += v;
                                if (SQRT) sum1 += sqrt(v);
#pragma unroll
                                for (unsigned t = 0; t < kMaxT; t++) hl[t] += other && r2[k] < p.thr2[t] ? 1u : 0u;
                            }
                        }
                        for (; j < lb; j++) {
                            if (j == self) continue;
                            double const r2 = pair_r2<BOX>(ax, ay, az, (double)Bp[j], (double)Bp[axis_stride + j], (double)Bp[2 * axis_stride + j], p.box);
                            sum2 += r2;
                            if (SQRT) sum1 += sqrt(r2);
#pragma unroll
                            for (unsigned t = 0; t < kMaxT; t++) hl[t] += r2 < p.thr2[t] ? 1u : 0u;
                        }
                    }
                }
            }
#pragma unroll
            for (unsigned t = 0; t < kMaxT; t++) hits[t] += hl[t];
        }
    unsigned long long *mine = p.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kWords * kBlock + tid;
    mine[0] = (unsigned long long)__double_as_longlong(sum1);
    mine[kBlock] = (unsigned long long)__double_as_longlong(sum2);
#pragma unroll
    for (unsigned t = 0; t < kMaxT; t++) mine[(2 + t) * kBlock] = hits[t];
}

struct ReduceArgs {
    const unsigned long long *partial;
    const uint2 *tiles;
    unsigned long long *out;        // (kWords, n_rows, n_cols) words
    unsigned ranges, n_tiles, B;
    unsigned row_first, n_rows, col_first, n_cols;
};

__global__ void __launch_bounds__(kBlock) k_dmap_reduce(ReduceArgs p)
{
    uint2 const tile = p.tiles[blockIdx.x];
    unsigned const tid = threadIdx.x, P = tid / kTB, Q = tid % kTB;
    unsigned const r = tile.x * kTB + P, c = tile.y * kTB + Q;
    if (r >= p.B || c >= p.B) return;
    const unsigned long long *mine = p.partial + (size_t)blockIdx.x * kWords * kBlock + tid;
    size_t const range_stride = (size_t)p.n_tiles * kWords * kBlock;
    unsigned long long w[kWords];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (unsigned t = 0; t < kMaxT; t++) w[2 + t] = 0;
    for (unsigned g = 0; g < p.ranges; g++) {      // ascending ranges; the first is added to +0, which changes no bit of a sum >= 0
        s1 += __longlong_as_double((long long)mine[g * range_stride]);
        s2 += __longlong_as_double((long long)mine[g * range_stride + kBlock]);
#pragma unroll
        for (unsigned t = 0; t < kMaxT; t++) w[2 + t] += mine[g * range_stride + (2 + t) * kBlock];
    }
    w[0] = (unsigned long long)__double_as_longlong(s1);
    w[1] = (unsigned long long)__double_as_longlong(s2);
    size_t const plane = (size_t)p.n_rows * p.n_cols;
    unsigned rr = r - p.row_first, cc = c - p.col_first;      // unsigned: a cell before the rectangle wraps to a large value
    if (rr < p.n_rows && cc < p.n_cols)
#pragma unroll
        for (unsigned k = 0; k < kWords; k++) p.out[k * plane + (size_t)rr * p.n_cols + cc] = w[k];
    if (tile.x != tile.y) {
        rr = c - p.row_first;
        cc = r - p.col_first;
        if (rr < p.n_rows && cc < p.n_cols)
#pragma unroll
            for (unsigned k = 0; k < kWords; k++) p.out[k * plane + (size_t)rr * p.n_cols + cc] = w[k];
    }
}

template <typename T, bool BOX, bool SQRT>
const void *tile_kernel()
{
    return reinterpret_cast<const void *>(&k_dmap_tile<T, BOX, SQRT>);
}

// the dynamic LDS a block of k_dmap_tile may ask for (gd::lds_opt_in).  A refusal only makes the chunks smaller.
int lds_budget(int device)
{
    static DeviceOnce<> once;
    return lds_opt_in(once, device, {tile_kernel<float, false, false>(), tile_kernel<float, false, true>(), tile_kernel<float, true, false>(),
                                     tile_kernel<float, true, true>(), tile_kernel<double, false, false>(), tile_kernel<double, false, true>(),
                                     tile_kernel<double, true, false>(), tile_kernel<double, true, true>()});
}

template <typename T, bool BOX>
void launch_tile(bool want_sqrt, dim3 grid, size_t lds, hipStream_t stream, const MapArgs &a)
{
    if (want_sqrt) hipLaunchKernelGGL((k_dmap_tile<T, BOX, true>), grid, dim3(kBlock), lds, stream, a);
    else hipLaunchKernelGGL((k_dmap_tile<T, BOX, false>), grid, dim3(kBlock), lds, stream, a);
}

}  // namespace

struct gd_dmap : gd::handle {
    unsigned knob = 0;
    int lds_bytes = 64 * 1024;
    History hist;
    BeadRanges bins;               // of hist.beads(); every bead its own bin without bins of the caller's
    // per call
    dbuf<uint2> tiles_dev;
    dbuf<unsigned long long> partial, out;

    unsigned B() const { return bins.count(); }
};

namespace {

History::Rebind rebind(gd_dmap *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads() || h->bins.host.empty()) GDCHK(h->bins.every_bead(n_beads));      // bins belonged to another N
        return GD_OK;
    };
}

}  // namespace

extern "C" {

int gd_dmap_abi_version(void) { return GD_DMAP_ABI_VERSION; }

int gd_dmap_create(const gd_dmap_desc *desc, gd_dmap **out)
{
    if (int rc = gd::open("gd_dmap_create", desc, out)) return rc;
    (*out)->knob = desc->max_frames_per_stage;
    (*out)->lds_bytes = lds_budget(desc->device);
    return GD_OK;
}

int gd_dmap_destroy(gd_dmap *h) { return gd::close(h); }

int gd_dmap_set_history(gd_dmap *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_dmap_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_dmap_set_history_live(gd_dmap *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_dmap_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_dmap_set_bins(gd_dmap *h, const uint32_t *ranges, uint32_t n_bins)
{
    const char *who = "gd_dmap_set_bins";
    if (!h || (!ranges && n_bins)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the bins are ranges of its beads)", who);
    return h->bins.set(who, "bin", h->device, ranges, n_bins, 28, h->hist.beads());
}

int gd_dmap_map(gd_dmap *h, uint32_t row_first, uint32_t n_rows, uint32_t col_first, uint32_t n_cols, uint32_t first_frame, uint32_t n_frames,
                const double *box, const double *thresholds, uint32_t n_thresholds, double *sum1, double *sum2, uint64_t *hits, uint64_t *count)
{
    const char *who = "gd_dmap_map";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (!count) return fail(GD_EINVAL, "%s: NULL argument", who);
    unsigned const B = h->B();
    if (n_rows == 0 || n_cols == 0 || (uint64_t)row_first + n_rows > B || (uint64_t)col_first + n_cols > B)
        return fail(GD_EINVAL, "%s: rows %u to %llu and columns %u to %llu of %u bins", who, row_first, (unsigned long long)row_first + n_rows, col_first,
                    (unsigned long long)col_first + n_cols, B);
    if (n_frames == 0 || (uint64_t)first_frame + n_frames > h->hist.frames())
        return fail(GD_EINVAL, "%s: frames %u to %llu of %u", who, first_frame, (unsigned long long)first_frame + n_frames, h->hist.frames());
    if (n_thresholds > kMaxT) return fail(GD_EINVAL, "%s: %u thresholds (at most %u)", who, n_thresholds, kMaxT);
    if (n_thresholds && !thresholds) return fail(GD_EINVAL, "%s: NULL argument", who);
    for (unsigned t = 0; t < n_thresholds; t++)
        if (!(thresholds[t] > 0.0) || !std::isfinite(thresholds[t])) return fail(GD_EINVAL, "%s: threshold %u is %g (positive and finite)", who, t, thresholds[t]);
    if (box)
        for (int k = 0; k < 3; k++)
            if (!(box[k] > 0.0) || !std::isfinite(box[k])) return fail(GD_EINVAL, "%s: box period %d is %g (positive and finite)", who, k, box[k]);
    GDCHK(h->bins.check(who, "bin", h->hist.beads()));
    HIPCHK(hipSetDevice(h->device));

    auto const cover = tile_cover(kTB, row_first, n_rows, col_first, n_cols);
    std::vector<uint2> tiles(cover.size());
    for (size_t k = 0; k < cover.size(); k++) tiles[k] = make_uint2(cover[k].first, cover[k].second);

    size_t const plane = (size_t)n_rows * n_cols;
    unsigned const nt = hits ? n_thresholds : 0;
    if (h->out.ensure(kWords * plane) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: the outputs of %u x %u cells do not fit on the device", who, n_rows, n_cols);
    }
    HIPCHK(h->tiles_dev.upload(tiles.data(), tiles.size()));

    unsigned longest = 1;
    for (unsigned b = 0; b < B; b++) longest = std::max(longest, h->bins.length(b));
    MapArgs a{};
    a.x = h->hist.x();
    a.bins = h->bins.dev.p;
    a.N = h->hist.beads();
    a.B = B;
    a.f0 = first_frame;
    a.f1 = first_frame + n_frames;
    a.g0 = first_frame / kRange;
    a.L = std::min(longest, kPiece);
    a.S = a.L | 1u;
    size_t const frame_bytes = (size_t)2 * 3 * kTB * a.S * h->hist.elem();
    unsigned const fit = (unsigned)std::max<size_t>(((size_t)h->lds_bytes - kStaticLds) / frame_bytes, 1);
    a.chunk = h->knob ? std::min(h->knob, fit) : (unsigned)std::max<size_t>(kAutoStageBytes / frame_bytes, 1);
    a.chunk = std::min(a.chunk, kRange);
    for (int k = 0; k < 3; k++) a.box[k] = box ? box[k] : 0.0;
    for (unsigned t = 0; t < kMaxT; t++) a.thr2[t] = t < nt ? thresholds[t] * thresholds[t] : -1.0;
    unsigned const ranges = (first_frame + n_frames - 1) / kRange - a.g0 + 1;
    if (ranges > 65535) return fail(GD_EINVAL, "%s: %u frames are more than 65535 frame ranges", who, n_frames);
    size_t const lds = a.chunk * frame_bytes;
    size_t const per_tile = (size_t)ranges * kWords * kBlock * sizeof(unsigned long long);
    size_t const batch = std::min(std::max<size_t>(kPartialBytes / per_tile, 1), std::min<size_t>(tiles.size(), 1u << 30));
    HIPCHK(h->partial.ensure(batch * ranges * kWords * kBlock));
    for (size_t t0 = 0; t0 < tiles.size(); t0 += batch) {
        unsigned const n = (unsigned)std::min(batch, tiles.size() - t0);
        a.tiles = h->tiles_dev.p + t0;
        a.partial = h->partial.p;
        dim3 const grid(n, ranges);
        if (h->hist.is_f64) {
            if (box) launch_tile<double, true>(sum1 != nullptr, grid, lds, h->stream, a);
            else launch_tile<double, false>(sum1 != nullptr, grid, lds, h->stream, a);
        } else {
            if (box) launch_tile<float, true>(sum1 != nullptr, grid, lds, h->stream, a);
            else launch_tile<float, false>(sum1 != nullptr, grid, lds, h->stream, a);
        }
        HIPCHK(hipGetLastError());
        ReduceArgs r{h->partial.p, a.tiles, h->out.p, ranges, n, B, row_first, n_rows, col_first, n_cols};
        hipLaunchKernelGGL(k_dmap_reduce, dim3(n), dim3(kBlock), 0, h->stream, r);
        HIPCHK(hipGetLastError());
    }
    if (sum1) HIPCHK(hipMemcpyAsync(sum1, h->out.p, plane * 8, hipMemcpyDeviceToHost, h->stream));
    if (sum2) HIPCHK(hipMemcpyAsync(sum2, h->out.p + plane, plane * 8, hipMemcpyDeviceToHost, h->stream));
    if (nt) HIPCHK(hipMemcpyAsync(hits, h->out.p + 2 * plane, nt * plane * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (unsigned i = 0; i < n_rows; i++) {
        uint64_t const li = h->bins.length(row_first + i);
        for (unsigned j = 0; j < n_cols; j++) {
            uint64_t const lj = h->bins.length(col_first + j);
            count[(size_t)i * n_cols + j] = (uint64_t)n_frames * (li * lj - (row_first + i == col_first + j ? li : 0));
        }
    }
    return GD_OK;
}

}  // extern "C"
