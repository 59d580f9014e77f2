// gdyn_dcov.hip -- displacement covariance maps of a trajectory history (include/gdyn_dcov.h): the row matrix A (bins x 3 origins) of
// binned displacements over a lag, or of positions about their time mean, and the symmetric product S = A A^T.  Beyond the reference,
// and the first kernel of this code base on the matrix cores (v_mfma_f64_16x16x4_f64).
//
// A is kept transposed and padded, At[c][b] with c < K (the columns rounded up to a multiple of 4) and b < Bp (the bins rounded up to a
// multiple of kTile), the padding zero: a row panel of a tile is then contiguous per column, in global memory and in LDS alike.
//
//   stage 1          k_dcov_mean (lag 0 only), k_dcov_raw, k_dcov_drift and k_dcov_apply (drift removal only): one lane per (column, bin),
//                    bins along the lanes, every sum serial in the order the header states.
//   k_dcov_product   one block of four waves per (canonical tile of kTile x kTile cells with ta <= tb, column range of
//                    GD_DCOV_COLUMN_RANGE columns).  The tile grid is fixed by the bins alone: tile t holds the bins [64 t, 64 t + 64).
//                    The two row panels go through LDS `columns_per_stage` columns at a time (one panel for a diagonal tile); wave
//                    (wr, wc) owns the 32 x 32 cells at (32 wr, 32 wc) as 2 x 2 accumulators of 16 x 16 cells and issues one
//                    instruction per accumulator and group of four columns, groups ascending.  The accumulators live across the
//                    stages, so no bit depends on the stage.  LDS holds [panel][column][kLd = 80 doubles]: a lane reads row l & 15 of
//                    column l >> 4, so the 32 lanes that one ds_read_b64 cycle serves read 16 consecutive doubles of each of two columns
//                    that lie 80 = 16 (mod 32) doubles apart: all 64 banks once.  (The compiler fuses the reads of rows r and r + 16 into
//                    one ds_read2_b64, served 16 lanes at a time: 16 consecutive doubles, 32 banks once, conflict-free whatever the
//                    padding.)  Staging writes 64 consecutive doubles per wave.
//                    On a diagonal tile the wave below the diagonal (wr > wc) only stages.
//   k_dcov_merge     adds a cell's partial sums over the column ranges in ascending order and writes the cell (I <= J) where the rectangle
//                    holds it, its mirror image where the rectangle holds that, and the diagonal cells into diag_rows / diag_cols.
// The history itself (upload, non-finite check) is gd::History's (gdyn_history.hpp).
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_dcov.h"
#include "gdyn_analysis.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr unsigned kTile = 64;                       // bins of a tile side
constexpr unsigned kCells = kTile * kTile;
constexpr unsigned kLd = kTile + 16;                 // doubles between two staged columns: 16 (mod 32), see above
constexpr unsigned kRange = GD_DCOV_COLUMN_RANGE;
constexpr unsigned kPiece = GD_DCOV_PIECE_BEADS;
constexpr unsigned kAhead = 4;                       // staging passes whose loads are in flight together
constexpr unsigned kAutoStage = 32;                  // automatic columns per stage: 40 KiB, four blocks (16 waves) per CU
constexpr size_t kPartialBytes = (size_t)1 << 30;    // tiles are walked in batches whose partial sums fit this
static_assert(kRange % 4 == 0 && kLd % 32 == 16 && kAutoStage % 4 == 0, "whole groups of four columns; conflict-free reads");

typedef double v4d __attribute__((ext_vector_type(4)));

struct RowArgs {
    const void *x;            // the history, (F, N, 3) of T
    const uint32_t *bins;     // (B, 2)
    const double *mean;       // (N, 3), lag 0 only
    double *At;               // (K, Bp)
    size_t N;
    unsigned B, Bp;
    unsigned lag, first, stride, count;      // count: origins (lag >= 1) or frames (lag 0)
};

// mean[i, axis] of the chosen frames: one lane per coordinate, frames ascending
template <typename T>
__global__ void __launch_bounds__(kBlock) k_dcov_mean(RowArgs p, double *mean)
{
    size_t const e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= 3 * p.N) return;
    const T *x = static_cast<const T *>(p.x);
    double s = 0.0;
    for (unsigned k = 0; k < p.count; k++) s += (double)x[((size_t)p.first + (size_t)k * p.stride) * 3 * p.N + e];
    mean[e] = s / (double)p.count;
}

// raw[b, c]: blockIdx.x is the column, the lanes walk the bins
template <typename T>
__global__ void __launch_bounds__(kBlock) k_dcov_raw(RowArgs p)
{
    unsigned const c = blockIdx.x, b = blockIdx.y * kBlock + threadIdx.x;
    if (b >= p.B) return;
    const T *x = static_cast<const T *>(p.x);
    unsigned const k = c / 3, axis = c % 3;
    size_t const f = (size_t)p.first + (size_t)k * p.stride;
    const T *x0 = x + f * 3 * p.N + axis, *x1 = x + (f + p.lag) * 3 * p.N + axis;
    unsigned const start = p.bins[2 * b], end = p.bins[2 * b + 1];
    double raw = 0.0;
    for (unsigned a = start; a < end; a += kPiece) {
        unsigned const stop = min(end, a + kPiece);      // a + kPiece <= 2^28 + 32
        double piece = 0.0;
        if (p.lag)
            for (unsigned i = a; i < stop; i++) piece += (double)x1[3 * (size_t)i] - (double)x0[3 * (size_t)i];
        else
            for (unsigned i = a; i < stop; i++) piece += (double)x0[3 * (size_t)i] - p.mean[3 * (size_t)i + axis];
        raw += piece;
    }
    p.At[(size_t)c * p.Bp + b] = raw;
}

// m[c]: one lane per column, bins ascending
__global__ void __launch_bounds__(kBlock) k_dcov_drift(const double *At, double *m, unsigned columns, unsigned B, unsigned Bp, double binned)
{
    unsigned const c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= columns) return;
    double s = 0.0;
    for (unsigned b = 0; b < B; b++) s += At[(size_t)c * Bp + b];
    m[c] = s / binned;
}

__global__ void __launch_bounds__(kBlock) k_dcov_apply(double *At, const double *m, const uint32_t *bins, unsigned B, unsigned Bp)
{
    unsigned const c = blockIdx.x, b = blockIdx.y * kBlock + threadIdx.x;
    if (b >= B) return;
    double const drift = (double)(bins[2 * b + 1] - bins[2 * b]) * m[c];      // rounded on its own: no contraction
    At[(size_t)c * Bp + b] -= drift;
}

// out (n, columns) = the rows [first, first + n) of A
__global__ void __launch_bounds__(kBlock) k_dcov_gather(const double *At, double *out, unsigned columns, unsigned Bp, unsigned first, unsigned n)
{
    unsigned const c = blockIdx.x, r = blockIdx.y * kBlock + threadIdx.x;
    if (r >= n) return;
    out[(size_t)r * columns + c] = At[(size_t)c * Bp + first + r];
}

struct ProductArgs {
    const double *At;         // (K, Bp)
    const uint2 *tiles;       // canonical tiles (ta <= tb) of this launch
    double *partial;          // (ranges, tiles, kCells)
    unsigned Bp, K;
    unsigned stage;           // columns staged at once, a multiple of 4
};

__global__ void __launch_bounds__(kBlock) k_dcov_product(ProductArgs p)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    uint2 const tile = p.tiles[blockIdx.x];
    unsigned const tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    bool const diag = tile.x == tile.y;
    double *pa = lds, *pb = diag ? lds : lds + (size_t)p.stage * kLd;
    unsigned const c0 = blockIdx.y * kRange, c1 = min(p.K, c0 + kRange);
    const double *ga = p.At + (size_t)tile.x * kTile, *gb = p.At + (size_t)tile.y * kTile;
    bool const idle = diag && wr > wc;      // wave-uniform
    unsigned const r = lane & 15, kl = lane >> 4;

    v4d acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};

    for (unsigned cs = c0; cs < c1; cs += p.stage) {
        unsigned const n = min(p.stage, c1 - cs);      // a multiple of 4: c0, K and stage are
        __syncthreads();                               // the last stage has been read
        // four columns per pass (n * kTile is a multiple of kBlock); the loads of kAhead passes are in flight before the first is stored
        for (unsigned e0 = tid; e0 < n * kTile; e0 += kAhead * kBlock) {
            double va[kAhead], vb[kAhead];
#pragma unroll
            for (unsigned u = 0; u < kAhead; u++) {
                unsigned const e = e0 + u * kBlock;
                if (e < n * kTile) {
                    va[u] = ga[(size_t)(cs + e / kTile) * p.Bp + e % kTile];
                    if (!diag) vb[u] = gb[(size_t)(cs + e / kTile) * p.Bp + e % kTile];
                }
            }
#pragma unroll
            for (unsigned u = 0; u < kAhead; u++) {
                unsigned const e = e0 + u * kBlock;
                if (e < n * kTile) {
                    pa[e / kTile * kLd + e % kTile] = va[u];
                    if (!diag) pb[e / kTile * kLd + e % kTile] = vb[u];
                }
            }
        }
        __syncthreads();
        if (idle) continue;
        const double *ra = pa + wr * 32 + r, *rb = pb + wc * 32 + r;
        for (unsigned kk = 0; kk < n; kk += 4) {
            unsigned const at = (kk + kl) * kLd;
            double const a0 = ra[at], a1 = ra[at + 16], b0 = rb[at], b1 = rb[at + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    if (idle) return;
    // the fp64 result layout: column = lane & 15, row = (lane >> 4) + 4 * register
    double *mine = p.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kCells;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) mine[(wr * 32 + i * 16 + kl + 4 * q) * kTile + wc * 32 + j * 16 + r] = acc[i][j][q];
}

struct MergeArgs {
    const double *partial;
    const uint2 *tiles;
    double *out, *diag_rows, *diag_cols;      // (n_rows, n_cols), (n_rows), (n_cols)
    unsigned ranges, n_tiles, B;
    unsigned row_first, n_rows, col_first, n_cols;
};

__global__ void __launch_bounds__(kBlock) k_dcov_merge(MergeArgs p)
{
    uint2 const tile = p.tiles[blockIdx.x];
    size_t const range_stride = (size_t)p.n_tiles * kCells;
    for (unsigned cell = threadIdx.x; cell < kCells; cell += kBlock) {
        unsigned const r = tile.x * kTile + cell / kTile, c = tile.y * kTile + cell % kTile;
        if (r >= p.B || c >= p.B || r > c) continue;      // r > c: below the diagonal of a diagonal tile
        const double *mine = p.partial + (size_t)blockIdx.x * kCells + cell;
        double s = 0.0;
        for (unsigned g = 0; g < p.ranges; g++) s += mine[g * range_stride];      // ascending ranges, from +0
        unsigned rr = r - p.row_first, cc = c - p.col_first;      // unsigned: a cell before the rectangle wraps to a large value
        if (rr < p.n_rows && cc < p.n_cols) p.out[(size_t)rr * p.n_cols + cc] = s;
        if (r != c) {
            rr = c - p.row_first;
            cc = r - p.col_first;
            if (rr < p.n_rows && cc < p.n_cols) p.out[(size_t)rr * p.n_cols + cc] = s;
        } else {
            if (r - p.row_first < p.n_rows) p.diag_rows[r - p.row_first] = s;
            if (r - p.col_first < p.n_cols) p.diag_cols[r - p.col_first] = s;
        }
    }
}

// the dynamic LDS a block of k_dcov_product may ask for (gd::lds_opt_in).  A refusal only makes the stages smaller.
int lds_budget(int device)
{
    static DeviceOnce<> once;
    return lds_opt_in(once, device, {reinterpret_cast<const void *>(&k_dcov_product)});
}

}  // namespace

struct gd_dcov : gd::handle {
    unsigned knob = 0;
    int lds_bytes = 64 * 1024;
    History hist;
    BeadRanges bins;               // of hist.beads(); every bead its own bin without bins of the caller's
    // the preparation: columns == 0 without one
    unsigned columns = 0, K = 0, Bp = 0;
    dbuf<double> At;
    // per call
    dbuf<double> mean, drift, rows_out;
    dbuf<uint2> tiles_dev;
    dbuf<double> partial, out;
    StageTimer timer;              // gd_dcov_last_times: stage 1, product, merge

    unsigned B() const { return bins.count(); }
};

namespace {

History::Rebind rebind(gd_dcov *h)
{
    return [h](unsigned n_beads) -> int {
        h->columns = 0;      // the preparation was of the last history
        if (n_beads != h->hist.beads() || h->bins.host.empty()) GDCHK(h->bins.every_bead(n_beads));      // bins belonged to another N
        return GD_OK;
    };
}

}  // namespace

extern "C" {

int gd_dcov_abi_version(void) { return GD_DCOV_ABI_VERSION; }

int gd_dcov_create(const gd_dcov_desc *desc, gd_dcov **out)
{
    if (int rc = gd::open("gd_dcov_create", desc, out)) return rc;
    (*out)->knob = desc->columns_per_stage;
    (*out)->lds_bytes = lds_budget(desc->device);
    if (hipError_t const rc = (*out)->timer.create()) {
        gd::close(*out);
        *out = nullptr;
        return fail(GD_EHIP, "gd_dcov_create: hipEventCreate failed: %s", hipGetErrorString(rc));
    }
    return GD_OK;
}

int gd_dcov_destroy(gd_dcov *h) { return gd::close(h); }

int gd_dcov_set_history(gd_dcov *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_dcov_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    int const rc = h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
    if (!h->hist.frames()) h->columns = 0;
    return rc;
}

int gd_dcov_set_history_live(gd_dcov *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_dcov_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    int const rc = h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
    if (!h->hist.frames()) h->columns = 0;
    return rc;
}

int gd_dcov_set_bins(gd_dcov *h, const uint32_t *ranges, uint32_t n_bins)
{
    const char *who = "gd_dcov_set_bins";
    if (!h || (!ranges && n_bins)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the bins are ranges of its beads)", who);
    GDCHK(h->bins.set(who, "bin", h->device, ranges, n_bins, 28, h->hist.beads()));
    h->columns = 0;      // the preparation was of the old bins
    return GD_OK;
}

int gd_dcov_prepare(gd_dcov *h, uint32_t lag, uint32_t first, uint32_t stride, uint32_t count, int remove_drift)
{
    const char *who = "gd_dcov_prepare";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames(), B = h->B();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    if (stride == 0) return fail(GD_EINVAL, "%s: stride 0", who);
    // the frames f with f + lag < F from `first` on, `stride` apart
    uint64_t const fit = frames_fit(F, first, stride, lag);
    if (count > fit || fit == 0)
        return fail(GD_EINVAL, "%s: %s from frame %u with stride %u and lag %u: %llu fit in %u frames", who, count ? "the origins asked for" : "no origin",
                    first, stride, lag, (unsigned long long)fit, F);
    uint64_t const origins = frames_served(fit, count);
    if (origins > (1u << 28)) return fail(GD_EINVAL, "%s: %llu origins exceed 2^28", who, (unsigned long long)origins);
    if ((B + kBlock - 1) / kBlock > 65535) return fail(GD_EINVAL, "%s: %u bins exceed %u", who, B, 65535 * kBlock);      // a grid dimension of stage 1
    GDCHK(h->bins.check(who, "bin", h->hist.beads()));
    HIPCHK(hipSetDevice(h->device));

    unsigned const columns = 3 * (unsigned)origins, K = (columns + 3) / 4 * 4, Bp = (B + kTile - 1) / kTile * kTile;
    dbuf<double> At;
    if (At.ensure((size_t)K * Bp) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: %u bins x %u columns do not fit on the device", who, B, columns);
    }
    HIPCHK(h->timer.mark(0, h->stream));
    HIPCHK(hipMemsetAsync(At.p, 0, (size_t)K * Bp * sizeof(double), h->stream));
    RowArgs a{h->hist.x(), h->bins.dev.p, nullptr, At.p, h->hist.beads(), B, Bp, lag, first, stride, (unsigned)origins};
    bool const f64 = h->hist.is_f64;
    if (lag == 0) {
        HIPCHK(h->mean.ensure(3 * a.N));
        dim3 const grid(blocks_for(3 * a.N, kBlock));
        if (f64) hipLaunchKernelGGL(k_dcov_mean<double>, grid, dim3(kBlock), 0, h->stream, a, h->mean.p);
        else hipLaunchKernelGGL(k_dcov_mean<float>, grid, dim3(kBlock), 0, h->stream, a, h->mean.p);
        HIPCHK(hipGetLastError());
        a.mean = h->mean.p;
    }
    dim3 const grid(columns, (B + kBlock - 1) / kBlock);
    if (f64) hipLaunchKernelGGL(k_dcov_raw<double>, grid, dim3(kBlock), 0, h->stream, a);
    else hipLaunchKernelGGL(k_dcov_raw<float>, grid, dim3(kBlock), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    if (remove_drift) {
        uint64_t binned = 0;
        for (unsigned b = 0; b < B; b++) binned += h->bins.length(b);
        HIPCHK(h->drift.ensure(columns));
        hipLaunchKernelGGL(k_dcov_drift, dim3(blocks_for(columns, kBlock)), dim3(kBlock), 0, h->stream, At.p, h->drift.p, columns, B, Bp, (double)binned);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_dcov_apply, grid, dim3(kBlock), 0, h->stream, At.p, h->drift.p, h->bins.dev.p, B, Bp);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(h->timer.mark(1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(h->timer.between(0, 1, &h->timer.ms[0]));
    h->At = std::move(At);      // the last preparation's block goes with `At`
    h->columns = columns;
    h->K = K;
    h->Bp = Bp;
    return GD_OK;
}

uint32_t gd_dcov_columns(const gd_dcov *h) { return h && h->hist.frames() ? h->columns : 0; }

int gd_dcov_last_times(const gd_dcov *h, double *stage1_ms, double *product_ms, double *merge_ms)
{
    if (!h) return fail(GD_EINVAL, "gd_dcov_last_times: NULL handle");
    h->timer.report(stage1_ms, product_ms, merge_ms);
    return GD_OK;
}

int gd_dcov_rows(gd_dcov *h, uint32_t first_bin, uint32_t n_bins, double *out)
{
    const char *who = "gd_dcov_rows";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (!h->columns) return fail(GD_ESTATE, "%s: nothing prepared (gd_dcov_prepare comes after the history and the bins)", who);
    if (!out) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (n_bins == 0 || (uint64_t)first_bin + n_bins > h->B())
        return fail(GD_EINVAL, "%s: rows %u to %llu of %u bins", who, first_bin, (unsigned long long)first_bin + n_bins, h->B());
    HIPCHK(hipSetDevice(h->device));
    size_t const n = (size_t)n_bins * h->columns;
    if (h->rows_out.ensure(n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: %u rows of %u columns do not fit on the device", who, n_bins, h->columns);
    }
    hipLaunchKernelGGL(k_dcov_gather, dim3(h->columns, (n_bins + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->At.p, h->rows_out.p, h->columns, h->Bp,
                       first_bin, n_bins);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->rows_out.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_dcov_map(gd_dcov *h, uint32_t row_first, uint32_t n_rows, uint32_t col_first, uint32_t n_cols, double *sum, uint64_t *count, double *diag_rows,
                double *diag_cols)
{
    const char *who = "gd_dcov_map";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set", who);
    if (!h->columns) return fail(GD_ESTATE, "%s: nothing prepared (gd_dcov_prepare comes after the history and the bins)", who);
    unsigned const B = h->B();
    if (n_rows == 0 || n_cols == 0 || (uint64_t)row_first + n_rows > B || (uint64_t)col_first + n_cols > B)
        return fail(GD_EINVAL, "%s: rows %u to %llu and columns %u to %llu of %u bins", who, row_first, (unsigned long long)row_first + n_rows, col_first,
                    (unsigned long long)col_first + n_cols, B);
    HIPCHK(hipSetDevice(h->device));

    // the canonical tiles the rectangle touches, each once, and the diagonal tiles of its bins where their cells are asked for
    auto const cover = tile_cover(kTile, row_first, n_rows, col_first, n_cols, sum != nullptr, diag_rows != nullptr, diag_cols != nullptr);
    std::vector<uint2> tiles(cover.size());
    for (size_t k = 0; k < cover.size(); k++) tiles[k] = make_uint2(cover[k].first, cover[k].second);

    size_t const plane = (size_t)n_rows * n_cols;
    if (!tiles.empty()) {
        if (h->out.ensure(plane + n_rows + n_cols) != hipSuccess) {
            (void)hipGetLastError();
            return fail(GD_ENOMEM, "%s: the outputs of %u x %u cells do not fit on the device", who, n_rows, n_cols);
        }
        HIPCHK(h->tiles_dev.upload(tiles.data(), tiles.size()));
        unsigned const ranges = (h->K + kRange - 1) / kRange;
        if (ranges > 65535) return fail(GD_EINVAL, "%s: %u columns are more than 65535 column ranges", who, h->columns);
        unsigned const fit = std::max((unsigned)((size_t)h->lds_bytes / (2 * kLd * sizeof(double))) / 4 * 4, 4u);
        unsigned const asked = h->knob ? (unsigned)std::min<uint64_t>(((uint64_t)h->knob + 3) / 4 * 4, kRange) : kAutoStage;
        ProductArgs a{h->At.p, nullptr, nullptr, h->Bp, h->K, std::min(asked, fit)};
        size_t const lds = (size_t)2 * a.stage * kLd * sizeof(double);
        size_t const per_tile = (size_t)ranges * kCells * sizeof(double);
        size_t const batch = std::min(std::max<size_t>(kPartialBytes / per_tile, 1), std::min<size_t>(tiles.size(), 1u << 30));
        if (h->partial.ensure(batch * ranges * kCells) != hipSuccess) {
            (void)hipGetLastError();
            return fail(GD_ENOMEM, "%s: the partial sums of %zu tiles do not fit on the device", who, batch);
        }
        double product_ms = 0.0, merge_ms = 0.0, ms = 0.0;
        for (size_t t0 = 0; t0 < tiles.size(); t0 += batch) {
            unsigned const n = (unsigned)std::min(batch, tiles.size() - t0);
            a.tiles = h->tiles_dev.p + t0;
            a.partial = h->partial.p;
            HIPCHK(h->timer.mark(0, h->stream));
            hipLaunchKernelGGL(k_dcov_product, dim3(n, ranges), dim3(kBlock), lds, h->stream, a);
            HIPCHK(hipGetLastError());
            HIPCHK(h->timer.mark(1, h->stream));
            MergeArgs m{h->partial.p, a.tiles, h->out.p, h->out.p + plane, h->out.p + plane + n_rows, ranges, n, B, row_first, n_rows, col_first, n_cols};
            hipLaunchKernelGGL(k_dcov_merge, dim3(n), dim3(kBlock), 0, h->stream, m);
            HIPCHK(hipGetLastError());
            HIPCHK(h->timer.mark(2, h->stream));
            HIPCHK(hipEventSynchronize(h->timer.ev[2]));      // the events serve the next batch
            HIPCHK(h->timer.between(0, 1, &ms));
            product_ms += ms;
            HIPCHK(h->timer.between(1, 2, &ms));
            merge_ms += ms;
        }
        h->timer.ms[1] = product_ms;
        h->timer.ms[2] = merge_ms;
        if (sum) HIPCHK(hipMemcpyAsync(sum, h->out.p, plane * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (diag_rows) HIPCHK(hipMemcpyAsync(diag_rows, h->out.p + plane, n_rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (diag_cols) HIPCHK(hipMemcpyAsync(diag_cols, h->out.p + plane + n_rows, n_cols * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (count) {
        uint64_t const origins = h->columns / 3;
        for (unsigned i = 0; i < n_rows; i++) {
            uint64_t const li = h->bins.length(row_first + i);
            for (unsigned j = 0; j < n_cols; j++)
                count[(size_t)i * n_cols + j] = origins * li * h->bins.length(col_first + j);
        }
    }
    return GD_OK;
}

}  // extern "C"
