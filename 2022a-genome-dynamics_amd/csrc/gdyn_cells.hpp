// gdyn_cells.hpp -- the cell grid of a batch of frames, which gdyn_dcorr.hip and gdyn_cluster.hip walk for their pairs: the selected
// beads of every frame of the batch sorted by (frame, cell) as records of the module's own type, the first sorted index of every cell
// and one work item per kCellChunk centres of a non-empty cell.  The pair rules (wrap, cell_of, min_image) are gdyn_pair_rules.hpp's,
// which gdyn_rdf.hip shares.
//
// Everything is defined here in an anonymous namespace: each translation unit keeps its own object code under its own flags.
//   k_cells_bbox     open box: the bounding box of each frame's selected beads (block reduction, integer atomicMin / atomicMax on an
//                    order-preserving image of the double)
//   k_cells_grid     the cells of each frame: of side >= Space::cell_side, of the periodic box or of the frame's own bounding box,
//                    coarsened until a frame has at most `cap` cells.  An axis of zero extent has one cell.
//   (the module's key kernel gathers its records and keys them with cell_key())
//   gd_sort_contacts, k_cells_sorted, k_cells_starts   the records in key order and the first sorted index of every cell
//   k_cells_work     one work item per kCellChunk centres of a non-empty cell (their order is arbitrary)
// gd::CellIndex<Rec> owns the buffers and runs these steps on the handle's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gdyn_analysis.hpp"
#include "gdyn_pair_rules.hpp"
#include "gdyn_types.h"

namespace gd {

struct Grid {      // the cells of one frame
    double lo[3];            // open: the low corner of the bounding box; periodic: 0
    double box[3];           // periodic: the periods
    double inv_side[3];      // cells per unit length (0 along an axis of zero extent)
    int n[3];                // cells per axis (>= 1)
    unsigned cells;
};

struct FrameSel {      // first + k * stride, k < count
    unsigned first, stride, count;
};

struct Space {
    int periodic;
    double box[3];
    double cell_side;        // the cutoff (1 + kCellSlack)
};

constexpr int kCellBlock = 256;
constexpr unsigned kCellChunk = kCellBlock;      // centres of one work item
constexpr double kCellSlack = 1e-9;              // cells are this much wider than the cutoff, against the rounding of the cell assignment

namespace {

// an image of a double under which unsigned order is numeric order
__device__ inline unsigned long long ordered(double x)
{
    unsigned long long const u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ inline double unordered(unsigned long long o)
{
    return __longlong_as_double((long long)((o >> 63) ? (o & ~(1ull << 63)) : ~o));
}

__device__ inline double wave_min(double v)
{
    for (int m = 32; m; m >>= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
__device__ inline double wave_max(double v)
{
    for (int m = 32; m; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// the same over a block of kCellBlock lanes (every lane calls; sh: kCellBlock / 64 doubles)
__device__ inline double block_min(double v, double *sh)
{
    v = wave_min(v);
    __syncthreads();      // sh is free again
    if (threadIdx.x % 64 == 0) sh[threadIdx.x / 64] = v;
    __syncthreads();
    for (int w = 0; w < kCellBlock / 64; w++) v = fmin(v, sh[w]);
    return v;
}
__device__ inline double block_max(double v, double *sh)
{
    v = wave_max(v);
    __syncthreads();
    if (threadIdx.x % 64 == 0) sh[threadIdx.x / 64] = v;
    __syncthreads();
    for (int w = 0; w < kCellBlock / 64; w++) v = fmax(v, sh[w]);
    return v;
}

__device__ inline void load3(const void *__restrict__ xyz, int is_f64, size_t at, double p[3])
{
    for (int a = 0; a < 3; a++) p[a] = is_f64 ? static_cast<const double *>(xyz)[at + a] : (double)static_cast<const float *>(xyz)[at + a];
}

// the sort key of a bead at p in frame o of its batch: (o, cell of g), `cap` cell slots a frame
__device__ inline unsigned long long cell_key(const Grid &g, const double p[3], int periodic, unsigned o, unsigned cap)
{
    int c[3];
    for (int a = 0; a < 3; a++) c[a] = cell_of(periodic ? wrap(p[a], g.box[a]) : p[a] - g.lo[a], g.inv_side[a], g.n[a]);
    unsigned const cell = ((unsigned)c[2] * (unsigned)g.n[1] + (unsigned)c[1]) * (unsigned)g.n[0] + (unsigned)c[0];
    return (unsigned long long)o * cap + cell;
}

// the distinct cells of one axis that the neighbours of cell c lie in: first and count
__device__ inline void axis_cells(int c, int n, int periodic, int &first, int &count)
{
    if (periodic) {
        first = n < 3 ? 0 : (c + n - 1) % n;
        count = n < 3 ? n : 3;
    } else {
        first = max(c - 1, 0);
        count = min(c + 1, n - 1) - first + 1;
    }
}

// bbox[o]: ordered images of (min x, y, z, max x, y, z), preset to (~0, ~0, ~0, 0, 0, 0); grid (a few blocks that stride over the selection, B)
__global__ void __launch_bounds__(kCellBlock) k_cells_bbox(const void *__restrict__ xyz, int is_f64, unsigned N, const unsigned *__restrict__ sel,
                                                           unsigned n_sel, FrameSel fs, unsigned o0, unsigned long long *__restrict__ bbox)
{
    __shared__ double sh[kCellBlock / 64];
    unsigned const o = blockIdx.y;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (unsigned k = blockIdx.x * kCellBlock + threadIdx.x; k < n_sel; k += gridDim.x * kCellBlock) {
        double p[3];
        load3(xyz, is_f64, ((size_t)(fs.first + (o0 + o) * fs.stride) * N + sel[k]) * 3, p);
        for (int a = 0; a < 3; a++) {
            lo[a] = fmin(lo[a], p[a]);
            hi[a] = fmax(hi[a], p[a]);
        }
    }
    for (int a = 0; a < 3; a++) {
        lo[a] = block_min(lo[a], sh);
        hi[a] = block_max(hi[a], sh);
    }
    if (threadIdx.x == 0 && lo[0] <= hi[0])
        for (int a = 0; a < 3; a++) {
            atomicMin(&bbox[6 * (size_t)o + a], ordered(lo[a]));
            atomicMax(&bbox[6 * (size_t)o + 3 + a], ordered(hi[a]));
        }
}

__global__ void __launch_bounds__(kCellBlock) k_cells_grid(const unsigned long long *__restrict__ bbox, unsigned B, Space sp, unsigned cap,
                                                           Grid *__restrict__ grids)
{
    unsigned const o = blockIdx.x * kCellBlock + threadIdx.x;
    if (o >= B) return;
    Grid g;
    double n[3], ext[3];
    for (int a = 0; a < 3; a++) {
        g.lo[a] = sp.periodic ? 0.0 : unordered(bbox[6 * (size_t)o + a]);
        g.box[a] = sp.periodic ? sp.box[a] : 0.0;
        ext[a] = sp.periodic ? sp.box[a] : unordered(bbox[6 * (size_t)o + 3 + a]) - g.lo[a];
        n[a] = fmin(fmax(1.0, floor(ext[a] / sp.cell_side)), 1048576.0);
    }
    while (n[0] * n[1] * n[2] > (double)cap) {
        int const a = (n[0] >= n[1] && n[0] >= n[2]) ? 0 : (n[1] >= n[2] ? 1 : 2);
        n[a] = fmax(1.0, floor(n[a] * 0.9));
    }
    g.cells = 1;
    for (int a = 0; a < 3; a++) {
        g.n[a] = (int)n[a];
        g.inv_side[a] = ext[a] > 0.0 ? n[a] / ext[a] : 0.0;
        g.cells *= (unsigned)g.n[a];
    }
    grids[o] = g;
}

template <typename Rec>
__global__ void __launch_bounds__(kCellBlock) k_cells_sorted(const Rec *__restrict__ grec, const unsigned *__restrict__ vals, size_t n, Rec *__restrict__ srec)
{
    size_t const s = (size_t)blockIdx.x * kCellBlock + threadIdx.x;
    if (s < n) srec[s] = grec[vals[s]];
}

// starts[t] = first sorted index whose key >= t, t in [0, count)
__global__ void __launch_bounds__(kCellBlock) k_cells_starts(const unsigned long long *__restrict__ keys, size_t n, size_t count, unsigned *__restrict__ starts)
{
    size_t const t = (size_t)blockIdx.x * kCellBlock + threadIdx.x;
    if (t >= count) return;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        size_t const mid = (lo + hi) / 2;
        if (keys[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    starts[t] = (unsigned)lo;
}

// work items (cell slot, chunk of kCellChunk centres) of the non-empty cells; slots = B * cap
__global__ void __launch_bounds__(kCellBlock) k_cells_work(const unsigned *__restrict__ starts, size_t slots, uint2 *__restrict__ work, unsigned *__restrict__ n_work)
{
    size_t const t = (size_t)blockIdx.x * kCellBlock + threadIdx.x;
    if (t >= slots) return;
    unsigned const c = starts[t + 1] - starts[t];
    if (!c) return;
    unsigned const items = (c + kCellChunk - 1) / kCellChunk, base = atomicAdd(n_work, items);
    for (unsigned k = 0; k < items; k++) work[base + k] = make_uint2((unsigned)t, k);
}

}  // namespace

// The cell index of one batch: B frames of n selected beads, `cap` cell slots a frame.  A batch goes room(), grids(), the module's key
// kernel into keys[0], vals[0] and grec, sort(), and, after whatever else the module queues, work_items(), which waits for the stream.
template <typename Rec>
struct CellIndex {
    dbuf<unsigned long long> bbox;
    dbuf<Grid> grids;
    dbuf<Rec> grec, srec;
    dbuf<unsigned long long> keys[2];
    dbuf<unsigned> vals[2], starts, n_work;
    dbuf<uint2> work;
    dbuf<char> sort_tmp;

    int room(unsigned B, unsigned n, unsigned cap)
    {
        size_t const nb = (size_t)B * n, slots = (size_t)B * cap;
        HIPCHK(bbox.ensure(6 * (size_t)B));
        HIPCHK(grids.ensure(B));
        HIPCHK(grec.ensure(nb));
        HIPCHK(srec.ensure(nb));
        for (int k = 0; k < 2; k++) {
            HIPCHK(keys[k].ensure(nb));
            HIPCHK(vals[k].ensure(nb));
        }
        HIPCHK(starts.ensure(slots + 1));
        HIPCHK(work.ensure(nb / kCellChunk + std::min(nb, slots) + 1));
        HIPCHK(n_work.ensure(1));
        return GD_OK;
    }

    // the grid of every frame of the batch; in an open box after the bounding boxes, whose preset waits for the stream once
    int make_grids(hipStream_t st, const void *xyz, int is_f64, unsigned N, const unsigned *sel, unsigned n, FrameSel fs, unsigned o0, unsigned B, const Space &sp,
                   unsigned cap)
    {
        if (!sp.periodic) {
            std::vector<unsigned long long> init(6 * (size_t)B);
            for (size_t k = 0; k < init.size(); k++) init[k] = k % 6 < 3 ? ~0ull : 0ull;
            HIPCHK(hipMemcpyAsync(bbox.p, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));      // init is about to go out of scope
            hipLaunchKernelGGL(k_cells_bbox, dim3(std::min(blocks_for(n, kCellBlock), 16u), B), dim3(kCellBlock), 0, st, xyz, is_f64, N, sel, n, fs, o0, bbox.p);
        }
        hipLaunchKernelGGL(k_cells_grid, dim3(blocks_for(B, kCellBlock)), dim3(kCellBlock), 0, st, bbox.p, B, sp, cap, grids.p);
        return GD_OK;
    }

    // the keyed records of the batch in key order (srec), the cell starts and the work items
    int sort(hipStream_t st, size_t nb, size_t slots)
    {
        unsigned bits = 1;
        while (bits < 64 && ((unsigned long long)slots >> bits)) bits++;
        size_t tmp_bytes = 0;
        HIPCHK(gd_sort_contacts(nullptr, &tmp_bytes, keys[0].p, keys[1].p, vals[0].p, vals[1].p, nb, bits, st));
        HIPCHK(sort_tmp.ensure(tmp_bytes));
        HIPCHK(gd_sort_contacts(sort_tmp.p, &tmp_bytes, keys[0].p, keys[1].p, vals[0].p, vals[1].p, nb, bits, st));
        hipLaunchKernelGGL(k_cells_sorted<Rec>, dim3(blocks_for(nb, kCellBlock)), dim3(kCellBlock), 0, st, grec.p, vals[1].p, nb, srec.p);
        hipLaunchKernelGGL(k_cells_starts, dim3(blocks_for(slots + 1, kCellBlock)), dim3(kCellBlock), 0, st, keys[1].p, nb, slots + 1, starts.p);
        HIPCHK(hipMemsetAsync(n_work.p, 0, sizeof(unsigned), st));
        hipLaunchKernelGGL(k_cells_work, dim3(blocks_for(slots, kCellBlock)), dim3(kCellBlock), 0, st, starts.p, slots, work.p, n_work.p);
        return GD_OK;
    }

    // the number of work items, read back once the stream is idle, and checked against the room for them (`who`: the call)
    int work_items(const char *who, hipStream_t st, unsigned *count)
    {
        HIPCHK(hipMemcpyAsync(count, n_work.p, sizeof *count, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (*count > work.n) return fail(GD_EHIP, "%s: %u work items for %zu", who, *count, work.n);
        return GD_OK;
    }
};

}  // namespace gd
