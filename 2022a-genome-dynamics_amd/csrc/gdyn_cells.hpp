// gdyn_cells.hpp -- the cell grid of a batch of frames and the walk over it, which gdyn_dcorr.hip, gdyn_cluster.hip and the distinct part
// of gdyn_vanhove.hip use for their pairs: the selected beads of every frame of the batch sorted by (frame, cell) as records of the
// module's own type, the first sorted index of every cell, one work item per kCellChunk centres of a non-empty cell, and the walk
// of a work item's block over the cells around its own in tiles staged through LDS.  The pair rules (wrap, cell_of, min_image) are
// gdyn_pair_rules.hpp's, which gdyn_rdf.hip shares; rdf's walk is of another design and its own.
//
// Everything is defined here in an anonymous namespace: each translation unit keeps its own object code under its own flags.
//   k_cells_bbox<Frames>   open box: the bounding box of each entry's selected beads over the frames that `Frames` names (BatchFrames: one;
//                    van Hove's: both of a pair), by block reduction and integer atomicMin / atomicMax on an order-preserving image
//   k_cells_grid     the cells of each frame: of side >= Space::cell_side, of the periodic box or of the frame's own bounding box,
//                    coarsened until a frame has at most `cap` cells.  An axis of zero extent has one cell.
//   k_cells_keys<Rec, Fill>   gathers the records, which the module's Fill writes, and keys them with cell_key()
//   gd_sort_contacts, k_cells_sorted, k_cells_starts   the records in key order and the first sorted index of every cell
//   k_cells_work     one work item per kCellChunk centres of a non-empty cell (their order is arbitrary)
//   cell_work, cell_tile_walk, pair_class   inside a module's pair kernel: see "the neighbour-cell tile walk" below
// gd::CellIndex<Rec> owns the buffers and runs these steps on the handle's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
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

// the index of the unordered pair of labels (a, b) among the K (K + 1) / 2 classes
__device__ inline unsigned pair_class(unsigned a, unsigned b, unsigned K)
{
    unsigned const la = min(a, b), lb = max(a, b);
    return la * K - la * (la - 1u) / 2u + (lb - la);      // (la = 0: 0 * 0xffffffff / 2 = 0)
}

// The frames of entry o of a batch, for k_cells_bbox: kFrames of them, frame(o, which).  One frame of a FrameSel, from its o0-th on.
struct BatchFrames {
    FrameSel fs;
    unsigned o0;
    static constexpr int kFrames = 1;
    __device__ unsigned frame(unsigned o, int) const { return fs.first + (o0 + o) * fs.stride; }
};

// bbox[o] over entry o's frames: ordered images of (min x, y, z, max x, y, z), preset to (~0, ~0, ~0, 0, 0, 0); grid (a few blocks, B)
template <typename Frames>
__global__ void __launch_bounds__(kCellBlock) k_cells_bbox(const void *__restrict__ xyz, int is_f64, unsigned N, const unsigned *__restrict__ sel,
                                                           unsigned n_sel, Frames fr, unsigned long long *__restrict__ bbox)
{
    __shared__ double sh[kCellBlock / 64];
    unsigned const o = blockIdx.y;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (unsigned k = blockIdx.x * kCellBlock + threadIdx.x; k < n_sel; k += gridDim.x * kCellBlock)
        for (int which = 0; which < Frames::kFrames; which++) {
            double p[3];
            load3(xyz, is_f64, ((size_t)fr.frame(o, which) * N + sel[k]) * 3, p);
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

// the records of the batch keyed (entry, cell); fill(o, bead, r) writes the record of `bead` in entry o's frame, r.p its position there
template <typename Rec, typename Fill>
__global__ void __launch_bounds__(kCellBlock) k_cells_keys(Fill fill, const unsigned *__restrict__ sel, unsigned n_sel, unsigned B,
                                                           const Grid *__restrict__ grids, int periodic, unsigned cap,
                                                           unsigned long long *__restrict__ keys, unsigned *__restrict__ vals, Rec *__restrict__ grec)
{
    size_t const idx = (size_t)blockIdx.x * kCellBlock + threadIdx.x;
    if (idx >= (size_t)B * n_sel) return;
    unsigned const o = (unsigned)(idx / n_sel), k = (unsigned)(idx % n_sel);
    Rec r;
    fill(o, sel[k], r);
    Grid const g = grids[o];
    keys[idx] = cell_key(g, r.p, periodic, o, cap);
    vals[idx] = (unsigned)idx;
    grec[idx] = r;
}

// The Fill of a record that is a position, a label and a bead index (cluster, van Hove): bead `bead` in frame `which` of entry o
template <typename Frames>
struct PositionFill {
    const void *xyz;
    int is_f64;
    unsigned N;
    const int *label;
    Frames fr;
    int which;
    template <typename Rec>
    __device__ void operator()(unsigned o, unsigned bead, Rec &r) const
    {
        load3(xyz, is_f64, ((size_t)fr.frame(o, which) * N + bead) * 3, r.p);
        r.label = label ? label[bead] : 0;
        r.bead = bead;
    }
};

// ---- the neighbour-cell tile walk of the pair kernels (k_dcorr_pairs, k_cluster_link, k_vh_pairs).  A block owns one work item: up to
// kCellChunk centres of one cell, held in registers.  Every bead of a cell wants the same 27 cells (fewer at an open edge, every cell
// once where an axis has fewer than 3), so the block stages them through LDS in tiles, one x-row span at a time, word-planar: word f of
// record k lies at tile_words[f * (tile + kCellTilePad) + k].  Lane = (centre, slice): the kCellBlock / centres (a power of two) lanes of a
// centre walk a tile interleaved, so a wave reads a few consecutive words of an array (no bank conflict for 8-byte reads, identical
// addresses broadcast) and small cells still fill the block.
constexpr unsigned kCellTilePad = 2;      // words between the arrays of a tile: staging writes the fields of 2 records per 16 lanes

struct CellWork {      // a work item as a lane sees it
    unsigned o, cell;          // entry of the batch, cell of its grid
    unsigned s_begin, nc;      // the centres: sorted indices [s_begin, s_begin + nc)
    unsigned gs, ci, sl;       // lanes per centre; this lane's centre and its slice
    bool active;               // ci < nc
};

// starts: the cell starts of the centres' index, `cap` a frame
__device__ inline CellWork cell_work(uint2 w, const unsigned *__restrict__ starts, unsigned cap)
{
    CellWork c;
    c.o = w.x / cap;
    c.cell = w.x % cap;
    const unsigned *st = starts + (size_t)c.o * cap;
    c.s_begin = st[c.cell] + w.y * kCellChunk;
    c.nc = min(st[c.cell + 1] - c.s_begin, kCellChunk);
    c.gs = 1;
    while (2 * c.gs * c.nc <= (unsigned)kCellBlock) c.gs *= 2;
    c.ci = threadIdx.x / c.gs;
    c.sl = threadIdx.x % c.gs;
    c.active = c.ci < c.nc;
    return c;
}

// Walks the cells around `cell` of grid g in the index (recs in sorted order, st: its cell starts of this frame) from sorted index j_min
// on, in tiles of `tile` records (unsigned, or a std::integral_constant where the LDS is static) of which the first kStaged of the kWords
// 8-byte words of a record are staged between the tile's two barriers; then the active lanes call body(j0, nt): the tile holds the
// records [j0, j0 + nt).  Every lane of the block calls this with the same g, cell, st, j_min and tile.
template <bool kPeriodic, unsigned kStaged, unsigned kWords, typename Rec, typename Tile, typename Body>
__device__ inline void cell_tile_walk(const Grid &g, unsigned cell, const unsigned *__restrict__ st, unsigned j_min, const Rec *__restrict__ recs,
                                      unsigned long long *tile_words, Tile tile, bool active, Body &&body)
{
    static_assert(sizeof(Rec) == 8 * kWords && kStaged <= kWords, "a record is kWords 8-byte words");
    unsigned const tsize = tile, stride = tsize + kCellTilePad;
    int const cx = (int)(cell % (unsigned)g.n[0]), cy = (int)(cell / (unsigned)g.n[0] % (unsigned)g.n[1]),
              cz = (int)(cell / ((unsigned)g.n[0] * (unsigned)g.n[1]));
    int x0, nx, y0, ny, z0, nz;
    axis_cells(cx, g.n[0], kPeriodic, x0, nx);
    axis_cells(cy, g.n[1], kPeriodic, y0, ny);
    axis_cells(cz, g.n[2], kPeriodic, z0, nz);
    int const xa1 = min(x0 + nx, g.n[0]), xb1 = x0 + nx - xa1;      // [x0, x0 + nx) split where it wraps past the last cell
    for (int iz = 0; iz < nz; iz++) {
        int const pz = (z0 + iz) % g.n[2];
        for (int iy = 0; iy < ny; iy++) {
            int const py = (y0 + iy) % g.n[1];
            unsigned const row = ((unsigned)pz * (unsigned)g.n[1] + (unsigned)py) * (unsigned)g.n[0];
            for (int span = 0; span < 2; span++) {
                unsigned const j_begin = max(span ? st[row] : st[row + x0], j_min);
                unsigned const j_end = span ? st[row + xb1] : st[row + xa1];
                for (unsigned j0 = j_begin; j0 < j_end; j0 += tsize) {
                    unsigned const nt = min(tsize, j_end - j0);
                    __syncthreads();      // the last tile has been read (and, the first time, whatever the kernel set up in LDS is there)
                    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(recs + j0);
                    for (unsigned e = threadIdx.x; e < nt * kWords; e += kCellBlock) {
                        unsigned const field = e % kWords;
                        if (kStaged == kWords || field < kStaged) tile_words[field * stride + e / kWords] = src[e];
                    }
                    __syncthreads();
                    if (active) body(j0, nt);
                }
            }
        }
    }
}

}  // namespace

// The cell index of one batch: B frames of n selected beads, `cap` cell slots a frame.  A batch goes room(), make_grids(), make_keys()
// into keys[0], vals[0] and grec, sort(), and, after whatever else the module queues, work_items(), which waits for the stream.
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

    // the grid of every entry of the batch; in an open box after the bounding boxes over its frames, whose preset waits for the stream once
    template <typename Frames>
    int make_grids(hipStream_t st, const void *xyz, int is_f64, unsigned N, const unsigned *sel, unsigned n, Frames fr, unsigned B, const Space &sp, unsigned cap)
    {
        if (!sp.periodic) {
            std::vector<unsigned long long> init(6 * (size_t)B);
            for (size_t k = 0; k < init.size(); k++) init[k] = k % 6 < 3 ? ~0ull : 0ull;
            HIPCHK(hipMemcpyAsync(bbox.p, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));      // init is about to go out of scope
            hipLaunchKernelGGL(k_cells_bbox<Frames>, dim3(std::min(blocks_for(n, kCellBlock), 16u), B), dim3(kCellBlock), 0, st, xyz, is_f64, N, sel, n, fr, bbox.p);
        }
        hipLaunchKernelGGL(k_cells_grid, dim3(blocks_for(B, kCellBlock)), dim3(kCellBlock), 0, st, bbox.p, B, sp, cap, grids.p);
        return GD_OK;
    }

    // the records of the batch (grec) and their keys on `on_grids` (this index's own, or another's of the same entries)
    template <typename Fill>
    int make_keys(hipStream_t st, Fill fill, const unsigned *sel, unsigned n, unsigned B, const Grid *on_grids, int periodic, unsigned cap)
    {
        hipLaunchKernelGGL((k_cells_keys<Rec, Fill>), dim3(blocks_for((size_t)B * n, kCellBlock)), dim3(kCellBlock), 0, st, fill, sel, n, B, on_grids, periodic, cap,
                           keys[0].p, vals[0].p, grec.p);
        HIPCHK(hipGetLastError());
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
