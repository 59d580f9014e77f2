// gdyn_gyr.hip -- gyration tensors of the segments of a trajectory history and the compaction profile along its chains
// (include/gdyn_gyr.h): per frame the centre and the six centred second-moment sums of every segment, and Rg^2 of a sliding window
// of w beads.  Beyond the reference.
//
//   k_gyr_pieces<T, PASS>   one block per (run of kRun pieces, frame).  A piece is up to GD_GYR_PIECE_BEADS beads of one segment.  The
//                           block loads its pieces' coordinates coalesced (a piece is 96 consecutive values of the history), converts
//                           them to fp64 and keeps them in LDS as [axis][piece][kLd = 33 doubles]; then a lane owns one (component,
//                           piece) and sums it serially.  Piece p of a wave's 64 lanes starts 33 doubles after piece p - 1: a
//                           ds_read_b64 of 64 lanes touches every bank pair once (with a stride of 32 all lanes would hit the same two
//                           banks).  PASS 1 sums the three coordinates, PASS 2 the six products of the coordinates less the
//                           segment's centre of pass 1.
//   k_gyr_segments<C>       one lane per (frame, segment, component): adds the segment's pieces ascending; C == 3 also divides by n.
//   k_gyr_windows<T, FRAMES> one launch per window size w, one block per (tile of window starts within a chain, range of GD_GYR_FRAME_RANGE
//                           selected frames).  For every frame of its range the block stages the tile's beads and the w - 1 after them,
//                           clipped to the chain, into LDS as fp64 [axis][bead], and every lane walks its windows, two passes of w beads
//                           each.  Consecutive lanes read consecutive doubles.  v and v * v are accumulated in registers over the frames
//                           of the range (FRAMES: v is written per frame instead).  No sum crosses lanes, so no bit depends on the tile.
//                           (One block looping over all window sizes of a call, staging once, was built first: unrolled over the eight
//                           sizes it took 167 VGPRs and spilled 64 SGPRs; the history is read once more per size instead.)
//   k_gyr_ranges            one lane per (window size, bead): adds the ranges ascending.
// The history itself (upload, non-finite check) is gd::History's (gdyn_history.hpp).
// fp64 throughout, -ffp-contract=off (csrc/Makefile), no fast-math, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_gyr.h"
#include "gdyn_analysis.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr unsigned kPiece = GD_GYR_PIECE_BEADS;
constexpr unsigned kRun = 64;                        // pieces of one block: a lane of a wave owns one
constexpr unsigned kLd = kPiece + 1;                 // doubles between two pieces in LDS
constexpr unsigned kRange = GD_GYR_FRAME_RANGE;
constexpr unsigned kMaxWindows = GD_GYR_MAX_WINDOWS;
constexpr unsigned kMaxWindow = GD_GYR_MAX_WINDOW;
constexpr unsigned kAutoTile = 256, kMaxTile = 512;
constexpr unsigned kSlots = kMaxTile / kBlock;       // window starts of one lane
constexpr size_t kScratchBytes = (size_t)1 << 28;    // piece partials of one launch (automatic frames_per_launch)
static_assert(3 * (kMaxTile + kMaxWindow - 1) * sizeof(double) <= 64 * 1024, "a tile and its longest windows fit the LDS that needs no opt-in");
static_assert(3 * kRun * kLd * sizeof(double) <= 64 * 1024 && kRun == 64 && kLd % 2 == 1, "one piece per lane of a wave, odd stride");

struct Piece {
    uint32_t start, len, segment;
};

struct PieceArgs {
    const void *x;            // the history, (F, N, 3) of T
    const Piece *pieces;      // (P)
    const double *centre;     // (K, S, 3), pass 2
    double *partial;          // (frames of the launch, P, 3 or 6)
    size_t N;
    unsigned P, S;
    unsigned first, stride, k0;      // the launch's frames are k0 + blockIdx.y
};

template <typename T, int PASS>
__global__ void __launch_bounds__(kBlock) k_gyr_pieces(PieceArgs p)
{
    __shared__ double lds[3][kRun * kLd];
    __shared__ Piece mine[kRun];
    unsigned const tid = threadIdx.x, p0 = blockIdx.x * kRun, k = p.k0 + blockIdx.y;
    size_t const f = (size_t)p.first + (size_t)k * p.stride;
    if (tid < kRun) mine[tid] = p0 + tid < p.P ? p.pieces[p0 + tid] : Piece{0, 0, 0};
    __syncthreads();
    const T *x = static_cast<const T *>(p.x) + f * 3 * p.N;
    for (unsigned e = tid; e < kRun * 3 * kPiece; e += kBlock) {
        unsigned const pl = e / (3 * kPiece), r = e % (3 * kPiece);
        if (r < 3 * mine[pl].len) lds[r % 3][pl * kLd + r / 3] = (double)x[3 * (size_t)mine[pl].start + r];      // start + len <= N
    }
    __syncthreads();
    constexpr unsigned C = PASS == 1 ? 3 : 6;
    for (unsigned item = tid; item < C * kRun; item += kBlock) {
        unsigned const c = item / kRun, pl = item % kRun;      // c is uniform over a wave
        if (p0 + pl >= p.P) continue;
        unsigned const len = mine[pl].len;
        double s = 0.0;
        if (PASS == 1) {
            const double *v = lds[c] + pl * kLd;
            for (unsigned j = 0; j < len; j++) s += v[j];
        } else {
            unsigned const a = c < 3 ? c : (c == 5 ? 1 : 0), b = c < 3 ? c : (c == 3 ? 1 : 2);      // xx yy zz xy xz yz
            const double *centre = p.centre + ((size_t)k * p.S + mine[pl].segment) * 3;
            double const ca = centre[a], cb = centre[b];
            const double *va = lds[a] + pl * kLd, *vb = lds[b] + pl * kLd;
            for (unsigned j = 0; j < len; j++) {
                double const da = va[j] - ca, db = vb[j] - cb;
                s += da * db;
            }
        }
        p.partial[((size_t)blockIdx.y * p.P + p0 + pl) * C + c] = s;
    }
}

// out[k0 + fl, s, c] = the pieces of segment s added ascending; C == 3: centre = out / n as well
template <unsigned C>
__global__ void __launch_bounds__(kBlock) k_gyr_segments(const double *partial, const uint32_t *first_piece, const uint32_t *segments, double *out, double *centre,
                                                         unsigned P, unsigned S, unsigned k0, unsigned frames)
{
    size_t const e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (size_t)frames * S * C) return;
    unsigned const c = e % C, s = (e / C) % S;
    size_t const fl = e / C / S;
    double total = 0.0;
    for (unsigned q = first_piece[s]; q < first_piece[s + 1]; q++) total += partial[(fl * P + q) * C + c];
    size_t const at = ((k0 + fl) * S + s) * C + c;
    out[at] = total;
    if (C == 3) centre[at] = total / (double)(segments[2 * s + 1] - segments[2 * s]);
}

struct Tile {
    uint32_t start, n, chain_end;      // the window starts [start, start + n) of a chain that ends at chain_end
};

struct WindowArgs {
    const void *x;
    const Tile *tiles;
    double *out, *out_sq;     // partial sums (ranges of the launch, n_windows, N) of window m, or, FRAMES, v (K, N)
    size_t N;
    unsigned K, first, stride;
    unsigned range0;          // the launch's ranges are range0 + blockIdx.y
    unsigned n_windows, w;    // the launch serves one window size
    unsigned ld;              // doubles between two axes in LDS: tile + w - 1
};

template <typename T, bool FRAMES>
__global__ void __launch_bounds__(kBlock) k_gyr_windows(WindowArgs p)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    Tile const tile = p.tiles[blockIdx.x];
    unsigned const tid = threadIdx.x, w = p.w;
    if (tile.start + w > tile.chain_end) return;      // the tile holds windows of a shorter size only (block-uniform)
    unsigned const staged = min(tile.n + w - 1, tile.chain_end - tile.start);      // <= ld
    unsigned const k0 = (p.range0 + blockIdx.y) * kRange, k1 = min(p.K, k0 + kRange);
    const double *X = lds, *Y = lds + p.ld, *Z = lds + 2 * p.ld;
    double const dw = (double)w;

    double acc[kSlots], acc_sq[kSlots];
#pragma unroll
    for (unsigned u = 0; u < kSlots; u++) acc[u] = acc_sq[u] = 0.0;

    for (unsigned k = k0; k < k1; k++) {
        size_t const f = (size_t)p.first + (size_t)k * p.stride;
        const T *x = static_cast<const T *>(p.x) + (f * p.N + tile.start) * 3;
        __syncthreads();      // the last frame has been read
        for (unsigned e = tid; e < 3 * staged; e += kBlock) lds[(e % 3) * p.ld + e / 3] = (double)x[e];      // start + staged <= chain_end <= N
        __syncthreads();
#pragma unroll
        for (unsigned u = 0; u < kSlots; u++) {
            unsigned const t = tid + u * kBlock;
            if (t >= tile.n || tile.start + t + w > tile.chain_end) continue;      // t + w <= staged
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (unsigned j = t; j < t + w; j++) {
                sx += X[j];
                sy += Y[j];
                sz += Z[j];
            }
            double const cx = sx / dw, cy = sy / dw, cz = sz / dw;
            double s = 0.0;
            for (unsigned j = t; j < t + w; j++) {
                double const dx = X[j] - cx, dy = Y[j] - cy, dz = Z[j] - cz;
                s += (dx * dx + dy * dy) + dz * dz;
            }
            double const v = s / dw;
            if (FRAMES) {
                p.out[(size_t)k * p.N + tile.start + t] = v;
            } else {
                acc[u] += v;
                acc_sq[u] += v * v;
            }
        }
    }
    if (FRAMES) return;
#pragma unroll
    for (unsigned u = 0; u < kSlots; u++) {
        unsigned const t = tid + u * kBlock;
        if (t >= tile.n || tile.start + t + w > tile.chain_end) continue;
        size_t const at = (size_t)blockIdx.y * p.n_windows * p.N + tile.start + t;
        p.out[at] = acc[u];
        p.out_sq[at] = acc_sq[u];
    }
}

// sum[m, i] and sum_sq[m, i]: the ranges added ascending, from +0; entries no block wrote are the +0 the partial sums were cleared to
__global__ void __launch_bounds__(kBlock) k_gyr_ranges(const double *partial, const double *partial_sq, double *sum, double *sum_sq, size_t cells, unsigned ranges)
{
    size_t const e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= cells) return;
    double s = 0.0, q = 0.0;
    for (unsigned r = 0; r < ranges; r++) {
        s += partial[r * cells + e];
        q += partial_sq[r * cells + e];
    }
    sum[e] = s;
    sum_sq[e] = q;
}

}  // namespace

struct gd_gyr : gd::handle {
    unsigned tile = kAutoTile, frames_per_launch = 0;
    History hist;
    bool have_segments = false, have_chains = false;      // false: one range [0, N)
    std::vector<uint32_t> segments, chains;               // (S, 2), (C, 2) ranges of hist.beads()
    unsigned P = 0;                                       // pieces of the segments
    dbuf<Piece> pieces;
    dbuf<uint32_t> first_piece, segments_dev;             // (S + 1), (S, 2)
    // per call
    dbuf<double> partial, partial_sq, out;
    dbuf<Tile> tiles;
    StageTimer timer;                                     // gd_gyr_last_times: tensors, windows, merge

    unsigned S() const { return (unsigned)(segments.size() / 2); }
};

namespace {

// the segments of a handle become `ranges`, with their pieces; the device copies are replaced only when all have been made
int install_segments(gd_gyr *h, std::vector<uint32_t> ranges, bool have)
{
    std::vector<Piece> pieces;
    std::vector<uint32_t> first(ranges.size() / 2 + 1, 0);
    for (size_t s = 0; s < ranges.size() / 2; s++) {
        for (uint32_t a = ranges[2 * s]; a < ranges[2 * s + 1]; a += kPiece) pieces.push_back({a, std::min(kPiece, ranges[2 * s + 1] - a), (uint32_t)s});
        first[s + 1] = (uint32_t)pieces.size();      // at most N / 32 + S
    }
    dbuf<Piece> pd;
    dbuf<uint32_t> fd, sd;
    HIPCHK(pd.upload(pieces.data(), pieces.size()));
    HIPCHK(fd.upload(first.data(), first.size()));
    HIPCHK(sd.upload(ranges.data(), ranges.size()));
    h->pieces = std::move(pd);
    h->first_piece = std::move(fd);
    h->segments_dev = std::move(sd);
    h->P = (unsigned)pieces.size();
    h->segments = std::move(ranges);
    h->have_segments = have;
    return GD_OK;
}

History::Rebind rebind(gd_gyr *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads() || h->segments.empty()) {      // the ranges belonged to another N
            GDCHK(install_segments(h, {0, n_beads}, false));
            h->chains = {0, n_beads};
            h->have_chains = false;
        }
        return GD_OK;
    };
}

// the selected frames of a call (include/gdyn_gyr.h, Frames): K of them, or a refusal
int select_frames(const char *who, unsigned F, uint32_t first, uint32_t stride, uint32_t count, unsigned *K)
{
    if (stride == 0) return fail(GD_EINVAL, "%s: stride 0", who);
    uint64_t const fit = frames_fit(F, first, stride);
    if (count > fit || fit == 0)
        return fail(GD_EINVAL, "%s: %s from frame %u with stride %u: %llu fit in %u frames", who, count ? "the frames asked for" : "no frame", first, stride,
                    (unsigned long long)fit, F);
    *K = (unsigned)frames_served(fit, count);
    return GD_OK;
}

int check_windows(const char *who, const uint32_t *windows, uint32_t n)
{
    if (n < 1 || n > kMaxWindows) return fail(GD_EINVAL, "%s: %u window sizes, 1 to %u are served at once", who, n, kMaxWindows);
    for (uint32_t m = 0; m < n; m++)
        if (windows[m] < 2 || windows[m] > kMaxWindow) return fail(GD_EINVAL, "%s: window %u of %u beads, 2 to %u are served", who, m, windows[m], kMaxWindow);
    return GD_OK;
}

// the tiles of the chains that hold a valid window of w_min beads: `tile` window starts each, cut from the chain's start
std::vector<Tile> make_tiles(const std::vector<uint32_t> &chains, unsigned tile, unsigned w_min)
{
    std::vector<Tile> out;
    for (size_t c = 0; c < chains.size() / 2; c++) {
        uint32_t const start = chains[2 * c], end = chains[2 * c + 1];
        if (end - start < w_min) continue;
        uint32_t const last = end - w_min;      // the last valid start
        for (uint64_t a = start; a <= last; a += tile) out.push_back({(uint32_t)a, (uint32_t)std::min<uint64_t>(tile, (uint64_t)last + 1 - a), end});
    }
    return out;
}

// the window kernel of every window size over all ranges of K frames, `per_launch` ranges a launch.  A launch serves one window size
// with the LDS that size needs
template <bool FRAMES>
int launch_windows(gd_gyr *h, WindowArgs a, const uint32_t *windows, unsigned n_tiles, unsigned ranges, unsigned per_launch)
{
    double *const out = a.out, *const out_sq = a.out_sq;
    for (unsigned m = 0; m < a.n_windows; m++) {
        a.w = windows[m];
        a.ld = h->tile + a.w - 1;
        size_t const lds = (size_t)3 * a.ld * sizeof(double);
        for (unsigned r0 = 0; r0 < ranges; r0 += per_launch) {
            unsigned const n = std::min(per_launch, ranges - r0);
            a.range0 = r0;
            if (!FRAMES) {      // the partial sums of range r0, window m
                a.out = out + ((size_t)r0 * a.n_windows + m) * a.N;
                a.out_sq = out_sq + ((size_t)r0 * a.n_windows + m) * a.N;
            }
            if (h->hist.is_f64) hipLaunchKernelGGL((k_gyr_windows<double, FRAMES>), dim3(n_tiles, n), dim3(kBlock), lds, h->stream, a);
            else hipLaunchKernelGGL((k_gyr_windows<float, FRAMES>), dim3(n_tiles, n), dim3(kBlock), lds, h->stream, a);
            HIPCHK(hipGetLastError());
        }
    }
    return GD_OK;
}

// what gd_gyr_profile and gd_gyr_profile_frames share: the checks, the tiles, the window kernel into h->partial(_sq) or h->out
template <bool FRAMES>
int run_windows(const char *who, gd_gyr *h, const uint32_t *windows, uint32_t n_windows, uint32_t first, uint32_t stride, uint32_t count, unsigned *K_out,
                unsigned *ranges_out)
{
    unsigned const F = h->hist.frames();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    if (!windows) return fail(GD_EINVAL, "%s: NULL argument", who);
    GDCHK(check_windows(who, windows, n_windows));
    unsigned K = 0;
    GDCHK(select_frames(who, F, first, stride, count, &K));
    HIPCHK(hipSetDevice(h->device));
    size_t const N = h->hist.beads();
    unsigned const w_min = *std::min_element(windows, windows + n_windows);
    unsigned const ranges = (K + kRange - 1) / kRange;
    std::vector<Tile> const tiles = make_tiles(h->chains, h->tile, w_min);
    if (tiles.size() > (1u << 30)) return fail(GD_EINVAL, "%s: %zu tiles exceed 2^30", who, tiles.size());
    size_t const cells = FRAMES ? (size_t)K * N : (size_t)ranges * n_windows * N;
    bool fits = FRAMES ? h->out.ensure(cells) == hipSuccess
                       : h->partial.ensure(cells) == hipSuccess && h->partial_sq.ensure(cells) == hipSuccess && h->out.ensure(2 * (size_t)n_windows * N) == hipSuccess;
    if (!fits) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: the outputs of %u frames x %zu beads do not fit on the device", who, K, N);
    }
    HIPCHK(h->tiles.upload(tiles.data(), tiles.size()));
    WindowArgs a{};
    a.x = h->hist.x();
    a.tiles = h->tiles.p;
    a.out = FRAMES ? h->out.p : h->partial.p;
    a.out_sq = FRAMES ? nullptr : h->partial_sq.p;
    a.N = N;
    a.K = K;
    a.first = first;
    a.stride = stride;
    a.n_windows = n_windows;
    HIPCHK(h->timer.mark(0, h->stream));
    // entries of windows that are not valid stay +0
    if (FRAMES) HIPCHK(hipMemsetAsync(h->out.p, 0, cells * sizeof(double), h->stream));
    else {
        HIPCHK(hipMemsetAsync(h->partial.p, 0, cells * sizeof(double), h->stream));
        HIPCHK(hipMemsetAsync(h->partial_sq.p, 0, cells * sizeof(double), h->stream));
    }
    if (!tiles.empty()) {
        unsigned const asked = h->frames_per_launch ? std::max(h->frames_per_launch / kRange, 1u) : 65535u;
        GDCHK(launch_windows<FRAMES>(h, a, windows, (unsigned)tiles.size(), ranges, std::min(asked, 65535u)));
    }
    HIPCHK(h->timer.mark(1, h->stream));
    *K_out = K;
    *ranges_out = ranges;
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_gyr_abi_version(void) { return GD_GYR_ABI_VERSION; }

int gd_gyr_create(const gd_gyr_desc *desc, gd_gyr **out)
{
    const char *who = "gd_gyr_create";
    if (desc && desc->beads_per_tile > kMaxTile) return fail(GD_EINVAL, "%s: beads_per_tile %u exceeds %u", who, desc->beads_per_tile, kMaxTile);
    if (int rc = gd::open(who, desc, out)) return rc;
    (*out)->tile = desc->beads_per_tile ? desc->beads_per_tile : kAutoTile;
    (*out)->frames_per_launch = desc->frames_per_launch;
    if (hipError_t const rc = (*out)->timer.create()) {
        gd::close(*out);
        *out = nullptr;
        return fail(GD_EHIP, "%s: hipEventCreate failed: %s", who, hipGetErrorString(rc));
    }
    return GD_OK;
}

int gd_gyr_destroy(gd_gyr *h) { return gd::close(h); }

int gd_gyr_set_history(gd_gyr *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_gyr_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_gyr_set_history_live(gd_gyr *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_gyr_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_gyr_set_segments(gd_gyr *h, const uint32_t *ranges, uint32_t n_segments)
{
    const char *who = "gd_gyr_set_segments";
    if (!h || (!ranges && n_segments)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the segments are ranges of its beads)", who);
    if (n_segments > (1u << 28)) return fail(GD_EINVAL, "%s: %u segments exceed 2^28", who, n_segments);
    HIPCHK(hipSetDevice(h->device));
    if (!n_segments) return install_segments(h, {0, h->hist.beads()}, false);
    if (int rc = check_ranges(who, "segment", false, ranges, n_segments, h->hist.beads())) return rc;
    return install_segments(h, std::vector<uint32_t>(ranges, ranges + 2 * (size_t)n_segments), true);
}

int gd_gyr_set_chains(gd_gyr *h, const uint32_t *ranges, uint32_t n_chains)
{
    const char *who = "gd_gyr_set_chains";
    if (!h || (!ranges && n_chains)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the chains are ranges of its beads)", who);
    if (n_chains > (1u << 28)) return fail(GD_EINVAL, "%s: %u chains exceed 2^28", who, n_chains);
    if (n_chains)
        if (int rc = check_ranges(who, "chain", true, ranges, n_chains, h->hist.beads())) return rc;
    h->chains = n_chains ? std::vector<uint32_t>(ranges, ranges + 2 * (size_t)n_chains) : std::vector<uint32_t>{0, h->hist.beads()};
    h->have_chains = n_chains != 0;
    return GD_OK;
}

int gd_gyr_tensors(gd_gyr *h, uint32_t first, uint32_t stride, uint32_t count, double *centre_sum, double *centre, double *moment)
{
    const char *who = "gd_gyr_tensors";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames(), S = h->S(), P = h->P;
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    unsigned K = 0;
    GDCHK(select_frames(who, F, first, stride, count, &K));
    HIPCHK(hipSetDevice(h->device));

    // out: centre_sum (K, S, 3), centre (K, S, 3), moment (K, S, 6)
    size_t const plane = (size_t)K * S * 3;
    unsigned const automatic = (unsigned)std::max<size_t>(kScratchBytes / ((size_t)P * 6 * sizeof(double)), 1);
    unsigned const per_launch = std::min({h->frames_per_launch ? h->frames_per_launch : automatic, K, 65535u});
    if (h->out.ensure(4 * plane) != hipSuccess || h->partial.ensure((size_t)per_launch * P * 6) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: the tensors of %u frames x %u segments do not fit on the device", who, K, S);
    }
    double *const d_sum = h->out.p, *const d_centre = h->out.p + plane, *const d_moment = h->out.p + 2 * plane;
    PieceArgs a{h->hist.x(), h->pieces.p, d_centre, h->partial.p, h->hist.beads(), P, S, first, stride, 0};
    bool const f64 = h->hist.is_f64;
    HIPCHK(h->timer.mark(0, h->stream));
    for (unsigned k0 = 0; k0 < K; k0 += per_launch) {
        unsigned const n = std::min(per_launch, K - k0);
        dim3 const grid((P + kRun - 1) / kRun, n);
        a.k0 = k0;
        if (f64) hipLaunchKernelGGL((k_gyr_pieces<double, 1>), grid, dim3(kBlock), 0, h->stream, a);
        else hipLaunchKernelGGL((k_gyr_pieces<float, 1>), grid, dim3(kBlock), 0, h->stream, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_gyr_segments<3>, dim3(blocks_for((size_t)n * S * 3, kBlock)), dim3(kBlock), 0, h->stream, h->partial.p, h->first_piece.p,
                           h->segments_dev.p, d_sum, d_centre, P, S, k0, n);
        HIPCHK(hipGetLastError());
        if (!moment) continue;
        if (f64) hipLaunchKernelGGL((k_gyr_pieces<double, 2>), grid, dim3(kBlock), 0, h->stream, a);
        else hipLaunchKernelGGL((k_gyr_pieces<float, 2>), grid, dim3(kBlock), 0, h->stream, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_gyr_segments<6>, dim3(blocks_for((size_t)n * S * 6, kBlock)), dim3(kBlock), 0, h->stream, h->partial.p, h->first_piece.p,
                           h->segments_dev.p, d_moment, (double *)nullptr, P, S, k0, n);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(h->timer.mark(1, h->stream));
    if (centre_sum) HIPCHK(hipMemcpyAsync(centre_sum, d_sum, plane * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (centre) HIPCHK(hipMemcpyAsync(centre, d_centre, plane * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (moment) HIPCHK(hipMemcpyAsync(moment, d_moment, 2 * plane * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(h->timer.between(0, 1, &h->timer.ms[0]));
    return GD_OK;
}

int gd_gyr_profile(gd_gyr *h, const uint32_t *windows, uint32_t n_windows, uint32_t first, uint32_t stride, uint32_t count, double *sum, double *sum_sq,
                   uint64_t *count_out)
{
    const char *who = "gd_gyr_profile";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned K = 0, ranges = 0;
    GDCHK(run_windows<false>(who, h, windows, n_windows, first, stride, count, &K, &ranges));
    size_t const N = h->hist.beads(), cells = (size_t)n_windows * N;
    hipLaunchKernelGGL(k_gyr_ranges, dim3(blocks_for(cells, kBlock)), dim3(kBlock), 0, h->stream, h->partial.p, h->partial_sq.p, h->out.p, h->out.p + cells, cells,
                       ranges);
    HIPCHK(hipGetLastError());
    HIPCHK(h->timer.mark(2, h->stream));
    if (sum) HIPCHK(hipMemcpyAsync(sum, h->out.p, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (sum_sq) HIPCHK(hipMemcpyAsync(sum_sq, h->out.p + cells, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(h->timer.between(0, 1, &h->timer.ms[1]));
    HIPCHK(h->timer.between(1, 2, &h->timer.ms[2]));
    if (count_out) {
        std::fill(count_out, count_out + cells, (uint64_t)0);
        for (uint32_t m = 0; m < n_windows; m++)
            for (size_t c = 0; c < h->chains.size() / 2; c++)
                for (uint64_t i = h->chains[2 * c]; i + windows[m] <= h->chains[2 * c + 1]; i++) count_out[m * N + i] = K;
    }
    return GD_OK;
}

int gd_gyr_profile_frames(gd_gyr *h, uint32_t window, uint32_t first, uint32_t stride, uint32_t count, double *out)
{
    const char *who = "gd_gyr_profile_frames";
    if (!h || !out) return fail(GD_EINVAL, "%s: NULL argument", who);
    unsigned K = 0, ranges = 0;
    GDCHK(run_windows<true>(who, h, &window, 1, first, stride, count, &K, &ranges));
    HIPCHK(hipMemcpyAsync(out, h->out.p, (size_t)K * h->hist.beads() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(h->timer.between(0, 1, &h->timer.ms[1]));
    h->timer.ms[2] = 0.0;
    return GD_OK;
}

int gd_gyr_last_times(const gd_gyr *h, double *tensors_ms, double *windows_ms, double *merge_ms)
{
    if (!h) return fail(GD_EINVAL, "gd_gyr_last_times: NULL handle");
    h->timer.report(tensors_ms, windows_ms, merge_ms);
    return GD_OK;
}

}  // extern "C"
