// gdyn_dwell.hip -- contact dwell times and the contact autocorrelation of given pairs of beads of a trajectory history
// (include/gdyn_dwell.h): the runs of the contact state of every pair by state, kind and length bin, the sums of their lengths, and
// the products c_k c_{k+lag} summed over pairs and frames.  Beyond the reference.  Every output is an integer.
//
// A launch takes a batch of pairs and ALL selected frames, so no state is carried from one launch to the next.  A lane is one pair:
// in separations mode lane t of row y (blockIdx.y, the separation) is the pair (i, i + s_y) of the first bead i = t0 + t, which takes
// part when both beads lie in one chain (chain_end[i], 0 for a bead in no chain); in pairs mode lane t is the pair t0 + t of the
// caller's list and its row is row[t0 + t], or the pair's own index.
//
//   k_dwell_states<T, SEP, BOX>  a lane walks the selected frames in order with its state in a register and packs 64 frames to a word:
//                                plane[(y W + w) n + t], so the lanes of a wave write (and the two kernels below read) consecutive
//                                words.  The bits of the last word beyond K are zero.  In separations mode consecutive lanes read
//                                consecutive beads of a frame, and the second stream is the first one shifted by s.
//   k_dwell_runs<SEP>            a lane walks its words and peels runs with the count of trailing zeros of (state ? ~word : word),
//                                masked to the K frames; a run may span any number of words.  SEP: the block shares a row, so the
//                                counts are gathered in LDS (64-bit: a block's lengths sum to 256 K) and flushed with one global
//                                atomic per touched cell.  Pairs mode: every pair may have a row of its own, so straight to global
//                                integer atomics.
//   k_dwell_corr<SEP>            per lag = 64 a + b the lane counts the bits of word[w] & ((word[w + a] >> b) | (word[w + a + 1] <<
//                                (64 - b))); words past the last are zero, and so are the bits past K, which is what keeps k + lag < K.
//                                SEP: reduced in the wave, then in LDS, then one global atomic per block and lag.
// Only integer atomics: every result is bit-identical from run to run and independent of the batch.  The history itself (upload,
// non-finite check) is gd::History's (gdyn_history.hpp).  fp64 pair term, -ffp-contract=off (csrc/Makefile), no fast-math.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_dwell.h"
#include "gdyn_analysis.hpp"
#include "gdyn_frames.hpp"
#include "gdyn_history.hpp"

using namespace gd;

namespace {

typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "the outputs are uint64");

constexpr int kBlock = 256;
constexpr unsigned kMaxBins = GD_DWELL_MAX_BINS, kMaxLags = GD_DWELL_MAX_LAGS, kMaxSeps = GD_DWELL_MAX_SEPARATIONS;
constexpr unsigned kCells = 8 * (kMaxBins + 2);      // of one row: (state, kind) x (the bins, outside, length_sum)
constexpr size_t kPlaneBytes = GD_DWELL_PLANE_BYTES;

struct Args {
    const void *x;                // the history, (F, N, 3) of T
    size_t N;
    unsigned K, first, stride;    // the selected frames first + k stride, k < K
    unsigned W;                   // words of a pair: ceil(K / 64)
    const uint32_t *chain_end;    // SEP: (N) the end of the chain of a bead, 0 for a bead in none
    const uint32_t *seps;         // SEP: (gridDim.y)
    const uint32_t *pairs;        // pairs mode: (P, 2)
    const uint32_t *row;          // pairs mode: (P) or nullptr
    unsigned t0, n;               // the launch's lanes are the first beads / the pairs [t0, t0 + n)
    double on2, off2;
    double box[3];
    u64 *plane;                   // (gridDim.y, W, n)
    const uint32_t *edges;        // (B + 1); B == 0: no bins
    const uint32_t *lags;         // (L)
    unsigned B, L;
    u64 *runs, *outside, *lsum, *hits;      // (R, 8, B), (R, 8), (R, 8), (R, L)
};

// the pair of lane t of row y, or false: no lane of the launch, or (SEP) no pair of one chain
template <bool SEP>
__device__ inline bool lane_pair(const Args &p, unsigned t, unsigned y, unsigned &i, unsigned &j, size_t &row)
{
    if (t >= p.n) return false;
    unsigned const g = p.t0 + t;      // < N, < P: the host cuts the last launch
    if (SEP) {
        uint64_t const far = (uint64_t)g + p.seps[y];
        if (far >= p.chain_end[g]) return false;      // chain_end <= N
        i = g;
        j = (unsigned)far;
        row = y;
    } else {
        i = p.pairs[2 * (size_t)g];
        j = p.pairs[2 * (size_t)g + 1];
        row = p.row ? p.row[g] : g;
    }
    return true;
}

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

template <typename T, bool SEP, bool BOX>
__global__ void __launch_bounds__(kBlock) k_dwell_states(Args p)
{
    unsigned const t = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y;
    unsigned i = 0, j = 0;
    size_t row = 0;
    if (!lane_pair<SEP>(p, t, y, i, j, row)) return;
    const T *x = static_cast<const T *>(p.x);
    u64 *out = p.plane + (size_t)y * p.W * p.n + t;
    size_t const frame = 3 * p.N, oi = 3 * (size_t)i, oj = 3 * (size_t)j;
    bool c = false;      // c_0 = on_0
    for (unsigned w = 0; w < p.W; w++) {
        unsigned const bits = min(64u, p.K - 64 * w);
        u64 word = 0;
#pragma unroll 4
        for (unsigned b = 0; b < bits; b++) {
            size_t const f = (size_t)p.first + (size_t)(64 * w + b) * p.stride;      // < F
            const T *a = x + f * frame;
            double const r2 = pair_r2<BOX>((double)a[oi], (double)a[oi + 1], (double)a[oi + 2], (double)a[oj], (double)a[oj + 1], (double)a[oj + 2], p.box);
            c = c ? r2 < p.off2 : r2 < p.on2;
            word |= (u64)c << b;
        }
        out[(size_t)w * p.n] = word;
    }
}

template <bool SEP>
__global__ void __launch_bounds__(kBlock) k_dwell_runs(Args p)
{
    __shared__ u64 cell[kCells];
    __shared__ uint32_t edges[kMaxBins + 1];
    unsigned const tid = threadIdx.x, t = blockIdx.x * kBlock + tid, y = blockIdx.y, B = p.B, K = p.K;
    unsigned const n_cells = 8 * (B + 2);      // the row's cells: (sk, b) at sk B + b, outside at 8 B + sk, length_sum at 8 B + 8 + sk
    if (SEP)
        for (unsigned c = tid; c < n_cells; c += kBlock) cell[c] = 0;
    if (B)
        for (unsigned e = tid; e <= B; e += kBlock) edges[e] = p.edges[e];
    __syncthreads();
    unsigned i = 0, j = 0;
    size_t row = 0;
    if (lane_pair<SEP>(p, t, y, i, j, row)) {
        auto emit = [&](unsigned state, unsigned start, unsigned end) {      // the run [start, end) of selected frames
            unsigned const len = end - start, sk = state * 4 + (start == 0 ? 1u : 0u) + (end == K ? 2u : 0u);
            if (SEP) atomicAdd(&cell[8 * B + 8 + sk], (u64)len);
            else atomicAdd(&p.lsum[row * 8 + sk], (u64)len);
            if (!B) return;
            unsigned lo = 0, hi = B + 1;      // the edges that are <= len
            while (lo < hi) {
                unsigned const mid = (lo + hi) / 2;
                if (edges[mid] <= len) lo = mid + 1;
                else hi = mid;
            }
            if (lo == 0 || lo == B + 1) {
                if (SEP) atomicAdd(&cell[8 * B + sk], (u64)1);
                else atomicAdd(&p.outside[row * 8 + sk], (u64)1);
            } else {
                if (SEP) atomicAdd(&cell[sk * B + lo - 1], (u64)1);
                else atomicAdd(&p.runs[(row * 8 + sk) * B + lo - 1], (u64)1);
            }
        };
        const u64 *pl = p.plane + (size_t)y * p.W * p.n + t;
        unsigned state = (unsigned)(pl[0] & 1), start = 0;
        for (unsigned w = 0; w < p.W; w++) {
            u64 const word = pl[(size_t)w * p.n];
            unsigned const bits = min(64u, K - 64 * w);
            u64 const frames = bits == 64 ? ~(u64)0 : (((u64)1 << bits) - 1);
            u64 differ = (state ? ~word : word) & frames;      // the frames of the word that are not in the run's state
            while (differ) {
                unsigned const at = (unsigned)__builtin_ctzll(differ);
                emit(state, start, 64 * w + at);
                start = 64 * w + at;
                state ^= 1;
                differ = (state ? ~word : word) & frames & (~(u64)0 << at);
            }
        }
        emit(state, start, K);
    }
    if (!SEP) return;
    __syncthreads();
    for (unsigned c = tid; c < n_cells; c += kBlock) {
        u64 const v = cell[c];
        if (!v) continue;
        if (c < 8 * B) atomicAdd(&p.runs[(size_t)y * 8 * B + c], v);
        else if (c < 8 * B + 8) atomicAdd(&p.outside[(size_t)y * 8 + (c - 8 * B)], v);
        else atomicAdd(&p.lsum[(size_t)y * 8 + (c - 8 * B - 8)], v);
    }
}

template <bool SEP>
__global__ void __launch_bounds__(kBlock) k_dwell_corr(Args p)
{
    __shared__ u64 sum[kMaxLags];
    unsigned const tid = threadIdx.x, t = blockIdx.x * kBlock + tid, y = blockIdx.y, W = p.W;
    if (SEP) {
        if (tid < kMaxLags) sum[tid] = 0;
        __syncthreads();
    }
    unsigned i = 0, j = 0;
    size_t row = 0;
    bool const mine = lane_pair<SEP>(p, t, y, i, j, row);
    const u64 *pl = p.plane + (size_t)y * W * p.n + t;
    for (unsigned l = 0; l < p.L; l++) {
        unsigned const lag = p.lags[l], a = lag >> 6, b = lag & 63;
        u64 count = 0;
        if (mine)
            for (unsigned w = 0; w + a < W; w++) {
                u64 const lo = pl[(size_t)(w + a) * p.n], hi = w + a + 1 < W ? pl[(size_t)(w + a + 1) * p.n] : 0;
                u64 const later = b ? (lo >> b) | (hi << (64 - b)) : lo;      // bit q: c at frame 64 w + q + lag, 0 past K
                count += (u64)__popcll(pl[(size_t)w * p.n] & later);
            }
        if (SEP) {
            for (int off = 32; off; off >>= 1) count += __shfl_xor(count, off);
            if ((tid & 63) == 0 && count) atomicAdd(&sum[l], count);
        } else if (count) {
            atomicAdd(&p.hits[row * p.L + l], count);
        }
    }
    if (!SEP) return;
    __syncthreads();
    if (tid < p.L && sum[tid]) atomicAdd(&p.hits[(size_t)y * p.L + tid], sum[tid]);
}

}  // namespace

struct gd_dwell : gd::handle {
    unsigned pairs_per_launch = 0;
    History hist;
    bool have_chains = false;               // false: one chain [0, N)
    std::vector<uint32_t> chains;           // (C, 2) ranges of hist.beads()
    dbuf<uint32_t> chain_end;               // (N)
    // per call
    dbuf<uint32_t> tables, pairs_dev, row_dev;      // the separations, lags and edges; the caller's pairs and rows
    dbuf<u64> plane, acc;
    StageTimer timer;                       // gd_dwell_last_times: states, runs, corr; its events mark a launch's first three stages
    hipEvent_t done = nullptr;              // and this one the end of the third

    ~gd_dwell()
    {
        if (done) (void)hipEventDestroy(done);
    }
};

namespace {

// the chains of a handle become `ranges`; the device copy is replaced only when the new one has been made
int install_chains(gd_dwell *h, std::vector<uint32_t> ranges, bool have, unsigned N)
{
    std::vector<uint32_t> end(N, 0);
    for (size_t c = 0; c < ranges.size() / 2; c++)
        for (uint32_t i = ranges[2 * c]; i < ranges[2 * c + 1]; i++) end[i] = ranges[2 * c + 1];
    dbuf<uint32_t> d;
    HIPCHK(d.upload(end.data(), end.size()));
    h->chain_end = std::move(d);
    h->chains = std::move(ranges);
    h->have_chains = have;
    return GD_OK;
}

History::Rebind rebind(gd_dwell *h)
{
    return [h](unsigned n_beads) -> int {
        if (n_beads != h->hist.beads() || h->chains.empty()) GDCHK(install_chains(h, {0, n_beads}, false, n_beads));      // the chains belonged to another N
        return GD_OK;
    };
}

// the rule of a call (include/gdyn_dwell.h: State, Frames): its K selected frames, or a refusal
int check_rule(const char *who, unsigned F, const gd_dwell_rule *r, unsigned *K)
{
    if (!r) return fail(GD_EINVAL, "%s: NULL rule", who);
    if (!std::isfinite(r->r_on) || !std::isfinite(r->r_off) || !(r->r_on > 0.0) || !(r->r_on <= r->r_off))
        return fail(GD_EINVAL, "%s: contact radii %g and %g (0 < r_on <= r_off, finite)", who, r->r_on, r->r_off);
    if (r->box)
        for (int k = 0; k < 3; k++)
            if (!(r->box[k] > 0.0) || !std::isfinite(r->box[k])) return fail(GD_EINVAL, "%s: box period %d is %g (positive and finite)", who, k, r->box[k]);
    if (r->stride == 0) return fail(GD_EINVAL, "%s: stride 0", who);
    uint64_t const fit = frames_fit(F, r->first, r->stride);
    if (r->count > fit || fit == 0)
        return fail(GD_EINVAL, "%s: %s from frame %u with stride %u: %llu fit in %u frames", who, r->count ? "the frames asked for" : "no frame", r->first,
                    r->stride, (unsigned long long)fit, F);
    *K = (unsigned)frames_served(fit, r->count);
    return GD_OK;
}

int check_spec(const char *who, const gd_dwell_spec *s, const gd_dwell_out *out)
{
    if (!s || !out) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (s->n_bins > kMaxBins) return fail(GD_EINVAL, "%s: %u bins, at most %u are served at once", who, s->n_bins, kMaxBins);
    if (s->n_lags > kMaxLags) return fail(GD_EINVAL, "%s: %u lags, at most %u are served at once", who, s->n_lags, kMaxLags);
    if ((s->n_bins && !s->edges) || (s->n_lags && !s->lags)) return fail(GD_EINVAL, "%s: NULL edges or lags", who);
    if ((out->runs || out->outside) && !s->n_bins) return fail(GD_EINVAL, "%s: runs by length need at least one bin", who);
    for (uint32_t b = 0; b <= s->n_bins && s->n_bins; b++)
        if (b ? s->edges[b] <= s->edges[b - 1] : s->edges[0] < 1)
            return fail(GD_EINVAL, "%s: edge %u is %u (1 <= e_0 < e_1 < ...)", who, b, s->edges[b]);
    return GD_OK;
}

Args base_args(const gd_dwell *h, const gd_dwell_rule *r, unsigned K)
{
    Args a{};
    a.x = h->hist.x();
    a.N = h->hist.beads();
    a.K = K;
    a.first = r->first;
    a.stride = r->stride;
    a.W = (K + 63) / 64;
    a.on2 = r->r_on * r->r_on;
    a.off2 = r->r_off * r->r_off;
    for (int k = 0; k < 3; k++) a.box[k] = r->box ? r->box[k] : 0.0;
    return a;
}

template <bool SEP>
void launch_states(const gd_dwell *h, dim3 grid, const Args &a, bool box)
{
    if (h->hist.is_f64) {
        if (box) hipLaunchKernelGGL((k_dwell_states<double, SEP, true>), grid, dim3(kBlock), 0, h->stream, a);
        else hipLaunchKernelGGL((k_dwell_states<double, SEP, false>), grid, dim3(kBlock), 0, h->stream, a);
    } else {
        if (box) hipLaunchKernelGGL((k_dwell_states<float, SEP, true>), grid, dim3(kBlock), 0, h->stream, a);
        else hipLaunchKernelGGL((k_dwell_states<float, SEP, false>), grid, dim3(kBlock), 0, h->stream, a);
    }
}

// the lanes of one launch: the handle's pairs_per_launch, or as many as keep `rows` planes of W words within GD_DWELL_PLANE_BYTES
unsigned lanes_per_launch(const gd_dwell *h, unsigned rows, unsigned W, unsigned total)
{
    size_t const automatic = std::max<size_t>(kPlaneBytes / ((size_t)rows * W * sizeof(u64)), 1);
    return (unsigned)std::min<size_t>(h->pairs_per_launch ? h->pairs_per_launch : automatic, total);
}

// What gd_dwell_separations and gd_dwell_pairs share once their arguments stand: the accumulators of R rows, the launches over
// `total` lanes of `rows` grid rows, the copies to the host.  a: base_args with the mode's pointers.
template <bool SEP>
int accumulate(const char *who, gd_dwell *h, Args a, const gd_dwell_rule *rule, const gd_dwell_spec *spec, const gd_dwell_out *out, size_t R, unsigned rows,
               unsigned total)
{
    unsigned const B = spec->n_bins, L = out->hits ? spec->n_lags : 0;
    bool const want_runs = out->runs || out->outside || out->length_sum;
    size_t const n_runs = R * 8 * B, n_side = R * 8, n_hits = R * L, n_acc = n_runs + 2 * n_side + n_hits;
    unsigned const per_launch = lanes_per_launch(h, rows, a.W, total);
    // the separations (set by the caller), the lags and the edges in one table
    std::vector<uint32_t> table(kMaxSeps + kMaxLags + kMaxBins + 1, 0);
    if (SEP) std::copy(a.seps, a.seps + rows, table.begin());
    std::copy(spec->lags, spec->lags + L, table.begin() + kMaxSeps);
    if (B) std::copy(spec->edges, spec->edges + B + 1, table.begin() + kMaxSeps + kMaxLags);
    if (h->acc.ensure(n_acc) != hipSuccess || h->plane.ensure((size_t)rows * a.W * per_launch) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: the outputs of %zu rows and the states of %u pairs x %u frames do not fit on the device", who, R, per_launch, a.K);
    }
    HIPCHK(h->tables.upload(table.data(), table.size()));
    a.seps = h->tables.p;
    a.lags = h->tables.p + kMaxSeps;
    a.edges = h->tables.p + kMaxSeps + kMaxLags;
    a.B = B;
    a.L = L;
    a.plane = h->plane.p;
    a.runs = h->acc.p;
    a.outside = a.runs + n_runs;
    a.lsum = a.outside + n_side;
    a.hits = a.lsum + n_side;
    HIPCHK(hipMemsetAsync(h->acc.p, 0, std::max<size_t>(n_acc, 1) * sizeof(u64), h->stream));
    double ms[3] = {0.0, 0.0, 0.0};
    for (unsigned t0 = 0; t0 < total; t0 += per_launch) {      // total >= 1
        a.t0 = t0;
        a.n = std::min(per_launch, total - t0);
        dim3 const grid(blocks_for(a.n, kBlock), rows);
        HIPCHK(h->timer.mark(0, h->stream));
        launch_states<SEP>(h, grid, a, rule->box != nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(h->timer.mark(1, h->stream));
        if (want_runs) {
            hipLaunchKernelGGL((k_dwell_runs<SEP>), grid, dim3(kBlock), 0, h->stream, a);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(h->timer.mark(2, h->stream));
        if (L) {
            hipLaunchKernelGGL((k_dwell_corr<SEP>), grid, dim3(kBlock), 0, h->stream, a);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(h->done, h->stream));
        HIPCHK(hipEventSynchronize(h->done));      // the events are marked again by the next launch
        double s = 0.0, r = 0.0;
        float c = 0.0f;
        HIPCHK(h->timer.between(0, 1, &s));
        HIPCHK(h->timer.between(1, 2, &r));
        HIPCHK(hipEventElapsedTime(&c, h->timer.ev[2], h->done));
        ms[0] += s;
        ms[1] += r;
        ms[2] += c;
    }
    if (out->runs && n_runs) HIPCHK(hipMemcpyAsync(out->runs, a.runs, n_runs * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    if (out->outside) HIPCHK(hipMemcpyAsync(out->outside, a.outside, n_side * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    if (out->length_sum) HIPCHK(hipMemcpyAsync(out->length_sum, a.lsum, n_side * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    if (out->hits && n_hits) HIPCHK(hipMemcpyAsync(out->hits, a.hits, n_hits * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::copy(ms, ms + 3, h->timer.ms);
    return GD_OK;
}

// the caller's pairs (and rows) checked and on the device
int take_pairs(const char *who, gd_dwell *h, const uint32_t *pairs, uint32_t P, const uint32_t *row, uint32_t R)
{
    if (!pairs) return fail(GD_EINVAL, "%s: NULL pairs", who);
    if (P == 0) return fail(GD_EINVAL, "%s: no pair", who);
    unsigned const N = h->hist.beads();
    for (size_t q = 0; q < P; q++) {
        uint32_t const i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i == j || i >= N || j >= N) return fail(GD_EINVAL, "%s: pair %zu is (%u, %u) (two different beads of %u)", who, q, i, j, N);
        if (row && row[q] >= R) return fail(GD_EINVAL, "%s: pair %zu is of row %u of %u", who, q, row[q], R);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(h->pairs_dev.upload(pairs, 2 * (size_t)P));
    if (row) HIPCHK(h->row_dev.upload(row, P));
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_dwell_abi_version(void) { return GD_DWELL_ABI_VERSION; }

int gd_dwell_create(const gd_dwell_desc *desc, gd_dwell **out)
{
    const char *who = "gd_dwell_create";
    if (int rc = gd::open(who, desc, out)) return rc;
    (*out)->pairs_per_launch = desc->pairs_per_launch;
    hipError_t rc = (*out)->timer.create();
    if (rc == hipSuccess) rc = hipEventCreate(&(*out)->done);
    if (rc != hipSuccess) {
        gd::close(*out);
        *out = nullptr;
        return fail(GD_EHIP, "%s: hipEventCreate failed: %s", who, hipGetErrorString(rc));
    }
    return GD_OK;
}

int gd_dwell_destroy(gd_dwell *h) { return gd::close(h); }

int gd_dwell_set_history(gd_dwell *h, const void *xyz, uint32_t frames, uint32_t n_beads, int is_f64)
{
    const char *who = "gd_dwell_set_history";
    if (!h) return fail(GD_EINVAL, "%s: NULL argument", who);
    return h->hist.set_host(who, h->device, h->stream, xyz, frames, n_beads, is_f64 != 0, rebind(h));
}

int gd_dwell_set_history_live(gd_dwell *h, gd_live_history *history, uint32_t replica)
{
    const char *who = "gd_dwell_set_history_live";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    return h->hist.set_live(who, h->device, h->stream, history, replica, rebind(h));
}

int gd_dwell_set_chains(gd_dwell *h, const uint32_t *ranges, uint32_t n_chains)
{
    const char *who = "gd_dwell_set_chains";
    if (!h || (!ranges && n_chains)) return fail(GD_EINVAL, "%s: NULL argument", who);
    if (!h->hist.frames()) return fail(GD_ESTATE, "%s: no history set (the chains are ranges of its beads)", who);
    if (n_chains > (1u << 28)) return fail(GD_EINVAL, "%s: %u chains exceed 2^28", who, n_chains);
    unsigned const N = h->hist.beads();
    if (n_chains)
        if (int rc = check_ranges(who, "chain", true, ranges, n_chains, N)) return rc;
    HIPCHK(hipSetDevice(h->device));
    return install_chains(h, n_chains ? std::vector<uint32_t>(ranges, ranges + 2 * (size_t)n_chains) : std::vector<uint32_t>{0, N}, n_chains != 0, N);
}

int gd_dwell_separations(gd_dwell *h, const uint32_t *separations, uint32_t n_separations, const gd_dwell_rule *rule, const gd_dwell_spec *spec,
                         const gd_dwell_out *out)
{
    const char *who = "gd_dwell_separations";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames(), N = h->hist.beads();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    if (!separations) return fail(GD_EINVAL, "%s: NULL separations", who);
    if (n_separations < 1 || n_separations > kMaxSeps) return fail(GD_EINVAL, "%s: %u separations, 1 to %u are served at once", who, n_separations, kMaxSeps);
    for (uint32_t m = 0; m < n_separations; m++)
        if (separations[m] < 1) return fail(GD_EINVAL, "%s: separation %u is 0", who, m);
    unsigned K = 0;
    GDCHK(check_rule(who, F, rule, &K));
    GDCHK(check_spec(who, spec, out));
    HIPCHK(hipSetDevice(h->device));
    Args a = base_args(h, rule, K);
    a.chain_end = h->chain_end.p;
    a.seps = separations;      // the host's; accumulate puts them on the device
    GDCHK(accumulate<true>(who, h, a, rule, spec, out, n_separations, n_separations, N));
    if (out->pairs)
        for (uint32_t m = 0; m < n_separations; m++) {
            uint64_t total = 0;
            for (size_t c = 0; c < h->chains.size() / 2; c++) {
                uint64_t const len = h->chains[2 * c + 1] - h->chains[2 * c];
                if (len > separations[m]) total += len - separations[m];
            }
            out->pairs[m] = total;
        }
    return GD_OK;
}

int gd_dwell_pairs(gd_dwell *h, const uint32_t *pairs, uint32_t n_pairs, const uint32_t *row, uint32_t n_rows, const gd_dwell_rule *rule,
                   const gd_dwell_spec *spec, const gd_dwell_out *out)
{
    const char *who = "gd_dwell_pairs";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    unsigned K = 0;
    GDCHK(check_rule(who, F, rule, &K));
    GDCHK(check_spec(who, spec, out));
    GDCHK(take_pairs(who, h, pairs, n_pairs, row, n_rows));
    size_t const R = row ? n_rows : n_pairs;
    Args a = base_args(h, rule, K);
    a.pairs = h->pairs_dev.p;
    a.row = row ? h->row_dev.p : nullptr;
    GDCHK(accumulate<false>(who, h, a, rule, spec, out, R, 1, n_pairs));
    if (out->pairs) {
        std::fill(out->pairs, out->pairs + R, (uint64_t)0);
        for (size_t q = 0; q < n_pairs; q++) out->pairs[row ? row[q] : q]++;
    }
    return GD_OK;
}

int gd_dwell_states(gd_dwell *h, const uint32_t *pairs, uint32_t n_pairs, const gd_dwell_rule *rule, uint8_t *out)
{
    const char *who = "gd_dwell_states";
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    unsigned const F = h->hist.frames();
    if (!F) return fail(GD_ESTATE, "%s: no history set", who);
    if (!out) return fail(GD_EINVAL, "%s: NULL argument", who);
    unsigned K = 0;
    GDCHK(check_rule(who, F, rule, &K));
    GDCHK(take_pairs(who, h, pairs, n_pairs, nullptr, 0));
    Args a = base_args(h, rule, K);
    a.pairs = h->pairs_dev.p;
    unsigned const per_launch = lanes_per_launch(h, 1, a.W, n_pairs);
    if (h->plane.ensure((size_t)a.W * per_launch) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: the states of %u pairs x %u frames do not fit on the device", who, per_launch, K);
    }
    a.plane = h->plane.p;
    std::vector<u64> words((size_t)a.W * per_launch);
    double ms = 0.0;
    for (unsigned t0 = 0; t0 < n_pairs; t0 += per_launch) {
        a.t0 = t0;
        a.n = std::min(per_launch, n_pairs - t0);
        HIPCHK(h->timer.mark(0, h->stream));
        launch_states<false>(h, dim3(blocks_for(a.n, kBlock), 1), a, rule->box != nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(h->timer.mark(1, h->stream));
        HIPCHK(hipMemcpyAsync(words.data(), a.plane, (size_t)a.W * a.n * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        double s = 0.0;
        HIPCHK(h->timer.between(0, 1, &s));
        ms += s;
        for (size_t k = 0; k < K; k++)
            for (unsigned q = 0; q < a.n; q++) out[k * n_pairs + t0 + q] = (uint8_t)((words[(k / 64) * a.n + q] >> (k % 64)) & 1);
    }
    h->timer.ms[0] = ms;
    h->timer.ms[1] = h->timer.ms[2] = 0.0;
    return GD_OK;
}

int gd_dwell_last_times(const gd_dwell *h, double *states_ms, double *runs_ms, double *corr_ms)
{
    if (!h) return fail(GD_EINVAL, "gd_dwell_last_times: NULL handle");
    h->timer.report(states_ms, runs_ms, corr_ms);
    return GD_OK;
}

}  // extern "C"
