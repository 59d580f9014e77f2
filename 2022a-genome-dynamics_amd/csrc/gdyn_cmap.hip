// gdyn_cmap.hip -- the contact-map analyses (include/gdyn_cmap.h): the accumulations of the reference's contact_map,
// gw_contact_matrix, nad_profile and power_law over stored (i, j, count) rows, as 32-bit integer sums on the device.
//
//   k_cmap_accumulate  one pass over a batch of rows for every target of the handle.  A lane takes four consecutive rows:
//                      the batch lies on a 16-byte aligned buffer padded to whole lanes, so its 48 bytes are three 16-byte
//                      loads; rows past the batch's end are masked by their index.  Per target kind:
//                        region   global atomic add at [i - beg, j - beg].  Stored rows are ordered by i, then j, so the
//                                 lanes of a wave add along one matrix row at increasing addresses.
//                        binned   only [b_i, b_j] is added here; the transposed add of the reference is made when the
//                                 target is fetched (k_cmap_symmetric_rows: A + A^T), which is the same integer sum, halves
//                                 the atomics and keeps every one of them on the row order of the input.  Runs of equal
//                                 (b_i, b_j) -- the common case for a rebin rate above one -- are summed first inside the
//                                 lane and then across neighbouring lanes of the wave (a segmented scan over the lanes'
//                                 last runs, shuffles only), so a run costs one atomic.
//                        profiles a histogram in LDS per block (the handle's first GD_CMAP_LDS_BINS profile bins, 48 KiB),
//                                 flushed with one global atomic per non-zero bin; profiles beyond that budget use global
//                                 atomics.
//                      Integer adds commute: no result depends on the batch size, the grid or the arrival order.
//   k_cmap_accumulate_tab  the same pass (accumulate_rows) with the slots of a stepper's contact tables as the rows, read in
//                      place (gd_live_contacts, include/gdyn_live.h)
//   k_cmap_symmetrize, k_cmap_max, k_cmap_diagonal   gd_cmap_finish of a region target
//   k_cmap_symmetric_rows                            A + A^T of a binned target for a block of rows, through an LDS tile
// Every index that addresses memory is checked against its array in the kernel: rows are data.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_cmap.h"
#include "gdyn_analysis.hpp"
#include "gdyn_live.hpp"

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr int kPerLane = 4;                   // rows per lane
constexpr int kWave = 64;
constexpr unsigned kMaxBlocks = 2048;         // grid of k_cmap_accumulate: blocks stride over the batch
constexpr unsigned kNoLds = 0xffffffffu;

enum kind : int { kRegion = 0, kBinned = 1, kNucleolus = 2, kSeparation = 3 };

struct target_desc {
    int kind;
    unsigned beg, end;        // region, nucleolus profile
    unsigned n;               // binned: length of the map; profiles: n_particles
    unsigned size;            // side of a matrix, length of a profile
    unsigned lds;             // first LDS bin of a profile, or kNoLds
    int *acc;                 // the accumulator
    const void *aux;          // rebin_map (int32), is_nucleolus (uint8) or chain_id (int32)
};

struct launch_args {
    int n_targets;
    unsigned lds_bins;        // LDS bins in use
    target_desc t[GD_CMAP_MAX_TARGETS];
};

// sums the values of runs of equal keys that continue from one lane into the next.  Every lane of the wave calls it.
//   head, tail   the key of the lane's first and last run
//   single       the lane holds one run only
//   x            the sum of the lane's last run
// Returns what lanes before this one add to its first run; *forward says that the last run continues in the next lane,
// which then carries its sum.
__device__ inline int carry_between_lanes(unsigned long long head, unsigned long long tail, bool single, int x, bool *forward)
{
    unsigned const lane = __lane_id();
    unsigned long long const prev_tail = __shfl_up(tail, 1, kWave);
    bool const link = lane > 0 && head == prev_tail;                 // my first run continues the previous lane's last run
    unsigned long long const links = __ballot(link);
    unsigned long long const stops = __ballot(!(single && link));    // lanes whose last run takes nothing from before
    int s = x;                                                       // inclusive segmented scan of x
    for (unsigned d = 1; d < kWave; d <<= 1) {
        int const t = __shfl_up(s, d, kWave);
        if (lane >= d) {
            unsigned long long const window = (stops >> (lane - d + 1)) & ((1ull << d) - 1ull);
            if (window == 0) s += t;
        }
    }
    int const before = __shfl_up(s, 1, kWave);
    *forward = lane + 1 < kWave && ((links >> (lane + 1)) & 1ull);
    return link ? before : 0;
}

// four rows of one lane through every target.  Every lane of the wave calls it (carry_between_lanes); a row that is not
// live is all zeros.  hist: the block's LDS histogram of the profile targets.
__device__ __forceinline__ void accumulate_rows(launch_args const &a, int *hist, const unsigned (&ri)[kPerLane], const unsigned (&rj)[kPerLane],
                                                const unsigned (&rv)[kPerLane], const bool (&live)[kPerLane], unsigned &requested, unsigned &issued)
{
    for (int ti = 0; ti < a.n_targets; ti++) {
        target_desc const &t = a.t[ti];
        if (t.kind == kRegion) {
#pragma unroll
            for (int k = 0; k < kPerLane; k++)
                if (live[k] && ri[k] >= t.beg && ri[k] < t.end && rj[k] >= t.beg && rj[k] < t.end)
                    atomicAdd(t.acc + (size_t)(ri[k] - t.beg) * t.size + (rj[k] - t.beg), (int)rv[k]);
        } else if (t.kind == kBinned) {
            const int *map = static_cast<const int *>(t.aux);
            unsigned long long key[kPerLane];
            int val[kPerLane];
            bool dead[kPerLane];
#pragma unroll
            for (int k = 0; k < kPerLane; k++) {
                bool const ok = live[k] && ri[k] < t.n && rj[k] < t.n;
                unsigned const bi = ok ? (unsigned)map[ri[k]] : 0u, bj = ok ? (unsigned)map[rj[k]] : 0u;
                bool const in = ok && bi < t.size && bj < t.size;
                key[k] = in ? (unsigned long long)bi * t.size + bj : ~0ull;
                val[k] = in ? (int)rv[k] : 0;
                dead[k] = false;
                requested += in;
            }
#pragma unroll
            for (int k = 0; k + 1 < kPerLane; k++)      // a run's sum ends up in its last row
                if (key[k] == key[k + 1]) {
                    val[k + 1] += val[k];
                    dead[k] = true;
                }
            int const first = dead[0] ? (dead[1] ? (dead[2] ? 3 : 2) : 1) : 0;      // where the lane's first run ends
            bool forward;
            int const carry = carry_between_lanes(key[0], key[kPerLane - 1], first == kPerLane - 1, val[kPerLane - 1], &forward);
#pragma unroll
            for (int k = 0; k < kPerLane; k++) {
                if (dead[k] || key[k] == ~0ull || (k == kPerLane - 1 && forward)) continue;
                atomicAdd(t.acc + key[k], val[k] + (k == first ? carry : 0));
                issued++;
            }
        } else if (t.kind == kNucleolus) {
            const unsigned char *nuc = static_cast<const unsigned char *>(t.aux);
#pragma unroll
            for (int k = 0; k < kPerLane; k++) {
                if (!live[k]) continue;
                bool const i_in = ri[k] >= t.beg && ri[k] < t.end, j_in = rj[k] >= t.beg && rj[k] < t.end;
                bool const i_nuc = ri[k] < t.n && nuc[ri[k]], j_nuc = rj[k] < t.n && nuc[rj[k]];
                if (i_in && j_nuc) {
                    if (t.lds != kNoLds) atomicAdd(&hist[t.lds + (ri[k] - t.beg)], (int)rv[k]);
                    else atomicAdd(t.acc + (ri[k] - t.beg), (int)rv[k]);
                }
                if (j_in && i_nuc) {
                    if (t.lds != kNoLds) atomicAdd(&hist[t.lds + (rj[k] - t.beg)], (int)rv[k]);
                    else atomicAdd(t.acc + (rj[k] - t.beg), (int)rv[k]);
                }
            }
        } else {
            const int *chain = static_cast<const int *>(t.aux);
#pragma unroll
            for (int k = 0; k < kPerLane; k++) {
                if (!live[k] || ri[k] >= t.n || rj[k] >= t.n) continue;
                int const ci = chain[ri[k]], cj = chain[rj[k]];
                unsigned const d = ri[k] > rj[k] ? ri[k] - rj[k] : rj[k] - ri[k];
                if (ci != cj || ci == -1 || d >= t.size) continue;      // d < size was checked when the target was added
                if (t.lds != kNoLds) atomicAdd(&hist[t.lds + d], (int)rv[k]);
                else atomicAdd(t.acc + d, (int)rv[k]);
            }
        }
    }
}

// what a block does before and after its rows: zeroes the LDS histogram and the block's counters / flushes them
__device__ __forceinline__ void block_begin(launch_args const &a, int *hist, unsigned *stat)
{
    for (unsigned b = threadIdx.x; b < a.lds_bins; b += kBlock) hist[b] = 0;
    if (threadIdx.x < 2) stat[threadIdx.x] = 0;
    __syncthreads();
}

__device__ __forceinline__ void block_end(launch_args const &a, const int *hist, unsigned *stat, unsigned requested, unsigned issued,
                                          unsigned long long *counters)
{
    if (requested) atomicAdd(&stat[0], requested);
    if (issued) atomicAdd(&stat[1], issued);
    __syncthreads();
    for (int ti = 0; ti < a.n_targets; ti++) {
        target_desc const &t = a.t[ti];
        if (t.kind < kNucleolus || t.lds == kNoLds) continue;
        for (unsigned b = threadIdx.x; b < t.size; b += kBlock) {
            int const v = hist[t.lds + b];
            if (v) atomicAdd(t.acc + b, v);
        }
    }
    if (threadIdx.x < 2 && stat[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
}

__global__ void __launch_bounds__(kBlock) k_cmap_accumulate(const uint4 *__restrict__ rows, unsigned n_rows, unsigned groups, launch_args a,
                                                           unsigned long long *__restrict__ counters)
{
    extern __shared__ int hist[];
    __shared__ unsigned stat[2];
    block_begin(a, hist, stat);
    unsigned const stride = gridDim.x * kBlock;
    unsigned const padded_groups = (groups + kBlock - 1) / kBlock * kBlock;
    unsigned requested = 0, issued = 0;
    for (unsigned base = blockIdx.x * kBlock; base < padded_groups; base += stride) {      // uniform over the block
        unsigned const g = base + threadIdx.x;
        unsigned ri[kPerLane], rj[kPerLane], rv[kPerLane];
        bool live[kPerLane];
        if (g < groups) {
            uint4 const p = rows[3 * (size_t)g], q = rows[3 * (size_t)g + 1], r = rows[3 * (size_t)g + 2];
            ri[0] = p.x; rj[0] = p.y; rv[0] = p.z;
            ri[1] = p.w; rj[1] = q.x; rv[1] = q.y;
            ri[2] = q.z; rj[2] = q.w; rv[2] = r.x;
            ri[3] = r.y; rj[3] = r.z; rv[3] = r.w;
        }
#pragma unroll
        for (int k = 0; k < kPerLane; k++) {
            live[k] = g < groups && g * kPerLane + k < n_rows;
            if (!live[k]) ri[k] = rj[k] = rv[k] = 0;
        }
        accumulate_rows(a, hist, ri, rj, rv, live, requested, issued);
    }
    block_end(a, hist, stat, requested, issued, counters);
}

// The same pass over the words of the stepper's contact tables (gdyn_types.h, ContactTab) in place: a lane takes four consecutive
// slots of replica r0 + blockIdx.y (the capacity is a power of two >= 1024 and the tables are 16-byte aligned: two 16-byte
// loads), an empty slot is a row that is not live.  Slots come in hash order: equal binned keys seldom meet, and where they do
// carry_between_lanes combines them as it does for sorted rows (it compares neighbours only and never assumes an order).
__global__ void __launch_bounds__(kBlock) k_cmap_accumulate_tab(const unsigned long long *__restrict__ words, unsigned long long cap, unsigned jbits,
                                                               unsigned r0, launch_args a, unsigned long long *__restrict__ counters)
{
    extern __shared__ int hist[];
    __shared__ unsigned stat[2];
    block_begin(a, hist, stat);
    const ulonglong2 *slots = reinterpret_cast<const ulonglong2 *>(words + (size_t)(r0 + blockIdx.y) * cap);
    unsigned long long const groups = cap / kPerLane, stride = (unsigned long long)gridDim.x * kBlock;
    unsigned const cbits = 64u - 2u * jbits;
    unsigned long long const jmask = (1ull << jbits) - 1ull, cmask = (1ull << cbits) - 1ull;
    unsigned requested = 0, issued = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kBlock; base < groups; base += stride) {      // uniform over the block
        unsigned long long const g = base + threadIdx.x;
        unsigned long long w[kPerLane] = {GD_CT_EMPTY, GD_CT_EMPTY, GD_CT_EMPTY, GD_CT_EMPTY};
        if (g < groups) {
            ulonglong2 const p = slots[2 * g], q = slots[2 * g + 1];
            w[0] = p.x; w[1] = p.y; w[2] = q.x; w[3] = q.y;
        }
        unsigned ri[kPerLane], rj[kPerLane], rv[kPerLane];
        bool live[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; k++) {
            live[k] = w[k] != GD_CT_EMPTY;
            unsigned long long const key = w[k] >> cbits;
            ri[k] = live[k] ? (unsigned)(key >> jbits) : 0u;
            rj[k] = live[k] ? (unsigned)(key & jmask) : 0u;
            rv[k] = live[k] ? (unsigned)(w[k] & cmask) : 0u;
        }
        accumulate_rows(a, hist, ri, rj, rv, live, requested, issued);
    }
    block_end(a, hist, stat, requested, issued, counters);
}

// M <- M + M^T: the thread of (r, c), c >= r, writes both cells
__global__ void __launch_bounds__(kBlock) k_cmap_symmetrize(int *__restrict__ m, unsigned n)
{
    unsigned const c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (c >= n || c < r) return;
    int const s = m[(size_t)r * n + c] + m[(size_t)c * n + r];
    m[(size_t)r * n + c] = s;
    m[(size_t)c * n + r] = s;
}

__global__ void __launch_bounds__(kBlock) k_cmap_max(const int *__restrict__ m, size_t count, int *__restrict__ out)
{
    int best = INT_MIN;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (size_t)gridDim.x * kBlock) best = max(best, m[k]);
    for (int d = kWave / 2; d > 0; d >>= 1) best = max(best, __shfl_xor(best, d, kWave));
    if (__lane_id() == 0) atomicMax(out, best);
}

__global__ void __launch_bounds__(kBlock) k_cmap_diagonal(int *__restrict__ m, unsigned n, const int *__restrict__ value)
{
    unsigned const r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) m[(size_t)r * n + r] = *value;
}

// out[(r - r0), c] = A[r, c] + A[c, r] for rows r0 .. r0 + rows - 1; grid (ceil(n / 32), ceil(rows / 32)), block (32, 8)
__global__ void __launch_bounds__(kBlock) k_cmap_symmetric_rows(const int *__restrict__ a, unsigned n, unsigned r0, unsigned rows, int *__restrict__ out)
{
    __shared__ int tile[32][33];
    unsigned const c0 = blockIdx.x * 32, rb = r0 + blockIdx.y * 32;
    for (unsigned q = threadIdx.y; q < 32; q += 8) {      // tile[q][x] = A[c0 + q, rb + x]
        unsigned const rr = c0 + q, cc = rb + threadIdx.x;
        tile[q][threadIdx.x] = rr < n && cc < n ? a[(size_t)rr * n + cc] : 0;
    }
    __syncthreads();
    for (unsigned q = threadIdx.y; q < 32; q += 8) {
        unsigned const r = rb + q, c = c0 + threadIdx.x;
        if (r < r0 + rows && r < n && c < n) out[(size_t)(r - r0) * n + c] = a[(size_t)r * n + c] + tile[threadIdx.x][q];
    }
}

constexpr size_t kAutoRows = (size_t)1 << 22;          // rows per launch when max_rows_per_launch is 0 (48 MiB)
constexpr size_t kMaxRows = (size_t)1 << 28;           // row indices of a batch stay 32-bit
constexpr size_t kFetchElements = (size_t)1 << 26;     // staging of a binned fetch (256 MiB)

struct target_state {
    target_desc d{};           // what the kernels see: plain pointers into acc and aux
    size_t count = 0;          // accumulator elements
    dbuf<int> acc;
    dbuf<char> aux;
};

}  // namespace

struct gd_cmap : gd::handle {
    unsigned max_rows = 0;
    dbuf<char> rows;                   // one batch, padded
    dbuf<int> stage;                   // binned fetch
    dbuf<unsigned long long> counters; // [2], then one int for gd_cmap_finish's maximum
    std::vector<target_state> targets;
    unsigned lds_bins = 0;

    void drop_targets()
    {
        targets.clear();
        lds_bins = 0;
    }
};

namespace {

// a zeroed accumulator of `count` int32 and a device copy of the target's array; nothing is left behind on failure
int new_target(gd_cmap *h, const char *who, target_desc d, size_t count, const void *aux, size_t aux_bytes, int32_t *out)
{
    if (h->targets.size() >= GD_CMAP_MAX_TARGETS) return fail(GD_EINVAL, "%s: a handle holds at most %d targets", who, GD_CMAP_MAX_TARGETS);
    HIPCHK(hipSetDevice(h->device));
    target_state t;
    t.count = count;
    if (t.acc.ensure(std::max<size_t>(count, 1)) != hipSuccess) {      // an empty target keeps one cell, which zero() and reset clear
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: no device memory for %zu accumulator cells", who, count);
    }
    if (t.aux.ensure(aux_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GD_ENOMEM, "%s: no device memory for %zu bytes", who, aux_bytes);
    }
    hipError_t e = aux_bytes ? hipMemcpy(t.aux.p, aux, aux_bytes, hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) return fail(GD_EHIP, "%s: hipMemcpy failed: %s", who, hipGetErrorString(e));
    e = t.acc.zero(h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(GD_EHIP, "%s: hipMemset failed: %s", who, hipGetErrorString(e));
    d.acc = t.acc.p;
    d.aux = t.aux.p;
    d.lds = kNoLds;
    if (d.kind >= kNucleolus && h->lds_bins + d.size <= GD_CMAP_LDS_BINS) {
        d.lds = h->lds_bins;
        h->lds_bins += d.size;
    }
    t.d = d;
    h->targets.push_back(std::move(t));
    *out = (int32_t)h->targets.size() - 1;
    return GD_OK;
}

int find(gd_cmap *h, const char *who, int32_t target, target_state **out)
{
    if (!h) return fail(GD_EINVAL, "%s: NULL handle", who);
    if (target < 0 || (size_t)target >= h->targets.size()) return fail(GD_EINVAL, "%s: target %d of %zu", who, target, h->targets.size());
    *out = &h->targets[(size_t)target];
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_cmap_abi_version(void) { return GD_CMAP_ABI_VERSION; }

int gd_cmap_create(const gd_cmap_desc *desc, gd_cmap **out)
{
    if (int rc = gd::open("gd_cmap_create", desc, out)) return rc;
    gd_cmap *h = *out;
    h->max_rows = desc->max_rows_per_launch;
    hipError_t e = h->counters.ensure(4);
    if (e == hipSuccess) e = hipMemset(h->counters.p, 0, 4 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        gd::close(h);
        *out = nullptr;
        return fail(GD_EHIP, "gd_cmap_create failed: %s", hipGetErrorString(e));
    }
    return GD_OK;
}

int gd_cmap_destroy(gd_cmap *h) { return gd::close(h); }

int gd_cmap_add_region(gd_cmap *h, uint32_t beg, uint32_t end, int32_t *target)
{
    if (!h || !target) return fail(GD_EINVAL, "gd_cmap_add_region: NULL argument");
    if (end < beg || end - beg > GD_CMAP_MAX_SIDE) return fail(GD_EINVAL, "gd_cmap_add_region: range [%u, %u) is reversed or wider than %d", beg, end, GD_CMAP_MAX_SIDE);
    target_desc d{};
    d.kind = kRegion;
    d.beg = beg;
    d.end = end;
    d.size = end - beg;
    return new_target(h, "gd_cmap_add_region", d, (size_t)d.size * d.size, nullptr, 0, target);
}

int gd_cmap_add_binned(gd_cmap *h, const int32_t *rebin_map, uint32_t n, uint32_t n_bins, int32_t *target)
{
    if (!h || !target || (n && !rebin_map)) return fail(GD_EINVAL, "gd_cmap_add_binned: NULL argument");
    if (n_bins > GD_CMAP_MAX_SIDE) return fail(GD_EINVAL, "gd_cmap_add_binned: %u bins exceed %d", n_bins, GD_CMAP_MAX_SIDE);
    for (uint32_t k = 0; k < n; k++)
        if (rebin_map[k] < 0 || (uint32_t)rebin_map[k] >= n_bins)
            return fail(GD_EINVAL, "gd_cmap_add_binned: rebin_map[%u] = %d is outside [0, %u)", k, rebin_map[k], n_bins);
    target_desc d{};
    d.kind = kBinned;
    d.n = n;
    d.size = n_bins;
    return new_target(h, "gd_cmap_add_binned", d, (size_t)n_bins * n_bins, rebin_map, (size_t)n * sizeof(int32_t), target);
}

int gd_cmap_add_nucleolus_profile(gd_cmap *h, uint32_t beg, uint32_t end, const uint8_t *is_nucleolus, uint32_t n_particles, int32_t *target)
{
    if (!h || !target || (n_particles && !is_nucleolus)) return fail(GD_EINVAL, "gd_cmap_add_nucleolus_profile: NULL argument");
    if (end < beg) return fail(GD_EINVAL, "gd_cmap_add_nucleolus_profile: range [%u, %u) is reversed", beg, end);
    target_desc d{};
    d.kind = kNucleolus;
    d.beg = beg;
    d.end = end;
    d.n = n_particles;
    d.size = end - beg;
    return new_target(h, "gd_cmap_add_nucleolus_profile", d, d.size, is_nucleolus, n_particles, target);
}

int gd_cmap_add_separation_profile(gd_cmap *h, const int32_t *chain_id, uint32_t n_particles, uint32_t size, int32_t *target)
{
    if (!h || !target || (n_particles && !chain_id)) return fail(GD_EINVAL, "gd_cmap_add_separation_profile: NULL argument");
    std::unordered_map<int32_t, std::pair<uint32_t, uint32_t>> extent;      // first and last bead of every chain
    for (uint32_t k = 0; k < n_particles; k++) {
        if (chain_id[k] == -1) continue;
        auto it = extent.find(chain_id[k]);
        if (it == extent.end()) extent.emplace(chain_id[k], std::make_pair(k, k));
        else it->second.second = k;
    }
    for (auto const &e : extent)
        if (e.second.second - e.second.first >= size)
            return fail(GD_EINVAL, "gd_cmap_add_separation_profile: chain %d spans beads %u to %u, a separation beyond the profile's %u bins", e.first,
                        e.second.first, e.second.second, size);
    target_desc d{};
    d.kind = kSeparation;
    d.n = n_particles;
    d.size = size;
    return new_target(h, "gd_cmap_add_separation_profile", d, size, chain_id, (size_t)n_particles * sizeof(int32_t), target);
}

int gd_cmap_accumulate(gd_cmap *h, const uint32_t *rows, uint64_t n_rows)
{
    if (!h) return fail(GD_EINVAL, "gd_cmap_accumulate: NULL handle");
    if (n_rows == 0) return GD_OK;
    if (!rows) return fail(GD_EINVAL, "gd_cmap_accumulate: NULL rows");
    if (h->targets.empty()) return fail(GD_ESTATE, "gd_cmap_accumulate: the handle has no target");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    size_t const B = (size_t)std::min<uint64_t>(std::min<size_t>(h->max_rows ? h->max_rows : kAutoRows, kMaxRows), n_rows);
    size_t const capacity = (B + kPerLane - 1) / kPerLane * kPerLane;
    HIPCHK(h->rows.ensure(capacity * 12));
    launch_args a{};
    a.n_targets = (int)h->targets.size();
    a.lds_bins = h->lds_bins;
    for (int k = 0; k < a.n_targets; k++) a.t[k] = h->targets[(size_t)k].d;
    for (uint64_t r0 = 0; r0 < n_rows; r0 += B) {
        unsigned const b = (unsigned)std::min<uint64_t>(B, n_rows - r0);
        unsigned const groups = (b + kPerLane - 1) / kPerLane;
        HIPCHK(hipMemcpyAsync(h->rows.p, rows + r0 * 3, (size_t)b * 12, hipMemcpyHostToDevice, st));
        unsigned const blocks = std::min((groups + kBlock - 1) / kBlock, kMaxBlocks);
        hipLaunchKernelGGL(k_cmap_accumulate, dim3(blocks), dim3(kBlock), h->lds_bins * sizeof(int), st, (const uint4 *)h->rows.p, b, groups, a, h->counters.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    return GD_OK;
}

int gd_cmap_finish(gd_cmap *h, int32_t target)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_cmap_finish", target, &t)) return rc;
    if (t->d.kind != kRegion) return fail(GD_EINVAL, "gd_cmap_finish: target %d is not a region", target);
    unsigned const n = t->d.size;
    if (n == 0) return GD_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int *best = reinterpret_cast<int *>(h->counters.p + 2);
    int const lowest = INT_MIN;
    HIPCHK(hipMemcpyAsync(best, &lowest, sizeof lowest, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_cmap_symmetrize, dim3((n + kBlock - 1) / kBlock, n), dim3(kBlock), 0, st, t->d.acc, n);
    hipLaunchKernelGGL(k_cmap_max, dim3((unsigned)std::min<size_t>((t->count + kBlock - 1) / kBlock, kMaxBlocks)), dim3(kBlock), 0, st, t->d.acc, t->count, best);
    hipLaunchKernelGGL(k_cmap_diagonal, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, t->d.acc, n, best);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return GD_OK;
}

int gd_cmap_target_size(gd_cmap *h, int32_t target, uint64_t *count)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_cmap_target_size", target, &t)) return rc;
    if (!count) return fail(GD_EINVAL, "gd_cmap_target_size: NULL argument");
    *count = t->count;
    return GD_OK;
}

int gd_cmap_fetch(gd_cmap *h, int32_t target, int32_t *out)
{
    target_state *t = nullptr;
    if (int rc = find(h, "gd_cmap_fetch", target, &t)) return rc;
    if (t->count == 0) return GD_OK;
    if (!out) return fail(GD_EINVAL, "gd_cmap_fetch: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (t->d.kind != kBinned) {
        HIPCHK(hipMemcpyAsync(out, t->d.acc, t->count * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return GD_OK;
    }
    unsigned const n = t->d.size;
    unsigned const piece = (unsigned)std::min<size_t>(n, std::max<size_t>(32, kFetchElements / n / 32 * 32));      // rows at a time
    HIPCHK(h->stage.ensure((size_t)piece * n));
    for (unsigned r0 = 0; r0 < n; r0 += piece) {
        unsigned const rows = std::min(piece, n - r0);
        hipLaunchKernelGGL(k_cmap_symmetric_rows, dim3((n + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, st, (const int *)t->d.acc, n, r0, rows, h->stage.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + (size_t)r0 * n, h->stage.p, (size_t)rows * n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return GD_OK;
}

int gd_cmap_reset(gd_cmap *h)
{
    if (!h) return fail(GD_EINVAL, "gd_cmap_reset: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    for (auto &t : h->targets) HIPCHK(t.acc.zero(h->stream));
    HIPCHK(hipMemsetAsync(h->counters.p, 0, 2 * sizeof(unsigned long long), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_cmap_clear(gd_cmap *h)
{
    if (!h) return fail(GD_EINVAL, "gd_cmap_clear: NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->drop_targets();
    return GD_OK;
}

int gd_cmap_counters(gd_cmap *h, uint64_t out[2])
{
    if (!h || !out) return fail(GD_EINVAL, "gd_cmap_counters: NULL argument");
    HIPCHK(hipSetDevice(h->device));
    unsigned long long v[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(v, h->counters.p, sizeof v, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    out[0] = v[0];
    out[1] = v[1];
    return GD_OK;
}

}  // extern "C"

// ---- the live seam (gdyn_live.hpp)

int gd_cmap_device(const gd_cmap *h) { return h->device; }

int gd_cmap_accumulate_tab(gd_cmap *h, const char *who, const ContactTab &tab, uint32_t r0, uint32_t nr, uint64_t rows)
{
    if (rows == 0 || nr == 0) return GD_OK;                  // as gd_cmap_accumulate: no rows, nothing asked of the handle
    if (h->targets.empty()) return fail(GD_ESTATE, "%s: the handle has no target", who);
    HIPCHK(hipSetDevice(h->device));
    launch_args a{};
    a.n_targets = (int)h->targets.size();
    a.lds_bins = h->lds_bins;
    for (int k = 0; k < a.n_targets; k++) a.t[k] = h->targets[(size_t)k].d;
    // the kernel's loop is uniform over a block only for whole blocks of lanes (the tables' capacity is a power of two >= 1024)
    if (tab.cap == 0 || tab.cap % (kPerLane * kBlock)) return fail(GD_ESTATE, "%s: a table of %llu slots", who, tab.cap);
    unsigned const blocks = (unsigned)std::min<unsigned long long>(tab.cap / kPerLane / kBlock, kMaxBlocks);
    for (uint32_t y0 = 0; y0 < nr; y0 += 65535u) {           // the replica is the grid's y
        hipLaunchKernelGGL(k_cmap_accumulate_tab, dim3(blocks, std::min(nr - y0, 65535u)), dim3(kBlock), h->lds_bins * sizeof(int), h->stream,
                           tab.words, tab.cap, tab.jbits, r0 + y0, a, h->counters.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return GD_OK;
}
