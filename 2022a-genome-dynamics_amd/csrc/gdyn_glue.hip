// gdyn_glue.hip -- the glue kinetics on the device (include/gdyn_glue.h; the rule: that header and DESIGN.md section 7k).  One
// update of all R replicas of a handle is, behind the pair search (k_pairs) that leaves every replica's candidates on the device:
//   k_glue_unbind   one thread per bound pair: still within reach?  released?  -> an alive flag beside the sorted set
//   k_glue_bind     one thread per candidate: bound and alive (binary search in the sorted set)?  else: fires?  The fired pairs are
//                   appended with their selection keys, one atomic per wave
//   (sort)          only the replicas where more pairs fired than fit: their fired records by (sel, pair), rocPRIM segmented sort
//   k_glue_merge    the survivors and the first `free` fired pairs into one array per replica
//   (sort)          that array by pair: the new set
// Every draw is Philox4x32-10 of (pair, epoch) under the replica's key (gdyn_glue.hpp), so neither the order in which the search
// emits candidates nor the order of the appends reaches the result.  Integer atomics only, on counters.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "gdyn_glue_types.h"
#include "gdyn_glue.hpp"

namespace {

__device__ __forceinline__ unsigned lanes_below(unsigned long long m)      // set bits of m below this lane
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// where this lane's record goes when the lanes of `m` append to a list counted by *counter (whole waves call this)
__device__ __forceinline__ unsigned wave_append(unsigned long long m, unsigned *counter)
{
    unsigned base = 0;
    if ((threadIdx.x & 63u) == 0 && m) base = atomicAdd(counter, (unsigned)__popcll(m));
    return (unsigned)__shfl((int)base, 0, 64) + lanes_below(m);
}

__global__ __launch_bounds__(256) void k_glue_unbind(const GlueP p)
{
    const unsigned r = blockIdx.y, k = blockIdx.x * 256u + threadIdx.x;
    bool alive = false;
    if (k < p.nkeys[r]) {
        const unsigned long long key = p.keys[(size_t)r * p.kstride + k];
        const unsigned i = gd::glue_i(key), j = gd::glue_j(key);
        const float4 xi = p.pos[(size_t)r * p.Np + p.slot_of[(size_t)r * p.N + i]], xj = p.pos[(size_t)r * p.Np + p.slot_of[(size_t)r * p.N + j]];
        float3 d = make_float3(xi.x - xj.x, xi.y - xj.y, xi.z - xj.z);
        if (p.periodic) {      // (k_pairs' minimum image)
            d.x -= p.box[0] * rintf(d.x * p.inv_box[0]);
            d.y -= p.box[1] * rintf(d.y * p.inv_box[1]);
            d.z -= p.box[2] * rintf(d.z * p.inv_box[2]);
        }
        alive = d.x * d.x + d.y * d.y + d.z * d.z < p.dcut2;
        if (alive) alive = !((unsigned long long)gd::glue_draw(i, j, p.epoch, p.seeds[r]).release < p.thr_off);
        p.alive[(size_t)r * p.kstride + k] = alive ? 1u : 0u;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(alive);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&p.cnt[r], (unsigned)__popcll(m));
}

__global__ __launch_bounds__(256) void k_glue_bind(const GlueP p)
{
    const unsigned r = blockIdx.y, nk = p.nkeys[r];
    const unsigned long long n = min(p.cand_count[2u * r], p.cand_cap), nround = (n + 63ull) & ~63ull;      // whole waves take part in the ballot
    const unsigned long long *__restrict__ keys = p.keys + (size_t)r * p.kstride;
    const uint2 *__restrict__ cand = p.cand + (size_t)r * p.cand_cap;
    const unsigned long long seed = p.seeds[r];
    for (unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x; k < nround; k += (unsigned long long)gridDim.x * 256u) {
        bool fire = false;
        unsigned long long key = 0, sel = 0;
        if (k < n) {
            const uint2 q = cand[k];      // (i < j: k_pairs emits a pair from its lower bead)
            key = gd::glue_pack(q.x, q.y);
            unsigned lo = 0, hi = nk;
            while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
            const bool bound = lo < nk && keys[lo] == key && p.alive[(size_t)r * p.kstride + lo] != 0u;
            if (!bound) {
                const gd::GlueDraw w = gd::glue_draw(q.x, q.y, p.epoch, seed);
                fire = (unsigned long long)w.fire < p.thr_on; sel = w.sel;
            }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(fire);
        const unsigned at = wave_append(m, &p.cnt[p.R + r]);
        if (fire && at < p.fstride) { p.fkey[(size_t)r * p.fstride + at] = key; p.fsel[(size_t)r * p.fstride + at] = sel; }
    }
}

__global__ __launch_bounds__(256) void k_glue_merge(const GlueP p)
{
    const unsigned r = blockIdx.y, k = blockIdx.x * 256u + threadIdx.x;
    const unsigned nalive = p.cnt[r], nnew = p.seg[3u * p.R + r] - p.seg[2u * p.R + r], take = nnew - nalive;
    unsigned long long *__restrict__ out = p.merged + (size_t)r * p.mstride;
    const bool keep = k < p.nkeys[r] && p.alive[(size_t)r * p.kstride + k] != 0u;
    const unsigned at = wave_append(__builtin_amdgcn_ballot_w64(keep), &p.cnt[2u * p.R + r]);
    if (keep && at < nalive) out[at] = p.keys[(size_t)r * p.kstride + k];
    if (k < take) out[nalive + k] = p.fkey[(size_t)r * p.fstride + k];
}

}      // namespace

void gd_launch_glue_unbind(const GlueP &p, unsigned max_keys, hipStream_t st)
{
    if (!max_keys) return;
    hipLaunchKernelGGL(k_glue_unbind, dim3((max_keys + 255u) / 256u, p.R), dim3(256), 0, st, p);
}

void gd_launch_glue_bind(const GlueP &p, unsigned long long max_cand, hipStream_t st)
{
    if (!max_cand) return;
    const unsigned nb = (unsigned)std::min<unsigned long long>((max_cand + 255ull) / 256ull, 4096ull);
    hipLaunchKernelGGL(k_glue_bind, dim3(nb, p.R), dim3(256), 0, st, p);
}

void gd_launch_glue_merge(const GlueP &p, unsigned max_rows, hipStream_t st)
{
    if (!max_rows) return;
    hipLaunchKernelGGL(k_glue_merge, dim3((max_rows + 255u) / 256u, p.R), dim3(256), 0, st, p);
}

hipError_t gd_glue_sort_select(void *tmp, size_t *tmp_bytes, unsigned long long *fkey, unsigned long long *fsel, unsigned long long *fkey2,
                               unsigned long long *fsel2, size_t n, unsigned segments, const unsigned *begin, const unsigned *end,
                               unsigned key_bits, hipStream_t st)
{
    if (!tmp) {
        size_t a = 0, b = 0;
        hipError_t e = rocprim::segmented_radix_sort_pairs(nullptr, a, fkey, fkey2, fsel, fsel2, (unsigned)n, segments, begin, end, 0u, key_bits, st);
        if (e != hipSuccess) return e;
        e = rocprim::segmented_radix_sort_pairs(nullptr, b, fsel2, fsel, fkey2, fkey, (unsigned)n, segments, begin, end, 0u, 64u, st);
        *tmp_bytes = std::max(a, b);
        return e;
    }
    // the sort is stable: ordered by pair first, records of equal sel stay in pair order
    hipError_t e = rocprim::segmented_radix_sort_pairs(tmp, *tmp_bytes, fkey, fkey2, fsel, fsel2, (unsigned)n, segments, begin, end, 0u, key_bits, st);
    if (e != hipSuccess) return e;
    return rocprim::segmented_radix_sort_pairs(tmp, *tmp_bytes, fsel2, fsel, fkey2, fkey, (unsigned)n, segments, begin, end, 0u, 64u, st);
}

hipError_t gd_glue_sort_keys(void *tmp, size_t *tmp_bytes, const unsigned long long *in, unsigned long long *out, size_t n, unsigned segments,
                             const unsigned *begin, const unsigned *end, unsigned key_bits, hipStream_t st)
{
    return rocprim::segmented_radix_sort_keys(tmp, *tmp_bytes, in, out, (unsigned)n, segments, begin, end, 0u, key_bits, st);
}
