// gdyn_lagwalk.hpp -- the lag-window walk of k_msd_lag (gdyn_msd.hip) and k_vh_self (gdyn_vanhove.hip), in an anonymous namespace so
// that each translation unit keeps its own object code under its own flags.  The host half, (W, windows), is gd::lag_windows (gdyn_frames.hpp).
//
// A *sequence* is a run of items (3 coordinates each) a fixed stride apart; a *tile* is kSeqs = 16 sequences side by side (LagTile).  A
// block of kLagBlock lanes calls lag_walk for one (tile, range of at most kRange origins) at a time.  The walk stages windows of W items
// in LDS, [item][sequence][3] in the stored type T with one element of padding per item row (kRow): origin windows A and, for each, only
// the partner windows B = A + d W that a requested lag connects (the lags of one d are a range of the sorted lags, found by bisection).
// When the longest sequence fits in one window the partners lie in A and the history is read from HBM once whatever the number of lags.
// The walk places the three barriers (before A is staged, before B is staged, before the body reads); the module's body supplies
//   bool wants(A0, nO)                  block-uniform: whether the origin window [A0, A0 + nO) is to be staged at all
//   void operator()(LagPair, A, Bw)     what is done with the lags [lo, hi) of partner window d; every lane of the block calls
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gd {
namespace {

constexpr int kLagBlock = 1024;              // one block per CU when the window is a whole history: it brings its own four waves per SIMD
constexpr unsigned kSeqs = 16;               // sequences of a tile
constexpr unsigned kSlots = kLagBlock / kSeqs;  // lanes of a sequence: lags (msd) or (lag, origin) pairs (van Hove) side by side
constexpr unsigned kRow = 3 * kSeqs + 1;     // elements of an item row in LDS: odd, so consecutive items start on different banks
constexpr unsigned kRange = 4096;            // origins of one block at a time: fixed, so that nothing depends on the launch

struct LagTile {      // where the sequences of a tile lie
    size_t base;                     // element offset of item 0 of sequence 0
    size_t seq_stride, item_stride;  // in elements
    unsigned valid;                  // sequences of the tile that exist (<= kSeqs)
    unsigned L;                      // items of a sequence
};

struct LagPair {      // one window pair: origins [A0, A0 + nO) of A (nA items staged), partners [A0 + d W, A0 + d W + nB) in Bw
    unsigned lo, hi;                 // the sorted lags of d: in ((d - 1) W, (d + 1) W)
    long long d, W, A0, nO, nA, nB;
};

__device__ inline unsigned lower_bound_dev(const uint32_t *__restrict__ v, unsigned n, unsigned long long key)      // first index with v[i] >= key
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        unsigned const mid = (lo + hi) / 2;
        if (v[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// items [i0, i0 + n) of the tile's sequences into dst ([item][sequence][3]); sequences beyond `valid` read as zeros
template <typename T>
__device__ inline void stage(T *dst, const T *__restrict__ base, size_t seq_stride, size_t item_stride, unsigned valid, size_t i0, unsigned n)
{
    unsigned const total = n * kSeqs * 3;
    if (item_stride >= seq_stride) {      // along time: an item row of the tile is contiguous in memory
        for (unsigned idx = threadIdx.x; idx < total; idx += kLagBlock) {
            unsigned const w = idx / (3 * kSeqs), e = idx % (3 * kSeqs), s = e / 3;
            dst[w * kRow + e] = s < valid ? base[(i0 + w) * item_stride + (size_t)s * seq_stride + e % 3] : T(0);
        }
    } else {      // along the chain: the items of a sequence are contiguous
        for (unsigned idx = threadIdx.x; idx < total; idx += kLagBlock) {
            unsigned const s = idx / (3 * n), e = idx % (3 * n), w = e / 3;
            dst[w * kRow + 3 * s + e % 3] = s < valid ? base[(size_t)s * seq_stride + (i0 + w) * item_stride + e % 3] : T(0);
        }
    }
}

// the window pairs of the origins [O0, O1) of tile t of x, for the ascending `lags`; A and B: W items each (B == A with one window)
template <typename T, typename Body>
__device__ inline void lag_walk(const T *__restrict__ x, const LagTile &t, const uint32_t *__restrict__ lags, unsigned n_lags, long long W, long long O0,
                                long long O1, T *A, T *B, Body &body)
{
    long long const L = t.L;
    for (long long A0 = O0; A0 < O1; A0 += W) {
        long long const nO = min(W, O1 - A0), nA = min(W, L - A0);      // origins; items staged
        if (!body.wants(A0, nO)) continue;
        __syncthreads();      // the last window pair has been read
        stage(A, x + t.base, t.seq_stride, t.item_stride, t.valid, (size_t)A0, (unsigned)nA);
        for (long long d = 0;;) {      // partner windows [A0 + d W, A0 + (d + 1) W): the lags of d lie in ((d - 1) W, (d + 1) W)
            unsigned const lo = d ? lower_bound_dev(lags, n_lags, (unsigned long long)((d - 1) * W + 1)) : 0;
            unsigned const hi = lower_bound_dev(lags, n_lags, (unsigned long long)((d + 1) * W));
            if (lo == hi) {
                if (hi >= n_lags) break;
                d = lags[hi] / W;      // >= d + 1
                continue;
            }
            long long const B0 = A0 + d * W;
            if (B0 >= L) break;
            long long const nB = d ? min(W, L - B0) : nA;
            const T *Bw = A;
            if (d) {
                __syncthreads();      // the last partner window has been read
                stage(B, x + t.base, t.seq_stride, t.item_stride, t.valid, (size_t)B0, (unsigned)nB);
                Bw = B;
            }
            __syncthreads();
            body(LagPair{lo, hi, d, W, A0, nO, nA, nB}, A, Bw);
            d++;
        }
    }
}

}  // namespace
}  // namespace gd
