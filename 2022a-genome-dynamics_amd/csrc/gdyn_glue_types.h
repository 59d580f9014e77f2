// gdyn_glue_types.h -- what gdyn_capi_glue.hip and gdyn_glue.hip share of the device glue kinetics: the kernels' parameter block, the
// launchers and the sorts.  (A header of its own: gdyn_types.h describes the timed kernels' source.)
#ifndef GDYN_GLUE_TYPES_H
#define GDYN_GLUE_TYPES_H

#include <hip/hip_runtime.h>

#include <cstddef>

// The device glue kinetics (gdyn_glue.hip, include/gdyn_glue.h).  A pair is the word i << 32 | j, i < j.
struct GlueP {
    const float4 *pos; const unsigned *slot_of;        // current positions (slot order), bead id -> slot
    unsigned N, Np, R;
    int periodic;
    float box[3], inv_box[3];
    float dcut2;                                        // the pair search's own bound: bound pairs stay while d2 < dcut2
    unsigned long long thr_off, thr_on, epoch;          // integer thresholds of the two events, the update's number
    const unsigned long long *seeds;                    // [R]
    const unsigned long long *keys; unsigned kstride;   // [R][kstride]: the sets before the update, ascending
    const unsigned *nkeys;                              // [R] their sizes
    unsigned *alive;                                    // [R][kstride]: 1 where the pair survives the unbinding
    unsigned *cnt;                                      // [3R]: survivors, fired pairs, survivors copied by the merge
    const uint2 *cand; unsigned long long cand_cap;     // the search's output: replica r's pairs at cand + r * cand_cap ...
    const unsigned long long *cand_count;               // ... and their number in cand_count[2r]
    unsigned long long *fkey, *fsel; unsigned fstride;  // [R][fstride]: the fired pairs and their selection keys, in any order
    unsigned long long *merged; unsigned mstride;       // [R][mstride]: survivors and newly bound pairs, unsorted
    const unsigned *seg;                                // [4R]: segments of the selection sort (begin, end), of the final sort (begin, end)
};
void gd_launch_glue_unbind(const GlueP &p, unsigned max_keys, hipStream_t st);
void gd_launch_glue_bind(const GlueP &p, unsigned long long max_cand, hipStream_t st);
void gd_launch_glue_merge(const GlueP &p, unsigned max_rows, hipStream_t st);
// rocPRIM's segmented radix sort (tmp == nullptr: only *tmp_bytes is set).  select: the fired records of every segment by (sel, key)
// -- two stable passes, key then sel -- from (fkey, fsel) through (fkey2, fsel2) back into (fkey, fsel).  keys: plain ascending.
hipError_t gd_glue_sort_select(void *tmp, size_t *tmp_bytes, unsigned long long *fkey, unsigned long long *fsel, unsigned long long *fkey2,
                               unsigned long long *fsel2, size_t n, unsigned segments, const unsigned *begin, const unsigned *end,
                               unsigned key_bits, hipStream_t st);
hipError_t gd_glue_sort_keys(void *tmp, size_t *tmp_bytes, const unsigned long long *in, unsigned long long *out, size_t n, unsigned segments,
                             const unsigned *begin, const unsigned *end, unsigned key_bits, hipStream_t st);

#endif
