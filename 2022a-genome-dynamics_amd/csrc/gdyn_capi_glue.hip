// gdyn_capi_glue.hip -- glue kinetics on the device (include/gdyn_glue.h): the host side over the kernels of gdyn_glue.hip.
// The rule is in the header and in DESIGN.md section 7k.  The host keeps a copy of every set (at most max_glues words a replica): it
// is what the managed slot is fed from, through the per-replica lists' own flattener.  Of the stepper (gdyn_capi.hip) it calls
// prepare and search_device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "gdyn_system.hpp"
#include "gdyn_glue.hpp"
#include "gdyn_glue_types.h"

extern "C" int gd_glue_abi_version(void) { return GD_GLUE_ABI_VERSION; }

// a replica's set into the managed slot, as gd_replica_pairs_set would install it
static void glue_install(gd_system *s, uint32_t r)
{
    const std::vector<uint64_t> &keys = s->gl.sets[r];
    std::vector<uint32_t> pairs(2 * keys.size());
    for (size_t k = 0; k < keys.size(); k++) { pairs[2 * k] = gd::glue_i(keys[k]); pairs[2 * k + 1] = gd::glue_j(keys[k]); }
    (void)s->rp.set(s->gl.slot, r, pairs.data(), (uint32_t)keys.size());      // (ids and i != j were checked when the set was made)
}

// the small pinned block: [R] seeds (64-bit), then 32-bit words: [R] set sizes, [4R] segments, [3R] counters
static unsigned *glue_small_words(gd_system *s) { return (unsigned *)(s->gl.small.p + s->R); }

extern "C" int gd_glue_define(gd_system *s, uint32_t slot, const gd_glue_params *p)
{
    if (!s || !p) return fail(GD_EINVAL, "gd_glue_define: NULL argument");
    gd::Glue &gl = s->gl;
    if (slot >= gd::RP_SLOTS) return fail(GD_EINVAL, "gd_glue_define: slot %u out of range", slot);
    if (!s->rp.defined(slot)) return fail(GD_ESTATE, "gd_glue_define: slot %u was never defined (gd_replica_pairs_define)", slot);
    if (gl.defined && slot != gl.slot) return fail(GD_ESTATE, "gd_glue_define: slot %u already holds the handle's glues (one glue slot per handle)", gl.slot);
    if (const char *bad = gd::glue_check_params(p->reach, p->binding_rate, p->unbinding_rate)) return fail(GD_EINVAL, "gd_glue_define: %s", bad);
    if (gl.defined)
        for (uint32_t r = 0; r < s->R; r++)
            if (gl.sets[r].size() > p->max_glues)
                return fail(GD_EINVAL, "gd_glue_define: max_glues %u is below the %zu pairs replica %u holds", p->max_glues, gl.sets[r].size(), r);
    if (!gl.defined) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(gl.small.ensure(5 * (size_t)s->R));      // (R 64-bit words and 8 R 32-bit words)
        HIPCHK(gl.seeds.resize(s->R, false)); HIPCHK(gl.nkeys.resize(s->R)); HIPCHK(gl.cnt.resize(3 * (size_t)s->R));
        HIPCHK(gl.seg.resize(4 * (size_t)s->R));
        gl.sets.assign(s->R, {});
        gl.slot = slot; gl.defined = true; gl.dev_dirty = true;
        for (uint32_t r = 0; r < s->R; r++) glue_install(s, r);      // (the slot holds the sets from here on: empty)
    }
    gl.par = *p;
    return GD_OK;
}

extern "C" int gd_glue_set(gd_system *s, uint32_t replica, const uint32_t *pairs, uint32_t n)
{
    if (!s || (n && !pairs)) return fail(GD_EINVAL, "gd_glue_set: NULL argument");
    if (!s->gl.defined) return fail(GD_ESTATE, "gd_glue_set: no glue slot (gd_glue_define)");
    if (replica >= s->R) return fail(GD_EINVAL, "gd_glue_set: replica %u out of range", replica);
    if (const char *bad = gd::glue_normalise(pairs, n, s->N, s->gl.par.max_glues, s->gl.sets[replica])) return fail(GD_EINVAL, "gd_glue_set: %s", bad);
    glue_install(s, replica);
    s->gl.dev_dirty = true;
    return GD_OK;
}

extern "C" int gd_glue_fetch(gd_system *s, uint32_t replica, uint32_t *pairs, uint32_t cap, uint32_t *n)
{
    if (!s || !n || (cap && !pairs)) return fail(GD_EINVAL, "gd_glue_fetch: NULL argument");
    if (!s->gl.defined) return fail(GD_ESTATE, "gd_glue_fetch: no glue slot (gd_glue_define)");
    if (replica >= s->R) return fail(GD_EINVAL, "gd_glue_fetch: replica %u out of range", replica);
    const std::vector<uint64_t> &keys = s->gl.sets[replica];
    for (size_t k = 0; k < keys.size() && k < cap; k++) { pairs[2 * k] = gd::glue_i(keys[k]); pairs[2 * k + 1] = gd::glue_j(keys[k]); }
    *n = (uint32_t)keys.size();
    return GD_OK;
}

extern "C" int gd_glue_counts(gd_system *s, uint32_t *n)
{
    if (!s || !n) return fail(GD_EINVAL, "gd_glue_counts: NULL argument");
    if (!s->gl.defined) return fail(GD_ESTATE, "gd_glue_counts: no glue slot (gd_glue_define)");
    for (uint32_t r = 0; r < s->R; r++) n[r] = (uint32_t)s->gl.sets[r].size();
    return GD_OK;
}

// the host's sets onto the device (after gd_glue_define and gd_glue_set; an update leaves its result there itself)
static int glue_upload(gd_system *s)
{
    gd::Glue &gl = s->gl;
    if (!gl.dev_dirty) return GD_OK;
    size_t most = 1;
    for (auto &k : gl.sets) most = std::max(most, k.size());
    const int c = gl.cur;
    const size_t stride = gd::grown_capacity(gl.kstride[c], most);
    if ((size_t)s->R * stride > 0xffffffffull) return fail(GD_ENOMEM, "gd_glue_update: %zu pairs a replica exceed the sort's 32-bit offsets", stride);
    HIPCHK(gl.keys[c].resize((size_t)s->R * stride, false));
    gl.kstride[c] = stride;
    HIPCHK(gl.pin.ensure(gd::grown_capacity(gl.pin.n, (size_t)s->R * most)));
    unsigned *nk = glue_small_words(s);
    for (uint32_t r = 0; r < s->R; r++) {
        std::copy(gl.sets[r].begin(), gl.sets[r].end(), gl.pin.p + (size_t)r * most);
        nk[r] = (unsigned)gl.sets[r].size();
    }
    HIPCHK(hipMemcpy2DAsync(gl.keys[c].p, stride * sizeof(unsigned long long), gl.pin.p, most * sizeof(unsigned long long),
                            most * sizeof(unsigned long long), s->R, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(gl.nkeys.p, nk, s->R * sizeof(unsigned), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    gl.dev_dirty = false;
    return GD_OK;
}

extern "C" int gd_glue_update(gd_system *s, double dt, uint64_t epoch, const uint64_t *seeds)
{
    if (!s || !seeds) return fail(GD_EINVAL, "gd_glue_update: NULL argument");
    if (!s->gl.defined) return fail(GD_ESTATE, "gd_glue_update: no glue slot (gd_glue_define)");
    if (!(dt > 0) || !std::isfinite(dt)) return fail(GD_EINVAL, "gd_glue_update: dt must be positive and finite");
    HIPCHK(hipSetDevice(s->device));
    const uint32_t R = s->R;
    gd::Glue &gl = s->gl;
    const gd_glue_params &par = gl.par;
    GDCHK(prepare(s));
    GDCHK(glue_upload(s));
    std::vector<unsigned long long> ccnt;
    GDCHK(search_device(s, 0, R, par.reach, gl.cand, gl.cand_count, ccnt));
    unsigned long long most_c = 0;
    size_t most_k = 0;
    for (uint32_t r = 0; r < R; r++) { most_c = std::max(most_c, ccnt[2 * r]); most_k = std::max(most_k, gl.sets[r].size()); }
    const int c = gl.cur, o = c ^ 1;
    if (gl.alive.n < gl.keys[c].n) HIPCHK(gl.alive.resize(gl.keys[c].n, false));

    GlueP q;
    memset(&q, 0, sizeof q);
    q.pos = s->pos[s->pcur].p; q.slot_of = s->slot_of.p; q.N = s->N; q.Np = s->Np; q.R = R;
    set_box(s, q);
    q.dcut2 = (float)(par.reach * par.reach);      // (search_device's own bound)
    q.thr_off = gd::glue_rate_threshold(par.unbinding_rate, dt); q.thr_on = gd::glue_rate_threshold(par.binding_rate, dt); q.epoch = epoch;
    q.seeds = gl.seeds.p; q.keys = gl.keys[c].p; q.kstride = (unsigned)gl.kstride[c]; q.nkeys = gl.nkeys.p;
    q.alive = gl.alive.p; q.cnt = gl.cnt.p; q.cand = gl.cand.p; q.cand_cap = gl.cand.n / R; q.cand_count = gl.cand_count.p;
    q.seg = gl.seg.p;

    unsigned *small = glue_small_words(s), *h_nk = small, *h_seg = small + R, *h_cnt = small + 5 * (size_t)R;
    std::copy(seeds, seeds + R, gl.small.p);
    HIPCHK(hipMemcpyAsync(gl.seeds.p, gl.small.p, R * sizeof(unsigned long long), hipMemcpyHostToDevice, s->stream));

    // unbind and bind; the fired records' buffer is sized like the search's output: grown until every replica fits (the draws are
    // counter-based: a second pass fires the same pairs)
    {
        const double p_on = -std::expm1(-par.binding_rate * dt);
        const size_t want = (size_t)std::min<double>((double)most_c, (double)most_c * p_on * 1.25 + 1024.0);
        if (want > gl.fstride) gl.fstride = gd::grown_capacity(gl.fstride, want);
    }
    for (int attempt = 0;; attempt++) {
        if (attempt == 4) return fail(GD_ESTATE, "gd_glue_update: the fired pairs' buffer did not converge");
        const size_t fs = std::max<size_t>(gl.fstride, 1);
        if ((size_t)R * fs > 0xffffffffull) return fail(GD_ENOMEM, "gd_glue_update: %zu fired pairs a replica exceed the sort's 32-bit offsets", fs);
        if (gl.fkey[0].n != (size_t)R * fs)
            for (int k = 0; k < 2; k++) { HIPCHK(gl.fkey[k].resize((size_t)R * fs, false)); HIPCHK(gl.fsel[k].resize((size_t)R * fs, false)); }
        gl.fstride = fs;
        q.fkey = gl.fkey[0].p; q.fsel = gl.fsel[0].p; q.fstride = (unsigned)fs;
        HIPCHK(hipMemsetAsync(gl.cnt.p, 0, 3 * (size_t)R * sizeof(unsigned), s->stream));
        gd_launch_glue_unbind(q, (unsigned)most_k, s->stream);
        gd_launch_glue_bind(q, most_c, s->stream);
        HIPCHK(hipMemcpyAsync(h_cnt, gl.cnt.p, 2 * (size_t)R * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipGetLastError());
        unsigned most_f = 0;
        for (uint32_t r = 0; r < R; r++) most_f = std::max(most_f, h_cnt[R + r]);
        if (most_f <= fs) break;
        gl.fstride = (size_t)most_f + most_f / 8 + 64;
    }

    // who binds: everything that fired where it fits, else the smallest selection keys
    size_t most_new = 0, most_rows = most_k;
    bool select = false;
    for (uint32_t r = 0; r < R; r++) {
        const size_t alive = h_cnt[r], fired = h_cnt[R + r], free_r = par.max_glues > alive ? par.max_glues - alive : 0;
        const size_t take = std::min(fired, free_r);
        h_seg[r] = (unsigned)(r * gl.fstride); h_seg[R + r] = h_seg[r] + (fired > free_r ? (unsigned)fired : 0u);
        select = select || fired > free_r;
        h_nk[r] = (unsigned)(alive + take);
        most_new = std::max<size_t>(most_new, h_nk[r]); most_rows = std::max(most_rows, take);
    }
    const size_t ms = gd::grown_capacity(gl.kstride[o], std::max<size_t>(most_new, 1));
    if ((size_t)R * ms > 0xffffffffull) return fail(GD_ENOMEM, "gd_glue_update: %zu pairs a replica exceed the sort's 32-bit offsets", ms);
    HIPCHK(gl.keys[o].resize((size_t)R * ms, false)); HIPCHK(gl.merged.resize((size_t)R * ms, false));
    for (uint32_t r = 0; r < R; r++) { h_seg[2 * R + r] = (unsigned)(r * ms); h_seg[3 * R + r] = h_seg[2 * R + r] + h_nk[r]; }
    q.merged = gl.merged.p; q.mstride = (unsigned)ms;
    HIPCHK(hipMemcpyAsync(gl.seg.p, h_seg, 4 * (size_t)R * sizeof(unsigned), hipMemcpyHostToDevice, s->stream));
    const unsigned key_bits = 32u + contact_jbits(s);
    if (most_new) {
        size_t tmp_sel = 0, tmp_keys = 0;
        if (select) HIPCHK(gd_glue_sort_select(nullptr, &tmp_sel, gl.fkey[0].p, gl.fsel[0].p, gl.fkey[1].p, gl.fsel[1].p, gl.fkey[0].n, R,
                                               gl.seg.p, gl.seg.p + R, key_bits, s->stream));
        HIPCHK(gd_glue_sort_keys(nullptr, &tmp_keys, gl.merged.p, gl.keys[o].p, gl.merged.n, R, gl.seg.p + 2 * R, gl.seg.p + 3 * R, key_bits, s->stream));
        size_t tmp_bytes = std::max<size_t>(std::max(tmp_sel, tmp_keys), 1);
        if (tmp_bytes > gl.tmp.n) HIPCHK(gl.tmp.resize(tmp_bytes, false));
        if (select) {
            tmp_bytes = gl.tmp.n;
            HIPCHK(gd_glue_sort_select(gl.tmp.p, &tmp_bytes, gl.fkey[0].p, gl.fsel[0].p, gl.fkey[1].p, gl.fsel[1].p, gl.fkey[0].n, R,
                                       gl.seg.p, gl.seg.p + R, key_bits, s->stream));
        }
        gd_launch_glue_merge(q, (unsigned)most_rows, s->stream);
        tmp_bytes = gl.tmp.n;
        HIPCHK(gd_glue_sort_keys(gl.tmp.p, &tmp_bytes, gl.merged.p, gl.keys[o].p, gl.merged.n, R, gl.seg.p + 2 * R, gl.seg.p + 3 * R, key_bits, s->stream));
        HIPCHK(gl.pin.ensure(gd::grown_capacity(gl.pin.n, (size_t)R * most_new)));
        HIPCHK(hipMemcpy2DAsync(gl.pin.p, most_new * sizeof(unsigned long long), gl.keys[o].p, ms * sizeof(unsigned long long),
                                most_new * sizeof(unsigned long long), R, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(hipMemcpyAsync(gl.nkeys.p, h_nk, R * sizeof(unsigned), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    gl.kstride[o] = ms; gl.cur = o;
    for (uint32_t r = 0; r < R; r++) {
        gl.sets[r].assign(gl.pin.p + (size_t)r * most_new, gl.pin.p + (size_t)r * most_new + h_nk[r]);
        glue_install(s, r);
    }
    return GD_OK;
}
