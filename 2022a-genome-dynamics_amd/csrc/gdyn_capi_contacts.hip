// gdyn_capi_contacts.hip -- what a caller observes of the pairs in contact: gd_search_pairs with its cache, the contact maps
// (gd_contacts_*), and the seam through which the live bridge reads their tables.  Of the stepper (gdyn_capi.hip) it calls prepare
// and search_device, which builds lists.
#include <algorithm>
#include <vector>

#include "gdyn_system.hpp"

// md::neighbor_searcher{box, dcut}.search(): served on the device from the resident Verlet list when that list is
// complete for dcut (dcut + 2 x largest displacement since the build <= list radius), after ONE list build otherwise -- a
// build at radius max(force-list radius, dcut), so the force list stays valid either way and the next gd_run does not rebuild.
// The result is cached for the repeated call of the count-then-fetch idiom.
extern "C" int gd_search_pairs(gd_system *s, uint32_t r, double dcut, uint32_t *pairs, uint64_t cap, uint64_t *n_pairs)
{
    if (!s || !n_pairs || (cap && !pairs)) return fail(GD_EINVAL, "gd_search_pairs: NULL argument");
    if (r >= s->R || !(dcut > 0)) return fail(GD_EINVAL, "gd_search_pairs: bad replica or cutoff");
    GDCHK(prepare(s));
    gd::SearchCache &sp = s->sp;
    if (!(sp.valid && sp.r == r && sp.dcut == dcut && sp.serial == s->state_serial)) {
        std::vector<unsigned long long> cnt;
        GDCHK(search_device(s, r, 1, dcut, sp.out, sp.count, cnt));
        sp.host.resize((size_t)cnt[0]);
        if (cnt[0]) HIPCHK(hipMemcpy(sp.host.data(), sp.out.p, (size_t)cnt[0] * sizeof(uint2), hipMemcpyDeviceToHost));
        sp.valid = true; sp.r = r; sp.dcut = dcut; sp.serial = s->state_serial;
    }
    const uint64_t n = sp.host.size();
    for (uint64_t k = 0; k < n && k < cap; k++) { pairs[2 * k] = sp.host[k].x; pairs[2 * k + 1] = sp.host[k].y; }
    *n_pairs = n;
    return GD_OK;
}

// ------------------------------------------------------------- contact maps
// contact_map (simulation_interphase/contact_map.cc:26-91) on the device, for all replicas of the handle at once: update() = one
// pair search over every replica + one insert launch into the per-replica count tables; nothing but R pair counts crosses PCIe
// until a map is dumped.  The tables share one capacity (a power of two) and are grown AHEAD of an update so that no table is more
// than half full after it, whatever the update adds (the search has already counted the pairs when the tables are sized).
static ContactTab contact_tab(gd_system *s)
{
    ContactTab t;
    t.words = s->ct.words.p; t.distinct = s->ct.distinct.p; t.cap = s->ct.cap; t.jbits = contact_jbits(s);
    return t;
}

extern "C" int gd_contacts_update(gd_system *s, double distance)
{
    if (!s) return fail(GD_EINVAL, "gd_contacts_update: NULL argument");
    if (!(distance > 0)) return fail(GD_EINVAL, "gd_contacts_update: the contact distance must be positive");
    if (contact_jbits(s) > 20) return fail(GD_EINVAL, "gd_contacts_update: contact maps take at most 1 048 576 beads (the count shares a 64-bit word with the pair)");
    GDCHK(prepare(s));
    gd::ContactTables &ct = s->ct;
    std::vector<unsigned long long> cnt;
    GDCHK(search_device(s, 0, s->R, distance, ct.pairs, ct.count, cnt));
    if (ct.distinct_h.size() != s->R) ct.distinct_h.assign(s->R, 0u);
    unsigned long long need = 0, most = 0;
    for (uint32_t r = 0; r < s->R; r++) { need = std::max(need, ct.distinct_h[r] + cnt[2 * r]); most = std::max(most, cnt[2 * r]); }
    size_t cap = std::max<size_t>(ct.cap, 1024);
    while (cap < 2 * need) cap *= 2;
    if (cap != ct.cap) {
        gd::dbuf<unsigned long long> words;
        HIPCHK(words.resize((size_t)s->R * cap, false));
        HIPCHK(hipMemsetAsync(words.p, 0xff, words.n * sizeof(unsigned long long), s->stream));
        if (ct.cap) {
            ContactTab to = contact_tab(s), from = to;
            to.words = words.p; to.cap = cap;
            HIPCHK(hipMemsetAsync(ct.distinct.p, 0, s->R * sizeof(unsigned), s->stream));      // (recounted by the rehash)
            gd_launch_contacts_rehash(from, to, s->R, s->stream);
            HIPCHK(hipStreamSynchronize(s->stream));      // the old tables are freed below
        } else HIPCHK(ct.distinct.resize(s->R));
        ct.words = std::move(words);      // (the old tables go with `words`)
        ct.cap = cap;
    }
    gd_launch_contacts_insert(contact_tab(s), ct.pairs.p, ct.pairs.n / s->R, ct.count.p, most, s->R, s->stream);
    HIPCHK(hipMemcpyAsync(ct.distinct_h.data(), ct.distinct.p, s->R * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    return GD_OK;
}

extern "C" int gd_contacts_fetch(gd_system *s, uint32_t r, uint32_t *rows, uint64_t cap, uint64_t *n_rows)
{
    if (!s || !n_rows || (cap && !rows)) return fail(GD_EINVAL, "gd_contacts_fetch: NULL argument");
    if (r >= s->R) return fail(GD_EINVAL, "gd_contacts_fetch: bad replica");
    gd::ContactTables &ct = s->ct;
    const uint64_t n = ct.cap ? ct.distinct_h[r] : 0;
    *n_rows = n;
    if (!n || !cap) return GD_OK;       // (the count of the count-then-fetch idiom costs nothing: the host mirrors the occupancy)
    HIPCHK(hipSetDevice(s->device));
    for (int k = 0; k < 2; k++)
        if (ct.ck[k].n < n) { HIPCHK(ct.ck[k].resize((size_t)(n + n / 4), false)); HIPCHK(ct.cv[k].resize((size_t)(n + n / 4), false)); }
    HIPCHK(ct.n.resize(1));
    HIPCHK(hipMemsetAsync(ct.n.p, 0, sizeof(unsigned), s->stream));
    gd_launch_contacts_compact(contact_tab(s), r, ct.ck[0].p, ct.cv[0].p, ct.n.p, s->stream);
    const unsigned jb = contact_jbits(s), bits = 2 * jb;      // key = i << jb | j
    size_t tmp_bytes = 0;
    HIPCHK(gd_sort_contacts(nullptr, &tmp_bytes, ct.ck[0].p, ct.ck[1].p, ct.cv[0].p, ct.cv[1].p, (size_t)n, bits, s->stream));
    if (ct.tmp.n < tmp_bytes) HIPCHK(ct.tmp.resize(tmp_bytes + tmp_bytes / 4, false));
    tmp_bytes = ct.tmp.n;
    HIPCHK(gd_sort_contacts(ct.tmp.p, &tmp_bytes, ct.ck[0].p, ct.ck[1].p, ct.cv[0].p, ct.cv[1].p, (size_t)n, bits, s->stream));
    std::vector<unsigned long long> hk((size_t)n); std::vector<unsigned> hv((size_t)n);
    unsigned found = 0;
    HIPCHK(hipMemcpyAsync(hk.data(), ct.ck[1].p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(hv.data(), ct.cv[1].p, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(&found, ct.n.p, sizeof found, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    if (found != n) return fail(GD_ESTATE, "gd_contacts_fetch: table occupancy %u differs from the %llu entries counted", found, (unsigned long long)n);
    for (uint64_t k = 0; k < n && k < cap; k++) {
        rows[3 * k] = (uint32_t)(hk[k] >> jb); rows[3 * k + 1] = (uint32_t)(hk[k] & ((1ull << jb) - 1ull)); rows[3 * k + 2] = hv[k];
    }
    return GD_OK;
}

extern "C" int gd_contacts_clear(gd_system *s, uint32_t r)
{
    if (!s) return fail(GD_EINVAL, "gd_contacts_clear: NULL argument");
    if (r != GD_ALL_REPLICAS && r >= s->R) return fail(GD_EINVAL, "gd_contacts_clear: bad replica");
    gd::ContactTables &ct = s->ct;
    if (!ct.cap) return GD_OK;
    HIPCHK(hipSetDevice(s->device));
    const uint32_t r0 = r == GD_ALL_REPLICAS ? 0 : r, nr = r == GD_ALL_REPLICAS ? s->R : 1;
    HIPCHK(hipMemsetAsync(ct.words.p + (size_t)r0 * ct.cap, 0xff, (size_t)nr * ct.cap * sizeof(unsigned long long), s->stream));
    HIPCHK(hipMemsetAsync(ct.distinct.p + r0, 0, nr * sizeof(unsigned), s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (uint32_t k = r0; k < r0 + nr; k++) ct.distinct_h[k] = 0;
    return GD_OK;
}

// The live bridge's seam to the tables (gdyn_live.hpp).  It needs no prepare(): the tables are what gd_contacts_fetch reads, which does
// not prepare either.  It ends with the stream idle, so no update is in flight when an analysis stream reads them.
int gd_live_contact_tab(gd_system *s, ContactTab *tab, const unsigned **occupancy)
{
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    *tab = contact_tab(s);
    *occupancy = s->ct.cap ? s->ct.distinct_h.data() : nullptr;
    return GD_OK;
}
