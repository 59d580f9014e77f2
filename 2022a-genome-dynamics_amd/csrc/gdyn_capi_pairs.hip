// gdyn_capi_pairs.hip -- the two terms that run as kernels of their own behind k_step: the droplet attraction (gd_set_pair_softwell)
// and the per-replica dynamic pairs (include/gdyn_replica.h).  They meet the stepper (gdyn_capi.hip) at four places: post_step_active,
// sync_replica_pairs, launch_softwell, launch_replica_pairs.
#include <algorithm>
#include <vector>

#include "gdyn_system.hpp"

// ---- the droplet term

extern "C" int gd_set_pair_softwell(gd_system *s, double energy, double decay, double cutoff, const uint32_t *targets, uint32_t n)
{
    if (!s || (n && !targets)) return fail(GD_EINVAL, "gd_set_pair_softwell: NULL argument");
    if (n > 4096) return fail(GD_EINVAL, "gd_set_pair_softwell: at most 4096 targets");
    if (n && (!(decay > 0) || !(cutoff > 0))) return fail(GD_EINVAL, "gd_set_pair_softwell: decay and cutoff must be positive");
    for (uint32_t k = 0; k < n; k++) if (targets[k] >= s->N) return fail(GD_EINVAL, "gd_set_pair_softwell: target %u out of range", k);
    {   // set_neighbor_targets takes a set of particles: a repeated index would make two threads update one bead
        std::vector<uint32_t> t(targets, targets + n);
        std::sort(t.begin(), t.end());
        for (uint32_t k = 1; k < n; k++) if (t[k] == t[k - 1]) return fail(GD_EINVAL, "gd_set_pair_softwell: target %u listed twice", t[k]);
    }
    HIPCHK(hipSetDevice(s->device));
    s->sw.n = 0;
    if (n) {
        HIPCHK(s->sw.targets.resize(n, false));
        HIPCHK(hipMemcpy(s->sw.targets.p, targets, n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(s->sw.esum.resize(s->R));
        s->sw.n = n; s->sw.eps = energy; s->sw.decay = decay; s->sw.cut = cutoff;
    }
    return GD_OK;
}

// the droplet term of the step / force / energy evaluation that `p` describes (same positions, same buffers)
void launch_softwell(gd_system *s, const StepParams &p, int mode)
{
    SoftwellP q;
    memset(&q, 0, sizeof q);
    q.pos_in = p.pos_in; q.pos_out = p.pos_out; q.fout = s->fout.p; q.esum = s->sw.esum.p;
    q.slot_of = s->slot_of.p; q.targets = s->sw.targets.p;
    q.mob_o = s->mob_uniform >= 0.f ? nullptr : s->mob_o.p; q.mob_uniform = s->mob_uniform; q.dt = p.dt;
    q.lo = p.lo; q.comp = p.comp;      // (a compensated step keeps the droplet's share of mu F dt in the residuals too)
    q.eps = (float)s->sw.eps; q.inv_d2 = (float)(1.0 / (s->sw.decay * s->sw.decay)); q.rc2 = (float)(s->sw.cut * s->sw.cut);
    q.N = s->N; q.Np = s->Np; q.R = s->R; q.M = s->sw.n;
    set_box(s, q);
    gd_launch_softwell(q, mode, s->stream);
}

// ---- per-replica dynamic pairs (include/gdyn_replica.h)
static_assert(gd::RP_SLOT_SHIFT == GD_RP_SLOT_SHIFT && gd::RP_PARTNER_MASK == GD_RP_PARTNER_MASK && GD_ADJ_MASK <= GD_RP_PARTNER_MASK, "entry format");
static_assert(gd::RP_RECORD_WORDS * sizeof(uint32_t) == gd::RP_SLOTS * sizeof(BondType), "record words");

// A kernel behind k_step moves beads after k_step has bounded their displacement (the droplet term, the per-replica pairs): the running
// bound then covers no step's output, so both list classes are walked and the list serves no observation after the run.
bool post_step_active(const gd_system *s) { return s->sw.n != 0 || s->rp.any(); }

static BondType bond_record(const gd_bond_params &p, int term)
{
    const bool harmonic = p.kind == GD_POT_HARMONIC;     // U = K r^2 / 2 is the spring with rest length 0
    return BondType{(float)p.k_a, (float)p.k_b, harmonic ? 0.f : (float)p.l_a, harmonic ? 0.f : (float)p.l_b,
                    (p.mix ? 1 : 0) | (p.scale_by_bond_scale ? 2 : 0) | (p.minimum_image ? 4 : 0) | (term << 8),
                    p.kind == GD_POT_SEMISPRING ? 0.f : -3.0e38f, p.kind, p.p | (p.q << 8)};
}

// The lists the caller set since the last evaluation: flattened, packed into the pinned block and sent with one asynchronous copy.
// (Every evaluation ends behind a stream synchronisation, so the copy before has left the block by now: the wait on its event returns
// at once, except after an evaluation that ended early on an error.)
int sync_replica_pairs(gd_system *s)
{
    if (!s->rp.dirty()) return GD_OK;
    gd::ReplicaUpload &u = s->rp_up;
    const gd::ReplicaLayout l = s->rp.flatten();
    if (l.words > 0xffffffffull) return fail(GD_ENOMEM, "per-replica pair lists: %zu words exceed the table's 32-bit offsets", l.words);
    if (!u.copied) HIPCHK(hipEventCreateWithFlags(&u.copied, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(u.copied));
    HIPCHK(u.stage.ensure(gd::grown_capacity(u.stage.n, l.words)));
    if (l.words > u.dev.n) HIPCHK(u.dev.resize(gd::grown_capacity(u.dev.n, l.words), false));
    if (!u.esum.p) HIPCHK(u.esum.resize(s->R));
    s->rp.pack(l, u.stage.p);
    BondType rec[gd::RP_SLOTS];
    for (uint32_t k = 0; k < gd::RP_SLOTS; k++) rec[k] = s->rp.defined(k) ? bond_record(u.params[k], GD_TERM_DYNAMIC) : BondType{};
    memcpy(u.stage.p + l.rec, rec, sizeof rec);
    HIPCHK(hipMemcpyAsync(u.dev.p, u.stage.p, l.words * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipEventRecord(u.copied, s->stream));
    u.layout = l;
    return GD_OK;
}

// the per-replica pairs of the step / force / energy evaluation that `p` describes (same positions, same buffers)
void launch_replica_pairs(gd_system *s, const StepParams &p, int mode)
{
    const gd::ReplicaLayout &l = s->rp_up.layout;
    const uint32_t *dev = s->rp_up.dev.p;
    ReplicaPairsP q;
    memset(&q, 0, sizeof q);
    q.pos_in = p.pos_in; q.pos_out = p.pos_out; q.fout = s->fout.p; q.esum = s->rp_up.esum.p; q.slot_of = s->slot_of.p;
    q.base = (const uint4 *)(dev + l.base); q.rec = (const BondType *)(dev + l.rec);
    q.row_bead = dev + l.row_bead; q.row_off = dev + l.row_off; q.ent = dev + l.ent;
    q.ctx = mode == 0 ? p.ctx_out : p.ctx_in;      // (a step's k_step has applied the pending callback and left the result there)
    q.ab_o = s->ab_o.p; q.ab_stride = s->ab_stride;
    q.mob_o = s->mob_uniform >= 0.f ? nullptr : s->mob_o.p; q.mob_uniform = s->mob_uniform; q.dt = p.dt;
    q.lo = p.lo; q.comp = p.comp;
    q.N = s->N; q.Np = s->Np; q.R = s->R; q.max_rows = l.max_rows;
    set_box(s, q);
    gd_launch_replica_pairs(q, mode, s->stream);
}

extern "C" int gd_replica_abi_version(void) { return GD_REPLICA_ABI_VERSION; }

extern "C" int gd_replica_pairs_define(gd_system *s, uint32_t slot, const gd_bond_params *p)
{
    if (!s || !p) return fail(GD_EINVAL, "gd_replica_pairs_define: NULL argument");
    if (slot >= gd::RP_SLOTS) return fail(GD_EINVAL, "gd_replica_pairs_define: slot %u out of range", slot);
    GDCHK(check_bond_params(p));
    s->rp_up.params[slot] = *p;
    s->rp.define(slot);
    return GD_OK;
}

extern "C" int gd_replica_pairs_set(gd_system *s, uint32_t slot, uint32_t replica, const uint32_t *pairs, uint32_t n)
{
    if (!s || (n && !pairs)) return fail(GD_EINVAL, "gd_replica_pairs_set: NULL argument");
    if (slot >= gd::RP_SLOTS) return fail(GD_EINVAL, "gd_replica_pairs_set: slot %u out of range", slot);
    if (replica >= s->R) return fail(GD_EINVAL, "gd_replica_pairs_set: replica %u out of range", replica);
    if (!s->rp.defined(slot)) return fail(GD_ESTATE, "gd_replica_pairs_set: slot %u was never defined (gd_replica_pairs_define)", slot);
    if (s->gl.defined && slot == s->gl.slot) return fail(GD_ESTATE, "gd_replica_pairs_set: slot %u is managed by gd_glue_define (use gd_glue_set)", slot);
    if (const size_t bad = s->rp.set(slot, replica, pairs, n))
        return fail(GD_EINVAL, "gd_replica_pairs_set: bad pair %zu (%u,%u)", bad - 1, pairs[2 * (bad - 1)], pairs[2 * (bad - 1) + 1]);
    return GD_OK;
}

extern "C" int gd_replica_pairs_count(gd_system *s, uint32_t slot, uint32_t replica, uint32_t *n)
{
    if (!s || !n) return fail(GD_EINVAL, "gd_replica_pairs_count: NULL argument");
    if (slot >= gd::RP_SLOTS) return fail(GD_EINVAL, "gd_replica_pairs_count: slot %u out of range", slot);
    if (replica >= s->R) return fail(GD_EINVAL, "gd_replica_pairs_count: replica %u out of range", replica);
    if (!s->rp.defined(slot)) return fail(GD_ESTATE, "gd_replica_pairs_count: slot %u was never defined (gd_replica_pairs_define)", slot);
    *n = s->rp.count(slot, replica);
    return GD_OK;
}
