// gdyn_capi.hip -- host side of libgdyn: the C-ABI of include/gdyn.h over the HIP kernels.
//
// One handle = one HIP device + one stream + R replicas of an N-bead system resident in HBM.
// gd_run() enqueues   [list build] + K x k_step   segments with no host round trip; the
// Verlet skin is VERIFIED on the device (every step checks each bead's displacement since
// the build) and a violated chunk is rolled back and re-run with a shorter interval, so
// the fixed build cadence never changes results (only the summation order of pair terms).
// What the host knows about the list in use is one gd::ResidentList (gdyn_list.hpp): this file calls its transitions -- a build, the
// caller's positions, a new topology, a rollback, a dropped list -- and assigns none of its members ("Resident list").
// The handle itself (gd_system) and the features that live in files of their own -- the kernels behind k_step, the contact maps and
// pair search, the glue kinetics -- are in gdyn_system.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_fp16.h>

#include "gdyn_system.hpp"
#include "gdyn_once.hpp"
#ifdef GD_DEV
#include "gdyn_dev.h"
#endif

// ------------------------------------------------------------------ errors
// (gd::fail, HIPCHK and GDCHK of gdyn_analysis.hpp write the message here, as every other file of the library does)

static thread_local char g_err[1024];
extern "C" const char *gd_last_error(void) { return g_err; }
int gd_report_error(int code, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

// Experiment hooks (environment variables, debug prints, the kernel micro-benchmark) exist in developer builds only
// (make dev -> libgdyn_dev.so, -DGD_DEV); the product library reads no environment variable.
#ifdef GD_DEV
static const char *dev_env(const char *name) { return getenv(name); }
#else
static const char *dev_env(const char *) { return nullptr; }
#endif
extern "C" const char *gd_backend_name(void) { return "hip"; }

static int valid_pq(int p, int q) { return (p == 2 || p == 4 || p == 6 || p == 8 || p == 12) && q >= 1 && q <= 4; }

extern "C" int gd_abi_version(void) { return GD_ABI_VERSION; }

extern "C" int gd_create_abi(int abi_version, const gd_desc *d, gd_system **out)
{
    if (abi_version != GD_ABI_VERSION)
        return fail(GD_EINVAL, "gd_create: the caller was built against gdyn.h ABI version %d, this library implements %d", abi_version, GD_ABI_VERSION);
    if (!d || !out) return fail(GD_EINVAL, "gd_create: NULL argument");
    if (d->n_beads == 0 || d->n_replicas == 0) return fail(GD_EINVAL, "gd_create: n_beads and n_replicas must be > 0");
    if (d->n_beads > GD_ADJ_MASK) return fail(GD_EINVAL, "gd_create: n_beads exceeds %u", GD_ADJ_MASK);
    if (d->box_kind != GD_BOX_OPEN && d->box_kind != GD_BOX_PERIODIC) return fail(GD_EINVAL, "gd_create: bad box_kind");
    if (d->box_kind == GD_BOX_PERIODIC)
        for (int k = 0; k < 3; k++) if (!(d->box[k] > 0)) return fail(GD_EINVAL, "gd_create: periodic box needs positive periods");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GD_ENODEVICE, "gd_create: no HIP device visible (libgdyn has no CPU fallback)");
    if (d->device < 0 || d->device >= ndev) return fail(GD_ENODEVICE, "gd_create: device %d not in [0,%d)", d->device, ndev);
    HIPCHK(hipSetDevice(d->device));
    {   // per-device set-up (LDS opt-in of the kernels): once per device ordinal, complete before any handle on it exists
        static gd::DeviceOnce<> once;
        const int rc = once.run(d->device, [](int) { return (int)gd_kernels_init_device(); });
        if (rc != (int)hipSuccess)
            return fail(GD_EHIP, "gd_create: kernel set-up on device %d failed: %s", d->device, rc < 0 ? "device ordinal beyond the guard's table" : hipGetErrorString((hipError_t)rc));
    }
    gd_system *s = new (std::nothrow) gd_system();
    if (!s) return fail(GD_ENOMEM, "gd_create: out of host memory");
    s->N = d->n_beads; s->R = d->n_replicas; s->device = d->device; s->box_kind = d->box_kind;
    memcpy(s->box, d->box, sizeof s->box);
    s->nblk = (s->N + GD_BLOCK - 1) / GD_BLOCK;
    s->Np = s->nblk * GD_BLOCK;
    s->cpb = (s->nblk + GD_XCDS - 1) / GD_XCDS;
    if (s->R % GD_XCDS == 0 && !dev_env("GDYN_SLICE_MAP")) s->cpb = 0;      // whole replicas per XCD (see block_map)
    s->ens.reset(s->N, s->R); s->mob.assign(s->N, 1.0); s->bend.assign(s->N, 0.0);
    s->hctx.assign(s->R, DevCtx{});
    for (auto &c : s->hctx) { c.bead_scale = 1; c.bond_scale = 1; }   // wall_semiaxes {0,0,0} until a wall is set (simulation_context.hpp:16)
    s->rp.reset(s->N, s->R);
    s->lcount.assign(2 * (size_t)s->R, 0ull);      // per replica: directed entries, then the near entries (in fours) of tiled lists
    s->ncell_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(8ull * s->N, 4096ull), 262144ull);
    if (const char *e = dev_env("GDYN_NEAR_FRAC")) s->near_frac = atof(e);
    if (const char *e = dev_env("GDYN_SKIN")) { s->pol.skin = atof(e); s->pol.skin_fixed = true; }
    if (dev_env("GDYN_AUTO_SKIN")) s->pol.tuner.enabled = true;
    if (const char *e = dev_env("GDYN_TILE_CAPS")) { auto &c = s->pol.tile_caps; c.clear(); for (const char *q = e; *q;) { c.push_back((unsigned)strtoul(q, (char **)&q, 10)); if (*q == ',') q++; } }
    if (const char *e = dev_env("GDYN_K_TARGET")) s->pol.k_target = atof(e);
    if (dev_env("GDYN_DEBUG")) s->pol.trace = stderr;
    size_t free_b = 0, total_b = 0;      // the list policy's memory guard (off when the query fails)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) s->pol.mem_total = total_b;
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete s; return fail(GD_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e)); }
    const size_t RNp = (size_t)s->R * s->Np, RN = (size_t)s->R * s->N;
    bool ok = true;
    for (int k = 0; k < 2; k++) {
        ok = ok && s->pos[k].resize(RNp) == hipSuccess && s->orig[k].resize(RNp) == hipSuccess && s->ctx[k].resize(s->R) == hipSuccess &&
             s->react_part[k].resize((size_t)s->R * s->nblk) == hipSuccess;
    }
    ok = ok && s->ctxf.resize(s->R) == hipSuccess;      // (prepared contexts of grouped spans: 128 bytes a replica)
    ok = ok && s->xb.resize(RNp) == hipSuccess && s->slot_of.resize(RN) == hipSuccess && s->bbox_enc.resize((size_t)2 * s->R * 6) == hipSuccess && s->bbox_w.resize((size_t)s->R * s->nblk * (GD_BLOCK / 64) * 6) == hipSuccess &&
         s->rank.resize(RNp) == hipSuccess && s->members.resize(RNp) == hipSuccess && s->cell_cnt.resize((size_t)s->R * (s->ncell_cap + 1)) == hipSuccess &&
         s->cell_start.resize((size_t)s->R * (s->ncell_cap + 1)) == hipSuccess && s->meta.resize(RNp) == hipSuccess &&
         s->flags.resize((size_t)s->R * GD_NFLAGS) == hipSuccess && s->bbox.resize((size_t)s->R * s->nblk * 6) == hipSuccess &&
         s->ab.resize(RNp) == hipSuccess && s->mobs.resize(RNp) == hipSuccess && s->grid.resize(s->R) == hipSuccess &&
         s->epart.resize((size_t)s->R * s->nblk) == hipSuccess &&
         s->lcount_d.resize(2 * (size_t)s->R) == hipSuccess && s->dmax.resize((size_t)s->R * GD_DMAX_STRIDE) == hipSuccess && s->fout.resize(RN) == hipSuccess && s->snap.resize(RN) == hipSuccess &&
         s->tiles.resize((size_t)s->R * s->nblk) == hipSuccess &&
         s->rec_x0.resize(RNp) == hipSuccess && s->rec_mo.resize(RNp) == hipSuccess && s->len_prev.resize((size_t)s->R * s->N) == hipSuccess &&
         s->wtab.resize(RNp / 64) == hipSuccess && s->need_prev.resize((size_t)s->R * s->N) == hipSuccess && s->pool.resize(4) == hipSuccess && s->rqueue.resize(RNp / 64) == hipSuccess &&
         s->lo.resize(RN) == hipSuccess;
    s->lo_valid = ok;      // (positions and residuals all zero)
    if (!ok) { delete s; return fail(GD_ENOMEM, "gd_create: device allocation failed (%zu slots)", RNp); }
    gd_launch_identity(s->orig[0].p, s->slot_of.p, s->N, s->Np, s->R, s->stream);
    if (hipStreamSynchronize(s->stream) != hipSuccess) { delete s; return fail(GD_EHIP, "gd_create: identity kernel failed"); }
    *out = s;
    return GD_OK;
}

extern "C" int gd_destroy(gd_system *s)
{
    if (!s) return GD_OK;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
    return GD_OK;
}

// ---------------------------------------------------------------- context

static int upload_ctx(gd_system *s)
{
    if (!s->ctx_dirty) return GD_OK;
    HIPCHK(hipMemcpyAsync(s->ctx[s->ccur].p, s->hctx.data(), s->R * sizeof(DevCtx), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->ctx_dirty = false;
    return GD_OK;
}
static int download_ctx(gd_system *s)
{
    HIPCHK(hipMemcpyAsync(s->hctx.data(), s->ctx[s->ccur].p, s->R * sizeof(DevCtx), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return GD_OK;
}

// ---------------------------------------------------------- model setters

extern "C" int gd_set_positions(gd_system *s, const double *xyz)
{
    if (!s || !xyz) return fail(GD_EINVAL, "gd_set_positions: NULL argument");
    HIPCHK(hipSetDevice(s->device));
    const size_t RN = (size_t)s->R * s->N;
    std::vector<float4> h(RN), hl(RN);
    for (size_t i = 0; i < RN; i++) {
        if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2]))
            return fail(GD_EINVAL, "gd_set_positions: non-finite coordinate at %zu", 3 * i);
        h[i] = make_float4((float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2], 0.f);
        // what the fp32 coordinate drops of the fp64 input: the residual of the compensated update starts from it
        hl[i] = make_float4((float)(xyz[3 * i] - (double)h[i].x), (float)(xyz[3 * i + 1] - (double)h[i].y), (float)(xyz[3 * i + 2] - (double)h[i].z), 0.f);
    }
    HIPCHK(hipMemcpy2DAsync(s->pos[s->pcur].p, (size_t)s->Np * sizeof(float4), h.data(), (size_t)s->N * sizeof(float4),
                            (size_t)s->N * sizeof(float4), s->R, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(s->lo.p, hl.data(), RN * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    s->lo_valid = true;
    gd_launch_identity(s->orig[s->ocur].p, s->slot_of.p, s->N, s->Np, s->R, s->stream);
    HIPCHK(hipStreamSynchronize(s->stream));
    s->list.positions_set(); s->state_serial++;
    return GD_OK;
}

// Snapshot download: gather to bead order and pack xyz on the device, one copy into a pinned staging buffer that
// lives with the handle (a fresh pageable buffer per call costs page faults and a slower copy).
static int fetch_xyz(gd_system *s, const float **out, int quantize)
{
    HIPCHK(hipSetDevice(s->device));
    const size_t n3 = (size_t)s->R * s->N * 3;
    HIPCHK(s->h_stage.ensure(n3));
    gd_launch_gather_xyz(s->pos[s->pcur].p, s->slot_of.p, (float *)s->fout.p, s->N, s->Np, s->R, quantize, s->stream);   // fout: R*N float4 >= n3 floats
    HIPCHK(hipMemcpyAsync(s->h_stage.p, s->fout.p, n3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    *out = s->h_stage.p;
    return GD_OK;
}

extern "C" int gd_get_positions(gd_system *s, double *xyz)
{
    if (!s || !xyz) return fail(GD_EINVAL, "gd_get_positions: NULL argument");
    const float *h = nullptr;
    GDCHK(fetch_xyz(s, &h, 0));
    const size_t n3 = (size_t)s->R * s->N * 3;
    for (size_t i = 0; i < n3; i++) xyz[i] = h[i];
    if (s->lo_valid) {      // compensated positions: the fp64 boundary gets pos + lo
        std::vector<float4> hl(n3 / 3);
        HIPCHK(hipMemcpy(hl.data(), s->lo.p, hl.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < hl.size(); i++) { xyz[3 * i] += (double)hl[i].x; xyz[3 * i + 1] += (double)hl[i].y; xyz[3 * i + 2] += (double)hl[i].z; }
    }
    return GD_OK;
}

extern "C" int gd_get_positions_f32(gd_system *s, float *xyz, int quantize)
{
    if (!s || !xyz) return fail(GD_EINVAL, "gd_get_positions_f32: NULL argument");
    const float *h = nullptr;
    GDCHK(fetch_xyz(s, &h, quantize));
    memcpy(xyz, h, (size_t)s->R * s->N * 3 * sizeof(float));
    return GD_OK;
}

extern "C" int gd_set_bead_params(gd_system *s, const double *a, const double *b, const double *mob, const double *bend)
{
    if (!s) return fail(GD_EINVAL, "gd_set_bead_params: NULL system");
    if (mob) for (uint32_t i = 0; i < s->N; i++) if (!(mob[i] >= 0)) return fail(GD_EINVAL, "gd_set_bead_params: negative mobility at %u", i);
    s->ens.set_shared(a, b);      // (a column replaces that column of every replica, gdyn_ensemble.h)
    if (mob) s->mob.assign(mob, mob + s->N);
    if (bend) s->bend.assign(bend, bend + s->N);
    s->topo_dirty = true;
    return GD_OK;
}

extern "C" int gd_set_pair_softcore(gd_system *s, const gd_pair_softcore *p)
{
    if (!s || !p) return fail(GD_EINVAL, "gd_set_pair_softcore: NULL argument");
    if (!valid_pq(p->p_a, p->q_a) || !valid_pq(p->p_b, p->q_b)) return fail(GD_EINVAL, "gd_set_pair_softcore: unsupported softcore powers");
    if (p->sigma_a < 0 || p->sigma_b < 0) return fail(GD_EINVAL, "gd_set_pair_softcore: negative diameter");
    s->pair = *p; s->has_pair = true; s->list.drop();
    return GD_OK;
}

int check_bond_params(const gd_bond_params *p)
{
    if (p->kind < GD_POT_HARMONIC || p->kind > GD_POT_SOFTCORE) return fail(GD_EINVAL, "bond params: bad kind %d", p->kind);
    if (p->kind == GD_POT_SOFTCORE && !valid_pq(p->p, p->q)) return fail(GD_EINVAL, "bond params: unsupported softcore powers");
    // a softcore bond is k_a (1 - (r/l_a)^p)^q as given (gdyn.h): mixing and bond_scale scaling are not defined for it
    if (p->kind == GD_POT_SOFTCORE && (p->mix || p->scale_by_bond_scale))
        return fail(GD_EINVAL, "bond params: a softcore bond takes neither mix nor scale_by_bond_scale");
    return GD_OK;
}

static int add_bond_type(gd_system *s, const gd_bond_params *p, int term)
{
    for (size_t i = 0; i < s->btypes.size(); i++)
        if (!memcmp(&s->btypes[i], p, sizeof *p) && s->bterm[i] == term) return (int)i;
    if (s->btypes.size() >= GD_MAX_BOND_TYPES) return -1;
    s->btypes.push_back(*p); s->bterm.push_back(term);
    return (int)s->btypes.size() - 1;
}

extern "C" int gd_add_bond_range(gd_system *s, const gd_bond_params *p, uint32_t start, uint32_t end, uint32_t stride)
{
    if (!s || !p) return fail(GD_EINVAL, "gd_add_bond_range: NULL argument");
    GDCHK(check_bond_params(p));
    if (start > end || end > s->N) return fail(GD_EINVAL, "gd_add_bond_range: range [%u,%u) outside [0,%u)", start, end, s->N);
    if (stride < 1 || stride > 2) return fail(GD_EINVAL, "gd_add_bond_range: stride must be 1 or 2");
    const int t = add_bond_type(s, p, GD_TERM_BOND);
    if (t < 0) return fail(GD_EINVAL, "gd_add_bond_range: too many bond parameter sets");
    for (uint32_t i = start; i + stride < end; i++) s->bonds.push_back({i, i + stride, t});
    s->topo_dirty = true;
    return GD_OK;
}

extern "C" int gd_add_bond_pairs(gd_system *s, const gd_bond_params *p, const uint32_t *pairs, uint32_t n)
{
    if (!s || !p || (n && !pairs)) return fail(GD_EINVAL, "gd_add_bond_pairs: NULL argument");
    GDCHK(check_bond_params(p));
    for (uint32_t k = 0; k < n; k++)
        if (pairs[2 * k] >= s->N || pairs[2 * k + 1] >= s->N || pairs[2 * k] == pairs[2 * k + 1])
            return fail(GD_EINVAL, "gd_add_bond_pairs: bad pair %u (%u,%u)", k, pairs[2 * k], pairs[2 * k + 1]);
    const int t = add_bond_type(s, p, GD_TERM_BOND);
    if (t < 0) return fail(GD_EINVAL, "gd_add_bond_pairs: too many bond parameter sets");
    for (uint32_t k = 0; k < n; k++) s->bonds.push_back({pairs[2 * k], pairs[2 * k + 1], t});
    s->topo_dirty = true;
    return GD_OK;
}

extern "C" int gd_set_dynamic_pairs(gd_system *s, uint32_t slot, const gd_bond_params *p, const uint32_t *pairs, uint32_t n)
{
    if (!s || !p || (n && !pairs)) return fail(GD_EINVAL, "gd_set_dynamic_pairs: NULL argument");
    if (slot >= 4) return fail(GD_EINVAL, "gd_set_dynamic_pairs: slot %u out of range", slot);
    GDCHK(check_bond_params(p));
    for (uint32_t k = 0; k < n; k++)
        if (pairs[2 * k] >= s->N || pairs[2 * k + 1] >= s->N || pairs[2 * k] == pairs[2 * k + 1])
            return fail(GD_EINVAL, "gd_set_dynamic_pairs: bad pair %u", k);
    s->dyn[slot].used = true; s->dyn[slot].p = *p;
    s->dyn[slot].pairs.assign(pairs, pairs + 2 * (size_t)n);
    s->topo_dirty = true;
    return GD_OK;
}

extern "C" int gd_add_bending_range(gd_system *s, uint32_t start, uint32_t end, double energy, int per_bead)
{
    if (!s) return fail(GD_EINVAL, "gd_add_bending_range: NULL system");
    if (start > end || end > s->N) return fail(GD_EINVAL, "gd_add_bending_range: range outside [0,N)");
    s->bends.push_back({start, end, energy, per_bead});
    s->topo_dirty = true;
    return GD_OK;
}

extern "C" int gd_add_point_source(gd_system *s, int kind, double k, double b, const double point[3], const uint32_t *targets, uint32_t nt)
{
    if (!s || !point) return fail(GD_EINVAL, "gd_add_point_source: NULL argument");
    if (kind != GD_POT_HARMONIC && kind != GD_POT_SEMISPRING && kind != GD_POT_SPRING) return fail(GD_EINVAL, "gd_add_point_source: unsupported kind");
    if (s->psrc.size() >= GD_MAX_POINT_SOURCES) return fail(GD_EINVAL, "gd_add_point_source: at most %d sources", GD_MAX_POINT_SOURCES);
    PointSource ps; ps.kind = kind; ps.k = k; ps.b = b; memcpy(ps.p, point, sizeof ps.p);
    if (targets) {
        for (uint32_t i = 0; i < nt; i++) if (targets[i] >= s->N) return fail(GD_EINVAL, "gd_add_point_source: target %u out of range", targets[i]);
        ps.mask.assign(s->N, 0);
        for (uint32_t i = 0; i < nt; i++) ps.mask[targets[i]] = 1;
    }
    s->psrc.push_back(std::move(ps));
    s->topo_dirty = true;
    return GD_OK;
}

extern "C" int gd_set_ellipsoid_wall(gd_system *s, const gd_wall *w)
{
    if (!s || !w) return fail(GD_EINVAL, "gd_set_ellipsoid_wall: NULL argument");
    if (!valid_pq(w->p_a, w->q_a) || !valid_pq(w->p_b, w->q_b)) return fail(GD_EINVAL, "gd_set_ellipsoid_wall: unsupported softcore powers");
    for (int k = 0; k < 3; k++) if (!(w->init_semiaxes[k] > 0)) return fail(GD_EINVAL, "gd_set_ellipsoid_wall: semiaxes must be positive");
    s->wall = *w; s->has_wall = true;
    for (auto &c : s->hctx) memcpy(c.semi, w->init_semiaxes, sizeof c.semi);
    s->ctx_dirty = true;
    return GD_OK;
}

// ------------------------------------------------------------- per-replica A/B tables (include/gdyn_ensemble.h)

extern "C" int gd_ensemble_abi_version(void) { return GD_ENSEMBLE_ABI_VERSION; }

extern "C" int gd_ensemble_set_ab(gd_system *s, uint32_t replica, const double *a, const double *b)
{
    if (!s) return fail(GD_EINVAL, "gd_ensemble_set_ab: NULL system");
    if (replica >= s->R) return fail(GD_EINVAL, "gd_ensemble_set_ab: replica %u out of range", replica);
    if (!a && !b) return fail(GD_EINVAL, "gd_ensemble_set_ab: a and b are both NULL");
    if (const size_t bad = s->ens.set(replica, a, b)) return fail(GD_EINVAL, "gd_ensemble_set_ab: non-finite factor at bead %zu", bad - 1);
    // the factors enter the device state in the gather of the next list build and nowhere else: what pos.w carries and the resident
    // list go, and finalize_topology decides again whether the bond records can be mixed on the host
    s->topo_dirty = true; s->list.topology_changed();
    return GD_OK;
}

extern "C" int gd_ensemble_get_ab(gd_system *s, uint32_t replica, double *a, double *b)
{
    if (!s) return fail(GD_EINVAL, "gd_ensemble_get_ab: NULL system");
    if (replica >= s->R) return fail(GD_EINVAL, "gd_ensemble_get_ab: replica %u out of range", replica);
    if (!a && !b) return fail(GD_EINVAL, "gd_ensemble_get_ab: a and b are both NULL");
    s->ens.get(replica, a, b);
    return GD_OK;
}

extern "C" int gd_ensemble_classes(gd_system *s, uint32_t *class_of, uint32_t *n_classes)
{
    if (!s) return fail(GD_EINVAL, "gd_ensemble_classes: NULL system");
    if (!class_of && !n_classes) return fail(GD_EINVAL, "gd_ensemble_classes: class_of and n_classes are both NULL");
    std::vector<uint32_t> c(s->R);
    const uint32_t n = s->ens.classes(c.data());
    if (class_of) std::copy(c.begin(), c.end(), class_of);
    if (n_classes) *n_classes = n;
    return GD_OK;
}

extern "C" int gd_set_inner_sphere_wall(gd_system *s, const gd_inner_sphere *w)
{
    if (!s || !w) return fail(GD_EINVAL, "gd_set_inner_sphere_wall: NULL argument");
    if (!valid_pq(w->p_a, w->q_a) || !valid_pq(w->p_b, w->q_b)) return fail(GD_EINVAL, "gd_set_inner_sphere_wall: unsupported softcore powers");
    if (!(w->radius > 0)) return fail(GD_EINVAL, "gd_set_inner_sphere_wall: radius must be positive");
    s->inner = *w; s->has_inner = true;
    return GD_OK;
}

extern "C" int gd_set_scaling(gd_system *s, double bi, double bt, double oi, double ot)
{
    if (!s) return fail(GD_EINVAL, "gd_set_scaling: NULL system");
    if (!(bt > 0) || !(ot > 0) || !(bi > 0) || !(oi > 0)) return fail(GD_EINVAL, "gd_set_scaling: init and tau must be positive");
    s->has_scaling = true; s->bs_init = bi; s->bs_tau = bt; s->bo_init = oi; s->bo_tau = ot;
    for (auto &c : s->hctx) { c.bead_scale = bi; c.bond_scale = oi; }
    s->ctx_dirty = true; s->list.drop();
    return GD_OK;
}

extern "C" int gd_get_context(gd_system *s, uint32_t r, gd_context *o)
{
    if (!s || !o) return fail(GD_EINVAL, "gd_get_context: NULL argument");
    if (r >= s->R) return fail(GD_EINVAL, "gd_get_context: replica out of range");
    memset(o, 0, sizeof *o);
    const DevCtx &c = s->hctx[r];
    o->step = c.step; o->time = c.time; o->bead_scale = c.bead_scale; o->bond_scale = c.bond_scale;
    memcpy(o->semiaxes, c.semi, sizeof c.semi); memcpy(o->axial_reaction, c.react, sizeof c.react);
    o->list_entries = s->lcount[r]; o->rebuilds = s->rebuilds; o->rollbacks = s->rollbacks;
    o->rebuild_interval = s->pol.K;
    o->callback_pending = c.pending ? 1u : 0u;
    o->compensated = s->comp_last ? 1u : 0u;
    s->list.fill_context(o, s->rebuilds, s->lcount[(size_t)s->R + r], s->pol.last_need_t, (uint64_t)s->R * s->Np);
    return GD_OK;
}

extern "C" int gd_begin_phase(gd_system *s, const double *semi)
{
    if (!s) return fail(GD_EINVAL, "gd_begin_phase: NULL system");
    for (uint32_t r = 0; r < s->R; r++) {
        DevCtx &c = s->hctx[r];
        c.step = 0; c.time = 0; c.pending = 0;
        if (s->has_scaling) { c.bead_scale = s->bs_init; c.bond_scale = s->bo_init; }
        if (semi) memcpy(c.semi, semi + 3 * r, sizeof c.semi);
    }
    s->ctx_dirty = true; s->list.drop();
    return GD_OK;
}

extern "C" int gd_set_context(gd_system *s, uint32_t r, int64_t step, double bead_scale, double bond_scale, const double semi[3])
{
    if (!s) return fail(GD_EINVAL, "gd_set_context: NULL system");
    if (r >= s->R) return fail(GD_EINVAL, "gd_set_context: replica out of range");
    if (!(bead_scale > 0) || !(bond_scale > 0)) return fail(GD_EINVAL, "gd_set_context: scales must be positive");
    DevCtx &c = s->hctx[r];
    c.step = step; c.bead_scale = bead_scale; c.bond_scale = bond_scale; c.pending = 0;
    if (semi) memcpy(c.semi, semi, sizeof c.semi);
    s->ctx_dirty = true; s->list.drop();
    return GD_OK;
}

extern "C" int gd_set_tuning(gd_system *s, const gd_tuning *t)
{
    if (!s || !t) return fail(GD_EINVAL, "gd_set_tuning: NULL argument");
    if (t->kernel_path > 2) return fail(GD_EINVAL, "gd_set_tuning: kernel_path must be 0..2");      // (validated before any state changes)
    if (t->near_fraction < 0 || t->near_fraction > 1) return fail(GD_EINVAL, "gd_set_tuning: near_fraction must be in [0,1]");
    HIPCHK(hipSetDevice(s->device));
    if (s->pol.set_tuning(t->skin, t->rebuild_interval, t->adapt_interval, t->list_width, t->auto_skin != 0 || dev_env("GDYN_AUTO_SKIN")))
        (void)s->nbr.resize(0);
    if (t->near_fraction > 0) s->near_frac = t->near_fraction;
    s->kernel_path = t->kernel_path;
    s->list.drop();
    return GD_OK;
}
extern "C" int gd_get_timing(gd_system *s, gd_timing *o) { if (!s || !o) return fail(GD_EINVAL, "gd_get_timing: NULL"); *o = s->timing; return GD_OK; }
// ---- replica groups of the step launches (include/gdyn_groups.h)
extern "C" int gd_groups_abi_version(void) { return GD_GROUPS_ABI_VERSION; }
extern "C" int gd_set_step_groups(gd_system *s, uint32_t mode)
{
    if (!s) return fail(GD_EINVAL, "gd_set_step_groups: NULL system");
    if (mode > gd::STEP_GROUPS_TWO) return fail(GD_EINVAL, "gd_set_step_groups: mode must be 0 (rule), 1 (one launch) or 2 (two groups wherever results allow)");
    s->group_mode = mode;
    return GD_OK;
}
extern "C" int gd_get_step_groups(gd_system *s, uint32_t *mode, uint32_t *last_groups)
{
    if (!s) return fail(GD_EINVAL, "gd_get_step_groups: NULL system");
    if (mode) *mode = s->group_mode;
    if (last_groups) *last_groups = s->groups_last;
    return GD_OK;
}
// ---- prepared contexts of grouped spans (include/gdyn_prep.h)
extern "C" int gd_prep_abi_version(void) { return GD_PREP_ABI_VERSION; }
extern "C" int gd_get_ctx_prepared(gd_system *s, uint64_t *launches)
{
    if (!s) return fail(GD_EINVAL, "gd_get_ctx_prepared: NULL system");
    if (launches) *launches = s->prep_last;
    return GD_OK;
}
extern "C" int gd_get_stream(gd_system *s, void **st) { if (!s || !st) return fail(GD_EINVAL, "gd_get_stream: NULL"); *st = (void *)s->stream; return GD_OK; }

// --------------------------------------------------------------- topology

static float pair_cutoff(const gd_system *s)
{
    double m = 0;
    if (s->has_pair) {
        if (s->pair.eps_a != 0 && s->pair.sigma_a > m) m = s->pair.sigma_a;
        if (s->pair.eps_b != 0 && s->pair.sigma_b > m) m = s->pair.sigma_b;
    }
    return (float)m;
}

// Flatten the host model into the bead-order device tables (bond adjacency in ELL form,
// bending energies of the three triplets of each bead, point-source masks).
static int finalize_topology(gd_system *s)
{
    if (!s->topo_dirty) return GD_OK;
    HIPCHK(hipSetDevice(s->device));
    const uint32_t N = s->N;
    // bond types: static + dynamic sets
    std::vector<gd_bond_params> types = s->btypes;
    std::vector<int> terms = s->bterm;
    std::vector<Bond> all = s->bonds;
    for (int d = 0; d < 4; d++) if (s->dyn[d].used) {
        if (types.size() >= GD_MAX_BOND_TYPES) return fail(GD_EINVAL, "too many bond parameter sets");
        types.push_back(s->dyn[d].p); terms.push_back(GD_TERM_DYNAMIC);
        const int t = (int)types.size() - 1;
        for (size_t k = 0; k + 1 < s->dyn[d].pairs.size(); k += 2) all.push_back({s->dyn[d].pairs[k], s->dyn[d].pairs[k + 1], t});
    }
    // AB-mixed bond sets (K = a Ka + b Kb, l = a la + b lb with a = (a_i + a_j)/2, b likewise: simulation_driver_forcefield.cc:58-88)
    // have few distinct (a, b) per set -- the bead types are a handful of values -- so every bond gets the index of its own,
    // already mixed, parameter record and the kernels skip the per-bond mixing arithmetic.  More records than the table holds:
    // the sets stay as given and the kernels mix at run time.
    // A handle whose replicas carry different tables (gdyn_ensemble.h) has no one (a, b) per bond: its sets stay as given as well.
    const bool hetero = !s->ens.homogeneous();
    s->bonds_premixed = false;
    if (!hetero) {
        std::vector<gd_bond_params> t2; std::vector<int> term2; std::vector<Bond> all2 = all;
        bool fits = true, any_mixed = false;
        for (auto &b : all2) {
            gd_bond_params q = types[b.type];
            if (q.mix) {
                any_mixed = true;
                const double a = 0.5 * (s->ens.a(0, b.i) + s->ens.a(0, b.j)), bb = 0.5 * (s->ens.b(0, b.i) + s->ens.b(0, b.j));
                q.k_a = a * q.k_a + bb * q.k_b; q.l_a = a * q.l_a + bb * q.l_b; q.k_b = 0; q.l_b = 0; q.mix = 0;
            }
            int found = -1;
            for (size_t k = 0; k < t2.size() && found < 0; k++)
                if (!memcmp(&t2[k], &q, sizeof q) && term2[k] == terms[b.type]) found = (int)k;
            if (found < 0) {
                if (t2.size() >= GD_MAX_BOND_TYPES) { fits = false; break; }
                t2.push_back(q); term2.push_back(terms[b.type]); found = (int)t2.size() - 1;
            }
            b.type = found;
        }
        if (fits && any_mixed) { types.swap(t2); terms.swap(term2); all.swap(all2); s->bonds_premixed = true; }
        else if (!any_mixed) s->bonds_premixed = true;      // nothing to mix at run time either way
    }
    std::vector<unsigned> deg(N, 0);
    for (auto &b : all) { deg[b.i]++; deg[b.j]++; }
    uint32_t WB = 0;
    for (auto v : deg) WB = std::max(WB, v);
    if (WB > 255) return fail(GD_EINVAL, "a bead has %u bonds (max 255)", WB);
    std::vector<unsigned> adj((size_t)std::max(WB, 1u) * N, 0u);
    std::vector<unsigned char> dg(N, 0);
    for (auto &b : all) {
        adj[(size_t)dg[b.i] * N + b.i] = b.j | ((unsigned)b.type << GD_ADJ_SHIFT); dg[b.i]++;
        adj[(size_t)dg[b.j] * N + b.j] = b.i | ((unsigned)b.type << GD_ADJ_SHIFT); dg[b.j]++;
    }
    std::vector<BondType> bt(std::max<size_t>(types.size(), 1));
    s->has_softcore_bonds = false;
    for (size_t i = 0; i < types.size(); i++) {
        const gd_bond_params &p = types[i];
        const bool harmonic = p.kind == GD_POT_HARMONIC;     // U = K r^2 / 2 is the spring with rest length 0
        bt[i] = BondType{(float)p.k_a, (float)p.k_b, harmonic ? 0.f : (float)p.l_a, harmonic ? 0.f : (float)p.l_b,
                         (p.mix ? 1 : 0) | (p.scale_by_bond_scale ? 2 : 0) | (p.minimum_image ? 4 : 0) | (terms[i] << 8),
                         p.kind == GD_POT_SEMISPRING ? 0.f : -3.0e38f, p.kind, p.p | (p.q << 8)};
        if (p.kind == GD_POT_SOFTCORE) s->has_softcore_bonds = true;
    }
    s->bonds_all_scaled = !types.empty();
    for (auto &p : types) if (!p.scale_by_bond_scale) s->bonds_all_scaled = false;
    // bending: energy of the triplet starting at each bead
    std::vector<double> tE(N, 0.0);
    for (auto &br : s->bends)
        for (uint32_t i = br.start; i + 2 < br.end; i++) tE[i] += br.per_bead ? s->bend[i + 1] : br.energy;
    std::vector<float4> bendE(N);
    std::vector<int4> chain(N);
    bool has_bend = false;
    for (uint32_t j = 0; j < N; j++) {
        const float el = j >= 2 ? (float)tE[j - 2] : 0.f, em = j >= 1 ? (float)tE[j - 1] : 0.f, ef = (float)tE[j];
        bendE[j] = make_float4(el, em, ef, 0.f);
        if (el != 0.f || em != 0.f || ef != 0.f) has_bend = true;
        int4 c = make_int4(-1, -1, -1, -1);
        if (el != 0.f) { c.x = (int)j - 2; c.y = (int)j - 1; }
        if (em != 0.f) { c.y = (int)j - 1; c.z = (int)j + 1; }
        if (ef != 0.f) { c.z = (int)j + 1; c.w = (int)j + 2; }
        chain[j] = c;
    }
    std::vector<unsigned char> psm(N, 0);
    for (size_t q = 0; q < s->psrc.size(); q++)
        for (uint32_t i = 0; i < N; i++) if (s->psrc[q].mask.empty() || s->psrc[q].mask[i]) psm[i] |= (unsigned char)(1u << q);
    // the source table of k_scatter's gather: one for the handle, or one per replica
    const uint32_t ab_tables = hetero ? s->R : 1u;
    std::vector<float2> ab((size_t)ab_tables * N);
    std::vector<float> mob(N);
    for (uint32_t r = 0; r < ab_tables; r++)
        for (uint32_t i = 0; i < N; i++) ab[(size_t)r * N + i] = make_float2((float)s->ens.a(r, i), (float)s->ens.b(r, i));
    for (uint32_t i = 0; i < N; i++) mob[i] = (float)s->mob[i];
    // (a,b) ride in pos.w as two fp16 when that is exact (0, .5, 1, 5 ... are) for every replica
    s->packed_ab = s->ens.fp16_exact();
    s->ab_stride = hetero ? N : 0u;

    HIPCHK(s->ab_o.resize(ab.size())); HIPCHK(s->mob_o.resize(N)); HIPCHK(s->bendE_o.resize(N)); HIPCHK(s->psmask_o.resize(N));
    HIPCHK(s->bdeg_o.resize(N)); HIPCHK(s->badj_o.resize(adj.size())); HIPCHK(s->chain_o.resize(N)); HIPCHK(s->btab.resize(GD_MAX_BOND_TYPES));   /* always the full table: k_step stages it with one DMA piece */
    HIPCHK(hipMemcpy(s->ab_o.p, ab.data(), ab.size() * sizeof(float2), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->mob_o.p, mob.data(), N * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->bendE_o.p, bendE.data(), N * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->psmask_o.p, psm.data(), N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->bdeg_o.p, dg.data(), N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->badj_o.p, adj.data(), adj.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->chain_o.p, chain.data(), N * sizeof(int4), hipMemcpyHostToDevice));
    if (bt.size() > GD_MAX_BOND_TYPES) return fail(GD_EINVAL, "too many bond types");
    HIPCHK(hipMemcpy(s->btab.p, bt.data(), bt.size() * sizeof(BondType), hipMemcpyHostToDevice));
    s->n_bond_types = (uint32_t)bt.size();
    const size_t RNp = (size_t)s->R * s->Np;
    const uint32_t WBp = std::max((WB + 3u) & ~3u, 4u);      // adjacency width in entries, chunks of 4
    if (WBp != s->WB || !s->badj.p) { HIPCHK(s->badj.resize((size_t)WBp * RNp)); }
    if (has_bend && !s->chain.p) { HIPCHK(s->chain.resize(RNp)); HIPCHK(s->bendE.resize(RNp)); }
    s->WB = WBp; s->has_bend = has_bend; s->has_bonds = !all.empty();
    s->mob_uniform = (float)s->mob[0];
    for (uint32_t i = 1; i < N; i++) if ((float)s->mob[i] != s->mob_uniform) { s->mob_uniform = -1.f; break; }
    s->mob_max = 0;
    for (uint32_t i = 0; i < N; i++) s->mob_max = std::max(s->mob_max, s->mob[i]);
    s->topo_dirty = false; s->list.topology_changed();
    return GD_OK;
}

// ------------------------------------------------------------ list builds

static double scale_at(const gd_system *s, double init, double tau, double time) { (void)s; return 1.0 - (1.0 - init) * std::exp(-time / tau); }

// Factor of the pair cutoff over the next `ahead` steps: the bead_scale bound (monotone in time) when the pair term scales with it
static double cut_scale(const gd_system *s, const gd_run_desc *run, uint32_t ahead)
{
    if (!s->pair.scale_by_bead_scale) return 1.0;
    double m = 0;
    for (auto &c : s->hctx) {
        m = std::max(m, c.bead_scale);
        if (run && (run->flags & GD_RUN_UPDATE_SCALES) && s->has_scaling)
            m = std::max(m, scale_at(s, s->bs_init, s->bs_tau, (double)(c.step + ahead + 1) * run->timestep));
    }
    return m;
}

static void fill_common(gd_system *s, StepParams &p)
{
    memset(&p, 0, sizeof p);
    p.N = s->N; p.Np = s->Np; p.R = s->R; p.nblk = s->nblk; p.stride = (size_t)s->R * s->Np;
    p.r0 = 0; p.nrep = s->R;      // (all replicas in one launch; gd_run's step groups narrow it, enqueue_chunk)
    set_box(s, p);
    p.pos_in = s->pos[s->pcur].p; p.pos_out = s->pos[s->pcur ^ 1].p; p.xb = s->xb.p; p.orig = s->orig[s->ocur].p;
    p.ab = s->ab.p; p.mob = s->mobs.p; p.bendE = s->bendE.p; p.mob_uniform = s->mob_uniform; p.WB = s->WB;
    p.nbr = s->nbr.p; p.nbr16 = s->nbr16.p; p.wtab = s->wtab.p; p.tiles = s->tiles.p; p.tiled = s->list.tiled ? 1 : 0; p.packed_ab = s->packed_ab ? 1 : 0;
    p.cpb = s->cpb; p.tile_cap = s->list.tiled ? s->list.tile_cap : s->pol.tile_cap;   // as at the build of the list in use
    p.pk = (s->has_pair && s->pair.p_a == 2 && s->pair.q_a == 3 && s->pair.p_b == 8 && s->pair.q_b == 3) ? (s->pair.mix ? 1 : 2) : 0;
    p.meta = s->meta.p; p.rec_x0 = s->rec_x0.p; p.rec_mo = s->rec_mo.p; p.W = s->list.W; p.badj = s->badj.p; p.chain = s->chain.p;
    p.ctx_in = s->ctx[s->ccur].p; p.ctx_out = s->ctx[s->ccur ^ 1].p; p.flags = s->flags.p;
    // wall-reaction partials ping-pong with the context: a launch reads the previous step's partials while its blocks
    // write this step's (one buffer would let late blocks read a mix of two steps)
    p.react_in = s->react_part[s->ccur].p; p.react_out = s->react_part[s->ccur ^ 1].p;
    if (s->has_pair) {
        const gd_pair_softcore &q = s->pair;
        p.pair = PairP{(float)q.eps_a, (float)q.sigma_a, (float)q.eps_b, (float)q.sigma_b, q.p_a, q.q_a, q.p_b, q.q_b,
                       q.mix, q.scale_by_bead_scale, pair_cutoff(s) > 0 ? 1 : 0, pair_cutoff(s)};
    }
    if (s->has_wall) {
        const gd_wall &w = s->wall;
        p.wall.eps_a = (float)w.eps_a; p.wall.sigma_a = (float)w.sigma_a; p.wall.eps_b = (float)w.eps_b; p.wall.sigma_b = (float)w.sigma_b;
        p.wall.p_a = w.p_a; p.wall.q_a = w.q_a; p.wall.p_b = w.p_b; p.wall.q_b = w.q_b;
        p.wall.wall_a = (float)w.wall_a_factor; p.wall.wall_b = (float)w.wall_b_factor; p.wall.scaled = w.scale_by_bead_scale;
        p.wall.enabled = 1; p.wall.packing_spring = (float)w.packing_spring;
        p.wall.fast2383 = (w.p_a == 2 && w.q_a == 3 && w.p_b == 8 && w.q_b == 3) ? 1 : 0;
        for (int k = 0; k < 3; k++) p.wall.spring[k] = w.semiaxes_spring[k];
        p.wall.mobility = w.mobility;
    }
    if (s->has_inner) {
        const gd_inner_sphere &w = s->inner;
        p.wall.inner_enabled = 1; p.wall.in_radius = (float)w.radius;
        p.wall.in_eps_a = (float)w.eps_a; p.wall.in_sigma_a = (float)w.sigma_a; p.wall.in_eps_b = (float)w.eps_b; p.wall.in_sigma_b = (float)w.sigma_b;
        p.wall.in_p_a = w.p_a; p.wall.in_q_a = w.q_a; p.wall.in_p_b = w.p_b; p.wall.in_q_b = w.q_b;
        p.wall.in_wall_a = (float)w.wall_a_factor; p.wall.in_wall_b = (float)w.wall_b_factor; p.wall.in_spring = (float)w.spring;
    }
    p.scaling = ScaleP{s->has_scaling ? 1 : 0, 0, s->bs_init, s->bs_tau, s->bo_init, s->bo_tau, 0.0, 0.0};
    p.btab = s->btab.p; p.nbt = (int)s->n_bond_types; p.has_softcore_bonds = s->has_softcore_bonds ? 1 : 0;
    p.bonds_premixed = s->bonds_premixed ? 1 : 0; p.bonds_all_scaled = s->bonds_all_scaled ? 1 : 0;
    p.nps = (int)s->psrc.size();
    for (int q = 0; q < p.nps; q++) {
        p.ps[q].kind = s->psrc[q].kind; p.ps[q].k = (float)s->psrc[q].k; p.ps[q].b = (float)s->psrc[q].b;
        for (int k = 0; k < 3; k++) p.ps[q].p[k] = (float)s->psrc[q].p[k];
    }
    p.has_bend = s->has_bend; p.has_bonds = s->has_bonds;
    p.rv = s->list.rv; p.rn = post_step_active(s) ? 0.f : s->list.rn; p.dmax = s->dmax.p; p.term_mask = GD_TERM_ALL;      // (a kernel behind k_step moves beads after k_step has bounded their displacement: both list classes then)
    if (dev_env("GDYN_FORCE_FAR")) p.rn = 0.f;      // (timing experiments: the far class in every step)
    if (dev_env("GDYN_FORCE_NEAR")) p.rn = 1e3f;    // (timing experiments with gd_debug_bench only: never the far class -- wrong forces late in an interval)
    p.fout = s->fout.p; p.epart = s->epart.p;
    p.lo = s->lo.p; p.comp = 0;
}

// Enqueue one list build (counting sort into slot order + ELL fill) with radius rv.
static int enqueue_build(gd_system *s, float rv, bool with_list, bool allow_tiled = true)
{
    gd::ListPolicy &pol = s->pol;
    gd::ResidentList::Build built;
    built.rv = rv; built.with_list = with_list; built.packed_ab = s->packed_ab;
    const bool tiled = built.tiled = with_list && allow_tiled && pol.want_tiled(s->kernel_path != 1 && s->packed_ab);
    if (with_list) {
        if (pol.W == 0) pol.W = 96;
        pol.W = (pol.W + GD_UNROLL - 1) & ~(GD_UNROLL - 1);
        // generic lists: uniform rows of W entries (chunked wave-interleaved layout, k_step), grown on demand -- with an eighth to spare
        // once the rows are long -- and given back when a dense transient has passed.  Tiled lists: ragged rows from a pool, below.
        const size_t need = (size_t)pol.W * s->R * s->Np;
        const size_t grow = pol.W >= 512 ? need + need / 8 : need;
        if (!tiled && (s->nbr.n < need || s->nbr.n > 4 * need)) HIPCHK(s->nbr.resize(grow, false));
    }
    built.W = pol.W; built.tile_cap = pol.tile_cap; built.all_near = pol.all_near;
    BuildParams b;
    memset(&b, 0, sizeof b);
    b.N = s->N; b.Np = s->Np; b.R = s->R; b.nblk = s->nblk; b.stride = (size_t)s->R * s->Np;
    set_box(s, b);
    b.rv = rv; b.ncell_cap = s->ncell_cap; b.dmax = s->dmax.p;
    b.kx = b.periodic ? 1 : 2;
    if (const char *e = dev_env("GDYN_KX")) b.kx = b.periodic ? 1 : std::max(1, atoi(e));      // (experiments: cells per list radius in x)
    b.scan_segments = std::min((pol.ncell_seen + pol.ncell_seen / 4 + 8191u) / 8192u, (s->ncell_cap + 8191u) / 8192u);      // (0 before the first build: one block per replica)
    {   // near-class radius: the (look-ahead) cutoff the list radius was derived from, plus a share of the skin
        const float cutb = rv - (float)(pair_cutoff(s) * pol.skin);
        built.rn = b.rn = (cutb > 0.f && cutb < rv && !pol.all_near) ? cutb + (float)s->near_frac * (rv - cutb) : rv;
    }
    b.pos_in = s->pos[s->pcur].p; b.pos_out = s->pos[s->pcur ^ 1].p; b.xb = s->xb.p;
    b.orig_in = s->orig[s->ocur].p; b.orig_out = s->orig[s->ocur ^ 1].p; b.slot_of = s->slot_of.p;
    b.rank = s->rank.p; b.members = s->members.p; b.cell_cnt = s->cell_cnt.p; b.cell_start = s->cell_start.p;
    b.bbox = s->bbox.p; b.grid = s->grid.p;
    b.bbox_cur = s->bbox_enc.p + (size_t)s->list.bbox_cur * s->R * 6; b.bbox_next = s->bbox_enc.p + (size_t)(s->list.bbox_cur ^ 1) * s->R * 6;
    b.warm = (b.periodic || s->list.bbox_valid) ? 1 : 0; b.bbox_w = s->bbox_w.p;
    b.ab_o = s->ab_o.p; b.ab_stride = s->ab_stride; b.mob_o = s->mob_o.p; b.bendE_o = s->bendE_o.p; b.psmask_o = s->psmask_o.p;
    b.badj_o = s->badj_o.p; b.bdeg_o = s->bdeg_o.p; b.chain_o = s->has_bend ? s->chain_o.p : nullptr; b.WB = s->WB;
    b.ab = s->ab.p; b.mob = s->mobs.p; b.bendE = s->bendE.p; b.badj = s->badj.p; b.has_bend = s->has_bend ? 1 : 0;
    b.mob_is_uniform = s->mob_uniform >= 0.f ? 1 : 0;
    b.chain = s->chain.p; b.nbr = (with_list && !tiled) ? s->nbr.p : nullptr; b.nbr16 = tiled ? s->nbr16.p : nullptr;
    b.meta = s->meta.p; b.rec_x0 = s->rec_x0.p; b.rec_mo = s->rec_mo.p; b.len_prev = s->len_prev.p; b.W = pol.W; b.tiles = s->tiles.p; b.tiled = tiled ? 1 : 0;
    b.packed_ab = s->packed_ab ? 1 : 0; b.cpb = s->cpb; b.tile_cap = pol.tile_cap;
    b.w_valid = (s->packed_ab && s->list.w_packed) ? 1 : 0;
    b.flags = s->flags.p; b.lcount = s->lcount_d.p; b.dbg = (unsigned long long *)s->fout.p;
    b.wtab = s->wtab.p; b.need_prev = s->need_prev.p; b.pool = s->pool.p; b.rqueue = s->rqueue.p; b.rq_cap = (unsigned)s->rqueue.n; b.rq_grid = pol.repair_wide > 0 ? b.rq_cap : std::min(GD_REPAIR_GRID, b.rq_cap);
    if (tiled) {
        // Ragged rows (BuildParams): every k_step wave's rows are as wide as its longest list, predicted from what each bead needed at
        // the build before (no history -- first build, positions from the caller, another list radius or class mode: W entries per
        // bead) and repaired inside k_fill where a list outgrows the prediction.  The pool (nbr16) is sized from the use of the last
        // build with an eighth + a KiB per wave to spare (the use is read back with every chunk; the builds in between grow with the
        // lists); a pool that turns out too small is flagged, its cursor has counted the need, and the chunk is rolled back.
        const size_t waves = (size_t)s->R * s->Np / 64;
        const bool predict = built.predicted = s->list.predicts(rv, pol.all_near);
        auto pool_kib = [&]() { return (size_t)(s->nbr16.n / 512); };
        const gd::PoolPlan plan = gd::plan_pool(s->list.pool_used, pool_kib(), waves, pol.W, predict);      // (the rule: gdyn_policy.hpp)
        if (plan.resize) HIPCHK(s->nbr16.resize(plan.alloc_kib * 512, false));      // (not preserved: the list in it is about to be rebuilt)
        if (dev_env("GDYN_DEBUG") && dev_env("GDYN_DEBUG")[0] == '2')
            fprintf(stderr, "[gdyn] build %llu: %s, rows used %u KiB, pool %zu KiB, rv %.4f\n", (unsigned long long)s->rebuilds, predict ? "predicted" : "no history", s->list.pool_used, pool_kib(), rv);
        built.pool_guess = (uint32_t)std::min<size_t>(plan.used, 0xffffffffu);
        b.predict = predict ? 1 : 0; b.nbr16 = s->nbr16.p; b.pool_cap = (unsigned)std::min<size_t>(pool_kib(), 0xffffffffu);
        // k_fill orders k_step's threads by len_prev, and the order decides the last digits of a block's wall-reaction partial: a key
        // left by a refused build, or by another state of the handle, is cleared (threads in slot order, as in a handle's first build)
        if (!s->list.orders_by_history()) HIPCHK(hipMemsetAsync(s->len_prev.p, 0, s->len_prev.n, s->stream));
    }
    s->list.build_enqueued(built);
    gd_launch_build(b, s->stream);
    s->pcur ^= 1; s->ocur ^= 1;
    s->rebuilds++;
    s->timing.rebuild_launches++;
    return GD_OK;
}

static int clear_flags(gd_system *s)
{
    HIPCHK(hipMemsetAsync(s->flags.p, 0, (size_t)s->R * GD_NFLAGS * sizeof(unsigned), s->stream));
    HIPCHK(hipMemsetAsync(s->pool.p + 1, 0, 2 * sizeof(unsigned), s->stream));      // the row pool's largest use and repair count of the builds to come
    return GD_OK;
}

// The list in use and the handle, as the list policy sees them
static gd::ListState list_state(const gd_system *s)
{
    return s->list.state(pair_cutoff(s), s->nbr16.n / 512, (double)s->R * (double)s->Np, post_step_active(s), s->kernel_path != 1 && s->packed_ab);
}

// A build or a chunk of gd_run: what it ran and the state before it (gd_run), what the device reported (read_chunk)
struct Chunk {
    int64_t steps = 0;
    bool full_interval = false, on_search_list = false;      // it holds the last step of a complete K-step interval / began on a search list
    std::vector<DevCtx> snap_ctx; bool snap_w_packed = false;      // the context before it, what pos.w carried then
    std::vector<std::pair<size_t, int>> spans; size_t ev_end = 0;      // (end event, kind: 0 step, 1 build) of each span; the chunk's end event
    gd::BuildReport rep; std::vector<DevCtx> ctx; float dmax2 = 0;      // flags, contexts and largest displacement bound read back
};

// One round trip for everything the host wants from a build or a chunk: flags, contexts, list counts, the running displacement bound
// of every replica (tiled path, one word per 128-byte line: it covers the positions the last step WROTE, which no step has checked
// yet) and the row pool's use (the list counts and the pool's use go to the handle)
static int read_chunk(gd_system *s, Chunk &c)
{
    HIPCHK(hipGetLastError());
    const size_t nf = (size_t)s->R * GD_NFLAGS * sizeof(unsigned), nc = s->R * sizeof(DevCtx), nl = 2 * (size_t)s->R * sizeof(unsigned long long), nd = s->R * sizeof(float);
    HIPCHK(s->h_chunk.ensure(nf + nc + nl + nd + 16));
    HIPCHK(hipMemcpyAsync(s->h_chunk.p + nf + nc + nl + nd, s->pool.p, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(s->h_chunk.p, s->flags.p, nf, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(s->h_chunk.p + nf, s->ctx[s->ccur].p, nc, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(s->h_chunk.p + nf + nc, s->lcount_d.p, nl, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpy2DAsync(s->h_chunk.p + nf + nc + nl, sizeof(float), s->dmax.p, GD_DMAX_STRIDE * sizeof(unsigned), sizeof(float), s->R,
                            hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    c.rep = gd::summarize((const unsigned *)s->h_chunk.p, s->R);
    c.ctx.resize(s->R); memcpy(c.ctx.data(), s->h_chunk.p + nf, nc); memcpy(s->lcount.data(), s->h_chunk.p + nf + nc, nl);
    c.dmax2 = 0; for (uint32_t r = 0; r < s->R; r++) { float d2; memcpy(&d2, s->h_chunk.p + nf + nc + nl + r * sizeof(float), 4); c.dmax2 = std::max(c.dmax2, d2); }
    unsigned used[4]; memcpy(used, s->h_chunk.p + nf + nc + nl + nd, 16);
    s->list.chunk_read(used);
    if (c.rep.tile_over && dev_env("GDYN_DEBUG")) {      // (developer builds: the grids of a tile overflow)
        std::vector<GridP> gp(s->R);
        (void)hipMemcpy(gp.data(), s->grid.p, s->R * sizeof(GridP), hipMemcpyDeviceToHost);
        for (uint32_t r = 0; r < std::min(s->R, 3u); r++)
            fprintf(stderr, "[gdyn] grid r%u: nc %d %d %d ncell %d org %g %g %g inv %g flags need_t %u\n", r, gp[r].nc[0], gp[r].nc[1], gp[r].nc[2],
                    gp[r].ncell, gp[r].org[0], gp[r].org[1], gp[r].org[2], gp[r].inv[0], ((const unsigned *)s->h_chunk.p)[r * GD_NFLAGS + GD_FLAG_NEED_TILE]);
    }
    return GD_OK;
}

// Synchronous build used outside gd_run: grows the list width until nothing overflows.
static int build_now(gd_system *s, float rv, bool with_list, bool allow_tiled = true, float rv_min = 0.f)
{
    const double skin0 = s->pol.skin;
    Chunk c;
    for (int attempt = 0; attempt < 10; attempt++) {
        GDCHK(clear_flags(s));
        // (a retry after the dense guard has narrowed the width builds at the narrowed radius -- not below what the caller needs
        // the list to cover, rv_min: a pair search at a contact distance beyond the force cutoff)
        const float rv_try = std::max(rv_min, rv - (float)(pair_cutoff(s) * (skin0 - s->pol.skin)));
        GDCHK(enqueue_build(s, rv_try, with_list, allow_tiled));
        GDCHK(read_chunk(s, c));
        if (!s->pol.on_report(list_state(s), c.rep)) return clear_flags(s);
        s->list.build_refused();
    }
    return fail(GD_ENOMEM, "neighbour list width did not converge (W=%u)", s->pol.W);
}

int prepare(gd_system *s)
{
    HIPCHK(hipSetDevice(s->device));
    GDCHK(finalize_topology(s));
    GDCHK(upload_ctx(s));
    GDCHK(sync_replica_pairs(s));
    return GD_OK;
}

static float list_radius(gd_system *s, const gd_run_desc *run, uint32_t ahead)
{
    const float cut = pair_cutoff(s);
    if (!(cut > 0)) return 1.0f;
    const double sc = cut_scale(s, run, ahead);
    // the skin is an absolute width, `skin` x the NOMINAL cutoff: with a scaled-down cutoff (bead_scale < 1 early in the
    // interphase run, simulation_driver_forcefield.cc:47-49) the displacement budget (rv - cutoff) / 2, and with it the
    // rebuild interval, stays what it is at full scale
    return (float)(cut * (sc + s->pol.skin));
}

static int ensure_fresh_list(gd_system *s)
{
    if (s->list.fresh(s->state_serial)) return GD_OK;
    s->pol.take_pending_skin(pair_cutoff(s));
    GDCHK(build_now(s, list_radius(s, nullptr, 0), pair_cutoff(s) > 0));
    s->list.enter_use(false);
    return GD_OK;
}

// ---------------------------------------------------------------- stepping

static hipEvent_t get_event(gd_system *s, size_t i)
{
    // (timing events only: no system-scope fence when one is recorded -- the cache write-back and invalidation of the default event
    // idle the device for ~5 us between the kernels on either side; what the host reads of a chunk it reads behind hipStreamSynchronize)
    while (s->events.size() <= i) { hipEvent_t e; if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr; s->events.push_back(e); }
    return s->events[i];
}

// The state updates a GD_RUN_DEFER_CALLBACK run left pending: one k_ctx launch with that run's timestep and flags (the wall-reaction
// partials of its last step are still the current ones), then the host mirror.
static int apply_pending(gd_system *s)
{
    bool any = false;
    for (auto &c : s->hctx) any |= c.pending != 0;
    if (!any) return GD_OK;
    HIPCHK(hipSetDevice(s->device));
    GDCHK(upload_ctx(s));
    StepParams p;
    fill_common(s, p);
    p.dt_d = s->pend_dt; p.dt = (float)s->pend_dt; p.run_flags = s->pend_flags;
    bool common = s->has_scaling && (s->pend_flags & GD_RUN_UPDATE_SCALES);
    for (uint32_t r = 1; r < s->R && common; r++) common = s->hctx[r].step == s->hctx[0].step && s->hctx[r].pending == s->hctx[0].pending;
    if (common) {      // same libm exp as a callback applied inside gd_run (see host_scales there)
        const double time = (double)(s->hctx[0].step + 1) * s->pend_dt;
        p.scaling.from_host = 1;
        p.scaling.bead_next = scale_at(s, s->bs_init, s->bs_tau, time);
        p.scaling.bond_next = scale_at(s, s->bo_init, s->bo_tau, time);
    }
    gd_launch_finalize(p, 0, s->stream);
    s->ccur ^= 1;
    GDCHK(download_ctx(s));
    s->state_serial++;
    return GD_OK;
}

// Whether a run steps with the compensated position update (k_step's p.comp).  The increment of a step is mu F dt + sigma xi with
// sigma = sqrt(2 mu kT dt); once sigma is within a few dozen ulp of an fp32 coordinate -- always at T = 0 -- the rounding of x + dx is no
// longer small against what a step adds, and summed over a run it is a systematic loss (simulation_fine_sampling: T = 0, dt = 1e-7; an
// fp32 coordinate of 3 ... 8 has an ulp of 2.4e-7 ... 4.8e-7).  Criterion: sigma < 64 ulp(X), X the coordinate range (largest wall
// semiaxis / box period; 16 when the model has neither).  GD_RUN_COMPENSATED / GD_RUN_UNCOMPENSATED override it.
static bool want_compensated(const gd_system *s, const gd_run_desc *run)
{
    if (run->flags & GD_RUN_UNCOMPENSATED) return false;
    if (run->flags & GD_RUN_COMPENSATED) return true;
    double X = 0;
    if (s->has_wall) for (auto &c : s->hctx) for (int k = 0; k < 3; k++) X = std::max(X, c.semi[k]);
    if (s->box_kind == GD_BOX_PERIODIC) for (int k = 0; k < 3; k++) X = std::max(X, s->box[k]);
    if (!(X > 0)) X = 16.0;
    const double ulp = std::ldexp(1.0, std::ilogb(X) - 23), sigma = std::sqrt(2.0 * s->mob_max * run->temperature * run->timestep);
    return sigma < 64.0 * ulp;
}

extern "C" int gd_apply_callback(gd_system *s)
{
    if (!s) return fail(GD_EINVAL, "gd_apply_callback: NULL system");
    return apply_pending(s);
}

// Replica groups (gd::step_group_split, gdyn_policy.hpp): group B's launches of a span go to a second stream that is forked off the
// handle's stream by an event in front of the span and joined to it by one behind, ahead of the span's end event -- so the span's
// time covers both groups, and everything behind the span (builds, finalize, readback, the caller's own work on gd_get_stream) sees one
// stream as before.  Between fork and join only kernels are launched: no call in there can return early and leave the streams apart.
static int fork_groups(gd_system *s)
{
    if (!s->stream2) HIPCHK(hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking));
    if (!s->grp_fork) HIPCHK(hipEventCreateWithFlags(&s->grp_fork, hipEventDisableTiming));
    if (!s->grp_join) HIPCHK(hipEventCreateWithFlags(&s->grp_join, hipEventDisableTiming));
    HIPCHK(hipEventRecord(s->grp_fork, s->stream));
    HIPCHK(hipStreamWaitEvent(s->stream2, s->grp_fork, 0));
    return GD_OK;
}
static int join_groups(gd_system *s)
{
    hipError_t e = hipEventRecord(s->grp_join, s->stream2);
    if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, s->grp_join, 0);
    if (e != hipSuccess) {      // (no event to wait on: the host waits for group B, so that the streams are joined on this way out too)
        (void)hipStreamSynchronize(s->stream2);
        return fail(GD_EHIP, "gd_run: joining the step groups failed: %s", hipGetErrorString(e));
    }
    return GD_OK;
}

static gd::StepGroupState group_state(const gd_system *s, bool host_noise)
{
    gd::StepGroupState st;
    st.R = s->R; st.nblk = s->nblk; st.tiled = s->list.valid && s->list.tiled; st.post_step = post_step_active(s);
    st.device_noise = !host_noise; st.whole_replica_map = s->cpb == 0;
    st.fast_pair = s->has_pair && s->pair.p_a == 2 && s->pair.q_a == 3 && s->pair.p_b == 8 && s->pair.q_b == 3;      // (fill_common's pk != 0)
    return st;
}

static int enqueue_chunk(gd_system *s, const gd_run_desc *run, int64_t done, bool comp, bool host_noise, Chunk &c)
{
    const size_t RN = (size_t)s->R * s->N;
    const bool with_list = pair_cutoff(s) > 0;
    const int64_t chunk = c.steps = s->pol.chunk_steps(run->steps - done);
    // snapshot for rollback: positions in bead order + context
    gd_launch_gather_positions(s->pos[s->pcur].p, s->slot_of.p, s->snap.p, s->N, s->Np, s->R, 0, s->stream);
    if (comp) HIPCHK(hipMemcpyAsync(s->snap_lo.p, s->lo.p, RN * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    c.snap_ctx = s->hctx; c.snap_w_packed = s->list.w_packed;
    GDCHK(clear_flags(s));
    StepParams p;
    // The scales a callback sets are pure functions of the step index (simulation_driver_interphase.cc:42-43): when every
    // replica is at the same step (the usual case) the host evaluates them and passes them with the launch
    bool common_step = s->has_scaling && (run->flags & GD_RUN_UPDATE_SCALES);
    const long long step0 = s->hctx[0].step;
    for (uint32_t r = 1; r < s->R && common_step; r++) common_step = s->hctx[r].step == step0;
    auto host_scales = [&](StepParams &q, int64_t launch) {      // launch: index within the chunk of the launch that applies the callback
        if (!common_step) return;
        const double time = (double)(step0 + launch) * run->timestep;
        q.scaling.from_host = 1;
        q.scaling.bead_next = scale_at(s, s->bs_init, s->bs_tau, time);
        q.scaling.bond_next = scale_at(s, s->bo_init, s->bo_tau, time);
    };
    size_t nev = 0;
    // Spans of step launches and of builds share their boundary events: the end of one is the start of the next (an event in the
    // stream costs the device ~5 us between two kernels: 10-12 us across the two that used to separate a build from the steps)
    HIPCHK(hipEventRecord(get_event(s, nev++), s->stream));
    int64_t k = 0;
    // (an interval that runs on a contact-search list has a wider skin than the force lists: its displacement is no measure
    // for the interval of those)
    c.on_search_list = s->list.valid && s->list.search_list;
    while (k < chunk) {
        if (!s->list.valid || s->list.steps_since_build >= s->pol.K) {
            s->pol.take_pending_skin(pair_cutoff(s));
            hipEvent_t e1 = get_event(s, nev++);
            GDCHK(enqueue_build(s, list_radius(s, run, (uint32_t)(k + s->pol.K)), with_list));
            s->list.enter_use(false);
            HIPCHK(hipEventRecord(e1, s->stream));
            c.spans.push_back({nev - 1, 1});
        }
        const int64_t n = std::min<int64_t>((int64_t)s->pol.K - s->list.steps_since_build, chunk - k);
        hipEvent_t e1 = get_event(s, nev++);
        // replicas of group A of this span's launches (0: one launch per step), decided on the list in use
        uint32_t min_blocks = gd::STEP_GROUPS_MIN_BLOCKS, a16 = gd::STEP_GROUPS_A16;
        if (const char *e = dev_env("GDYN_GROUP_MIN_BLOCKS")) min_blocks = (uint32_t)atoi(e);      // (timing experiments)
        if (const char *e = dev_env("GDYN_GROUP_A16")) a16 = (uint32_t)atoi(e);
        const uint32_t ra = gd::step_group_split(s->group_mode, group_state(s, host_noise), min_blocks, a16);
        // ... and whether its steps run on prepared contexts: k_ctx_prep -> k_step on each group's stream (gd::ctx_prepared)
        uint32_t prep_mode = gd::CTX_PREP_RULE, prep_min_blocks = gd::CTX_PREP_MIN_BLOCKS;
        if (const char *e = dev_env("GDYN_CTX_PREP")) prep_mode = (uint32_t)atoi(e);                   // (the threshold table: 0 never, 1 the rule, 2 every grouped span)
        if (const char *e = dev_env("GDYN_CTX_PREP_MIN_BLOCKS")) prep_min_blocks = (uint32_t)atoi(e);
        const bool prepared = gd::ctx_prepared(s->group_mode, ra, group_state(s, host_noise), prep_mode, prep_min_blocks);
        if (ra) { GDCHK(fork_groups(s)); s->groups_last = 2; }
        for (int64_t q = 0; q < n; q++) {
            fill_common(s, p);
            p.dt_d = run->timestep; p.dt = (float)run->timestep; p.kT = (float)run->temperature; p.seed = run->seed;
            p.seeds = run->replica_seeds ? s->seeds_d.p : nullptr;
            p.noise_mode = run->noise_mode; p.run_flags = run->flags; p.comp = comp ? 1 : 0;
            p.host_noise = host_noise ? s->noise.p + (size_t)(done + k + q) * RN * 3 : nullptr;
            host_scales(p, k + q);
            // the interval adaptation needs the displacement at K steps since the build: recorded at the last force
            // evaluation of a COMPLETE interval only (a chunk that ends mid-interval records nothing and adapts nothing)
            p.record_disp = (s->list.steps_since_build + (uint32_t)q + 1u == s->pol.K);
            c.full_interval |= p.record_disp != 0;
            if (ra) {      // (same parameters, same buffers: the groups differ in the replicas they cover)
                if (prepared) p.ctxf = s->ctxf.p;
                p.r0 = 0; p.nrep = ra;
                if (prepared) gd_launch_ctx_prep(p, s->stream);
                gd_launch_step(p, GD_MODE_STEP, s->stream);
                p.r0 = ra; p.nrep = s->R - ra;
                if (prepared) gd_launch_ctx_prep(p, s->stream2);
                gd_launch_step(p, GD_MODE_STEP, s->stream2);
                if (prepared) s->prep_last += 2;
            } else gd_launch_step(p, GD_MODE_STEP, s->stream);
            if (s->sw.n) launch_softwell(s, p, 0);
            if (s->rp.any()) launch_replica_pairs(s, p, 0);      // (a step evaluates every term: GD_TERM_DYNAMIC is in its mask)
            s->pcur ^= 1; s->ccur ^= 1;
        }
        if (ra) GDCHK(join_groups(s));
        HIPCHK(hipEventRecord(e1, s->stream));
        c.spans.push_back({nev - 1, 0});
        s->timing.step_launches += (uint64_t)n;
        s->list.stepped((uint32_t)n);
        k += n;
    }
    // apply the callback of the last step (unless the caller wants to observe the state its callback sees first)
    const bool defer = (run->flags & GD_RUN_DEFER_CALLBACK) && done + chunk == run->steps;
    if (!defer) {
        fill_common(s, p);
        p.dt_d = run->timestep; p.dt = (float)run->timestep; p.run_flags = run->flags;
        host_scales(p, chunk);
        gd_launch_finalize(p, 0, s->stream);
        s->ccur ^= 1;
    } else {
        s->pend_dt = run->timestep; s->pend_flags = run->flags;
        // axial_reaction is that of the last step's force evaluation, as an observer of the deferred state reads it: folded into the
        // context IN PLACE (one wave per replica reads and writes its own entry), so that context and partials do not swap sides and
        // the pending callback still finds the last step's partials where it reads them
        if (s->has_wall) {
            fill_common(s, p);
            p.ctx_out = s->ctx[s->ccur].p;
            gd_launch_finalize(p, 1, s->stream);
        }
    }
    c.ev_end = nev;
    HIPCHK(hipEventRecord(get_event(s, nev++), s->stream));
    return GD_OK;
}

// Roll a chunk back to the positions, residuals and context before it, without a list.  Every cause of a rollback changes what the
// retry runs with, so a chunk converges in a few attempts; one that does not is a defect, reported from the restored state.
static int rollback_chunk(gd_system *s, const Chunk &c, bool over, bool comp, int retries)
{
    const size_t RN = (size_t)s->R * s->N;
    s->rollbacks++;
    HIPCHK(hipMemcpy2DAsync(s->pos[s->pcur].p, (size_t)s->Np * sizeof(float4), s->snap.p, (size_t)s->N * sizeof(float4),
                            (size_t)s->N * sizeof(float4), s->R, hipMemcpyDeviceToDevice, s->stream));
    gd_launch_identity(s->orig[s->ocur].p, s->slot_of.p, s->N, s->Np, s->R, s->stream);
    if (comp) HIPCHK(hipMemcpyAsync(s->lo.p, s->snap_lo.p, RN * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    s->hctx = c.snap_ctx; s->ctx_dirty = true; s->list.rolled_back(c.snap_w_packed);
    GDCHK(upload_ctx(s));
    s->pol.hold_for_retries();      // (the width and the interval before the chunk's first rollback: a chunk given up returns them)
    if (retries > 24) {
        s->pol.retries_over(true);
        return fail(GD_ESTATE, "gd_run: a chunk of %lld steps at step %lld was rolled back %d times (%s): giving up",
                    (long long)c.steps, (long long)s->hctx[0].step, retries, over ? "list / tile / pool overflow" : "skin violation");
    }
    if (dev_env("GDYN_DEBUG")) fprintf(stderr, "[gdyn] rollback %llu: %s, K %u, skin %.3f, chunk of %lld steps at step %lld\n", (unsigned long long)s->rollbacks,
                                       over ? "overflow" : "skin violation", s->pol.K, s->pol.skin, (long long)c.steps, (long long)s->hctx[0].step);
    if (c.rep.violated && !over && !s->pol.on_violation()) {
        s->pol.retries_over(true);
        return fail(GD_ESTATE, "gd_run: Verlet skin cannot cover one step (timestep too large?)");
    }
    s->timing.step_launches -= std::min<uint64_t>(s->timing.step_launches, (uint64_t)c.steps);
    s->pol.on_rollback(post_step_active(s));
    return GD_OK;
}

// Accept a chunk: timing, context mirror, then the policy (tiled-path back-off, interval adaptation, skin, repair width)
static int accept_chunk(gd_system *s, const gd_run_desc *run, const Chunk &c)
{
    float ms = 0, step_ms = 0, build_ms = 0;
    for (auto &sp : c.spans) {
        HIPCHK(hipEventElapsedTime(&ms, s->events[sp.first - 1], s->events[sp.first]));
        (sp.second ? build_ms : step_ms) += ms;
    }
    HIPCHK(hipEventElapsedTime(&ms, s->events[0], s->events[c.ev_end]));
    s->timing.total_ms += ms; s->timing.step_kernel_ms += step_ms; s->timing.rebuild_ms += build_ms;
    s->hctx = c.ctx;
    unsigned long long L = 0; for (uint32_t r = 0; r < s->R; r++) L += s->lcount[r];
    s->timing.list_entries_visited += L * (uint64_t)c.steps;   // L of the last build, per step
    const gd::Accepted a{ms, c.steps, c.rep.maxd2, cut_scale(s, nullptr, 0), c.full_interval, c.on_search_list};
    if (s->pol.on_accepted(list_state(s), a, [&](uint32_t ahead) { return cut_scale(s, run, ahead); })) s->list.drop();
    return GD_OK;
}

extern "C" int gd_run(gd_system *s, const gd_run_desc *run)
{
    if (!s || !run) return fail(GD_EINVAL, "gd_run: NULL argument");
    if (run->spacestep != 0) return fail(GD_EUNSUPPORTED, "gd_run: spacestep != 0 (adaptive timestep) is not supported");
    if (run->steps < 0 || !(run->timestep > 0) || run->temperature < 0) return fail(GD_EINVAL, "gd_run: bad steps/timestep/temperature");
    if (run->noise_mode < 0 || run->noise_mode > GD_NOISE_HOST)
        return fail(run->noise_mode == 3 ? GD_EUNSUPPORTED : GD_EINVAL, "gd_run: noise_mode %d not available on the device", run->noise_mode);
    if (run->noise_mode == GD_NOISE_HOST && !run->host_noise) return fail(GD_EINVAL, "gd_run: host noise requested without array");
    if ((run->flags & GD_RUN_WALL_DYNAMICS) && !s->has_wall) return fail(GD_ESTATE, "gd_run: wall dynamics requested without a wall");
    if ((run->flags & GD_RUN_UPDATE_SCALES) && !s->has_scaling) return fail(GD_ESTATE, "gd_run: scale updates requested without gd_set_scaling");
    GDCHK(prepare(s));
    GDCHK(apply_pending(s));
    s->state_serial++;
    if (run->timestep != s->last_dt || run->temperature != s->last_kT) { s->pol.a2_ema = 0; s->last_dt = run->timestep; s->last_kT = run->temperature; }   // another regime: measure afresh
    // The wall or the scales start (or stop) moving with this run -- a relaxation is followed by the production phase: the
    // displacement statistics the interval was adapted on are those of the other regime, and the first intervals of the new one used
    // to end in a rolled-back chunk every few runs (bench.py: flags 0 for the relaxation, wall dynamics + scale updates after it).
    // A fifth off the interval until complete intervals of the new regime have been measured.
    if (s->pol.adapt && s->pol.K > 4 && ((run->flags ^ s->last_flags) & (GD_RUN_WALL_DYNAMICS | GD_RUN_UPDATE_SCALES)) != 0 && s->rebuilds > 0)
        s->pol.K -= s->pol.K / 5;
    s->last_flags = run->flags;
    const bool with_list = pair_cutoff(s) > 0;
    const size_t RN = (size_t)s->R * s->N;
    memset(&s->timing, 0, sizeof s->timing);
    s->groups_last = 1; s->prep_last = 0;

    // injected noise lives on the device as float (R,N,3) per step
    const bool host_noise = run->noise_mode == GD_NOISE_HOST && run->temperature > 0;
    if (host_noise) {
        const size_t n = (size_t)run->steps * RN * 3;
        std::vector<float> h(n);
        for (size_t i = 0; i < n; i++) h[i] = (float)run->host_noise[i];
        HIPCHK(s->noise.resize(n, false));
        HIPCHK(hipMemcpy(s->noise.p, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }

    const bool comp = run->steps > 0 && want_compensated(s, run);
    if (comp) {
        if (!s->lo_valid) { HIPCHK(hipMemsetAsync(s->lo.p, 0, RN * sizeof(float4), s->stream)); s->lo_valid = true; }
        HIPCHK(s->snap_lo.resize(RN, false));
    }
    if (run->steps > 0) s->comp_last = comp;
    if (run->steps > 0 && !comp) s->lo_valid = false;      // the positions are about to move without their residuals (set here, not on the way
                                                          // out: an early error return must not leave residuals that describe other positions)

    if (run->replica_seeds) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "seed width");
        HIPCHK(s->seeds_d.resize(s->R, false));
        HIPCHK(hipMemcpy(s->seeds_d.p, run->replica_seeds, s->R * sizeof(uint64_t), hipMemcpyHostToDevice));
    }

    int64_t done = 0;
    int retries = 0;           // consecutive rollbacks of the chunk in progress
    s->pol.retries_over(false);      // (a run that ended on a device error between two rollbacks holds nothing for this one)
    float last_dmax2 = 0;      // largest bound, over the replicas, of the squared displacement since the build of the positions the last accepted chunk WROTE
    while (done < run->steps) {
        Chunk c;
        GDCHK(enqueue_chunk(s, run, done, comp, host_noise, c));
        GDCHK(read_chunk(s, c));
        const bool over = s->pol.on_report(list_state(s), c.rep);
        if (c.rep.violated || over) { GDCHK(rollback_chunk(s, c, over, comp, ++retries)); continue; }
        s->pol.retries_over(false);      // (accepted: what the retries arrived at stays)
        GDCHK(accept_chunk(s, run, c));
        done += c.steps; retries = 0; last_dmax2 = c.dmax2;
    }
    // The last chunk was accepted: every bead is within the margin the list in use was built for, at the cutoff of the last step --
    // still the cutoff an observation sees when the scales did not move behind that step (callback deferred, or no scale updates):
    // the resident list then serves gd_compute_energy as it is (not with a kernel behind k_step -- the droplet term, the per-replica
    // pairs: it moves beads behind k_step's check).  The positions the last step WROTE are covered by the running bound of the tiled path (dmax, read back with the chunk)
    // only: the list serves an observation if that bound is inside the margin too.  The generic path's observations build a list.
    const bool settled = run->steps > 0 && with_list && !post_step_active(s) && (!(run->flags & GD_RUN_UPDATE_SCALES) || (run->flags & GD_RUN_DEFER_CALLBACK));
    s->list.run_ended(settled, pair_cutoff(s) * cut_scale(s, nullptr, 0), last_dmax2, s->state_serial);
    return GD_OK;
}

// ------------------------------------------------------------- observation

extern "C" int gd_compute_energy(gd_system *s, uint32_t mask, double *energy)
{
    if (!s || !energy) return fail(GD_EINVAL, "gd_compute_energy: NULL argument");
    GDCHK(prepare(s));
    GDCHK(ensure_fresh_list(s));
    StepParams p;
    fill_common(s, p);
    p.term_mask = mask;
    gd_launch_step(p, GD_MODE_ENERGY, s->stream);
    const bool droplet = s->sw.n && (mask & GD_TERM_PAIR);
    const bool replica_pairs = s->rp.any() && (mask & GD_TERM_DYNAMIC);
    std::vector<double> esw(s->R, 0.0), erp(s->R, 0.0);
    if (replica_pairs) {
        HIPCHK(hipMemsetAsync(s->rp_up.esum.p, 0, s->R * sizeof(double), s->stream));
        launch_replica_pairs(s, p, 2);
        HIPCHK(hipMemcpyAsync(erp.data(), s->rp_up.esum.p, s->R * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    if (droplet) {
        HIPCHK(hipMemsetAsync(s->sw.esum.p, 0, s->R * sizeof(double), s->stream));
        launch_softwell(s, p, 2);
        HIPCHK(hipMemcpyAsync(esw.data(), s->sw.esum.p, s->R * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    std::vector<double> part((size_t)s->R * s->nblk);
    HIPCHK(hipMemcpyAsync(part.data(), s->epart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (uint32_t r = 0; r < s->R; r++) {
        double e = esw[r] + erp[r];
        for (uint32_t b = 0; b < s->nblk; b++) e += part[(size_t)r * s->nblk + b];
        energy[r] = e;
    }
    return GD_OK;
}

extern "C" int gd_compute_forces(gd_system *s, uint32_t mask, double *forces)
{
    if (!s || !forces) return fail(GD_EINVAL, "gd_compute_forces: NULL argument");
    GDCHK(prepare(s));
    GDCHK(apply_pending(s));      // a force evaluation replaces the wall-reaction partials: the pending callback consumes its own first
    GDCHK(ensure_fresh_list(s));
    StepParams p;
    fill_common(s, p);
    p.term_mask = mask;
    HIPCHK(hipMemsetAsync(p.react_out, 0, s->react_part[0].n * sizeof(float4), s->stream));
    gd_launch_step(p, GD_MODE_FORCE, s->stream);
    if (s->sw.n && (mask & GD_TERM_PAIR)) launch_softwell(s, p, 1);
    if (s->rp.any() && (mask & GD_TERM_DYNAMIC)) launch_replica_pairs(s, p, 1);
    // (a mask without the wall leaves axial_reaction as the last evaluation of the wall set it: no fold of the zeroed partials)
    const bool fold = s->has_wall && (mask & GD_TERM_WALL);
    if (fold) { p.react_in = p.react_out; gd_launch_finalize(p, 1, s->stream); s->ccur ^= 1; }
    const size_t RN = (size_t)s->R * s->N;
    std::vector<float4> h(RN);
    HIPCHK(hipMemcpyAsync(h.data(), s->fout.p, RN * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < RN; i++) { forces[3 * i] = h[i].x; forces[3 * i + 1] = h[i].y; forces[3 * i + 2] = h[i].z; }
    if (fold) GDCHK(download_ctx(s));
    return GD_OK;
}

// Pairs within dcut of replicas r0 .. r0 + nrep - 1, one launch: replica r0 + y's pairs at out + y * (out.n / nrep), their number in
// cnt[2 y] (and left on the device in `count`).  The buffer grows until every replica fits.
int search_device(gd_system *s, uint32_t r0, uint32_t nrep, double dcut, gd::dbuf<uint2> &out, gd::dbuf<unsigned long long> &count,
                  std::vector<unsigned long long> &cnt)
{
    const bool with_list = pair_cutoff(s) > 0;
    if (!out.p || out.n % nrep) HIPCHK(out.resize((size_t)nrep * std::max<size_t>((size_t)s->N * 8, 4096), false));
    HIPCHK(count.resize(2 * (size_t)nrep));
    cnt.assign(2 * (size_t)nrep, 0ull);
    for (int attempt = 0; attempt < 6; attempt++) {
        if (!s->list.serves_search(dcut)) {
            // the list stays in use as the force list of the next run: built with that run's look-ahead (a growing bead
            // scale over the rest of an interval), like the builds inside gd_run
            gd_run_desc ahead{};
            ahead.timestep = s->last_dt; ahead.flags = s->last_flags;
            s->pol.take_pending_skin(pair_cutoff(s));
            const float rv_force = with_list ? list_radius(s, s->last_dt > 0 ? &ahead : nullptr, s->pol.K) : 0.f;
            const float rv_search = (float)(dcut * (1.0 + 1e-6));
            GDCHK(build_now(s, std::max(rv_force, rv_search), true, true, rv_search));
            s->list.enter_use(rv_search > rv_force);
        }
        const double lim = 0.5 * ((double)s->list.rv - dcut);
        PairsP q;
        memset(&q, 0, sizeof q);
        q.pos = s->pos[s->pcur].p; q.x0 = s->list.tiled ? s->rec_x0.p : s->xb.p; q.rec_mo = s->rec_mo.p; q.meta = s->meta.p;
        q.orig = s->orig[s->ocur].p; q.nbr = s->nbr.p; q.nbr16 = s->nbr16.p; q.tiles = s->tiles.p; q.wtab = s->wtab.p;
        q.N = s->N; q.Np = s->Np; q.nblk = s->nblk; q.r = r0; q.nrep = nrep; q.W = s->list.W;
        q.tiled = s->list.tiled ? 1 : 0; q.s16 = (s->list.tiled && gd_tile_s16(s->list.tile_cap)) ? 1 : 0;
        set_box(s, q);
        q.dcut2 = (float)(dcut * dcut); q.lim2 = (float)(lim * lim);
        q.out = out.p; q.cap = out.n / nrep; q.count = count.p;
        q.dmax = s->dmax.p;
        HIPCHK(hipMemsetAsync(count.p, 0, 2 * (size_t)nrep * sizeof(unsigned long long), s->stream));
        gd_launch_pairs(q, s->stream);
        HIPCHK(hipMemcpyAsync(cnt.data(), count.p, 2 * (size_t)nrep * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipGetLastError());
        unsigned long long moved = 0, most = 0;
        for (uint32_t y = 0; y < nrep; y++) { most = std::max(most, cnt[2 * y]); moved |= cnt[2 * y + 1]; }
        if (moved) { s->list.drop(); continue; }                      // a bead moved beyond the margin: fresh list
        if (most > q.cap) { HIPCHK(out.resize((size_t)nrep * (size_t)(most + most / 8 + 64), false)); continue; }
        return GD_OK;
    }
    return fail(GD_ESTATE, "pair search: did not converge");
}

// ------------------------------------------------------------- live seams (gdyn_live.hpp)
// What the live bridge reads of a handle (the contact tables: gd_live_contact_tab, gdyn_capi_contacts.hip).  No call needs prepare():
// the tables and the positions are what gd_contacts_fetch and gd_get_positions_f32 read, which do not prepare either.  Each ends with
// the stream idle, so no chunk of a gd_run and no update is in flight when an analysis stream reads the buffers.
gd_live_shape gd_live_shape_of(const gd_system *s)
{
    gd_live_shape v{};
    v.device = s->device; v.N = s->N; v.R = s->R;
    v.periodic = s->box_kind == GD_BOX_PERIODIC; v.has_wall = s->has_wall;
    memcpy(v.box, s->box, sizeof v.box);
    return v;
}

int gd_live_positions(gd_system *s, int quantize, const float **xyz)
{
    HIPCHK(hipSetDevice(s->device));
    gd_launch_gather_xyz(s->pos[s->pcur].p, s->slot_of.p, (float *)s->fout.p, s->N, s->Np, s->R, quantize, s->stream);      // as fetch_xyz
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    *xyz = (const float *)s->fout.p;
    return GD_OK;
}

// ------------------------------------------------------------ micro-benchmark (developer builds only)
#ifdef GD_DEV
extern "C" int gd_debug_bench(gd_system *s, int what, int n, double *mean_ms)
{
    if (!s || !mean_ms || n < 1) return fail(GD_EINVAL, "gd_debug_bench: bad argument");
    GDCHK(prepare(s));
    GDCHK(ensure_fresh_list(s));
    hipEvent_t e0 = get_event(s, 0), e1 = get_event(s, 1);
    const float rv = list_radius(s, nullptr, 0);
    StepParams p;
    fill_common(s, p);
    p.dt_d = 1e-5; p.dt = 1e-5f; p.kT = 1.0f; p.seed = 1; p.noise_mode = GD_NOISE_PHILOX; p.run_flags = 0;
    p.ctx_out = s->ctx[s->ccur ^ 1].p;     // scratch: the current context is not replaced
    GDCHK(clear_flags(s));
    if (what >= 10) HIPCHK(hipMemsetAsync(s->fout.p, 0, s->fout.n * sizeof(float4), s->stream));
    HIPCHK(hipEventRecord(e0, s->stream));
    for (int i = 0; i < n; i++) {
        if (what == 0 || what >= 30) { GDCHK(enqueue_build(s, rv, pair_cutoff(s) > 0)); }
        else gd_launch_step(p, GD_MODE_STEP, s->stream);
    }
    HIPCHK(hipEventRecord(e1, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *mean_ms = ms / n;
    if (what >= 10) {
        // section stamps of a timing-only kernel build (-DGD_ABL=30): mean shader-clock cycles per wave spent in
        // section what-10 (zeros with the product kernels, which never write the force buffer in step mode)
        // (one 8-word record per wave: 7 section times of the last launch + a presence flag)
        std::vector<unsigned long long> rec(std::min<size_t>(s->fout.n * 2, (size_t)1 << 22));
        HIPCHK(hipMemcpy(rec.data(), s->fout.p, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        double sum = 0, waves = 0;
        const int idx = what >= 30 ? what - 30 : what - 10;
        for (size_t w = 0; w + 16 <= rec.size(); w += 16)
            if (rec[w + 15] == 1ull && idx >= 0 && idx < 12) { sum += (double)rec[w + idx]; waves += 1; }
        *mean_ms = waves > 0 ? sum / waves : 0.0;
    }
    GDCHK(clear_flags(s));
    return GD_OK;
}
#endif
