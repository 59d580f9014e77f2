// gdyn_system.hpp -- the handle of the stepper (gd_system) as its host files share it: the host model, the device state of the core
// and one struct per feature that keeps state on the handle, each owning its buffers; below them the few functions that cross from
// one host file to another.  Internal: C++ linkage, hidden, none of it exported.
//   gdyn_capi.hip           create and destroy, the model setters, topology, list builds, gd_run, energy and forces, search_device
//   gdyn_capi_pairs.hip     the droplet term and the per-replica pairs: the kernels behind k_step
//   gdyn_capi_contacts.hip  gd_search_pairs with its cache, the contact maps, the live bridge's seam to their tables
//   gdyn_capi_glue.hip      the glue kinetics
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_replica.h"
#include "../../include/gdyn_ensemble.h"
#include "../../include/gdyn_groups.h"
#include "../../include/gdyn_prep.h"
#include "../../include/gdyn_glue.h"

#include "gdyn_types.h"
#include "gdyn_analysis.hpp"
#include "gdyn_policy.hpp"
#include "gdyn_list.hpp"
#include "gdyn_live.hpp"
#include "gdyn_replica_pairs.hpp"
#include "gdyn_ensemble.hpp"

using gd::fail;

struct Bond { uint32_t i, j; int type; };
struct BendRange { uint32_t start, end; double energy; int per_bead; };
struct PointSource { int kind; double k, b, p[3]; std::vector<uint8_t> mask; };
struct DynSet { bool used = false; gd_bond_params p; std::vector<uint32_t> pairs; };

namespace gd {

// droplet attraction (gd_set_pair_softwell)
struct Droplet {
    uint32_t n = 0; double eps = 0, decay = 1, cut = 0;
    dbuf<unsigned> targets; dbuf<double> esum;
};

// per-replica dynamic pairs (gdyn_replica.h): the block of the last upload (layout, pinned staging, device copy; both grown
// geometrically, never shrunk), the slots' parameters, the energy sums.  What the caller set is gd_system::rp.
struct ReplicaUpload {
    ReplicaLayout layout; gd_bond_params params[RP_SLOTS] = {};
    pinned<uint32_t> stage; hipEvent_t copied = nullptr;      // (copied: the last upload has left the staging block)
    dbuf<uint32_t> dev; dbuf<double> esum;
    ~ReplicaUpload() { if (copied) (void)hipEventDestroy(copied); }
};

// device glue kinetics (gdyn_glue.h): the sets as sorted pair words (the host copy is what fetch returns and what is installed in
// the managed slot; the device copy keys[cur], kstride words a replica, feeds the next update and is laid out again from
// the host copy after gd_glue_set), the buffers of an update (grown, never shrunk), two pinned blocks (small: seeds, counters,
// segments; large: the sets on their way up or down)
struct Glue {
    bool defined = false, dev_dirty = true; uint32_t slot = 0; gd_glue_params par{};
    std::vector<std::vector<uint64_t>> sets;
    dbuf<unsigned long long> keys[2], merged, fkey[2], fsel[2], seeds, cand_count; dbuf<uint2> cand;
    dbuf<unsigned> alive, nkeys, cnt, seg; dbuf<char> tmp;
    size_t kstride[2] = {0, 0}, fstride = 0; int cur = 0;
    pinned<unsigned long long> small, pin;
};

// gd_search_pairs: device output, counters, and the cached result of the last call
struct SearchCache {
    dbuf<uint2> out; dbuf<unsigned long long> count; std::vector<uint2> host;
    bool valid = false; uint32_t r = 0; double dcut = 0; uint64_t serial = 0;
};

// gd_contacts_*: per-replica count tables (ContactTab), the pair buffer of an update, dump buffers
struct ContactTables {
    dbuf<unsigned long long> words; dbuf<unsigned> distinct; size_t cap = 0;
    dbuf<uint2> pairs; dbuf<unsigned long long> count; std::vector<unsigned> distinct_h;
    dbuf<unsigned long long> ck[2]; dbuf<unsigned> cv[2], n; dbuf<char> tmp;
};

}      // namespace gd

struct gd_system {
    uint32_t N = 0, R = 0, Np = 0, nblk = 0;
    int device = 0, box_kind = 0;
    double box[3] = {0, 0, 0};
    hipStream_t stream = nullptr;

    // host model
    gd::EnsembleAB ens;            // the (a, b) factors: the shared table and what single replicas carry instead (gdyn_ensemble.hpp)
    std::vector<double> mob, bend;
    bool has_pair = false; gd_pair_softcore pair{};
    std::vector<gd_bond_params> btypes; std::vector<int> bterm;
    std::vector<Bond> bonds;
    DynSet dyn[4];
    std::vector<BendRange> bends;
    std::vector<PointSource> psrc;
    bool has_wall = false; gd_wall wall{};
    bool has_scaling = false; double bs_init = 1, bs_tau = 1, bo_init = 1, bo_tau = 1;
    std::vector<DevCtx> hctx;      // host mirror of the device context

    bool topo_dirty = true, ctx_dirty = true;
    bool has_bend = false, has_bonds = false;
    uint32_t WB = 0, ncell_cap = 0;
    int pcur = 0, ccur = 0;
    uint32_t kernel_path = 0;      // 0 auto, 1 generic, 2 tiled
    bool packed_ab = false;
    bool has_inner = false; gd_inner_sphere inner{};
    bool has_softcore_bonds = false;
    bool bonds_premixed = false;   // every bond parameter record is unmixed (AB mixing resolved per bond by finalize_topology)
    bool bonds_all_scaled = false; // every bond parameter record has scale_by_bond_scale set
    gd::pinned<float> h_stage;     // pinned host staging for snapshot downloads (R*N*3 floats)
    gd::pinned<char> h_chunk;      // pinned host block for the per-chunk readback (flags, contexts, list counts): copies into pageable
                                   // memory are staged by the runtime and cost ~20 us each
    uint32_t cpb = 1;
    gd::ListPolicy pol;            // list width, rebuild interval, tile class, list path of the builds to come (gdyn_policy.hpp)
    gd::ResidentList list;         // the list in use and what its build left for the next one (gdyn_list.hpp)
    uint64_t rebuilds = 0, rollbacks = 0;
    uint32_t n_bond_types = 0;
    std::vector<unsigned long long> lcount;
    gd_timing timing{};

    // device: static (bead order)
    gd::dbuf<float2> ab_o; uint32_t ab_stride = 0;      // [N], stride 0: one table for all replicas; [R][N], stride N: one each (gdyn_ensemble.h)
    gd::dbuf<float> mob_o; gd::dbuf<float4> bendE_o; gd::dbuf<unsigned char> psmask_o, bdeg_o;
    gd::dbuf<unsigned> badj_o; gd::dbuf<int4> chain_o; gd::dbuf<BondType> btab;
    // device: per slot
    gd::dbuf<float4> pos[2], xb, fout, snap;
    gd::dbuf<unsigned> orig[2], slot_of, rank, members, cell_cnt, cell_start, nbr, meta, badj, flags;
    gd::dbuf<float> bbox_enc, bbox_w;      // box of the last build's positions (two halves: read / written), k_scatter's per-wave partials
    gd::dbuf<unsigned short> nbr16; gd::dbuf<TileDesc> tiles;
    gd::dbuf<float4> rec_x0; gd::dbuf<uint2> rec_mo; gd::dbuf<unsigned char> len_prev;
    // Ragged rows of the tiled lists (BuildParams): per-wave row table, what every bead needed at the last build, the pool's cursor.
    // nbr16 IS the pool: pool KiB = nbr16.n / 512 entries.
    gd::dbuf<uint2> wtab, rqueue; gd::dbuf<unsigned short> need_prev; gd::dbuf<unsigned> pool;
    gd::dbuf<float> bbox;
    gd::dbuf<float2> ab; gd::dbuf<float> mobs; gd::dbuf<float4> bendE; gd::dbuf<int4> chain;
    float mob_uniform = -1.f;
    gd::dbuf<GridP> grid; gd::dbuf<DevCtx> ctx[2]; gd::dbuf<float4> react_part[2]; gd::dbuf<double> epart;   // react_part ping-pongs with ctx
    gd::dbuf<unsigned long long> lcount_d; gd::dbuf<float> noise;
    gd::dbuf<unsigned long long> seeds_d;     // gd_run_desc.replica_seeds of the run in progress
    gd::dbuf<unsigned> dmax;          // [R] largest squared displacement since the list build (k_step keeps it; zeroed by the build)
    double last_dt = 0, last_kT = -1;
    int last_flags = 0;             // flags of the last gd_run (the look-ahead of a list built between runs, gd_search_pairs)
    double pend_dt = 0; int pend_flags = 0;      // timestep and flags of the run that left its last callback pending (GD_RUN_DEFER_CALLBACK)
    double near_frac = 0.65;        // near-class radius = cutoff + near_frac x (list radius - cutoff)
    uint64_t state_serial = 1;     // bumped by everything that changes positions or the model (invalidates the search cache)
    int ocur = 0;   // which orig[] buffer is current
    // Compensated positions (small-dt / T = 0 runs, k_step's p.comp): fp32 residuals by bead index, so that the position of a bead is
    // pos + lo.  gd_set_positions fills them from the fp64 input, a compensated run keeps them, any other run invalidates them.
    gd::dbuf<float4> lo, snap_lo;
    bool lo_valid = false;         // lo describes the current positions (else: taken as zero)
    bool comp_last = false;        // the last gd_run stepped with the compensated update (diagnostics)
    double mob_max = 1.0;
    std::vector<hipEvent_t> events;
    // Replica groups of the step launches (gdyn_groups.h, gd::step_group_split): the second stream and the two events that fork it off
    // the handle's stream in front of a span of steps and join it behind -- created on first use; between two calls nothing is in flight
    // on it that the handle's stream does not wait for.
    hipStream_t stream2 = nullptr; hipEvent_t grp_fork = nullptr, grp_join = nullptr;
    uint32_t group_mode = gd::STEP_GROUPS_RULE, groups_last = 1;      // gd_set_step_groups; groups of the step launches of the last gd_run
    // Prepared contexts of grouped spans (gdyn_prep.h, gd::ctx_prepared): the float constants k_ctx_prep leaves for the step kernels of
    // the same step -- one buffer: stream order separates its writer from the previous step's readers
    gd::dbuf<CtxF> ctxf;           // [R], allocated on first use
    uint64_t prep_last = 0;        // preparation launches of the last gd_run

    // the features, each with the state and the buffers it owns (gd_destroy leaves the stream idle before they go)
    gd::Droplet sw;
    gd::ReplicaPairs rp;           // per-replica dynamic pairs: what the caller set (gdyn_replica_pairs.hpp)
    gd::ReplicaUpload rp_up;
    gd::Glue gl;
    gd::SearchCache sp;
    gd::ContactTables ct;

    ~gd_system()
    {
        for (auto e : events) (void)hipEventDestroy(e);
        if (grp_fork) (void)hipEventDestroy(grp_fork);
        if (grp_join) (void)hipEventDestroy(grp_join);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ---- what crosses from one host file to another

// the box of a kernel's parameter block: periodic flag, periods and their inverses
template <class P>
static void set_box(const gd_system *s, P &p)
{
    p.periodic = s->box_kind == GD_BOX_PERIODIC;
    for (int k = 0; k < 3; k++) { p.box[k] = (float)s->box[k]; p.inv_box[k] = s->box[k] > 0 ? (float)(1.0 / s->box[k]) : 0.f; }
}

inline unsigned contact_jbits(const gd_system *s)      // bits of a bead id
{
    unsigned b = 1;
    while (((uint64_t)(s->N - 1) >> b) != 0) b++;
    return b;
}

// gdyn_capi.hip
GD_SEAM int check_bond_params(const gd_bond_params *p);
GD_SEAM int prepare(gd_system *s);
GD_SEAM int search_device(gd_system *s, uint32_t r0, uint32_t nrep, double dcut, gd::dbuf<uint2> &out, gd::dbuf<unsigned long long> &count,
                          std::vector<unsigned long long> &cnt);
// gdyn_capi_pairs.hip
GD_SEAM bool post_step_active(const gd_system *s);
GD_SEAM int sync_replica_pairs(gd_system *s);
GD_SEAM void launch_softwell(gd_system *s, const StepParams &p, int mode);
GD_SEAM void launch_replica_pairs(gd_system *s, const StepParams &p, int mode);
