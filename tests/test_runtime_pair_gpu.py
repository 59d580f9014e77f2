"""The runtime-power pair kernels (StepParams.pk = 0: any soft-core powers but (2, 3, 8, 3)) on the device against the oracle.

Every workload and golden state sets (2, 3, 8, 3) and so runs the two specialised pair forms; the runtime form is what the spindle
driver launches (host/gd_spindle.cpp: (2, 3, 2, 3)) and what every other valid (P, Q) takes.  Here:

  1. known answers: all 20 valid (P, Q) on isolated pairs at separations from 0 to beyond the edge, forces, energy and one compensated
     step against the closed form in numpy fp64 (tests/test_oracle_kat.py holds the oracle to the same numbers at 1e-12);
  2. every tile class of launch_step_mode -- 16-bit unsplit, 16-bit split at 3 312, plain-index split at 3 312 and at 5 072, and the
     periodic variants -- on dense blobs with powers (4, 2, 12, 1): forces and energies term by term before and after five noisy steps
     with a rebuild, and the trajectory;
  3. step groups asked for on a runtime-power handle (the policy keeps it on one launch) and per-replica A/B tables next to it;
  4. the spindle driver's coarse model built through the Python API.

tests/test_term_parity_gpu.py runs the runtime-power states of tests/stressed_states.py term by term.  Tolerances are those of
tests/util.py; every test asserts the list path (and tile class) it ran on."""
import importlib

import numpy as np
import pytest

import stressed_states as ss
from bit_identity import assert_identical
from util import ENERGY_RTOL, FORCE_RTOL, PKG, POS_ATOL_20STEP, g

ensemble = importlib.import_module(PKG + ".ensemble")

pytestmark = pytest.mark.gpu
PATHS = {"generic": 1, "tiled": 2}
SEED = 20220101


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


def _compare_forces(Fh, Fo, what, keep=None):
    """per replica: |dF| <= FORCE_RTOL max|F_ref| (the maximum over all beads; `keep`: the beads compared)"""
    for r in range(Fo.shape[0]):
        scale = np.abs(Fo[r]).max()
        err = np.abs(Fh[r] - Fo[r])[slice(None) if keep is None else keep].max()
        print(f"  {what} r{r}: |dF| / max|F| {err / scale:.2e}")
        assert scale > 0 and err <= FORCE_RTOL * scale, (what, r, err / scale)


# ------------------------------------------------------------------------------------------------ 1: known answers

_kat = {}


def _kat_reference(form):
    if form not in _kat:
        _kat[form] = ss.isolated_pairs_reference(form)
    return _kat[form]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("form", ss.FORMS, ids=[f"P{p}Q{q}" for p, q in ss.FORMS])
def test_known_answers_of_every_valid_form(hip, form, path):
    """`form` in channel A and a second form in channel B (ss.second_form: (2, 3) meets (8, 3), the one specialised handle of the
    twenty), mixed, on 54 isolated pairs: separations (0, 2^-10, 0.25, 0.5, 0.9, 0.999, 1, the next fp32 above 1, 1.5) sigma_a times
    the six pairings of the types A, B, u.  Every bead's list holds one neighbour and padding.

    The one exclusion: with Q = 1 the force jumps at u = 1, and fp32 r^2 / sigma^2 may round either way, so in those handles the pairs
    with |u - 1| <= 4 x 2^-24 -- the grid points u = 1 and the next fp32 above it, six pairs each, nothing else -- are left out of the
    force comparisons (not of the energy's, which is continuous)."""
    x, a, b, pairs, u, axis = ss.isolated_pairs_layout()
    F_ref, e_ref = _kat_reference(form)
    keep = np.ones(len(x), dtype=bool)
    if form[1] == 1:
        out = np.abs(u - 1) <= 4 * 2.0 ** -24
        assert out.sum() == 2 * len(ss.PAIR_KINDS) and set(u[out]) == {ss.U_GRID[6], ss.U_GRID[7]}
        keep[pairs[out].ravel()] = False
    assert (~keep).sum() == (4 * len(ss.PAIR_KINDS) if form[1] == 1 else 0)
    coincident = pairs[u == 0].ravel()
    assert len(coincident) == 2 * len(ss.PAIR_KINDS)

    s = ss.isolated_pairs(hip, form)
    s.set_tuning(kernel_path=PATHS[path])
    F, E = s.forces(), s.energy()
    _assert_path(s, path)
    _compare_forces(F, F_ref[None], (form, "forces"), keep)
    assert np.all(F[0][coincident] == 0)
    S = np.abs(e_ref).sum()
    print(f"  energy: |dE| / sum|e| {abs(E[0] - e_ref.sum()) / S:.2e}")
    assert np.isfinite(E[0]) and abs(E[0] - e_ref.sum()) <= ENERGY_RTOL * S, (form, E[0], e_ref.sum())
    assert np.array_equal(s.forces(g.TERM_PAIR), F) and np.array_equal(s.energy(g.TERM_PAIR), E)

    # one zero-noise compensated step (test_term_parity_gpu.py::test_step_mode_per_term): the force STEP mode used
    t = ss.isolated_pairs(hip, form)
    t.set_tuning(kernel_path=PATHS[path])
    mu = np.array(ss.MOBILITY)[np.arange(t.N) % 3][None, :, None]
    dt = 1e-5
    t.run(1, dt, 0.0, noise=g.NOISE_ZERO, flags=g.RUN_COMPENSATED)
    assert t.context().compensated == 1 and t.context().step == 1
    _assert_path(t, path)
    x1 = t.positions()
    _compare_forces((x1 - x[None]) / (mu * dt), F_ref[None], (form, "step"), keep)
    assert np.array_equal(x1[0][coincident], x[coincident])


# ------------------------------------------------------------------------------------------------ 2: the tile classes

# launch_step_mode's variants by (tile_capacity, largest_tile) of the list in use; "generic": the global-gather lists (no tiles)
CLASSES = {
    "generic": lambda cap, big: True,
    "unsplit_16bit": lambda cap, big: cap <= 3312 and big <= 3312,
    "split_3312_16bit": lambda cap, big: 3312 < cap < 4096 and big > 3312,
    "split_3312_index": lambda cap, big: 4096 <= cap <= 5072 and big >= 4096,
    "split_5072_index": lambda cap, big: cap > 5072 and big > 5072,
}
# the families, per class from the smallest member on: (beads, compression); each tried at the library's own list width and at
# the skins of test_parity_gpu.py::test_step_split_by_tile_class_matches_oracle until one lands in the class
SKINS = (0.0, 1.1, 1.05, 1.15, 1.0, 1.2)
# (a tile holds at most the whole handle, so a class needs more beads than its lower bound; among bead counts in steps of 1 000 up
# to 12 000 and compressions of 0.35 and more, the first member of each list is the smallest handle that reached its class on an
# MI355X -- 4 000 beads for tiles beyond 3 312, 5 000 beyond 4 096, 6 000 beyond 5 072 -- the others are there for a library whose
# list widths have moved)
BLOBS = {
    "generic": [(1500, 0.7)],
    "unsplit_16bit": [(1500, 0.7), (1500, 1.0)],
    "split_3312_16bit": [(4000, 0.4), (4000, 0.45), (5000, 0.45), (6000, 0.5), (8000, 0.6), (12000, 0.6)],
    "split_3312_index": [(5000, 0.35), (5000, 0.4), (6000, 0.4), (8000, 0.45), (12000, 0.5)],
    "split_5072_index": [(6000, 0.35), (8000, 0.35), (8000, 0.4), (12000, 0.4), (12000, 0.35)],
}
BOXES = {
    "generic": [(3000, 0.6)],
    "unsplit_16bit": [(3000, 0.6), (3000, 1.0)],
    "split_3312_16bit": [(6000, 0.5), (6000, 0.55), (6000, 0.6), (8000, 0.7), (12000, 0.7)],
    "split_3312_index": [(6000, 0.45), (6000, 0.42), (8000, 0.5), (8000, 0.6), (12000, 0.6)],
    "split_5072_index": [(6000, 0.4), (6000, 0.38), (8000, 0.4), (8000, 0.45), (12000, 0.45)],
}
assert max(n for fam in list(BLOBS.values()) + list(BOXES.values()) for n, _ in fam) <= 12000


def _land_in_class(hip, make, family, wanted, path):
    """(handle, (beads, compression, skin)) of the first member and list width whose first build lands in the class; fails if none does"""
    seen = {}
    for n, c in family:
        for skin in SKINS:
            s = make(hip, n, c)
            s.set_tuning(kernel_path=path, skin=skin, adapt_interval=0, rebuild_interval=3)
            s.energy()                                    # builds the list: the tile class of this state and width
            ctx = s.context()
            seen[(n, c, skin)] = (ctx.tile_capacity, ctx.largest_tile, ctx.list_path)
            if ctx.list_path == path and wanted(ctx.tile_capacity, ctx.largest_tile):
                print(f"  {(n, c, skin)}: tile capacity {ctx.tile_capacity}, largest tile {ctx.largest_tile}, entries per bead {ctx.list_entries / (n * s.R):.0f}")
                return s, (n, c, skin)
            s.close()
    raise AssertionError(("no member of the family in the class", seen))


def _term_by_term(sh, so, make_oracle, terms, parts, what):
    """test_term_parity_gpu.py::test_every_term_on_its_own_scale: forces within FORCE_RTOL of each term's largest, energies within
    ENERGY_RTOL of |E_t| (of the sum of its one-signed parts' magnitudes where `parts` names them), per replica"""
    x = so.positions()
    for t in terms:
        m = ss.TERM_BITS[t]
        _compare_forces(sh.forces(m), so.forces(m), (what, t))
        eh, eo = sh.energy(m), so.energy(m)
        if t in parts:
            S = 0.0
            for mod in parts[t]:
                sp = make_oracle()
                sp.set_positions(x)
                mod(sp)
                S = S + np.abs(sp.energy(m))
                sp.close()
        else:
            S = np.abs(eo)
        print(f"  {what} {t}: |dE| / S {np.abs(eh - eo) / S}")
        assert np.all(np.abs(eh - eo) <= ENERGY_RTOL * S), (what, t, (eh - eo) / S)
    _compare_forces(sh.forces(), so.forces(), (what, "all"))


def _class_run(hip, oracle, make, family, cls, dt, terms, parts, edge, grid=None):
    """One handle in the tile class `cls`: term-by-term forces and energies, five noisy Philox steps with a rebuild on the way against
    the oracle, forces and energies again at the state the device reached.

    The B channel is a (12, 1) soft core: its force jumps by |eps_b| 12 / sigma_b at r = sigma_b.  Force comparisons are made at
    positions cleared of pairs within 2^-19 sigma_b of that edge (ss.clear_of_edge: the fp32 rounding of r^2 / sigma^2 is a few 1e-7),
    which conditions the state and touches no other pair.  Along a trajectory a pair may still cross the edge a step earlier on one
    side than on the other; `dt` is chosen so that one such event moves a bead by less than half the position tolerance
    (mobility x dt x jump), while the noise of a single step (sqrt(2 mu kT dt) per coordinate) stays several times above it: a bead
    that a split launch skips or moves twice is off by that much."""
    path = 1 if cls == "generic" else 2
    sh, (n, c, skin) = _land_in_class(hip, make, family, CLASSES[cls], path)
    so = make(oracle, n, c)
    x0 = ss.clear_of_edge(so, edge, grid=grid)
    sh.set_positions(x0)
    _term_by_term(sh, so, lambda: make(oracle, n, c), terms, parts, "before")
    ctx = sh.context()
    assert ctx.list_path == path and CLASSES[cls](ctx.tile_capacity, ctx.largest_tile), (ctx.tile_capacity, ctx.largest_tile)
    b0 = ctx.rebuilds
    for s in (sh, so):
        s.run(5, dt, 1.0, seed=SEED)
    ctx = sh.context()
    assert ctx.list_path == path and CLASSES[cls](ctx.tile_capacity, ctx.largest_tile), (ctx.tile_capacity, ctx.largest_tile)
    assert ctx.step == 5 and ctx.rebuilds > b0 and ctx.rollbacks == 0 and ctx.rebuild_interval == 3
    d = sh.positions() - so.positions()
    if grid is not None:
        d -= np.array(so.box) * np.rint(d / np.array(so.box))       # (a bead within rounding of a face may be wrapped on one side only)
    print(f"  |dx| after 5 steps {np.abs(d).max():.2e}, moved {np.abs(sh.positions() - x0).max():.2e}")
    assert np.abs(d).max() <= 3 * POS_ATOL_20STEP                   # (forces ten times the benchmark state's and more)
    assert np.all(np.abs(sh.positions() - x0).max(axis=-1) > 0)     # every bead of every replica was moved
    # the state the device reached, on both sides
    so.set_positions(sh.positions())
    x1 = ss.clear_of_edge(so, edge, grid=grid)
    sh.set_positions(x1)
    _term_by_term(sh, so, lambda: make(oracle, n, c), terms, parts, "after")
    ctx = sh.context()
    assert ctx.list_path == path and CLASSES[cls](ctx.tile_capacity, ctx.largest_tile), (ctx.tile_capacity, ctx.largest_tile)


# jump of the (12, 1) B channel of the blobs: eps_b 12 / sigma_b = 100, largest mobility 1.75: one event moves a bead by
# 1.75 x 100 x dt = 4.4e-5 < 3 POS_ATOL_20STEP / 2; noise per step and coordinate sqrt(2 x 0.5 x dt) = 5e-4 at the least
BLOB_DT = 2.5e-7
assert max(ss.MOBILITY) * 2.0 * 12 / 0.24 * BLOB_DT <= 1.5 * POS_ATOL_20STEP < (2 * min(ss.MOBILITY) * BLOB_DT) ** 0.5 / 5


@pytest.mark.parametrize("cls", list(CLASSES))
def test_tile_classes_with_runtime_powers(hip, oracle, cls):
    """Open box, powers (4, 2, 12, 1), mixed, R = 2, on the blob family of tests/stressed_states.py::runtime_blob."""
    assert ss.BLOB_POWERS == (4, 2, 12, 1)
    _class_run(hip, oracle, ss.runtime_blob, BLOBS[cls], cls, BLOB_DT, ss.CONFIGURED["runtime_blob"], {}, edge=0.24)


def _kb_channel(a):
    def mod(s):
        p = ss.kb_pair(ss.BLOB_POWERS)
        s.set_pair_softcore(*((p[0], p[1], 0.0, 0.0) if a else (0.0, 0.0, p[2], p[3])), *p[4:], mix=False)
    return mod


def _kb_slot(keep):
    return lambda s: s.set_dynamic_pairs(1 - keep, ss.KB_LOOP, np.zeros((0, 2), dtype=np.uint32))


# the attractive (12, 1) B channel of the 1 kb field jumps by 0.2 x 12 / 1.5 = 1.6 at r = 1.5; mobility 1
BOX_DT = 2e-5
assert 1.6 * BOX_DT <= 1.5 * POS_ATOL_20STEP < (2 * BOX_DT) ** 0.5 / 5


@pytest.mark.parametrize("cls", list(BOXES))
def test_periodic_tile_classes_with_runtime_powers(hip, oracle, cls):
    """Periodic box, the 1 kb force field (unmixed, attractive B channel, loops and minimum-image glue) with powers (4, 2, 12, 1),
    compressed with its box until the box is a few list radii wide: tiles wrap around it.  All four classes (the periodic variants are
    kernels of their own)."""
    parts = {"pair": [_kb_channel(True), _kb_channel(False)], "dynamic": [_kb_slot(0), _kb_slot(1)]}
    _class_run(hip, oracle, ss.runtime_box, BOXES[cls], cls, BOX_DT, ss.CONFIGURED["runtime_box"], parts, edge=1.5, grid=ss.GRID)


# ------------------------------------------------------------------------------------------------ 3: step groups, per-replica tables

SMOOTH = ss.RUNTIME_POWERS[1]        # (6, 4, 2, 3): no jump in the force, the suite's usual time step
N_SMALL, COMPRESS_SMALL, DT = 1500, 0.7, 1e-5
TUNE = dict(kernel_path=2, rebuild_interval=4, adapt_interval=0)


def _seeds(nrep):
    return np.arange(nrep, dtype=np.uint64) * np.uint64(7919) + np.uint64(SEED)


@pytest.mark.parametrize("nrep", [4, 16])
def test_step_groups_asked_for_on_a_runtime_power_handle(hip, oracle, nrep):
    """k_step adds the replica-group offset only in the specialised pair forms, so a runtime-power handle must never run in two
    groups (csrc/gdyn_policy.hpp: step_group_split, tests/native/test_step_groups.cpp).  Mode 2 asked for on such a handle -- tiled,
    device noise, one seed per replica; R = 4, and R = 16, which is the size a specialised handle does run in two groups at: the
    policy reports one group, every replica advances by exactly 6 steps, the positions are those of mode 1 bit for bit and every
    replica's those of a one-replica oracle run on its seed."""
    handles = []
    for mode in (1, 2):
        s = ss.runtime_blob(hip, N_SMALL, COMPRESS_SMALL, powers=SMOOTH, n_replicas=nrep)
        s.set_tuning(**TUNE)
        s.set_step_groups(mode)
        assert s.step_groups() == (mode, 1)
        handles.append(s)
    one, two = handles
    x0 = one.positions()
    t1, t2 = (s.run(6, DT, 1.0, replica_seeds=_seeds(nrep)) for s in handles)
    assert one.step_groups() == (1, 1) and two.step_groups() == (2, 1)          # what the policy decided: not a specialised form
    assert [two.context(r).step for r in range(nrep)] == [6] * nrep
    assert two.context().list_path == 2 and two.context().rebuilds >= 2
    assert_identical(one, two, t1, t2)
    x = two.positions()
    assert np.all(np.abs(x - x0).max(axis=(1, 2)) > 0)
    for r in range(nrep):
        so = ss.runtime_blob(oracle, N_SMALL, COMPRESS_SMALL, powers=SMOOTH, n_replicas=1)
        so.set_positions(x0[r][None])
        so.run(6, DT, 1.0, seed=int(_seeds(nrep)[r]))
        assert np.abs(x[r] - so.positions()[0]).max() <= POS_ATOL_20STEP, r
        so.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_per_replica_tables_next_to_runtime_powers(hip, oracle, path):
    """ensemble.set_ab on a mixed runtime-power handle, R = 3: replica 0 keeps the model's table, replicas 1 and 2 hold
    permutations of it.  The runtime branch takes its weights from the factors packed with the neighbour's position: forces, energy
    and five noisy steps of every replica against a one-replica oracle that holds that replica's table."""
    sh = ss.runtime_blob(hip, N_SMALL, COMPRESS_SMALL, powers=SMOOTH, n_replicas=3)
    sh.set_tuning(**dict(TUNE, kernel_path=PATHS[path]))
    a0, b0, _ = ss._types(N_SMALL)
    tables = [(a0, b0)]
    for r in (1, 2):
        perm = np.random.default_rng(50 + r).permutation(N_SMALL)
        tables.append((a0[perm].copy(), b0[perm].copy()))
        assert np.mean((tables[r][0] != a0) | (tables[r][1] != b0)) >= 0.25
        ensemble.set_ab(sh, r, *tables[r])
    assert list(ensemble.classes(sh)[0]) == [0, 1, 2]
    x0 = sh.positions()
    Fh, Eh = sh.forces(), sh.energy()
    seeds = _seeds(3)
    sh.run(5, DT, 1.0, replica_seeds=seeds)
    _assert_path(sh, path)
    xh = sh.positions()
    for r in range(3):
        so = ss.runtime_blob(oracle, N_SMALL, COMPRESS_SMALL, powers=SMOOTH, n_replicas=1)
        so.set_bead_params(a=tables[r][0], b=tables[r][1])
        so.set_positions(x0[r][None])
        Fo, Eo = so.forces(), so.energy()
        _compare_forces(Fh[r:r + 1], Fo, ("table", r))
        S = sum(abs(so.energy(ss.TERM_BITS[t])[0]) for t in ss.CONFIGURED["runtime_blob"])
        assert abs(Eh[r] - Eo[0]) <= ENERGY_RTOL * S, (r, Eh[r], Eo[0])
        if r:       # a table that is ignored cannot pass: the model's table gives other forces at these positions
            so.set_bead_params(a=a0, b=b0)
            assert np.abs(so.forces() - Fo).max() > 100 * FORCE_RTOL * np.abs(Fo).max()
            so.set_bead_params(a=tables[r][0], b=tables[r][1])
        so.run(5, DT, 1.0, seed=int(seeds[r]))
        assert np.abs(xh[r] - so.positions()[0]).max() <= POS_ATOL_20STEP, r
        so.close()


# ------------------------------------------------------------------------------------------------ 4: the spindle driver's model

@pytest.mark.parametrize("path", list(PATHS))
def test_spindle_driver_model_forces_match_oracle(hip, oracle, path):
    """The sibling of test_host_driver.py::test_spindle_driver_on_gpu (positions of a few hundred beads after 70 steps within 2e-4,
    on whichever path): the coarse model the driver builds, through the Python API, on both list paths -- forces term by term and
    energies at the driver's initial rods, where only the pair term and the spindle source act, and at the state 40 oracle steps of
    the spindle phase lead to, where bonds and bending act as well."""
    sh, so = ss.spindle_coarse(hip), ss.spindle_coarse(oracle)
    sh.set_tuning(kernel_path=PATHS[path])
    cfg = so.cfg
    for what, acting in (("rods", ("pair", "point")), ("after 40 steps", ("pair", "bond", "bend", "point"))):
        assert ss.idle_terms(so, acting) == [], (what, ss.term_ratios(so))
        for t in acting:
            m = ss.TERM_BITS[t]
            _compare_forces(sh.forces(m), so.forces(m), (what, t))
            eh, eo = sh.energy(m), so.energy(m)
            assert np.all(np.abs(eh - eo) <= ENERGY_RTOL * np.abs(eo)), (what, t, (eh - eo) / eo)
        _compare_forces(sh.forces(), so.forces(), (what, "all"))
        assert np.isfinite(sh.energy()).all()
        _assert_path(sh, path)
        if what == "rods":
            so.begin_phase()
            so.run(40, cfg["init_timestep"], cfg["init_temperature"], seed=SEED)
            x = ss.f32(so.positions())
            so.set_positions(x)
            sh.set_positions(x)
