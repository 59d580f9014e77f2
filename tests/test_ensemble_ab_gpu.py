"""Per-replica A/B tables (include/gdyn_ensemble.h, ensemble.py) on the device against the oracle.

The oracle has one table per handle: its side is always ONE-REPLICA oracle systems, replica r of the heterogeneous handle against the
oracle system that holds table r, replica r's positions and replica r's pairs.  Tolerances are the suite's (tests/util.py): forces
within FORCE_RTOL of the largest all-term oracle force of the replica, positions within POS_ATOL_20STEP, semiaxes within the 1e-8 of
test_parity_gpu.  Energies: every term and the total within ENERGY_RTOL of the sum of the |term energies| (util.py's definition, as
test_forces_and_energies_vs_golden applies it), the bond energy within 3 x ENERGY_RTOL of itself (the bound of
test_mixed_bond_sets_beyond_the_premixed_table: a heterogeneous handle mixes its bond records at run time).

The model is the genome workload's with bond sets whose A and B parameters differ (k_a != k_b, l_a != l_b: with equal ones, as in
wl.genome_interphase, a bond does not see the table) and one per-replica pair slot with `mix`.  N = 1500 (Np = 1536: an [R][N] /
[R][Np] mix-up shows), R = 3 (every XCD runs a slice of each replica) and R = 8 (whole replicas per XCD).  Both kernel paths run, and
the tests assert which one ran."""
import importlib

import numpy as np
import pytest

from util import ENERGY_RTOL, FORCE_RTOL, PKG, POS_ATOL_20STEP, TERMS, g, wl

ensemble = importlib.import_module(PKG + ".ensemble")
replica = importlib.import_module(PKG + ".replica")

pytestmark = pytest.mark.gpu
PATHS = {"generic": 1, "tiled": 2}
EINVAL = 1
N = 1500
SEED = 20220101
FLAGS = g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
DT, KT = 1e-5, 1.0
ORDER8 = [0, 1, 2, 1, 0, 2, 2, 1]
PAIR_SLOT = g.System.bond_params(g.POT_SPRING, k_a=9.0, k_b=3.0, l_a=0.2, l_b=0.4, mix=True)


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


def _tables():
    """T0: the workload's; T1: T0 under a seeded permutation of the beads; T2: A (1, 0) or B (0, 1) at random"""
    a0, b0 = wl.ab_types(N, np.random.default_rng(SEED))
    perm = np.random.default_rng(5).permutation(N)
    a2 = np.random.default_rng(6).integers(0, 2, N).astype(float)
    return [(a0, b0), (a0[perm].copy(), b0[perm].copy()), (a2, 1.0 - a2)]


def _positions(R):
    lens = wl.chain_lengths(N)
    radius = 0.27 * (N / (8 * 0.30)) ** (1 / 3)
    x = np.stack([wl.confined_random_walks(lens, radius, 0.2, np.random.default_rng(SEED + 1 + r)) for r in range(R)])
    return x.astype(np.float32).astype(np.float64), radius


def _pairs(r):
    """The per-replica pairs of replica r: 60 pairs (i, i + 3 + r), a bead apart by a few bonds"""
    i = np.random.default_rng(40 + r).choice(N - 16, 60, replace=False)
    return np.stack([i, i + 3 + r], axis=1).astype(np.uint32)


def _model(lib, R, table, x):
    """The genome workload with A/B-dependent bond sets; `table` is the shared one"""
    lens = wl.chain_lengths(N)
    radius = _positions(1)[1]
    s = g.System(lib, N, R)
    s.set_bead_params(a=table[0], b=table[1], mobility=np.ones(N))
    s.set_pair_softcore(2.0, 0.30, 2.0, 0.24, 2, 3, 8, 3, mix=True, scale_by_bead_scale=True)
    chain = g.System.bond_params(g.POT_SEMISPRING, k_a=70.0, k_b=40.0, l_a=0.2, l_b=0.25, mix=True, scale_by_bond_scale=True)
    loop = g.System.bond_params(g.POT_HARMONIC, k_a=5.0, k_b=3.0, mix=True, scale_by_bond_scale=True)
    st = 0
    for n in lens:
        s.add_bond_range(chain, st, st + int(n), 1)
        s.add_bond_range(loop, st, st + int(n), 2)
        st += int(n)
    s.set_ellipsoid_wall(2.0, 0.30, 2.0, 0.24, wall_a_factor=5.0, wall_b_factor=5.0, packing_spring=5000.0,
                         semiaxes_spring=(1.0e4,) * 3, mobility=1.0e-4, init_semiaxes=(radius,) * 3)
    s.set_scaling(0.8, 1.0, 0.8, 1.0)
    s.set_positions(x)
    return s


def _device(hip, path, order, x, set_tables=True, **tuning):
    """A handle whose replica r holds table order[r] (T0 stays the shared one) and its own pairs"""
    T = _tables()
    sh = _model(hip, len(order), T[0], x)
    sh.set_tuning(kernel_path=PATHS[path], **tuning)
    replica.define(sh, 0, PAIR_SLOT)
    for r, k in enumerate(order):
        replica.set_pairs(sh, 0, r, _pairs(r))
        if set_tables and k != 0:
            ensemble.set_ab(sh, r, *T[k])
    return sh


def _oracle(oracle, table, x_r, r):
    so = _model(oracle, 1, table, x_r[None])
    so.set_dynamic_pairs(0, PAIR_SLOT, _pairs(r))
    return so


_ref = {}


def _reference(oracle):
    """The oracle side, computed once: at the positions of R = 8 replicas (the first three are those of the R = 3 handles) the all-term
    forces of replica r under table ORDER8[r]; for r < 3 every term's forces and energies under table r; the 20-step run of test 2;
    the preconditions on the tables."""
    if _ref:
        return _ref
    T = _tables()
    x, _ = _positions(8)
    for k in (1, 2):
        differ = np.mean((T[k][0] != T[0][0]) | (T[k][1] != T[0][1]))
        assert differ >= 0.25, (k, differ)
    F8, F, E, run = [], [], [], []
    seeds = np.array([101, 102, 103], dtype=np.uint64)
    for r in range(8):
        so = _oracle(oracle, T[ORDER8[r]], x[r], r)
        F8.append(so.forces()[0])
        if r < 3:      # (ORDER8[r] == r there)
            F.append({t: so.forces(m)[0] for t, m in TERMS.items()})
            E.append({t: so.energy(m)[0] for t, m in TERMS.items()})
            assert np.abs(F[r]["dynamic"]).max() > 0 and np.abs(F[r]["wall"]).max() > 0 and np.abs(F[r]["bond"]).max() > 0
            so.begin_phase()
            so.run(20, DT, KT, seed=int(seeds[r]), flags=FLAGS)
            run.append((so.positions()[0], np.array(so.context().semiaxes)))
        so.close()
    # a table that is ignored cannot pass: at replica 0's positions and pairs, T1 moves the forces by far more than the tolerance
    so = _oracle(oracle, T[1], x[0], 0)
    moved = np.abs(so.forces()[0] - F8[0]).max()
    so.close()
    assert moved > 100 * FORCE_RTOL * np.abs(F8[0]).max(), (moved, np.abs(F8[0]).max())
    _ref.update(T=T, x=x, F8=F8, F=F, E=E, run=run, seeds=seeds)
    return _ref


def _compare_forces(Fh, Fo, scale, what):
    err = np.abs(Fh - Fo).max()
    print(f"  {what}: |dF| / max|F| {err / scale:.2e}")
    assert scale > 0 and err <= FORCE_RTOL * scale, (what, err / scale)


def _check_forces(sh, oracle, tables, x, what):
    """All-term forces of every replica of `sh` against a fresh one-replica oracle with tables[r] at x[r]"""
    Fh = sh.forces()
    for r, t in enumerate(tables):
        so = _oracle(oracle, t, x[r], r)
        Fo = so.forces()[0]
        so.close()
        _compare_forces(Fh[r], Fo, np.abs(Fo).max(), (what, r))


# ------------------------------------------------------------------------------------------------ 1: forces and energies

@pytest.mark.parametrize("path", list(PATHS))
def test_forces_and_energies_per_term(hip, oracle, path):
    ref = _reference(oracle)
    sh = _device(hip, path, [0, 1, 2], ref["x"][:3])
    cls, n = ensemble.classes(sh)
    assert list(cls) == [0, 1, 2] and n == 3
    for t, m in TERMS.items():
        Fh, Eh = sh.forces(m), sh.energy(m)
        for r in range(3):
            _compare_forces(Fh[r], ref["F"][r][t], np.abs(ref["F"][r]["all"]).max(), (t, r))
            Eo = ref["E"][r]
            tol = 3 * ENERGY_RTOL * abs(Eo["bond"]) if t == "bond" else ENERGY_RTOL * sum(abs(Eo[u]) for u in TERMS if u != "all")
            print(f"  energy {t} r{r}: |dE| {abs(Eh[r] - Eo[t]):.3e}, bound {tol:.3e}")
            assert abs(Eh[r] - Eo[t]) <= tol, (t, r, Eh[r], Eo[t], tol)
    _assert_path(sh, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_forces_of_eight_replicas(hip, oracle, path):
    ref = _reference(oracle)
    sh = _device(hip, path, ORDER8, ref["x"])
    cls, n = ensemble.classes(sh)
    assert list(cls) == ORDER8 and n == 3
    Fh = sh.forces()
    for r in range(8):
        _compare_forces(Fh[r], ref["F8"][r], np.abs(ref["F8"][r]).max(), ("all", r))
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ 2: a run past a list rebuild

@pytest.mark.parametrize("path", list(PATHS))
def test_run_past_a_rebuild(hip, oracle, path):
    """20 Philox steps with per-replica seeds, the scale and the wall callbacks; the list is rebuilt on the way, so the factors
    reach the second list through the positions (or the slot-order array) of the first."""
    ref = _reference(oracle)
    sh = _device(hip, path, [0, 1, 2], ref["x"][:3], rebuild_interval=6, adapt_interval=0)
    sh.begin_phase()
    sh.forces()
    b0 = sh.context().rebuilds
    sh.run(20, DT, KT, seed=0, flags=FLAGS, replica_seeds=ref["seeds"])
    assert sh.context().rebuilds - b0 >= 2, (b0, sh.context().rebuilds)
    _assert_path(sh, path)
    xh = sh.positions()
    for r in range(3):
        xo, semi = ref["run"][r]
        print(f"  r{r}: |dx| {np.abs(xh[r] - xo).max():.2e}, |dsemi| {np.abs(np.array(sh.context(r).semiaxes) - semi).max():.2e}")
        assert np.abs(xh[r] - xo).max() <= POS_ATOL_20STEP, r
        assert np.allclose(np.array(sh.context(r).semiaxes), semi, rtol=0, atol=1e-8), r


# ------------------------------------------------------------------------------------------------ 3: order of calls

@pytest.mark.parametrize("path", list(PATHS))
def test_order_of_calls(hip, oracle, path):
    ref = _reference(oracle)
    T, x = ref["T"], ref["x"]
    # set, then set_positions (other positions than the handle was built on)
    sh = _device(hip, path, [0, 1, 2], x[:3])
    x2 = x[3:6]
    sh.set_positions(x2)
    _check_forces(sh, oracle, [T[0], T[1], T[2]], x2, "set, set_positions")
    # set_positions, run(5), then T2 on replica 0: the positions on the device carry the old factors
    sh.begin_phase()
    sh.run(5, DT, KT, seed=0, replica_seeds=ref["seeds"])
    ensemble.set_ab(sh, 0, *T[2])
    x3 = sh.positions()
    _check_forces(sh, oracle, [T[2], T[1], T[2]], x3, "run, set")
    assert list(ensemble.classes(sh)[0]) == [0, 1, 0]
    # b alone: a is kept
    ensemble.set_ab(sh, 1, b=T[0][1])
    a1, b1 = ensemble.get_ab(sh, 1)
    assert np.array_equal(a1, T[1][0]) and np.array_equal(b1, T[0][1])
    _check_forces(sh, oracle, [T[2], (T[1][0], T[0][1]), T[2]], x3, "b alone")
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ 4: collapse

def _forces_and_run(sh, seeds):
    F = sh.forces()
    sh.begin_phase()
    sh.run(20, DT, KT, seed=0, flags=FLAGS, replica_seeds=seeds)
    return F, sh.positions(), [tuple(sh.context(r).semiaxes) for r in range(sh.R)]


@pytest.mark.parametrize("path", list(PATHS))
def test_equal_tables_collapse_bit_for_bit(hip, oracle, path):
    """A handle whose replicas all hold one table takes the path of a handle that never made the call: same bits."""
    ref = _reference(oracle)
    T, x, seeds = ref["T"], ref["x"][:3], ref["seeds"]
    tuning = dict(rebuild_interval=6, adapt_interval=0)
    plain = _device(hip, path, [0, 0, 0], x, set_tables=False, **tuning)
    Fp, xp, sp = _forces_and_run(plain, seeds)
    _assert_path(plain, path)
    # every replica set to T0
    same = _device(hip, path, [0, 0, 0], x, set_tables=False, **tuning)
    for r in range(3):
        ensemble.set_ab(same, r, *T[0])
    assert ensemble.classes(same)[1] == 1
    Fs, xs, ss_ = _forces_and_run(same, seeds)
    assert np.array_equal(Fs, Fp) and np.array_equal(xs, xp) and ss_ == sp
    # heterogeneous, evaluated as such, then set_bead_params: the columns replace those of every replica
    het = _device(hip, path, [0, 1, 2], x, **tuning)
    assert not np.array_equal(het.forces(), Fp)
    het.set_bead_params(a=T[0][0], b=T[0][1])
    assert ensemble.classes(het)[1] == 1
    Fh, xh, sh_ = _forces_and_run(het, seeds)
    assert np.array_equal(Fh, Fp) and np.array_equal(xh, xp) and sh_ == sp
    _assert_path(het, path)


# ------------------------------------------------------------------------------------------------ 5: a value fp16 does not hold

@pytest.mark.parametrize("path", list(PATHS))
def test_value_not_exact_in_fp16(hip, oracle, path):
    """One value of one replica that fp16 does not hold: the whole handle runs the generic lists, whatever was asked for."""
    ref = _reference(oracle)
    T, x = ref["T"], ref["x"][:3]
    sh = _device(hip, path, [0, 1, 2], x)
    a2 = T[2][0].copy()
    a2[777] = 0.3
    ensemble.set_ab(sh, 2, a=a2)
    _check_forces(sh, oracle, [T[0], T[1], (a2, T[2][1])], x, "0.3")
    assert sh.context().list_path == 1


# ------------------------------------------------------------------------------------------------ 6: errors

def test_errors_leave_the_tables(hip, oracle):
    ref = _reference(oracle)
    T, x = ref["T"], ref["x"][:3]
    sh = _device(hip, "tiled", [0, 1, 2], x)
    bad = T[2][0].copy()
    bad[N - 1] = np.nan
    for call in (lambda: ensemble.set_ab(sh, 3, *T[2]), lambda: ensemble.set_ab(sh, 1), lambda: ensemble.set_ab(sh, 1, a=T[2][0], b=bad),
                 lambda: ensemble.set_ab(sh, 1, a=bad), lambda: ensemble.get_ab(sh, 3)):
        with pytest.raises(g.GdynError) as e:
            call()
        assert e.value.code == EINVAL, e.value
    for r in range(3):
        a, b = ensemble.get_ab(sh, r)
        assert np.array_equal(a, T[r][0]) and np.array_equal(b, T[r][1]), r
    assert list(ensemble.classes(sh)[0]) == [0, 1, 2]
    Fh = sh.forces()
    for r in range(3):
        _compare_forces(Fh[r], ref["F"][r]["all"], np.abs(ref["F"][r]["all"]).max(), ("after errors", r))
