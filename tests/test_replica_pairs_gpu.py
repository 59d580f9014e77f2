"""Per-replica dynamic pair lists (include/gdyn_replica.h, replica.py) on the device against the oracle.

The oracle has no per-replica lists: its side is always ONE-REPLICA oracle systems, one per replica, each given that replica's
positions, context and lists through set_dynamic_pairs.  Tolerances are the suite's (tests/util.py): forces within FORCE_RTOL of the
largest oracle force of the compared term and replica, energies within ENERGY_RTOL of |E_loops| + |E_glue| (the one-signed parts,
each evaluated on the oracle alone, as test_term_parity_gpu._energy_scale does), positions within POS_ATOL_1STEP / POS_ATOL_20STEP
(x max(1, |x|max / 8) on the 1 kb model, the bound of test_replica_batch_matches_oracle).

Both kernel paths run where a pair list is configured, and the tests assert which one ran."""
import importlib

import numpy as np
import pytest

import stressed_states as ss
from util import ENERGY_RTOL, FORCE_RTOL, PKG, POS_ATOL_1STEP, POS_ATOL_20STEP, g

replica = importlib.import_module(PKG + ".replica")

pytestmark = pytest.mark.gpu
PATHS = {"generic": 1, "tiled": 2}
EINVAL, ESTATE = 1, 5
N_KB, R_KB = 3000, 3
EMPTY = np.zeros((0, 2), dtype=np.uint32)
DYN, ALL = g.TERM_DYNAMIC, g.TERM_ALL


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


def _compare_forces(Fh, Fo, what):
    scale = np.abs(Fo).max()
    err = np.abs(Fh - Fo).max()
    print(f"  {what}: |dF| / max|F| {err / scale:.2e}")
    assert scale > 0 and err <= FORCE_RTOL * scale, (what, err / scale)


# ------------------------------------------------------------------------------------------------ the 1 kb model

def _kb_lists(base):
    """(loops, glues) of replica r = kb_pairs(N, base + r)"""
    return [ss.kb_pairs(N_KB, base + r) for r in range(R_KB)]


def _kb_lists_test1():
    """Replica 1: a hub (bead 1500 glued to 1501 .. 1509 and to 1497: degree >= 10, more than one chunk of four entries) and one glue pair
    listed twice; replica 2: no loops."""
    lists = [list(l) for l in _kb_lists(5)]
    hub = np.array([(1500, j) for j in range(1501, 1510)] + [(1500, 1497)], dtype=np.uint32)
    lists[1][1] = np.concatenate([lists[1][1], hub, lists[1][1][:1]])
    lists[2][0] = EMPTY
    return [tuple(l) for l in lists]


def _kb_device(hip, path, **tuning):
    """The 1 kb model across the box faces, R = 3, its shared slots emptied and per-replica slots 0 = loops, 1 = glue defined"""
    sh = ss.chromatin_1kb_images(hip, shifted=True, n_beads=N_KB, n_replicas=R_KB)
    sh.set_dynamic_pairs(0, ss.KB_LOOP, EMPTY)
    sh.set_dynamic_pairs(1, ss.KB_GLUE, EMPTY)
    sh.set_tuning(kernel_path=PATHS[path], **tuning)
    replica.define(sh, 0, ss.KB_LOOP)
    replica.define(sh, 1, ss.KB_GLUE)
    return sh


def _set_lists(sh, lists):
    for r, (loops, glues) in enumerate(lists):
        replica.set_pairs(sh, 0, r, loops)
        replica.set_pairs(sh, 1, r, glues)


def _kb_oracle(oracle, x_r, loops, glues):
    so = ss.chromatin_1kb_images(oracle, shifted=True, n_beads=N_KB, n_replicas=1)
    so.set_positions(x_r[None])
    so.set_dynamic_pairs(0, ss.KB_LOOP, loops)
    so.set_dynamic_pairs(1, ss.KB_GLUE, glues)
    return so


def _dyn_energy_scale(so, loops, glues, p_loop, p_glue):
    """|E_loops| + |E_glue| of a one-replica oracle; its lists are put back"""
    so.set_dynamic_pairs(1, p_glue, EMPTY)
    e_loops = abs(so.energy(DYN)[0])
    so.set_dynamic_pairs(1, p_glue, glues)
    so.set_dynamic_pairs(0, p_loop, EMPTY)
    e_glue = abs(so.energy(DYN)[0])
    so.set_dynamic_pairs(0, p_loop, loops)
    return e_loops + e_glue


_kb_ref = {}


def _kb_reference(oracle):
    """The oracle side of tests 1 and 3, computed once: positions, per replica the dynamic and total forces, the dynamic energy and its
    scale, under the lists of test 1; replica 0 under replica 1's lists; whether a glue pair acts across a face."""
    if _kb_ref:
        return _kb_ref
    s3 = ss.chromatin_1kb_images(oracle, shifted=True, n_beads=N_KB, n_replicas=R_KB)
    x, box = s3.positions(), np.array(s3.box)
    s3.close()
    lists = _kb_lists_test1()
    Fd, Fa, E, S, across = [], [], [], [], False
    for r, (loops, glues) in enumerate(lists):
        so = _kb_oracle(oracle, x[r], loops, glues)
        Fd.append(so.forces(DYN)[0]); Fa.append(so.forces(ALL)[0]); E.append(so.energy(DYN)[0])
        S.append(_dyn_energy_scale(so, loops, glues, ss.KB_LOOP, ss.KB_GLUE))
        # every non-empty part acts
        so.set_dynamic_pairs(1, ss.KB_GLUE, EMPTY)
        assert len(loops) == 0 or np.abs(so.forces(DYN)).max() > 0
        so.set_dynamic_pairs(1, ss.KB_GLUE, glues)
        so.set_dynamic_pairs(0, ss.KB_LOOP, EMPTY)
        Fg = so.forces(DYN)[0]
        assert np.abs(Fg).max() > 0
        raw = x[r][glues[:, 0]] - x[r][glues[:, 1]]
        crosses = np.any(np.abs(raw) > box / 2, axis=1)
        acts = np.abs(Fg[glues[:, 0]]).max(axis=1) > 0
        across |= bool(np.any(crosses & acts))
        so.close()
    so = _kb_oracle(oracle, x[0], *lists[1])
    mixup = np.abs(so.forces(DYN)[0] - Fd[0]).max()
    so.close()
    _kb_ref.update(x=x, lists=lists, Fd=Fd, Fa=Fa, E=E, S=S, across=across, mixup=mixup)
    return _kb_ref


@pytest.mark.parametrize("path", list(PATHS))
def test_forces_and_energies_periodic(hip, oracle, path):
    ref = _kb_reference(oracle)
    # the preconditions, on the oracle alone: a replica mix-up would be visible, and a glue pair acts across a box face
    assert ref["mixup"] > 100 * FORCE_RTOL * np.abs(ref["Fd"][0]).max()
    assert ref["across"]
    sh = _kb_device(hip, path)
    _set_lists(sh, ref["lists"])
    Fd, Fa, E = sh.forces(DYN), sh.forces(ALL), sh.energy(DYN)
    for r in range(R_KB):
        _compare_forces(Fd[r], ref["Fd"][r], ("dynamic", r))
        _compare_forces(Fa[r], ref["Fa"][r], ("all", r))
        print(f"  energy r{r}: |dE| / S {abs(E[r] - ref['E'][r]) / ref['S'][r]:.2e}")
        assert abs(E[r] - ref["E"][r]) <= ENERGY_RTOL * ref["S"][r], (r, E[r], ref["E"][r], ref["S"][r])
    _assert_path(sh, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_same_lists_through_both_apis(hip, oracle, path):
    """Identical lists for all replicas: per-replica slots on one handle, set_dynamic_pairs on another."""
    ref = _kb_reference(oracle)
    loops, glues = ref["lists"][1]
    sa = _kb_device(hip, path)
    _set_lists(sa, [(loops, glues)] * R_KB)
    sb = ss.chromatin_1kb_images(hip, shifted=True, n_beads=N_KB, n_replicas=R_KB)
    sb.set_tuning(kernel_path=PATHS[path])
    sb.set_dynamic_pairs(0, ss.KB_LOOP, loops)
    sb.set_dynamic_pairs(1, ss.KB_GLUE, glues)
    Ea, Eb = sa.energy(DYN), sb.energy(DYN)
    for m, what in ((DYN, "dynamic"), (ALL, "all")):
        Fa, Fb = sa.forces(m), sb.forces(m)
        for r in range(R_KB):
            so = _kb_oracle(oracle, ref["x"][r], loops, glues)
            Fo = so.forces(m)[0]
            _compare_forces(Fa[r], Fo, (what, "per-replica", r))
            _compare_forces(Fb[r], Fo, (what, "shared", r))
            assert np.abs(Fa[r] - Fb[r]).max() <= FORCE_RTOL * np.abs(Fo).max()
            if m == DYN:
                Eo, S = so.energy(DYN)[0], _dyn_energy_scale(so, loops, glues, ss.KB_LOOP, ss.KB_GLUE)
                assert abs(Ea[r] - Eo) <= ENERGY_RTOL * S and abs(Eb[r] - Eo) <= ENERGY_RTOL * S and abs(Ea[r] - Eb[r]) <= ENERGY_RTOL * S
            so.close()
    _assert_path(sa, path)
    _assert_path(sb, path)


# ------------------------------------------------------------------------------------------------ the composite model (open box)

NO_DYN = ALL & ~DYN


def _composite_lists():
    """Replica 0: loop_pairs() / glue_pairs(); replica 1: every other pair of each, in reversed order"""
    lo, gl = ss.loop_pairs(), ss.glue_pairs()
    return [(lo, gl), (lo[::2][::-1].copy(), gl[::2][::-1].copy())]


def _composite_device(hip, terms):
    sh = ss.composite(hip, terms=terms)
    if terms & DYN:      # (a dynamic-only copy: its shared slots emptied, the pairs come per replica)
        sh.set_dynamic_pairs(0, ss.LOOP, EMPTY)
        sh.set_dynamic_pairs(1, ss.GLUE, EMPTY)
    replica.define(sh, 0, ss.LOOP)       # mixed, scaled with the replica's bond_scale
    replica.define(sh, 1, ss.GLUE)
    for r, (lo, gl) in enumerate(_composite_lists()):
        replica.set_pairs(sh, 0, r, lo)
        replica.set_pairs(sh, 1, r, gl)
    return sh


def _composite_oracle(oracle, terms, r):
    """One-replica oracle of replica r: its positions, its (bead_scale, bond_scale), its lists in the shared slots"""
    so = ss.composite(oracle, terms=terms & ~DYN, n_replicas=1)
    lo, gl = _composite_lists()[r]
    so.set_dynamic_pairs(0, ss.LOOP, lo)
    so.set_dynamic_pairs(1, ss.GLUE, gl)
    so.set_positions(ss.f32(ss.composite_positions(11, r))[None])
    so.set_context(0, 0, *ss.COMPOSITE_SCALES[r])
    return so


@pytest.mark.parametrize("path", list(PATHS))
def test_forces_and_energies_open_box(hip, oracle, path):
    """mix, scale_by_bond_scale with a per-replica scale, non-uniform mobility (the composite model), next to every other term"""
    sh = _composite_device(hip, NO_DYN)
    sh.set_tuning(kernel_path=PATHS[path])
    Fd, Fa, E = sh.forces(DYN), sh.forces(ALL), sh.energy(DYN)
    for r in range(2):
        so = _composite_oracle(oracle, ALL, r)
        lo, gl = _composite_lists()[r]
        _compare_forces(Fd[r], so.forces(DYN)[0], ("dynamic", r))
        _compare_forces(Fa[r], so.forces(ALL)[0], ("all", r))
        Eo, S = so.energy(DYN)[0], _dyn_energy_scale(so, lo, gl, ss.LOOP, ss.GLUE)
        print(f"  energy r{r}: |dE| / S {abs(E[r] - Eo) / S:.2e}")
        assert S > 0 and abs(E[r] - Eo) <= ENERGY_RTOL * S, (r, E[r], Eo, S)
    _assert_path(sh, path)


def test_step_mode(hip, oracle):
    """One zero-noise, T = 0 step of a dynamic-only copy of the composite model: (x1 - x0) / (mu dt) is the force the step used (a wrong
    slot order, mobility or replica in the position update shows); then an uncompensated step on positions."""
    mu = np.array(ss.MOBILITY)[np.arange(ss.N_COMPOSITE) % 3][:, None]
    sh = _composite_device(hip, DYN)
    x0 = sh.positions()
    dt = 1e-5
    sh.run(1, dt, 0.0, noise=g.NOISE_ZERO, flags=g.RUN_COMPENSATED)
    assert sh.context().compensated == 1 and sh.context().step == 1
    x1 = sh.positions()
    for r in range(2):
        so = _composite_oracle(oracle, DYN, r)
        assert np.array_equal(so.positions()[0], x0[r])
        Fo = so.forces(DYN)[0]
        assert np.array_equal(Fo, so.forces(ALL)[0])                     # the isolated copy configures this term alone
        _compare_forces((x1[r] - x0[r]) / (mu * dt), Fo, ("step", r))
    sh = _composite_device(hip, DYN)
    dt = 1e-3
    sh.run(1, dt, 0.0, noise=g.NOISE_ZERO, flags=g.RUN_UNCOMPENSATED)
    assert sh.context().compensated == 0
    x1 = sh.positions()
    for r in range(2):
        so = _composite_oracle(oracle, DYN, r)
        so.run(1, dt, 0.0, noise=g.NOISE_ZERO)
        xo = so.positions()[0]
        assert np.abs(xo - x0[r]).max() > 100 * POS_ATOL_1STEP           # (the step moves beads by far more than the bound)
        err = np.abs(x1[r] - xo).max()
        print(f"  uncompensated step r{r}: |dx| {err:.2e}")
        assert err <= POS_ATOL_1STEP, (r, err)


# ------------------------------------------------------------------------------------------------ trajectories

KB_DT, KB_KT = 1e-4, 1.0          # the model's timestep and temperature (workloads.chromatin_1kb)
SEEDS = [11, 12, 13]


def _updated_lists():
    lists = [list(l) for l in _kb_lists(40)]
    lists[0][1] = EMPTY            # replica 0's glue list emptied
    return [tuple(l) for l in lists]


def _oracle_trajectory(oracle, x, segments, kT, noise, dt=KB_DT):
    """Three one-replica oracle runs: segments = [(lists of every replica, steps), ...]; the final positions (R, N, 3)"""
    out = []
    for r in range(R_KB):
        so = None
        for lists, steps in segments:
            if so is None:
                so = _kb_oracle(oracle, x[r], *lists[r])
            else:
                so.set_dynamic_pairs(0, ss.KB_LOOP, lists[r][0])
                so.set_dynamic_pairs(1, ss.KB_GLUE, lists[r][1])
            so.run(steps, dt, kT, seed=SEEDS[r], noise=noise)
        out.append(so.positions()[0])
        so.close()
    return np.stack(out)


def _assert_positions(sh, xo):
    err = np.abs(sh.positions() - xo).max()
    bound = POS_ATOL_20STEP * max(1.0, np.abs(xo).max() / 8)
    print(f"  |dx| vs oracle {err:.2e} (bound {bound:.1e})")
    assert err <= bound, (err, bound)


_traj_ref = {}


def _philox_reference(oracle):
    """6 steps under the lists of test 1, new lists, 6 more steps: shared by the trajectory and the rollback test"""
    if not _traj_ref:
        ref = _kb_reference(oracle)
        _traj_ref["x"] = _oracle_trajectory(oracle, ref["x"], [(ref["lists"], 6), (_updated_lists(), 6)], KB_KT, g.NOISE_PHILOX)
    return _traj_ref["x"]


@pytest.mark.parametrize("path", list(PATHS))
def test_trajectory_with_updates_and_philox_noise(hip, oracle, path):
    ref = _kb_reference(oracle)
    xo = _philox_reference(oracle)
    sh = _kb_device(hip, path)
    _set_lists(sh, ref["lists"])
    sh.run(6, KB_DT, KB_KT, seed=999, replica_seeds=SEEDS)
    _set_lists(sh, _updated_lists())
    assert replica.count(sh, 1, 0) == 0 and replica.count(sh, 1, 1) == 60
    sh.run(6, KB_DT, KB_KT, seed=999, replica_seeds=SEEDS)
    assert sh.context().step == 12
    _assert_positions(sh, xo)
    assert np.abs(xo[0] - xo[1]).max() > 1e-4
    _assert_path(sh, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_an_update_keeps_the_resident_list(hip, oracle, path):
    """A fixed interval of 8: builds at steps 0 and 8, so the tenth step is the second on its list.  New lists before it must cost no
    build.  The timestep is a hundredth of the model's: the chain bonds of this state cross the box unimaged and pull a shifted bead with
    forces up to 1.6e4, which at T = 0 move it 0.016 per step at 1e-6 -- eight steps stay within a quarter of the margin of 0.56, where
    the model's 1e-4 would violate every interval and have it cut.  The update still moves beads by 6e-4 in the tenth step, beyond the
    position bound (asserted on the oracle)."""
    ref = _kb_reference(oracle)
    dt = 0.01 * KB_DT
    sh = _kb_device(hip, path, rebuild_interval=8, adapt_interval=0)
    _set_lists(sh, ref["lists"])
    sh.forces()                                        # (sizes the lists: a run that has to widen its first list rolls a chunk back)
    sh.run(9, dt, 0.0, noise=g.NOISE_ZERO)
    c = sh.context()
    rebuilds = c.rebuilds
    print(f"  after 9 steps: rebuilds {c.rebuilds}, rollbacks {c.rollbacks}, interval {c.rebuild_interval}")
    assert rebuilds >= 2 and c.rollbacks == 0 and c.rebuild_interval == 8
    _set_lists(sh, _updated_lists())
    sh.run(1, dt, 0.0, noise=g.NOISE_ZERO)
    c = sh.context()
    assert c.rebuilds == rebuilds and c.rollbacks == 0 and c.step == 10
    xo = _oracle_trajectory(oracle, ref["x"], [(ref["lists"], 9), (_updated_lists(), 1)], 0.0, g.NOISE_ZERO, dt=dt)
    stale = _oracle_trajectory(oracle, ref["x"], [(ref["lists"], 10)], 0.0, g.NOISE_ZERO, dt=dt)
    assert np.abs(stale - xo).max() > 2 * POS_ATOL_20STEP * max(1.0, np.abs(xo).max() / 8)      # (the old lists in step 10 would show)
    _assert_positions(sh, xo)
    _assert_path(sh, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_rollback_reapplies_the_same_lists(hip, oracle, path):
    """A pinned skin of 0.02 cutoffs (a margin of 0.015) at a fixed interval of 6: the thermal step of this model, 0.014 per axis, breaks
    it at the first check, the chunk is rolled back and re-run at shorter intervals down to 1, where every step has a fresh list.  The
    lists are outside the snapshot: the re-run chunk uses them unchanged, and the trajectory is the oracle's."""
    ref = _kb_reference(oracle)
    xo = _philox_reference(oracle)
    sh = _kb_device(hip, path, skin=0.02, rebuild_interval=6, adapt_interval=0)
    _set_lists(sh, ref["lists"])
    sh.run(6, KB_DT, KB_KT, seed=999, replica_seeds=SEEDS)
    _set_lists(sh, _updated_lists())
    sh.run(6, KB_DT, KB_KT, seed=999, replica_seeds=SEEDS)
    c = sh.context()
    print(f"  rollbacks {c.rollbacks}, interval {c.rebuild_interval}")
    assert c.rollbacks > 0 and c.step == 12
    _assert_positions(sh, xo)
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ arguments and state

def test_arguments_and_state(hip):
    dll = replica.load_replica_library()
    assert dll.gd_replica_abi_version() == replica.REPLICA_ABI_VERSION
    sh = ss.chromatin_1kb_images(hip, shifted=True, n_beads=N_KB, n_replicas=R_KB)
    sh.set_dynamic_pairs(0, ss.KB_LOOP, EMPTY)
    sh.set_dynamic_pairs(1, ss.KB_GLUE, EMPTY)
    loops, glues = ss.kb_pairs(N_KB, 5)

    def code(call):
        with pytest.raises(g.GdynError) as e:
            call()
        return e.value.code

    # before any slot is defined
    assert code(lambda: replica.set_pairs(sh, 0, 0, loops)) == ESTATE
    assert code(lambda: replica.count(sh, 0, 0)) == ESTATE
    replica.define(sh, 0, ss.KB_LOOP)
    replica.define(sh, 1, ss.KB_GLUE)
    assert np.all(sh.forces(DYN) == 0)                       # defined, empty: exactly zero
    assert np.all(sh.energy(DYN) == 0)
    replica.set_pairs(sh, 0, 1, loops)
    replica.set_pairs(sh, 1, 2, glues)
    F0 = sh.forces(DYN)
    assert np.all(F0[0] == 0) and np.abs(F0[1]).max() > 0 and np.abs(F0[2]).max() > 0
    counts = lambda: [[replica.count(sh, s, r) for r in range(R_KB)] for s in (0, 1)]
    c0 = counts()
    assert c0 == [[0, 30, 0], [0, 0, 60]]
    P = g.System.bond_params
    one = np.array([[0, 1]], dtype=np.uint32)
    bad = [
        (EINVAL, lambda: dll.gd_replica_pairs_define(None, 0, None)),
        (EINVAL, lambda: dll.gd_replica_pairs_define(sh._h, 0, None)),
        (EINVAL, lambda: dll.gd_replica_pairs_set(sh._h, 0, 0, None, 1)),
        (EINVAL, lambda: dll.gd_replica_pairs_count(sh._h, 0, 0, None)),
        (EINVAL, lambda: code(lambda: replica.define(sh, 4, ss.KB_LOOP))),
        (EINVAL, lambda: code(lambda: replica.define(sh, 0, P(g.POT_SOFTCORE, k_a=-1.0, l_a=1.5, p=8, q=3, mix=True)))),
        (EINVAL, lambda: code(lambda: replica.define(sh, 0, P(g.POT_SOFTCORE, k_a=-1.0, l_a=1.5, p=8, q=3, scale_by_bond_scale=True)))),
        (EINVAL, lambda: code(lambda: replica.define(sh, 0, P(g.POT_SOFTCORE, k_a=-1.0, l_a=1.5, p=3, q=3)))),
        (EINVAL, lambda: code(lambda: replica.set_pairs(sh, 4, 0, one))),
        (EINVAL, lambda: code(lambda: replica.set_pairs(sh, 0, R_KB, one))),
        (EINVAL, lambda: code(lambda: replica.set_pairs(sh, 0, 1, np.array([[0, 1], [5, N_KB]], dtype=np.uint32)))),
        (EINVAL, lambda: code(lambda: replica.set_pairs(sh, 0, 1, np.array([[0, 1], [7, 7]], dtype=np.uint32)))),
        (ESTATE, lambda: code(lambda: replica.set_pairs(sh, 2, 0, one))),
        (ESTATE, lambda: code(lambda: replica.count(sh, 3, 0))),
        (EINVAL, lambda: code(lambda: replica.count(sh, 4, 0))),
        (EINVAL, lambda: code(lambda: replica.count(sh, 0, R_KB))),
    ]
    for k, (want, call) in enumerate(bad):
        assert call() == want, k
        assert counts() == c0, k
        assert np.array_equal(sh.forces(DYN), F0), k          # the previous lists and parameters stay in force
    # define again: new parameters, the lists kept (harmonic: the forces follow the spring constant)
    replica.define(sh, 2, P(g.POT_HARMONIC, k_a=3.0))
    replica.set_pairs(sh, 2, 0, loops)
    F1 = sh.forces(DYN)
    assert np.abs(F1[0]).max() > 0 and np.array_equal(F1[1:], F0[1:])
    replica.define(sh, 2, P(g.POT_HARMONIC, k_a=6.0))
    assert replica.count(sh, 2, 0) == 30
    F2 = sh.forces(DYN)
    assert np.allclose(F2[0], 2.0 * F1[0], rtol=1e-6, atol=0) and np.array_equal(F2[1:], F0[1:])
    # emptied again: exactly zero
    for s in range(3):
        for r in range(R_KB):
            replica.set_pairs(sh, s, r, EMPTY)
    assert np.all(sh.forces(DYN) == 0)
    sh.close()
    # a second handle after the first is gone
    s2 = ss.chromatin_1kb_images(hip, shifted=True, n_beads=N_KB, n_replicas=2)
    assert code(lambda: replica.count(s2, 0, 0)) == ESTATE   # (nothing carried over)
    replica.define(s2, 3, ss.KB_GLUE)
    replica.set_pairs(s2, 3, 1, glues)
    assert replica.count(s2, 3, 1) == 60
    s2.run(2, KB_DT, KB_KT, seed=3)
    assert s2.context().step == 2
    s2.close()
