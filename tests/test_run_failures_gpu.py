"""gd_run where it does not succeed, or succeeds only after rollbacks (csrc/gdyn_capi.hip: rollback_chunk; csrc/gdyn_policy.hpp:
ListPolicy::on_violation), and what the handle is worth afterwards.  The drivers in host/ catch GD_ESTATE and then read positions
and energies for a last snapshot: a refused run has to leave the handle at the last accepted chunk, with nothing left of the rejected
one -- positions, the compensated residuals, the per-replica context, the bead order, the lists.

The tool is injected noise (noise=NOISE_HOST): one variate of one bead at one step is made large, so the displacement that breaks the
Verlet skin is deterministic, finite and a few length units at most.  Sizes follow from the policy's own numbers:

  * margin: a list holds while no bead has moved more than (list radius - cutoff) / 2 since its build; with the default skin of
    0.75 nominal cutoffs of 0.30 that is 0.1125 (read from context().list_radius below, not assumed);
  * the skin widens by 1.5 per violation at K = 1: 0.75, 1.125, ... 8.54, the first above 8, whose margin would be 1.28;
  * the interval shrinks K -> K - max(1, K / 4) per violation at K > 1; gd_run gives a chunk up at its 25th rollback.

What a kick can and cannot reach.  k_step checks a bead's displacement since the build when it EVALUATES FORCES, i.e. at the step after
the one that moved the bead.  At K = 1 that step has a fresh list, whatever the displacement: a kick at K = 1 costs no rollback, and the
exit "Verlet skin cannot cover one step" is not reachable by a displacement at all (test_a_kick_at_interval_one_needs_no_rollback pins
that).  A violation at K = 1 needs a margin that is not positive; a skin below the fp32 resolution of the cutoff is one, and it is how
the widening branch is reached here.  The refused-run properties are checked through the exit that a kick does reach: the chunk
given up after 25 rollbacks."""
import math

import numpy as np
import pytest

from util import CASES, ENERGY_RTOL, FORCE_RTOL, POS_ATOL_20STEP, TERMS, build, g

pytestmark = pytest.mark.gpu
SEED = 20220101
PATHS = {"generic": 1, "tiled": 2}
CUT = 0.30                       # nominal pair cutoff of both models (the larger soft-core diameter)
SKIN0, SKIN_GROWTH, SKIN_MAX = 0.75, 1.5, 8.0      # gdyn_policy.hpp: ListPolicy::skin, on_violation
GIVE_UP_AT = 25                  # rollback_chunk: retries > 24
ESTATE = 5


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


def _largest_margin():
    """Margin of the widest skin on_violation tries: the first of 0.75 x 1.5^n above 8."""
    skin = SKIN0
    while not skin > SKIN_MAX:
        skin *= SKIN_GROWTH
    return 0.5 * skin * CUT


def _intervals(K):
    """K and what on_violation makes of it, down to 1."""
    out = [K]
    while K > 1:
        K = max(1, K - max(1, K // 4))
        out.append(K)
    return out


def _violates(K, j):
    """A kick in the noise of step j of a chunk (lists built at the chunk's steps 0, K, 2K, ...) is seen by the force evaluation of
    step j + 1 -- unless that step begins with a build."""
    return (j + 1) % K != 0


def _interval_that_gives_up(j):
    """Smallest rebuild interval from which a kick at step j of a chunk violates the skin at K and at each of the 24 intervals
    after it: the chunk's 25th rollback is the one gd_run gives up at."""
    K0 = 2
    while True:
        ks = _intervals(K0)[:GIVE_UP_AT]
        if len(ks) == GIVE_UP_AT and all(_violates(K, j) for K in ks):
            return K0
        K0 += 1


def _sigma(dt, kT):
    return math.sqrt(2.0 * kT * dt)          # per step and axis, mobility 1 (both models)


def _kick(z, step, replica, bead, length, dt, kT):
    """The variates of one bead at one step: `length` along x (an fp32 value: the device takes the noise as float)."""
    z[step, replica, bead] = (float(np.float32(length / _sigma(dt, kT))), 0.0, 0.0)


def _current_margin(s, scaled):
    c = s.context()
    return 0.5 * (c.list_radius - CUT * (c.bead_scale if scaled else 1.0))


def _ctx_tuple(c):
    return (c.step, c.time, c.bead_scale, c.bond_scale, tuple(c.semiaxes))


def _assert_state_matches(sh, so, steps, wall):
    """Positions and context of every replica against the oracle's: the tolerances of test_injected_noise_trajectory and
    test_rollback_with_replicas."""
    xh, xo = sh.positions(), so.positions()
    scale = max(1.0, np.abs(xo).max() / 8)
    err = np.abs(xh - xo).max()
    print(f"  |dx| vs oracle at step {steps}: {err:.2e} (bound {POS_ATOL_20STEP * scale:.1e})")
    assert err <= POS_ATOL_20STEP * scale, err
    for r in range(sh.R):
        ch, co = sh.context(r), so.context(r)
        assert ch.step == co.step == steps, (r, ch.step, co.step)
        assert ch.time == pytest.approx(co.time, rel=1e-12)
        assert ch.bead_scale == pytest.approx(co.bead_scale, rel=1e-12) and ch.bond_scale == pytest.approx(co.bond_scale, rel=1e-12)
        if wall:
            assert np.allclose(np.array(ch.semiaxes), np.array(co.semiaxes), rtol=0, atol=1e-8), r


def _assert_observations_match(sh, oracle, name, over, wall, box):
    """forces(), energy() and the pair set of search_pairs(0.3) on the handle against an oracle at the handle's own positions and
    contexts.  The first of them has to build a list: a handle that still believed in the list of the rejected chunk would not."""
    xh = sh.positions()
    sf, *_ = build(oracle, name, n_replicas=sh.R, **over)
    sf.set_positions(xh)
    for r in range(sh.R):
        c = sh.context(r)
        sf.set_context(r, c.step, c.bead_scale, c.bond_scale, list(c.semiaxes) if wall else None)
    rb = sh.context().rebuilds
    Fh, Fo = sh.forces(), sf.forces()
    assert sh.context().rebuilds > rb, "forces() on a handle whose run was refused must build its list"
    ferr = np.abs(Fh - Fo).max() / np.abs(Fo).max()
    print(f"  |dF|/max|F| {ferr:.2e}")
    assert ferr <= FORCE_RTOL
    Eh, Eo = sh.energy(), sf.energy()
    escale = sum(np.abs(sf.energy(m)) for t, m in TERMS.items() if t != "all")
    assert np.all(np.abs(Eh - Eo) <= ENERGY_RTOL * escale), (Eh, Eo, escale)
    for r in range(sh.R):
        ph = {tuple(p) for p in sh.search_pairs(CUT, replica=r)}
        po = {tuple(p) for p in sf.search_pairs(CUT, replica=r)}
        assert len(po) > 50
        for i, j in ph ^ po:          # only pairs within fp32 rounding of the cutoff may differ
            d = xh[r][i] - xh[r][j]
            if box is not None:
                d -= box * np.rint(d / box)
            assert abs(np.linalg.norm(d) - CUT) < 1e-6
    sf.close()


# ------------------------------------------------------------------------------------------------ 1. rollbacks a run recovers from

@pytest.mark.parametrize("nrep", [1, 3])
@pytest.mark.parametrize("path", ["generic", "tiled"])
def test_a_kick_at_interval_one_needs_no_rollback(hip, oracle, path, nrep):
    """rebuild_interval = 1: a bead kicked by 2.5 margins at step 5 of 10 meets a fresh list at step 6.  No rollback, the interval
    and the list radius stay, and the trajectory (kick included) is the oracle's."""
    _run_with_a_kick(hip, oracle, path, nrep, interval=1, kick_step=4, rollbacks=0, interval_after=1)


@pytest.mark.parametrize("nrep", [1, 3])
@pytest.mark.parametrize("path", ["generic", "tiled"])
def test_a_kick_rolls_back_to_interval_one_and_the_run_recovers(hip, oracle, path, nrep):
    """rebuild_interval = 2: the same kick in the first step of an interval is seen by the second.  One rollback, K = 1 from there
    (the last cut of on_violation's K > 1 branch), the run returns OK and every replica -- only replica 1 of 3 is kicked -- is the
    oracle's."""
    _run_with_a_kick(hip, oracle, path, nrep, interval=2, kick_step=4, rollbacks=1, interval_after=1)


def _run_with_a_kick(hip, oracle, path, nrep, interval, kick_step, rollbacks, interval_after):
    _, _, dt, kT, flags = CASES["genome"]
    sh, *_ = build(hip, "genome", n_replicas=nrep)
    so, *_ = build(oracle, "genome", n_replicas=nrep)
    sh.set_tuning(kernel_path=PATHS[path], rebuild_interval=interval, adapt_interval=0)
    for s in (sh, so):
        s.begin_phase()
    sh.forces()                                        # (a list, for its radius)
    margin = _current_margin(sh, scaled=True)
    assert abs(margin - 0.5 * SKIN0 * CUT) < 2e-3, margin
    kick = 2.5 * margin
    assert margin < kick < _largest_margin()
    z = np.random.default_rng(SEED).normal(size=(10, nrep, sh.N, 3))
    replica, bead = (1 if nrep > 1 else 0), sh.N // 2
    _kick(z, kick_step, replica, bead, kick, dt, kT)
    c0 = sh.context()
    for s in (sh, so):
        s.run(10, dt, kT, noise=g.NOISE_HOST, host_noise=z, flags=flags)       # returns OK
    c1 = sh.context()
    print(f"  margin {margin:.4f}, kick {kick:.4f}, rollbacks {c1.rollbacks - c0.rollbacks}, K {c1.rebuild_interval}, "
          f"list radius {c0.list_radius:.4f} -> {c1.list_radius:.4f}")
    _assert_path(sh, path)
    assert c1.rollbacks - c0.rollbacks == rollbacks
    assert c1.rebuild_interval == interval_after
    assert abs(c1.list_radius - c0.list_radius) < 1e-3          # (no wider skin)
    _assert_state_matches(sh, so, 10, wall=True)


@pytest.mark.parametrize("path", ["generic", "tiled"])
def test_a_margin_of_zero_widens_the_skin_at_interval_one_and_the_run_recovers(hip, oracle, path):
    """The K = 1 branch of on_violation: a skin of 1e-9 cutoffs is below half an ulp of the fp32 list radius, the margin is zero and
    every step violates it, whatever the beads do.  Each rollback widens the skin by 1.5 until the radius is an ulp above the
    cutoff; the run returns OK on lists that hold just the cutoff (complete at K = 1) and is the oracle's."""
    _, _, dt, kT, flags = CASES["ab_box"]
    sh, *_ = build(hip, "ab_box", n_replicas=3)
    so, *_ = build(oracle, "ab_box", n_replicas=3)
    skin = 1e-9
    sh.set_tuning(skin=skin, kernel_path=PATHS[path], rebuild_interval=1, adapt_interval=0)
    cut32 = np.float32(CUT)
    radius = lambda sk: np.float32(np.float64(cut32) * (1.0 + sk))       # list_radius() of gdyn_capi.hip
    expected = 0
    while not radius(skin * SKIN_GROWTH ** expected) > cut32:
        expected += 1
    assert 1 <= expected < GIVE_UP_AT - 1, expected
    z = np.random.default_rng(SEED + 1).normal(size=(10, 3, sh.N, 3))
    for s in (sh, so):
        s.begin_phase()
    c0 = sh.context()
    for s in (sh, so):
        s.run(10, dt, kT, noise=g.NOISE_HOST, host_noise=z, flags=flags)       # returns OK
    c1 = sh.context()
    print(f"  rollbacks {c1.rollbacks - c0.rollbacks} (expected {expected}), list radius {c1.list_radius!r}, K {c1.rebuild_interval}")
    _assert_path(sh, path)
    assert c1.rollbacks - c0.rollbacks == expected
    assert c1.rebuild_interval == 1 and c1.list_radius == float(radius(skin * SKIN_GROWTH ** expected)) and c1.list_radius > float(cut32)
    _assert_state_matches(sh, so, 10, wall=False)


# ------------------------------------------------------------------------------------------------ 2., 3., 5. a run that is refused

def _refused_run(sh, steps, dt, kT, z, flags):
    with pytest.raises(g.GdynError) as e:
        sh.run(steps, dt, kT, noise=g.NOISE_HOST, host_noise=z, flags=flags)
    assert e.value.code == ESTATE and "giving up" in str(e.value) and "skin violation" in str(e.value), str(e.value)


@pytest.mark.parametrize("comp", ["compensated", "uncompensated"])
@pytest.mark.parametrize("path", ["generic", "tiled"])
def test_a_run_given_up_leaves_the_handle_at_the_last_accepted_chunk(hip, oracle, path, comp):
    """Three replicas of the genome model with moving scales and wall; 10 ordinary steps, then a 10-step run whose step 6 kicks one
    bead of replica 1 by two length units -- beyond the margin of any skin -- at a rebuild interval from which 25 cuts do not reach an
    interval that would hide the kick: the chunk is rolled back 25 times and given up, GD_ESTATE.

    The handle then stands at step 10, all replicas: positions (bit for bit what they were, residuals of the compensated update
    included), context, forces, energies and pair set are those of the oracle after 10 steps; the interval and the width of the
    lists are what they were before the refused run (the policy's state is rolled back too); and the handle runs on, as the oracle
    does -- at the fine timestep of the compensated update to the agreement test_fp64_positions_survive_... requires, which residuals
    of other positions would miss."""
    _, _, dt, kT, flags = CASES["genome"]
    over = dict(n_beads=600)
    R = 3
    cflag = g.RUN_COMPENSATED if comp == "compensated" else g.RUN_UNCOMPENSATED
    sh, *_ = build(hip, "genome", n_replicas=R, **over)
    so, *_ = build(oracle, "genome", n_replicas=R, **over)
    N = sh.N
    rng = np.random.default_rng(SEED + 2)
    z1, z2, z3 = (rng.normal(size=(n, R, N, 3)) for n in (10, 10, 5))
    sh.set_tuning(kernel_path=PATHS[path], rebuild_interval=4, adapt_interval=0)
    for s in (sh, so):
        s.begin_phase()
    sh.run(10, dt, kT, noise=g.NOISE_HOST, host_noise=z1, flags=flags | cflag)
    so.run(10, dt, kT, noise=g.NOISE_HOST, host_noise=z1, flags=flags)
    _assert_path(sh, path)
    assert sh.context().compensated == (1 if comp == "compensated" else 0)

    kick_step, bead, kick = 5, N // 2, 2.0
    assert kick > _largest_margin()
    K0 = _interval_that_gives_up(kick_step)
    sh.set_tuning(kernel_path=PATHS[path], rebuild_interval=K0, adapt_interval=0)
    _kick(z2, kick_step, 1, bead, kick, dt, kT)
    before = [sh.context(r) for r in range(R)]
    per_bead = [c.list_entries / N for c in before]
    xb = sh.positions()
    _refused_run(sh, 10, dt, kT, z2, flags | cflag)

    after = [sh.context(r) for r in range(R)]
    s0 = after[0].step
    assert all(c.step == s0 for c in after) and 10 <= s0 <= 15
    assert s0 == 10          # (a 10-step run is one chunk)
    print(f"  K0 {K0}, rollbacks {after[0].rollbacks - before[0].rollbacks}, K after {after[0].rebuild_interval}, "
          f"list radius {before[0].list_radius:.4f} -> {after[0].list_radius:.4f}")
    assert after[0].rollbacks - before[0].rollbacks == GIVE_UP_AT
    xa = sh.positions()
    assert np.array_equal(xa, xb), np.abs(xa - xb).max()
    assert abs(xa[1, bead, 0] - so.positions()[1, bead, 0]) < 1e-3 * kick
    for a, b in zip(after, before):
        assert _ctx_tuple(a) == _ctx_tuple(b)
    assert after[0].rebuild_interval == before[0].rebuild_interval == K0          # the policy's state is rolled back as well
    _assert_state_matches(sh, so, s0, wall=True)
    _assert_observations_match(sh, oracle, "genome", over, wall=True, box=None)

    if comp == "compensated":
        so.set_positions(xb)          # the oracle from the handle's fp64 positions: what follows measures displacements of ~1e-4
        for s, fl in ((sh, flags | cflag), (so, flags)):
            s.run(50, 1e-7, 0.0, seed=3, flags=fl)          # (50 steps: median 4.1e-5, bound 8.3e-8 -- measured 1.8e-9, with stale residuals 1.15e-7)
        assert sh.context().compensated == 1
        dh, do = sh.positions() - xb, so.positions() - xb
        print(f"  fine timestep: |dh - do| {np.abs(dh - do).max():.2e}, median |do| {np.median(np.abs(do)):.2e}")
        assert np.abs(dh - do).max() <= 2e-3 * np.median(np.abs(do)), (np.abs(dh - do).max(), np.median(np.abs(do)))
        s0 += 50
    sh.run(5, dt, kT, noise=g.NOISE_HOST, host_noise=z3, flags=flags | cflag)
    so.run(5, dt, kT, noise=g.NOISE_HOST, host_noise=z3, flags=flags)
    _assert_path(sh, path)
    _assert_state_matches(sh, so, s0 + 5, wall=True)
    # the lists of the continuation are those of the handle before the refused run: as many entries per bead (they grow with the
    # cube of the radius: a skin widened once, x 1.5, would nearly double them), the same radius to the growth of the bead scale
    end = [sh.context(r) for r in range(R)]
    per_bead_end = [c.list_entries / N for c in end]
    print(f"  list entries per bead {per_bead} -> {per_bead_end}, list radius {end[0].list_radius:.4f}, K {end[0].rebuild_interval}")
    assert 0.9 * min(per_bead) <= min(per_bead_end) and max(per_bead_end) <= 1.1 * max(per_bead)
    assert abs(end[0].list_radius - before[0].list_radius) <= 0.02 * before[0].list_radius
    assert end[0].rollbacks == after[0].rollbacks


def test_a_long_interval_is_cut_25_times_and_the_run_given_up(hip, oracle):
    """The give-up exit from the interval alone: 200 beads of the A/B box, a 400-step run at a rebuild interval from which 24 cuts of
    on_violation end above 1, with a kick of 3 margins in its first step -- seen at the second step by every interval above 1.
    (From 400 the cuts reach K = 1 after 21 rollbacks and the run succeeds: 400, 300, 225, ... 3, 2, 1.)  GD_ESTATE after exactly 25
    rollbacks; the handle stands where it stood before the run and runs on."""
    _, _, dt, kT, flags = CASES["ab_box"]
    over = dict(n_chains=10)
    box = np.array([CASES["ab_box"][1]["box"]] * 3)
    sh, *_ = build(hip, "ab_box", **over)
    so, *_ = build(oracle, "ab_box", **over)
    N = sh.N
    assert N == 200
    rng = np.random.default_rng(SEED + 3)
    z1, z2, z3 = (rng.normal(size=(n, 1, N, 3)) for n in (10, 400, 5))
    for s in (sh, so):
        s.begin_phase()
        s.run(10, dt, kT, noise=g.NOISE_HOST, host_noise=z1, flags=flags)
    sh.forces()
    margin = _current_margin(sh, scaled=False)
    assert abs(margin - 0.5 * SKIN0 * CUT) < 1e-6, margin
    K0 = _interval_that_gives_up(0)
    assert len(_intervals(400)) - 1 < GIVE_UP_AT <= len(_intervals(K0)) - 1
    sh.set_tuning(rebuild_interval=K0, adapt_interval=0)
    _kick(z2, 0, 0, N // 2, 3.0 * margin, dt, kT)
    before, xb = sh.context(), sh.positions()
    _refused_run(sh, 400, dt, kT, z2, flags)
    after = sh.context()
    print(f"  K0 {K0}, margin {margin:.4f}, rollbacks {after.rollbacks - before.rollbacks}, K after {after.rebuild_interval}")
    assert after.rollbacks - before.rollbacks == GIVE_UP_AT
    assert after.step == before.step == 10 and _ctx_tuple(after) == _ctx_tuple(before)
    assert np.array_equal(sh.positions(), xb)
    assert after.rebuild_interval == K0
    _assert_state_matches(sh, so, 10, wall=False)
    _assert_observations_match(sh, oracle, "ab_box", over, wall=False, box=box)
    for s in (sh, so):
        s.run(5, dt, kT, noise=g.NOISE_HOST, host_noise=z3, flags=flags)
    _assert_state_matches(sh, so, 15, wall=False)


# ------------------------------------------------------------------------------------------------ 4. refused calls change nothing

def refused_calls(s, dt, kT):
    """Every call gd_run and its neighbours refuse before they touch the device, on a handle without wall or scaling; returns how
    many were refused.  (test_parity_gpu.test_errors_match_oracle calls into this as well.)"""
    bond = g.System.bond_params(g.POT_HARMONIC, 1.0)
    calls = [
        (6, lambda: s.run(1, dt, kT, spacestep=0.1)),
        (1, lambda: s.run(-1, dt, kT)),
        (1, lambda: s.run(1, 0.0, kT)),
        (1, lambda: s.run(1, -dt, kT)),
        (1, lambda: s.run(1, dt, -1.0)),
        (1, lambda: s.run(1, dt, kT, noise=7)),
        (1, lambda: s.run(1, dt, kT, noise=-1)),
        (1, lambda: s.run(1, dt, kT, noise=g.NOISE_HOST)),
        (ESTATE, lambda: s.run(1, dt, kT, flags=g.RUN_WALL_DYNAMICS)),
        (ESTATE, lambda: s.run(1, dt, kT, flags=g.RUN_UPDATE_SCALES)),
        (1, lambda: s.add_bond_range(bond, 0, s.N + 1)),
        (1, lambda: s.add_bond_range(bond, 5, 4)),
        (1, lambda: s.set_positions(np.full((s.R, s.N, 3), np.inf))),
        (1, lambda: s.search_pairs(0.0)),
        (1, lambda: s.search_pairs(-0.3)),
        (1, lambda: s.contacts_update(0.0)),
    ]
    for code, call in calls:
        with pytest.raises(g.GdynError) as e:
            call()
        assert e.value.code == code, str(e.value)
    return len(calls)


@pytest.mark.parametrize("path", ["generic", "tiled"])
def test_refused_calls_change_nothing_bit_for_bit(hip, path):
    """Two handles, one seed: handle A is refused every call of refused_calls() between its runs, handle B sees none of them.
    Positions, contexts (list counters included) and contact maps stay equal byte for byte."""
    _, _, dt, kT, flags = CASES["ab_box"]
    R = 2
    A, B = (build(hip, "ab_box", n_replicas=R)[0] for _ in range(2))
    for s in (A, B):
        s.set_tuning(kernel_path=PATHS[path])
        s.begin_phase()

    def same():
        assert A.positions().tobytes() == B.positions().tobytes()
        for r in range(R):
            assert bytes(A.context(r)) == bytes(B.context(r)), r
            rows = A.contacts(r)
            assert rows.tobytes() == B.contacts(r).tobytes() and len(rows) > 50

    assert refused_calls(A, dt, kT) >= 12
    for _ in range(3):
        for s in (A, B):
            s.run(15, dt, kT, seed=SEED, flags=flags)
            s.contacts_update(0.4)
        _assert_path(A, path)
        same()
        refused_calls(A, dt, kT)
        same()
