"""The wall's axial reaction and semiaxis ODE on the device, at states where the wall acts (tests/stressed_states.py: pressed_genome,
composite; tests/test_stressed_states.py asserts on the CPU that hundreds of beads press on the wall there).

The reaction is the one part of the stepper's state that feeds back into every later step: k_step's blocks write per-block fp32
partials, wave 0 of every block of the NEXT step (apply_callback) or k_ctx re-reduces them, and the semiaxes move by
dt * mobility * (reaction - spring * semiaxes).  Where the other device tests read that state the reaction is zero
(test_production_size_initial_states_leave_the_wall_idle).  Here it is 0.1 ... 0.8 of spring * semiaxes, at

    1 500 beads (3 blocks of 512), 33 280 (65 blocks: one beyond the 64 lanes that fold the partials),
    33 280 x 12 (780 blocks: more than are resident at once), 62 178 x 2 in the tile class whose step is two launches,

on both kernel paths where a pair list exists, the path asserted.

Bound of one evaluation, per replica r and axis k, from the oracle alone:

    |react_k(dev) - react_k(oracle)|  <=  B_k = FORCE_RTOL * S_k + N_k

S_k = sum_i |F_wall,ik q_ik| / a_k (tests/wall_restatement.py) is the reaction's own scale -- its contributions share one sign, so
S_k = react_k -- and FORCE_RTOL the per-term force tolerance of DESIGN.md section 2.  N_k is the largest change of the ORACLE's react_k
over three copies of the state whose fp32 coordinates are moved by one ulp up or down (stressed_states.nudged): the device forms a
bead's distance to the surface from fp32 coordinates of size 6, the wall's harmonic outer branch turns that rounding into force with
a spring of 5 000, and no arithmetic downstream can undo it (the role _energy_floor has for the wall energy).

Over a run the compared quantity is the INTEGRATED reaction, read back from the semiaxes:

    sum_n react_k(n) = (semi_end - semi_0) / (dt mobility) + spring * sum_n semi_k(n)        (semi(n): the semiaxes step n started from)

with the bound  sum_n FORCE_RTOL * S_k(n) + 4 * (spread of the same quantity over the three nudged oracle runs); the factor 4 covers
the fp32 rounding of the positions at each of the five or six steps against the one initial nudge of the oracle's.

Every comparison prints  WALLCTX <what> err/(FORCE_RTOL*S) <worst> noise/S <worst>; the worst figures are in DESIGN.md section 2.
"""
import numpy as np
import pytest

import stressed_states as ss
import wall_restatement as wr
from util import FORCE_RTOL, POS_ATOL_20STEP, g

pytestmark = pytest.mark.gpu
PATHS = {"generic": 1, "tiled": 2}
FLAGS = g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
DT, SEED = 1.0e-5, 20220101
GAIN = DT * ss.WALL_MOBILITY                  # what a unit of reaction moves a semiaxis by in one step
NUDGE_SEEDS = (101, 102, 103)

STATES = {
    "pressed_1500": lambda lib: ss.pressed_genome(lib, 1500, 2),
    "pressed_33280": lambda lib: ss.pressed_genome(lib, 33280, 2),
    "composite": ss.composite,
    "pressed_1500_R3": lambda lib: ss.pressed_genome(lib, 1500, 3),           # one block map of k_step's grid ...
    "pressed_1500_R8": lambda lib: ss.pressed_genome(lib, 1500, 8),           # ... and the other
}
STEP_STATES = ("pressed_1500", "pressed_33280", "composite")


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


def _reactions(s):
    return np.array([tuple(s.context(r).axial_reaction) for r in range(s.R)])


def _semiaxes(s):
    return np.array([tuple(s.context(r).semiaxes) for r in range(s.R)])


def _ulp4(a):
    return 4 * np.spacing(np.abs(a))


# ------------------------------------------------------------------------------------------------ the oracle's side, once per state

_REF = {}


def _reference(oracle, state):
    """x0, semi0, the oracle's reaction at x0, its scale S, the nudge noise N and the bound B (each (R, 3)), and the semiaxes after
    one zero-noise step with wall dynamics."""
    if state not in _REF:
        so = STATES[state](oracle)
        x0, semi0 = so.positions(), _semiaxes(so)
        restated, S, react = wr.oracle_reaction(so)
        assert np.all(np.abs(restated - react) <= 1e-12 * S) and np.all(S > 0)
        N = np.zeros_like(S)
        for seed in NUDGE_SEEDS:
            so.set_positions(ss.nudged(x0, seed))
            so.forces(g.TERM_WALL)
            N = np.maximum(N, np.abs(_reactions(so) - react))
        so.set_positions(x0)
        so.run(1, DT, 0.0, noise=g.NOISE_ZERO, flags=FLAGS)
        assert np.array_equal(_reactions(so), react)                  # the step's force evaluation is the one at x0
        _REF[state] = dict(x0=x0, semi0=semi0, react=react, S=S, N=N, B=FORCE_RTOL * S + N, semi1=_semiaxes(so))
    return _REF[state]


def _check_reaction(what, dev, ref, S, noise, noise_factor=1.0):
    """|dev - ref| <= FORCE_RTOL * S + noise_factor * noise, per replica and axis, the measured ratios printed first."""
    err = np.abs(dev - ref)
    print(f"WALLCTX {what}: err/(FORCE_RTOL*S) {np.max(err / (FORCE_RTOL * S)):.3f}  noise/S {np.max(noise / S):.2e}  "
          f"err/bound {np.max(err / (FORCE_RTOL * S + noise_factor * noise)):.3f}")
    assert np.all(err <= FORCE_RTOL * S + noise_factor * noise), (what, err / (FORCE_RTOL * S + noise_factor * noise))


def _device(hip, state, path):
    sh = STATES[state](hip)
    sh.set_tuning(kernel_path=PATHS[path])
    return sh


# ------------------------------------------------------------------------------------------------ (i) force mode

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("state", list(STATES))
def test_reaction_of_a_force_evaluation(hip, oracle, state, path):
    ref = _reference(oracle, state)
    sh = _device(hip, state, path)
    sh.forces(g.TERM_ALL)
    first = _reactions(sh)
    _check_reaction(f"force {state} {path}", first, ref["react"], ref["S"], ref["N"])
    sh.forces(g.TERM_ALL)
    assert _reactions(sh).tobytes() == first.tobytes()                # the fold has one order: a second evaluation, the same bytes
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ (ii) masked evaluation

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("state", ["pressed_1500", "pressed_33280", "composite"])
def test_masked_evaluation_keeps_or_sets_the_reaction_as_the_oracle_does(hip, oracle, state, path):
    """include/gdyn.h: axial_reaction is that of the last force evaluation that INCLUDED the wall.  The oracle keeps the value through
    an evaluation whose mask lacks the wall; so must the device (which zeroes its partials for every evaluation)."""
    ref = _reference(oracle, state)
    sh, so = _device(hip, state, path), STATES[state](oracle)
    for s in (sh, so):
        s.forces(g.TERM_PAIR)
        assert np.all(_reactions(s) == 0)                             # nothing has evaluated the wall yet
        s.forces(g.TERM_ALL)
    set_by_all, oracle_all = _reactions(sh), _reactions(so)
    assert np.array_equal(oracle_all, ref["react"])
    for mask in (g.TERM_PAIR, g.TERM_ALL & ~g.TERM_WALL):
        sh.forces(mask), so.forces(mask)
        assert np.array_equal(_reactions(so), oracle_all)
        assert _reactions(sh).tobytes() == set_by_all.tobytes(), mask
        _check_reaction(f"masked {mask} {state} {path}", _reactions(sh), _reactions(so), ref["S"], ref["N"])
    for mask in (g.TERM_WALL, g.TERM_WALL | g.TERM_BOND):             # with the wall in the mask: set anew
        sh.forces(mask), so.forces(mask)
        assert np.array_equal(_reactions(so), oracle_all)
        _check_reaction(f"masked {mask} {state} {path}", _reactions(sh), _reactions(so), ref["S"], ref["N"])
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ (iii), (iv) one step

def _check_one_step(what, sh, ref):
    """After one T = 0, zero-noise, compensated step with scale updates and wall dynamics: the reaction is the one at x0, and the
    semiaxes moved by the wall ODE with it."""
    react, semi1 = _reactions(sh), _semiaxes(sh)
    for r in range(sh.R):
        assert sh.context(r).step == 1 and sh.context(r).callback_pending == 0 and sh.context(r).compensated == 1
    _check_reaction(what, react, ref["react"], ref["S"], ref["N"])
    semi0 = ref["semi0"]
    assert np.all(semi1 != semi0)
    # the device's own arithmetic: its ODE step with its own reported reaction
    assert np.all(np.abs(semi1 - (semi0 + GAIN * (react - ss.WALL_SPRING * semi0))) <= _ulp4(semi0)), what
    # and against the oracle's step
    assert np.all(np.abs((semi1 - semi0) - (ref["semi1"] - semi0)) <= GAIN * ref["B"] + _ulp4(semi0)), what


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("state", STEP_STATES)
def test_one_step_moves_the_semiaxes_by_the_reaction_at_x0(hip, oracle, state, path):
    ref = _reference(oracle, state)
    sh = _device(hip, state, path)
    sh.run(1, DT, 0.0, noise=g.NOISE_ZERO, flags=FLAGS | g.RUN_COMPENSATED)
    _check_one_step(f"step {state} {path}", sh, ref)
    _assert_path(sh, path)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("state", STEP_STATES)
def test_deferred_step_reports_the_reaction_and_applies_it_later(hip, oracle, state, path):
    """GD_RUN_DEFER_CALLBACK: the semiaxes are still those the step started from, the reaction is already that of the step's force
    evaluation (as on the oracle, which sets it there), and gd_apply_callback moves the semiaxes with exactly that value -- folding
    the partials for the observer must leave them where the pending callback reads them."""
    ref = _reference(oracle, state)
    sh, so = _device(hip, state, path), STATES[state](oracle)
    for s in (sh, so):
        s.run(1, DT, 0.0, noise=g.NOISE_ZERO, flags=FLAGS | g.RUN_COMPENSATED | g.RUN_DEFER_CALLBACK)
        for r in range(s.R):
            assert s.context(r).callback_pending == 1 and s.context(r).step == 0
        assert np.array_equal(_semiaxes(s), ref["semi0"])
    assert np.array_equal(_reactions(so), ref["react"])
    deferred = _reactions(sh)
    _check_reaction(f"deferred {state} {path}", deferred, ref["react"], ref["S"], ref["N"])
    sh.energy()                                                        # what a driver does at its observation point
    assert _reactions(sh).tobytes() == deferred.tobytes() and np.array_equal(_semiaxes(sh), ref["semi0"])
    sh.apply_callback()
    assert _reactions(sh).tobytes() == deferred.tobytes()             # the callback folded the same partials
    _check_one_step(f"deferred+applied {state} {path}", sh, ref)
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ (v), (vi) runs

def _integrated(semis):
    """sum over the steps of the reaction, from the semiaxes recorded before the first and after every step ((steps + 1, R, 3))."""
    return (semis[-1] - semis[0]) / GAIN + ss.WALL_SPRING * np.sum(semis[:-1], axis=0)


def _stepwise(s, steps, scales=False):
    """`steps` noisy steps one gd_run each: the semiaxes before and after each; on the oracle also S_k of every step's evaluation."""
    semis, S = [_semiaxes(s)], []
    for _ in range(steps):
        if scales:
            S.append(wr.oracle_reaction(s)[1])         # (the wall's forces at the state the next step evaluates: the same reaction)
        s.run(1, DT, 1.0, seed=SEED, flags=FLAGS)
        semis.append(_semiaxes(s))
    return np.array(semis), np.array(S)


def _run_reference(oracle, key, make, steps):
    """The oracle's walk and three walks from nudged coordinates: integrated and final reaction, their scales and spreads."""
    if key not in _REF:
        so = make(oracle)
        x0 = so.positions()
        semis, S = _stepwise(so, steps, scales=True)
        I, final = _integrated(semis), _reactions(so)
        assert np.all(S > 0) and np.all(final > 0)
        spread_I, spread_final = np.zeros_like(I), np.zeros_like(I)
        for seed in NUDGE_SEEDS:
            sn = make(oracle)
            sn.set_positions(ss.nudged(x0, seed))
            In = _integrated(_stepwise(sn, steps)[0])
            spread_I, spread_final = np.maximum(spread_I, np.abs(In - I)), np.maximum(spread_final, np.abs(_reactions(sn) - final))
            sn.close()
        _REF[key] = dict(x=so.positions(), semis=semis, I=I, final=final, S_sum=S.sum(axis=0), S_last=S[-1],
                         spread_I=spread_I, spread_final=spread_final)
        so.close()
    return _REF[key]


def _check_run(what, hip_handles, ref, steps):
    """hip_handles: (stepwise, whole) -- one handle stepped by `steps` runs of one step (every callback applied by k_ctx at the end
    of its chunk), one by a single run (every callback but the last applied by the next step's blocks, from the double-buffered
    partials).  Both against the oracle's integrated and final reaction."""
    sa, sb = hip_handles
    semis, _ = _stepwise(sa, steps)
    sb.run(steps, DT, 1.0, seed=SEED, flags=FLAGS)
    for s in (sa, sb):
        for r in range(s.R):
            assert s.context(r).step == steps and s.context(r).rollbacks == 0
        assert s.context().list_path == 2
        assert np.abs(s.positions() - ref["x"]).max() <= POS_ATOL_20STEP
    _check_reaction(f"{what} stepwise final", _reactions(sa), ref["final"], ref["S_last"], ref["spread_final"], 4.0)
    _check_reaction(f"{what} stepwise integrated", _integrated(semis), ref["I"], ref["S_sum"], ref["spread_I"], 4.0)
    _check_reaction(f"{what} whole final", _reactions(sb), ref["final"], ref["S_last"], ref["spread_final"], 4.0)
    # the single run's semiaxes between its steps are not observable: those of the stepwise handle stand in for them in the spring
    # part of the integral.  The two differ by at most GAIN * (difference of the integrated reactions so far), so the substitution
    # adds at most steps * spring * GAIN = 6e-5 of the bound; it is added to the noise term
    whole = np.concatenate([semis[:-1], _semiaxes(sb)[None]])
    slack = steps * ss.WALL_SPRING * GAIN * (FORCE_RTOL * ref["S_sum"] + 4.0 * ref["spread_I"])
    _check_reaction(f"{what} whole integrated", _integrated(whole), ref["I"], ref["S_sum"], ref["spread_I"] + slack / 4.0, 4.0)


def test_reaction_over_a_grid_larger_than_the_chip(hip, oracle):
    """33 280 beads x 12 replicas = 780 blocks, more than are resident at once (256 CUs x 3), 65 partials per replica: six noisy steps
    with scale updates and wall dynamics on the tiled path, lists rebuilt every third step.  (The pressed version of
    test_parity_gpu.py::test_wall_context_on_a_grid_larger_than_the_chip, whose reaction is zero.)"""
    make = lambda lib: ss.pressed_genome(lib, 33280, 12)
    ref = _run_reference(oracle, "grid", make, 6)
    handles = []
    for _ in range(2):
        sh = make(hip)
        sh.set_tuning(kernel_path=2, rebuild_interval=3, adapt_interval=0)
        sh.energy()                                   # builds the list (as the split test below): its widths settle here, not in a rolled-back chunk
        handles.append(sh)
    _check_run("grid 33280x12", handles, ref, 6)


SPLIT_SKINS = (1.1, 1.05, 1.15, 1.0, 1.2, 0.95, 1.25, 0.9, 1.3, 0.85, 1.35, 0.8)


def test_reaction_of_a_step_split_by_tile_class(hip, oracle):
    """62 178 beads x 2 in the tile class whose step is two launches (3 312 < capacity < 4 096; the skin search of
    test_parity_gpu.py::test_step_split_by_tile_class_matches_oracle): block 0 writes the context in one of the two launches only,
    every block its partial in one only.  Five noisy steps: positions, integrated and final reaction."""
    make = lambda lib: ss.pressed_genome(lib, 62178, 2)

    def tuned(skin):
        sh = make(hip)
        sh.set_tuning(skin=skin, adapt_interval=0, rebuild_interval=4)
        sh.energy()                                   # builds the list: the tile class of this width
        return sh

    chosen, seen = None, {}
    for skin in SPLIT_SKINS:
        sh = tuned(skin)
        seen[skin] = sh.context().tile_capacity
        sh.close()
        if 3312 < seen[skin] < 4096:
            chosen = skin
            break
    assert chosen is not None, ("no list width in the split class", seen)
    ref = _run_reference(oracle, "split", make, 5)
    handles = [tuned(chosen), tuned(chosen)]
    _check_run("split 62178x2", handles, ref, 5)
    for sh in handles:
        assert 3312 < sh.context().tile_capacity < 4096
