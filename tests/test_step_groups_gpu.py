"""Replica groups of the step launches (include/gdyn_groups.h; csrc/gdyn_policy.hpp: step_group_split; csrc/gdyn_capi.hip: enqueue_chunk).

Between two list builds gd_run may launch every step as two kernels, replicas [0, A) on the handle's stream and [A, R) on a second one.
Every word k_step reads or writes is addressed by the global replica or by a bead of it, so the results may not depend on it: mode 2 (two
groups wherever the results allow it) against mode 1 (one launch) from the same start, compared bit for bit -- positions, every
replica's context, rollbacks and launch counts --

    on the pressed genome at 1 500 beads (3 blocks of 512, the last one partly filled) x 16 replicas (groups of 8 + 8), rebuild interval 8,
    wall dynamics and scale updates on, per-replica seeds; once more with a chunk boundary inside an interval;
    in the tile class whose step is two launches per group (62 178 beads, 3 312 < largest tile);
    through a chunk that violates the skin and is rolled back, and the run after it;
    on every state the rule sends to the single path (droplet term, per-replica pairs, generic lists, R = 6, and mode 0 at this size):
    one group reported, results those of mode 1;
    and for energy(), forces() and positions() right after a grouped run.

Two ONE-launch handles built and run alike agree bit for bit among themselves, which is what makes the comparison of the modes
meaningful: tests/test_state_alone_gpu.py holds equal handles to that through builds whose repairs are refused and through rolled-back
chunks, the states at which they once did not (33 280 x 16 beads, 62 178 x 16 at skin 1.1: the thread order of a retry's first build
followed what the rejected builds had left; DESIGN.md section 7l, "Equal handles").
"""
import importlib

import numpy as np
import pytest

import stressed_states as ss
from bit_identity import assert_identical as _assert_identical
from util import CASES, g

pytestmark = pytest.mark.gpu
replica = importlib.import_module(g.__name__ + ".replica")
SEED = 20220101
N, R = 1500, 16          # CASES["genome"]: the smallest genome the parity tests use; 3 blocks of 512, 36 slots of the last one empty
_, _, DT, KT, FLAGS = CASES["genome"]
assert N == CASES["genome"][1]["n_beads"] and N % 512 != 0 and -(-N // 512) >= 3
assert FLAGS == g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
TUNE = dict(rebuild_interval=8, adapt_interval=0)


def _seeds(nrep):
    return np.arange(nrep, dtype=np.uint64) * np.uint64(7919) + np.uint64(SEED)


def _handle(hip, mode, n=N, nrep=R, tune=TUNE, prepare=None):
    s = ss.pressed_genome(hip, n, nrep)
    s.set_tuning(**tune)
    if prepare:
        prepare(s)
    s.set_step_groups(mode)
    assert s.step_groups() == (mode, 1)
    return s


def _run(s, steps):
    return s.run(steps, DT, KT, flags=FLAGS, replica_seeds=_seeds(s.R))


def _both(hip, runs, expect_groups, **kw):
    """The same runs on a mode-1 and a mode-2 handle; returns them after asserting bit identity after every run."""
    one, two = _handle(hip, 1, **kw), _handle(hip, 2, **kw)
    for steps in runs:
        t1, t2 = _run(one, steps), _run(two, steps)
        assert one.step_groups() == (1, 1) and two.step_groups() == (2, expect_groups)
        assert t2.step_launches == steps                     # steps, not launches
        _assert_identical(one, two, t1, t2)
    return one, two


# ------------------------------------------------------------------------------------------------ bit identity

@pytest.mark.parametrize("runs", [(40,), (20, 20)], ids=["one_run", "chunk_boundary_inside_an_interval"])
def test_two_groups_are_bit_identical_to_one_launch(hip, runs):
    one, two = _both(hip, runs, 2)
    c = two.context()
    assert c.step == 40 and c.list_path == 2 and c.rollbacks == 0 and c.rebuild_interval == 8
    x = two.positions()
    assert np.isfinite(x).all() and not np.array_equal(x[0], x[8])      # (replicas of both groups moved, each on its own seed)
    fresh = ss.pressed_genome(hip, N, R).positions()
    assert np.all(np.abs(x - fresh).max(axis=(1, 2)) > 0)               # every replica was stepped


SPLIT_SKINS = (0.0, 1.1, 1.05, 1.15, 1.0, 1.2, 0.95, 1.25, 0.9, 1.3, 0.85, 1.35, 0.8)      # (0: the library's own width)


def test_two_groups_in_the_split_tile_class(hip):
    """A largest tile beyond 3 312 entries with byte-offset lists: every group's step is the two launches of launch_step_mode (the
    skin search of test_wall_context_gpu.py::test_reaction_of_a_step_split_by_tile_class)."""
    def tuned(skin, mode):
        s = _handle(hip, mode, n=62178, tune=dict(skin=skin, adapt_interval=0, rebuild_interval=4))
        s.energy()                                           # builds the list: the tile class of this width
        return s

    one, seen = None, {}
    for skin in SPLIT_SKINS:
        s = tuned(skin, 1)
        seen[skin] = (s.context().tile_capacity, s.context().largest_tile)
        if 3312 < seen[skin][0] < 4096 and seen[skin][1] > 3312:
            one, two = s, tuned(skin, 2)
            break
        s.close()
    assert one is not None, ("no list width in the split class", seen)
    t1, t2 = _run(one, 6), _run(two, 6)
    assert two.step_groups() == (2, 2) and one.step_groups() == (1, 1)
    _assert_identical(one, two, t1, t2)
    c = two.context()
    assert 3312 < c.tile_capacity < 4096 and c.largest_tile > 3312 and c.list_path == 2 and c.step == 6


# ------------------------------------------------------------------------------------------------ rollback

def test_a_rolled_back_chunk_in_two_groups(hip):
    """test_parity_gpu.py::test_rollback_with_replicas' interval of 40 steps on the stressed state: the skin is violated inside the
    chunk, which is rolled back and run again on a shorter interval -- both groups with it.  A following run works."""
    tune = dict(rebuild_interval=40, adapt_interval=0, list_width=128)       # (wide list: only skin violations can roll back)
    one, two = _both(hip, (40,), 2, tune=tune)
    assert two.context().rollbacks >= 1 and two.context().step == 40
    t1, t2 = _run(one, 12), _run(two, 12)
    assert two.step_groups() == (2, 2)
    _assert_identical(one, two, t1, t2)
    assert two.context().step == 52


# ------------------------------------------------------------------------------------------------ fallbacks

def _droplet(s):
    s.set_pair_softwell(0.8, 0.2, 0.4, np.arange(0, s.N, 7, dtype=np.uint32))


def _replica_pairs(s):
    replica.define(s, 0, ss.LOOP)
    for r in range(s.R):
        i = np.arange(r, s.N - 9, 11, dtype=np.uint32)
        replica.set_pairs(s, 0, r, np.stack([i, i + 5 + r % 3], axis=1))


FALLBACKS = {
    "droplet": dict(prepare=_droplet),
    "replica_pairs": dict(prepare=_replica_pairs),
    "generic_lists": dict(tune=dict(TUNE, kernel_path=1)),
    "R6": dict(nrep=6),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_states_that_stay_on_one_launch(hip, case):
    one, two = _both(hip, (20,), 1, **FALLBACKS[case])
    assert two.context().step == 20
    if case == "generic_lists":
        assert two.context().list_path == 1


def test_the_rule_keeps_a_small_handle_on_one_launch(hip):
    """Mode 0 (the default): 2 x 8 replicas x 3 blocks are far below the size at which two groups pay."""
    one, rule = _handle(hip, 1), ss.pressed_genome(hip, N, R)
    rule.set_tuning(**TUNE)
    assert rule.step_groups() == (0, 1)                       # the default mode
    t1, t0 = _run(one, 20), _run(rule, 20)
    assert rule.step_groups() == (0, 1)
    _assert_identical(one, rule, t1, t0)
    with pytest.raises(g.GdynError) as e:
        rule.set_step_groups(3)
    assert e.value.code == 1 and rule.step_groups() == (0, 1)


# ------------------------------------------------------------------------------------------------ observation after a grouped run

def test_observations_after_a_grouped_run(hip):
    one, two = _both(hip, (20,), 2)
    assert np.array_equal(one.energy(), two.energy())
    assert np.array_equal(one.forces(), two.forces())
    assert np.array_equal(one.positions(), two.positions())
    assert np.array_equal(one.positions_f32(), two.positions_f32())
    _assert_identical(one, two)
