"""Prepared contexts of the grouped step launches (include/gdyn_prep.h; csrc/gdyn_policy.hpp: ctx_prepared; csrc/gdyn_kernels.hip:
k_ctx_prep and the prepared k_step variants; csrc/gdyn_capi.hip: enqueue_chunk).

In a span that runs in two replica groups every step of a group is k_ctx_prep -> k_step: one wave per replica applies the pending
callback (reaction sum, step, time, scales, wall ODE) and derives the step's float constants, the stepping blocks copy them.  The same
functions on the same values, so nothing may depend on it: mode 2 (every grouped span runs prepared) against mode 1 (one launch, the
kernel that does the work in every block) from the same start, bit for bit with tests/bit_identity.py -- positions, every replica's
context, rollbacks and launch counts.  System.ctx_prepared() is non-zero on the mode-2 handle and zero on the mode-1 handle.

    strided reaction sum      33 280 x 16: 65 blocks a replica, the smallest shape at which the lane-strided sum of the reaction partials
                              takes its second trip (b = lane + 64)
    device-side scale path    replicas at different step counts: the host passes no scales, apply_callback evaluates them on the device
    run flags                 none, wall dynamics only, scale updates only, both: the callback advances step and time in all four
    deferred callback         a run ending with RUN_DEFER_CALLBACK, observed, applied, continued
    single steps              twelve run(1) against one run(12): k_ctx at every chunk end against k_ctx_prep between steps
    the rule live             handles the rule keeps on one launch: no preparation launch, results those of mode 1
"""
import numpy as np
import pytest

import stressed_states as ss
from bit_identity import assert_identical, ctx
from util import CASES, g

pytestmark = pytest.mark.gpu
SEED = 20220101
N, R = 1500, 16
_, _, DT, KT, FLAGS = CASES["genome"]
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
    assert s.ctx_prepared() == 0
    return s


def _run(s, steps, flags=FLAGS):
    return s.run(steps, DT, KT, flags=flags, replica_seeds=_seeds(s.R))


def _pair(hip, **kw):
    return _handle(hip, 1, **kw), _handle(hip, 2, **kw)


def _step_both(one, two, steps, flags=FLAGS, prepared=True):
    """The same run on the mode-1 and the mode-2 handle: bit-identical, and the preparation launches counted -- two per step."""
    t1, t2 = _run(one, steps, flags), _run(two, steps, flags)
    assert one.ctx_prepared() == 0 and one.step_groups() == (1, 1)
    if prepared:
        assert two.step_groups() == (2, 2) and two.ctx_prepared() >= 2 * steps      # (more: the steps of a rolled-back chunk)
        if two.context().rollbacks == 0:
            assert two.ctx_prepared() == 2 * steps
    else:
        assert two.ctx_prepared() == 0
    assert t2.step_launches == steps
    assert_identical(one, two, t1, t2)


def test_strided_reaction_sum(hip):
    """65 blocks a replica: lanes 0 of the preparation wave sum two partials each, in the order of the stepping blocks' wave 0."""
    n = 33280
    assert -(-n // 512) == 65
    one, two = _pair(hip, n=n)
    c0 = two.context()
    _step_both(one, two, 24)
    c = two.context()
    assert c.step == 24 and c.list_path == 2
    assert all(a != 0.0 for a in c.axial_reaction)                      # the wall acts: the sum is of non-zero partials
    assert tuple(c.semiaxes) != tuple(c0.semiaxes)


def _staggered(s):
    for r in range(s.R):
        c = s.context(r)
        s.set_context(r, 5 * r, c.bead_scale, c.bond_scale, semiaxes=list(c.semiaxes))


def test_device_side_scale_path(hip):
    """Replicas at different steps: no common step for the host to evaluate the scales at, apply_callback's own exponentials run."""
    one, two = _pair(hip, prepare=_staggered)
    before = ctx(two)
    _step_both(one, two, 16)
    after = ctx(two)
    assert [c[0] for c in after] == [5 * r + 16 for r in range(R)]
    assert all(a[2] != b[2] and a[3] != b[3] for a, b in zip(after, before))      # both scales moved, in every replica
    assert len({c[2] for c in after}) == R                                        # ... each to its own time's value


@pytest.mark.parametrize("flags", [0, g.RUN_WALL_DYNAMICS, g.RUN_UPDATE_SCALES, FLAGS], ids=["none", "wall_dynamics", "scale_updates", "both"])
def test_run_flags(hip, flags):
    one, two = _pair(hip)
    c0 = two.context()
    _step_both(one, two, 16, flags)
    c = two.context()
    assert c.step == 16 and c.time == 16 * DT
    assert (tuple(c.semiaxes) != tuple(c0.semiaxes)) == bool(flags & g.RUN_WALL_DYNAMICS)
    assert (c.bead_scale != c0.bead_scale) == bool(flags & g.RUN_UPDATE_SCALES)


def test_deferred_callback(hip):
    one, two = _pair(hip)
    _step_both(one, two, 12, FLAGS | g.RUN_DEFER_CALLBACK)
    assert two.context().callback_pending == 1
    assert np.array_equal(one.energy(), two.energy())
    assert np.array_equal(one.forces(), two.forces())
    assert_identical(one, two)
    one.apply_callback(), two.apply_callback()
    assert two.context().callback_pending == 0 and two.context().step == 12
    assert_identical(one, two)
    _step_both(one, two, 12)
    assert two.context().step == 24


def test_single_steps_against_one_run(hip):
    """Twelve run(1) -- every callback applied by k_ctx at the chunk's end -- against one run(12) -- eleven of them by k_ctx_prep
    between the steps --, both on mode-2 handles; and each against its mode-1 handle.

    One list for the twelve steps (rebuild interval 12): a build inside a chunk and a build at the start of a run's first chunk do
    not leave the same slot order -- with wall dynamics on, run(12) and twelve run(1) differ from the step behind the second build
    on by an ulp of the reaction sum, on mode-1 handles exactly as on mode-2 handles (measured at interval 8: equal through step 8,
    max |dx| 1.2e-7 from step 9; with flags 0 equal throughout).  That is the builds' business, not the callback's: here no build
    separates the two ways of applying it."""
    tune = dict(TUNE, rebuild_interval=12)
    one, whole, single, single_one = (_handle(hip, m, tune=tune) for m in (1, 2, 2, 1))
    _step_both(one, whole, 12)
    for k in range(12):
        _step_both(single_one, single, 1)
        assert single.ctx_prepared() == 2 and single.context().step == k + 1
    assert whole.context().rollbacks == 0 and single.context().rollbacks == 0 and whole.context().rebuilds == single.context().rebuilds == 1
    assert np.array_equal(single.positions(), whole.positions())
    assert ctx(single) == ctx(whole)


FALLBACKS = {"R6": dict(nrep=6), "generic_lists": dict(tune=dict(TUNE, kernel_path=1))}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_the_rule_keeps_single_launch_handles_unprepared(hip, case):
    one, two = _pair(hip, **FALLBACKS[case])
    t1, t2 = _run(one, 16), _run(two, 16)
    assert two.step_groups() == (2, 1) and two.ctx_prepared() == 0 and one.ctx_prepared() == 0
    assert_identical(one, two, t1, t2)
    assert two.context().step == 16


def test_the_rule_keeps_a_small_handle_unprepared(hip):
    """Mode 0 (the default) at 1 500 x 16: one launch per step, no preparation launch."""
    one, rule = _handle(hip, 1), _handle(hip, 0)
    t1, t0 = _run(one, 16), _run(rule, 16)
    assert rule.step_groups() == (0, 1) and rule.ctx_prepared() == 0
    assert_identical(one, rule, t1, t0)
