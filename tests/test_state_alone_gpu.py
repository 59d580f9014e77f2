"""What a handle computes is a function of its state alone: positions, context, model, tuning and seeds -- not of what the handle ran
before, and not of the order in which the atomics of a list build happened to arrive (csrc/gdyn_list.hpp: order_valid; DESIGN.md
section 7l, "Equal handles").

k_fill orders k_step's threads by len_prev, the near-chunk count each bead's list had at the build before, and a block's fp32
wall-reaction partial is summed in thread order: the order decides the last digits of the semiaxes.  A build whose repairs are refused
(more than GD_REPAIR_GRID = 1 024 waves queued, or a full row pool) stores counts clamped to the rows of whichever waves were turned
away, its chunk is rolled back, and the retry's first build was ordered by that; gd_set_positions kept the key of the state before.
The key is now cleared wherever it does not describe an accepted build of the trajectory being listed.

Pressed genome, tiled lists (kernel_path=2), wall dynamics and scale updates on, per-replica seeds, skin, interval and width fixed so
that no policy choice can differ.  Compared with np.array_equal / ==, no tolerance: positions(), every replica's context (step, time,
scales, semiaxes, axial_reaction, rollbacks, rebuilds, rebuild_interval, list_path, callback_pending), energy(), forces().

    a  a handle that ran 24 steps and was put back to the start (set_positions, set_context) against a fresh one, 1 500 x 16;
    b  four equal handles of 3 000 x 24 (1 152 k_step waves) at list_width NARROW, whose first build cannot have its repairs served:
       every handle rolls back, all four agree after 24 steps and after 16 more;
    c  the same with rebuild_interval 40, where a skin violation rolls a later attempt back as well, and 12 steps behind it;
    d  energy() and forces() of four fresh handles at that width: the first build outside gd_run is refused and run again.

Against the library before the fix (one MI355X): (a) failed in the one run made -- all sixteen replicas' semiaxes off in the last three
or four digits, one force word with them, positions and axial_reaction bit-equal; (b), (c) and (d) failed in five fresh processes out
of five each, at the second handle every time: semiaxes, energies and a few dozen force words of most replicas, in (b) two
position words too, in (d) the axial_reaction forces() folds in.  rollbacks and rebuilds agreed in every handle on either library
(1 and 6 + 3 in (b), 5 and 12 + 2 in (c), 2 builds in (d)): the row history of a rolled-back chunk stays in use.
"""
import numpy as np
import pytest

import stressed_states as ss
from bit_identity import assert_observed_identical, ctx, observed
from util import CASES, g

pytestmark = pytest.mark.gpu
SEED = 20220101
_, _, DT, KT, FLAGS = CASES["genome"]
assert FLAGS == g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
SKIN = 0.75                     # the library's own width, given: nothing may move it
N_BIG, R_BIG = 3000, 24         # 8 waves x 6 blocks x 24 replicas = 1 152 k_step waves > GD_REPAIR_GRID = 1 024
assert 8 * -(-N_BIG // 512) * R_BIG > 1024 and R_BIG % 8 == 0
NARROW = 8                      # list_width: one chunk per lane where nothing predicts the rows -- every wave's lists outgrow it


def _seeds(nrep):
    return np.arange(nrep, dtype=np.uint64) * np.uint64(7919) + np.uint64(SEED)


def _handle(hip, n, nrep, **tune):
    s = ss.pressed_genome(hip, n, nrep)
    s.set_tuning(skin=SKIN, adapt_interval=0, kernel_path=2, **tune)
    return s


def _run(s, steps):
    return s.run(steps, DT, KT, flags=FLAGS, replica_seeds=_seeds(s.R))


def _report(tag, s):
    c = s.context()
    print(f"{tag}: step {c.step} rollbacks {c.rollbacks} rebuilds {c.rebuilds} row_repairs {c.row_repairs} list_path {c.list_path} "
          f"interval {c.rebuild_interval} semiaxes[0] {tuple(c.semiaxes)}")


# ------------------------------------------------------------------------------------------------ a: a reused handle

def test_a_reused_handle_equals_a_fresh_one(hip):
    """Deterministic witness: B runs 24 steps, is put back to A's start and then runs A's 40 steps.  (rebuilds counts a handle's
    builds since it was created: B's are counted from the moment it was put back.)"""
    n, nrep, tune = 1500, 16, dict(rebuild_interval=8, list_width=128)
    a = _handle(hip, n, nrep, **tune)
    x0 = a.positions()
    c0 = [a.context(r) for r in range(nrep)]
    start = [(c.bead_scale, c.bond_scale, tuple(c.semiaxes)) for c in c0]
    _run(a, 40)
    _report("a fresh", a)
    oa = observed(a)

    b = _handle(hip, n, nrep, **tune)
    assert np.array_equal(b.positions(), x0)
    _run(b, 24)
    assert not np.array_equal(b.positions(), x0)                            # B's history moved the beads ...
    assert np.all(np.abs(b.positions() - x0).max(axis=(1, 2)) > 0)          # ... of every replica
    assert b.context().rollbacks == 0
    b.set_positions(x0)
    for r, (bs, os_, semi) in enumerate(start):
        b.set_context(r, 0, bs, os_, semiaxes=semi)
    before = b.context().rebuilds
    assert before >= 3
    _run(b, 40)
    _report("a reused", b)
    ob = observed(b, rebuilds_before=before)

    for o in (oa, ob):                                                      # the test's power: no rollback, and the wall acts
        for r, c in enumerate(o["context"]):
            assert c[0] == 40 and c[6] == 0 and c[9] == 2, c                # step, rollbacks, list_path
            assert all(v != 0.0 for v in c[5]), (r, c[5])                   # axial_reaction
            assert all(v != w for v, w in zip(c[4], start[r][2])), (r, c[4])      # semiaxes moved
    assert_observed_identical(oa, ob)


# ------------------------------------------------------------------------------------------------ b, c: refused repairs

def _four_alike(hip, tune, runs, rolled_back_by=None):
    """Four handles built and run alike, one after the other; all four bit-identical after every run.  Returns the first one's records."""
    first = None
    for k in range(4):
        s = _handle(hip, N_BIG, R_BIG, **tune)
        recs = []
        for steps in runs:
            _run(s, steps)
            _report(f"handle {k} after {steps} steps", s)
            recs.append(observed(s))
        s.close()
        assert recs[0]["context"][0][6] >= 1, "no rollback: the first build's repairs were all served"
        if first is None:
            first = recs
        else:
            for want, got in zip(first, recs):
                assert_observed_identical(want, got)
    return first


def test_b_equal_handles_through_a_build_whose_repairs_are_refused(hip):
    """list_width 8: rows of one chunk per lane where nothing predicts them, so all 1 152 waves of the first build queue for repair --
    128 more than the repair launch serves -- and its chunk is rolled back once for the overflow (measured: rollbacks 1 in every
    handle, before and after the fix; the run is not refused at this width, so no wider one was looked for).  The retry's rows are
    predicted from the rejected builds' counts and need no repair."""
    recs = _four_alike(hip, dict(rebuild_interval=8, list_width=NARROW), (24, 16))
    assert [c[0] for c in recs[0]["context"]] == [24] * R_BIG and [c[0] for c in recs[1]["context"]] == [40] * R_BIG
    assert all(all(v != 0.0 for v in c[5]) for c in recs[1]["context"])     # the wall acts in every replica


def test_c_equal_handles_through_a_rollback_inside_a_later_attempt(hip):
    """test_step_groups_gpu.py::test_a_rolled_back_chunk_in_two_groups' first run (interval 40 on the stressed state: the skin is
    violated inside the chunk) at the narrow width: the overflow's retry is rolled back again for the violation, so the retries'
    builds follow rejected builds twice over."""
    recs = _four_alike(hip, dict(rebuild_interval=40, list_width=NARROW), (40, 12))
    assert recs[0]["context"][0][6] >= 2                                    # the overflow and the skin violation
    assert [c[0] for c in recs[1]["context"]] == [52] * R_BIG


# ------------------------------------------------------------------------------------------------ d: a refused build outside gd_run

def test_d_observations_through_a_refused_build(hip):
    """energy() and forces() of a fresh handle at the narrow width: the build they need is refused like (b)'s and run again on the same
    positions -- ordered by slot, not by what the refused one left."""
    first = None
    for k in range(4):
        s = _handle(hip, N_BIG, R_BIG, rebuild_interval=8, list_width=NARROW)
        rec = dict(energy=s.energy(), forces=s.forces(), positions=s.positions(), context=ctx(s), context_observed=ctx(s))
        _report(f"handle {k} observed", s)
        assert s.context().rebuilds >= 2, "the first build was not refused"
        s.close()
        assert all(all(v != 0.0 for v in c[5]) for c in rec["context"])     # forces() folded a wall reaction into every replica
        if first is None:
            first = rec
        else:
            assert_observed_identical(first, rec)
