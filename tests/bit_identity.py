"""Bit identity of two handles, for the tests that hold one way of running a state to another (test_step_groups_gpu.py: two replica
groups against one launch; test_state_alone_gpu.py: equal handles, a reused handle against a fresh one).  No tolerances anywhere:
np.array_equal and ==."""
import numpy as np


def ctx(s, rebuilds_before=0):
    """Every replica's context: step, time, both scales, semiaxes, axial_reaction, rollbacks, rebuilds, rebuild_interval, list_path,
    callback_pending.  rebuilds_before: builds of the handle that belong to an earlier life of it (rebuilds counts a handle's builds
    since it was created)."""
    out = []
    for r in range(s.R):
        c = s.context(r)
        out.append((c.step, c.time, c.bead_scale, c.bond_scale, tuple(c.semiaxes), tuple(c.axial_reaction), c.rollbacks,
                    c.rebuilds - rebuilds_before, c.rebuild_interval, c.list_path, c.callback_pending))
    return out


def assert_identical(a, b, ta=None, tb=None):
    """Handles a and b (and the timing of their last runs) hold the same state, bit for bit."""
    assert np.array_equal(a.positions(), b.positions())
    assert ctx(a) == ctx(b)
    if ta is not None:
        assert (ta.step_launches, ta.rebuild_launches) == (tb.step_launches, tb.rebuild_launches)


def observed(s, rebuilds_before=0):
    """What a caller can read of a handle, in one fixed order: positions and contexts as the last run left them, then energy() and
    forces() -- which may build a list and fold the wall reaction of their evaluation into the context -- and the contexts behind them."""
    x, c0 = s.positions(), ctx(s, rebuilds_before)
    e, f = s.energy(), s.forces()
    return dict(positions=x, context=c0, energy=e, forces=f, context_observed=ctx(s, rebuilds_before))


CTX_FIELDS = ("step", "time", "bead_scale", "bond_scale", "semiaxes", "axial_reaction", "rollbacks", "rebuilds", "rebuild_interval",
              "list_path", "callback_pending")


def differences(a, b):
    """Where two observed() records differ, in words (empty: bit-identical)."""
    out = []
    for key in ("positions", "energy", "forces"):
        if not np.array_equal(a[key], b[key]):
            d = np.argwhere(np.asarray(a[key]) != np.asarray(b[key]))
            out.append(f"{key}: {len(d)} words differ, first at {tuple(d[0])}, replicas {sorted(set(int(i[0]) for i in d))[:8]}")
    for key in ("context", "context_observed"):
        for r, (ca, cb) in enumerate(zip(a[key], b[key])):
            for name, va, vb in zip(CTX_FIELDS, ca, cb):
                if va != vb:
                    out.append(f"{key}[{r}].{name}: {va!r} != {vb!r}")
    return out


def assert_observed_identical(a, b):
    """Two observed() records are the same, bit for bit."""
    diff = differences(a, b)
    assert not diff, "\n".join(diff[:12] + ([f"... {len(diff) - 12} more"] if len(diff) > 12 else []))
