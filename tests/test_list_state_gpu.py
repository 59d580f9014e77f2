"""The resident list of a handle through its events, as gd_get_context reports it (csrc/gdyn_list.hpp, the transition table of
DESIGN.md; the transitions themselves are pinned on the CPU by test_resident_list.py).  Every case walks one handle through
observations, runs, a context set to its own values, a pair search beyond the list radius and the caller's own positions, and counts
list builds exactly, in both directions: an event that needs no list build costs none, an invalidation costs one -- each is preceded
by a converged build of the same state, so no build is repeated for a row width or a tile class.

The rebuild interval is fixed at 8 steps with the adaptation off (set before the first build: gd_set_tuning drops the list), and the
runs move no scale, so the force radius is one number per case and the interval is counted in steps."""
import numpy as np
import pytest

from util import CASES, build, g

pytestmark = pytest.mark.gpu
SEED = 20220101
PATHS = {"tiled": 2, "generic": 1}
K = 8


def _handle(hip, name, path):
    s, dt, kT, flags = build(hip, name, n_replicas=2)
    s.set_tuning(kernel_path=PATHS[path], rebuild_interval=K, adapt_interval=0)
    return s, dt, kT, flags & ~g.RUN_UPDATE_SCALES          # (a moving bead scale moves the cutoff behind the last step: never verified)


def _builds(s, call):
    """What `call` returns and the list builds it cost."""
    before = s.context().rebuilds
    out = call()
    return out, s.context().rebuilds - before


def _set_own_context(s):
    for r in range(s.R):
        c = s.context(r)
        s.set_context(r, c.step, c.bead_scale, c.bond_scale, list(c.semiaxes))


def _assert_in_use(s, path, radius=None):
    c = s.context()
    assert c.list_path == PATHS[path] and c.list_bytes > 0 and c.list_entries > 0
    assert (c.tile_capacity > 0 and c.largest_tile > 0 and c.near_entries > 0) if path == "tiled" else (c.tile_capacity == 0 and c.near_entries == 0)
    if radius is not None:
        assert c.list_radius == radius
    return c


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["genome", "ab_box"])
def test_list_state_through_its_events(hip, name, path):
    s, dt, kT, flags = _handle(hip, name, path)
    run = lambda n: s.run(n, dt, kT, seed=SEED, flags=flags)
    c = s.context()
    assert (c.list_path, c.rebuilds, c.list_bytes, c.tile_capacity, c.list_entries) == (0, 0, 0, 0, 0)      # before any build

    # observations: the first builds (as often as the row width and the tile class need), the second builds nothing
    e0, n = _builds(s, s.energy)
    assert n >= 1
    force_radius = _assert_in_use(s, path).list_radius
    e1, n = _builds(s, s.energy)
    assert n == 0 and np.array_equal(e0, e1)

    # a run of one interval steps on that list; behind it the tiled list is the verified one, the generic path builds
    _, n = _builds(s, lambda: run(K))
    c = _assert_in_use(s, path, force_radius)
    assert n == 0 and c.rollbacks == 0 and c.step == K
    _, n = _builds(s, s.energy)
    assert n == (0 if path == "tiled" else 1)
    _assert_in_use(s, path, force_radius)

    # the context set to its own values: the list is dropped, what describes the list in use reads 0, the path stays
    _, n = _builds(s, lambda: _set_own_context(s))
    c = s.context()
    assert n == 0 and (c.list_bytes, c.tile_capacity, c.largest_tile) == (0, 0, 0) and c.list_path == PATHS[path] and c.list_radius == force_radius
    _, n = _builds(s, s.energy)
    assert n == 1
    _assert_in_use(s, path, force_radius)

    # a pair search beyond the list radius: one build at its distance, which serves the next steps as the force list
    d = 1.1 * force_radius
    pairs, n = _builds(s, lambda: s.search_pairs(d))
    c = _assert_in_use(s, path)
    assert n == 1 and len(pairs) > s.N and c.list_radius >= d
    search_radius = c.list_radius
    pairs2, n = _builds(s, lambda: s.search_pairs(d))
    assert n == 0 and np.array_equal(pairs, pairs2)
    _, n = _builds(s, lambda: run(K // 2))
    assert n == 0
    _assert_in_use(s, path, search_radius)
    _, n = _builds(s, lambda: run(K))          # the interval passes at this run's step K / 2: one build, at the force radius again
    assert n == 1
    c = _assert_in_use(s, path, force_radius)
    assert c.rollbacks == 0 and c.step == 2 * K + K // 2

    # the caller's positions -- the handle's own: one build at the next observation, the same energies to the bit.  (Sums follow the
    # order of the list, the list the cell grid, and a tiled build lays its grid on the box the build before it recorded: the energies
    # before come from the second of two builds at these positions, whose grid is the one a build from the caller's positions measures.)
    for _ in range(2):
        _set_own_context(s)
        e0, n = _builds(s, s.energy)
        assert n == 1
    x = s.positions()
    _, n = _builds(s, lambda: s.set_positions(x))
    c = s.context()
    assert n == 0 and (c.list_bytes, c.tile_capacity) == (0, 0) and c.list_path == PATHS[path]
    e1, n = _builds(s, s.energy)
    assert n == 1 and np.array_equal(e0, e1), (n, e0, e1)
    _assert_in_use(s, path, force_radius)
    s.close()


def test_a_model_without_a_pair_term_has_no_list(hip):
    """Both pair energies zero: no cutoff, no list.  The handle sorts its beads at the same cadence (a build each, counted as one) and
    steps; list_bytes and list_entries stay 0 throughout."""
    s, dt, kT, flags = _handle(hip, "genome", "tiled")
    s.set_pair_softcore(0.0, 0.30, 0.0, 0.24, 2, 3, 8, 3, mix=True, scale_by_bead_scale=True)

    def no_list(rebuilds):
        for r in range(s.R):
            c = s.context(r)
            assert (c.list_bytes, c.list_entries, c.near_entries, c.tile_capacity, c.row_repairs) == (0, 0, 0, 0, 0) and c.rebuilds == rebuilds
        return s.context()

    assert no_list(0).list_path == 0
    e0 = s.energy()
    assert np.all(np.isfinite(e0)) and np.all(s.energy(g.TERM_PAIR) == 0.0)
    assert no_list(1).list_path == 1
    s.run(K, dt, kT, seed=SEED, flags=flags)
    assert no_list(1).step == K
    s.run(K, dt, kT, seed=SEED, flags=flags)          # the interval has passed
    c = no_list(2)
    assert c.step == 2 * K and c.rollbacks == 0
    assert not np.array_equal(s.energy(), e0)
    no_list(3)
    s.close()
