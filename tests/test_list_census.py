"""tests/list_census.py against an O(N^2) double loop and hand values (CPU only): the census is what the device tests of
test_list_census_gpu.py hold gd_context's list statistics to, so it is checked on its own first."""
import numpy as np
import pytest

from list_census import (PUSH, boundary_pairs, boundary_window, census, clear_of_boundaries, near_radius)

N = 400


def _loop_census(x, box, rv, rn, r_pairs):
    """The same by a double loop over all pairs, minimum image by rounding to the nearest period."""
    n = len(x)
    n_all, n_near, pairs = np.zeros(n, dtype=int), np.zeros(n, dtype=int), set()
    for i in range(n):
        for j in range(i + 1, n):
            d = x[i] - x[j]
            if box is not None:
                d = d - np.asarray(box) * np.round(d / np.asarray(box))
            r = float(np.sqrt(d @ d))
            if r < rv:
                n_all[i] += 1; n_all[j] += 1
            if r < rn:
                n_near[i] += 1; n_near[j] += 1
            if r < r_pairs:
                pairs.add((i, j))
    return n_all, n_near, pairs


def _cloud(box, seed, spread):
    rng = np.random.default_rng(seed)
    if box is None:
        return (rng.random((N, 3)) - 0.5) * spread
    x = rng.random((N, 3)) * np.asarray(box)
    x += np.asarray(box) * rng.integers(-3, 4, size=(N, 3))        # several periods outside the box, both signs
    return x


# open; a cubic box; a box with an axis of exactly three cells of the radius and one of fewer than three (2.1, 1.2 cells)
@pytest.mark.parametrize("box", [None, (2.9, 2.9, 2.9), (3 * 0.525, 2.1 * 0.525, 1.2 * 0.525)])
def test_census_equals_a_double_loop(box):
    rv, rn, rs = 0.525, 0.446, 0.5
    x = _cloud(box, 3, 2.5)
    if box is not None:
        assert x.min() < -2 * max(box) and x.max() > 3 * max(box)
    c = census(x, box, rv, rn)
    n_all, n_near, pairs = _loop_census(x, box, rv, rn, rs)
    assert n_all.sum() > 4 * N and 0 < n_near.sum() < n_all.sum()
    assert np.array_equal(c.n_all, n_all) and np.array_equal(c.n_near, n_near)
    assert c.list_entries == n_all.sum()
    assert c.near_entries == sum(4 * -(-int(k) // 4) for k in n_near)
    assert c.pairs(rs) == pairs and len(pairs) > N
    assert np.array_equal(c.chunks(), -(-n_near // 8) + -(-(n_all - n_near) // 8))
    assert np.array_equal(c.chunks(two_class=False), -(-n_all // 8))
    # single-class lists: rn = rv, every entry is a near entry
    c1 = census(x, box, rv, rv)
    assert np.array_equal(c1.n_near, n_all) and c1.near_entries == sum(4 * -(-int(k) // 4) for k in n_all)


def test_census_counts_a_pair_on_the_radius_as_outside():
    x = np.array([[0.0, 0, 0], [0.5, 0, 0], [0, 0.25, 0]])
    c = census(x, None, 0.5, 0.25)
    assert c.list_entries == 2 and list(c.n_near) == [0, 0, 0] and c.pairs(0.5) == {(0, 2)} and c.pairs(0.25) == set()
    c = census(x, None, np.nextafter(0.5, 1), np.nextafter(0.25, 1))
    assert c.list_entries == 4 and list(c.n_near) == [1, 0, 1] and c.near_entries == 8 and c.pairs(c.rv) == {(0, 1), (0, 2)}


def test_near_radius_hand_values():
    f = np.float32
    # cutoff 0.3, bead scale 1, skin 0.75: rv = 0.525, cutb = 0.3, rn = 0.3 + 0.65 x 0.225 = 0.44625 (in fp32 arithmetic)
    rv = float(f(float(f(0.3)) * 1.75))
    assert abs(rv - 0.525) < 1e-7
    rn = near_radius(rv, 0.3, 1.0, 0.75, 0.65)
    cutb = f(rv) - f(float(f(0.3)) * 0.75)
    assert rn == float(cutb + f(0.65) * (f(rv) - cutb)) and abs(rn - 0.44625) < 1e-7
    assert abs(near_radius(rv, 0.3, 1.0, 0.75, 0.3) - 0.3675) < 1e-7
    # a scaled cutoff: rv = 0.3 x (0.8 + 0.75) = 0.465, cutb = 0.24 = cutoff x bead_scale, rn = 0.24 + 0.65 x 0.225
    rv8 = float(f(float(f(0.3)) * 1.55))
    assert abs(near_radius(rv8, 0.3, 0.8, 0.75, 0.65) - 0.38625) < 1e-7
    with pytest.raises(AssertionError):
        near_radius(rv8, 0.3, 1.0, 0.75, 0.65)           # (the radius was not derived with this scale)
    # single-class lists
    assert near_radius(rv, 0.3, 1.0, 0.75, 0.65, single_class=True) == rv
    # the 1 kb model: cutoff 1.5, skin 0.75: rv = 2.625, rn = 1.5 + 0.65 x 1.125 = 2.23125
    assert abs(near_radius(2.625, 1.5, 1.0, 0.75, 0.65) - 2.23125) < 1e-6


@pytest.mark.parametrize("box", [None, (4.0, 4.0, 4.0)])
def test_clear_of_boundaries_moves_pairs_off_both_radii(box):
    rv, rn = 0.525, 0.446
    rng = np.random.default_rng(8)
    x = (rng.random((3000, 3)) * 4.0).astype(np.float32).astype(np.float64)
    # pairs placed on both radii (as exactly as fp32 coordinates allow), along different directions, one across the periodic boundary
    seeds = [(10, 11, rv, (1, 0, 0)), (20, 21, rn, (0, 1, 0)), (30, 31, rv, (0.6, 0, 0.8)), (40, 41, rn, (0, 0.8, -0.6))]
    for i, j, r, u in seeds:
        x[j] = x[i] + r * np.asarray(u)
    if box is not None:
        x[50] = [0.01, 2.0, 2.0]; x[51] = [0.01 - rv + 4.0, 2.0, 2.0]
        seeds.append((50, 51, rv, None))
    x = x.astype(np.float32).astype(np.float64)
    w = boundary_window(x, box)
    # (16 ulps of the largest magnitude: the period 4 has an ulp of 2^-21, coordinates in [2, 4) one of 2^-22)
    assert w == 16 * 2.0 ** (-21 if box is not None or np.abs(x).max() >= 4 else -22)
    before = {tuple(p) for p in boundary_pairs(x, box, [rv, rn], w)}
    assert {(i, j) for i, j, _, _ in seeds} <= before
    y, moved = clear_of_boundaries(x, box, [rv, rn], w)
    assert len(boundary_pairs(y, box, [rv, rn], w)) == 0
    assert len(before) <= moved < 30 and np.array_equal(y, y.astype(np.float32))
    changed = np.flatnonzero(np.any(y != x, axis=1))
    assert len(changed) == moved and {j for _, j, _, _ in seeds} <= set(changed)
    assert np.abs(np.linalg.norm(y[changed] - x[changed], axis=1) / PUSH - np.rint(np.linalg.norm(y[changed] - x[changed], axis=1) / PUSH)).max() < 1e-3
    y2, _ = clear_of_boundaries(x, box, [rv, rn], w)
    assert np.array_equal(y, y2)                         # deterministic
    # the census of the cleared input does not depend on which side of a window the radius is taken
    for r_lo, r_hi in ((rv - w, rv + w), (rn - w, rn + w)):
        assert census(y, box, r_lo, r_lo).list_entries == census(y, box, r_hi, r_hi).list_entries
    assert census(x, box, rv - w, rn).list_entries < census(x, box, rv + w, rn).list_entries


def test_clear_of_boundaries_refuses_an_input_it_would_have_to_rewrite():
    x = np.zeros((50, 3)); x[:, 0] = 0.525 * np.arange(50)          # a rod with every neighbour pair on the radius
    with pytest.raises(AssertionError):
        clear_of_boundaries(x, None, [0.525])
