"""gd_context's list statistics against an exact census of the lists (tests/list_census.py, fp64 on the CPU).

list_entries, near_entries and list_bytes are what bench.py prices the roofline fraction and design_min_bytes_per_launch from.  Every case
pins skin and near_fraction, lists positions that clear_of_boundaries() has moved off the fp32 windows around the radii -- so the
device has to EQUAL the census, with no bracket that could hide a missing entry -- and builds with forces() right after
set_positions, so that the positions of the build are the inputs.  The pair set gd_search_pairs serves from the resident list just
under the full list radius sees an entry dropped from the outer skin, which no force at the build does."""
import numpy as np
import pytest

from list_census import (boundary_window, census, clear_of_boundaries, near_radius, pair_keys)
from util import g, wl

pytestmark = pytest.mark.gpu

SKIN = 0.75
BLOCK = 512                 # GD_BLOCK: slots of a replica are padded to whole blocks (Np)
MAX_FAR = 504               # GD_TILED_MAX_FAR: a far class beyond it does not fit the tiled record -> single-class lists


def _f32(v):
    return float(np.float32(v))


def list_radius(cutoff, scale, skin=SKIN):
    """list radius = cutoff x (bead_scale + skin) (gdyn.h, gd_tuning.skin), in the host's arithmetic: fp32 cutoff, fp64 product, fp32 result."""
    return _f32(_f32(cutoff) * (scale + skin))


def generic_width(w0, longest):
    """Row width of generic lists after the build that fits: it starts at w0 (96, or the caller's list_width) rounded up to whole batches of
    8; a list that outgrows it is rebuilt at need + need / 16 + 8 (need: the longest list padded to a batch), at least 8 more."""
    w = (max(w0, 8) + 7) & ~7
    need = (int(longest) + 7) & ~7
    if need > w:
        w = (max(need + need // 16 + 8, w + 8) + 7) & ~7
    return w


def clear_all(x, box, rv, rn, max_moved=0.01):
    """Every replica's positions cleared of the windows around the list radius, the near radius and the search radius rv - 2 w."""
    out, ws = [], []
    for xr in x:
        w = boundary_window(np.asarray(xr, dtype=np.float32), box)
        y, moved = clear_of_boundaries(xr, box, [rv, rn, rv - 2 * w], w, max_moved=max_moved)
        out.append(y); ws.append(w)
        print(f"  cleared: w {w:.3e}, beads moved {moved} of {len(xr)}")
    return np.stack(out), ws


def check_lists(s, x, box, ws, rv, rn, path, label, w0=96, two_class=True):
    """The handle's list statistics and full-radius pair sets against the census of x (R, N, 3), replica by replica."""
    R, n = x.shape[0], x.shape[1]
    npad = (n + BLOCK - 1) // BLOCK * BLOCK
    cen = [census(x[r], box, rv, rn if (path == 2 and two_class) else rv) for r in range(R)]
    failed = []
    for r in range(R):
        c = s.context(r)
        near_expected = cen[r].near_entries if path == 2 else 0          # (generic lists: 0, gdyn.h)
        print(f"{label} r{r}: path {c.list_path} rv {c.list_radius:.7f} | list_entries device {c.list_entries} census {cen[r].list_entries}"
              f" | near_entries device {c.near_entries} census {near_expected} | longest {cen[r].n_all.max()} shortest {cen[r].n_all.min()}"
              f" | row_repairs {c.row_repairs}")
        assert c.list_path == path
        assert c.list_radius == rv, (c.list_radius, rv)
        # the pair set served from the resident list just under the full list radius (dcut + 2 D <= rv holds with D = 0: no build)
        rb = s.context().rebuilds
        dcut = rv - 2 * ws[r]
        ph = pair_keys(s.search_pairs(dcut, replica=r), n)
        pc = cen[r].pair_keys(dcut)
        only_dev, only_cen = np.setdiff1d(ph, pc), np.setdiff1d(pc, ph)
        print(f"{label} r{r}: pairs within {dcut:.7f}: device {len(ph)} census {len(pc)}, only device {len(only_dev)}, only census {len(only_cen)}"
              + "".join(f" ({k // n},{k % n})" for k in list(only_dev[:4]) + list(only_cen[:4])))
        assert s.context().rebuilds == rb and len(pc) > 0
        # (every figure is printed before the first of them is judged: a failing run's log shows all that differs)
        if c.list_entries != cen[r].list_entries:
            failed.append((r, "list_entries", c.list_entries, cen[r].list_entries))
        if c.near_entries != near_expected:
            failed.append((r, "near_entries", c.near_entries, near_expected))
        if len(only_dev) or len(only_cen):
            failed.append((r, "pair set", len(only_dev), len(only_cen)))
    assert not failed, (label, failed)
    c = s.context()
    chunks = [cen[r].chunks(two_class=two_class and path == 2) for r in range(R)]
    if path == 2:
        # lower bound: every bead's own chunks of 8 entries, 16 bytes each, each class padded to whole chunks
        lower = 16 * int(sum(ch.sum() for ch in chunks))
        # upper bound: rows come from the pool in KiB (one chunk for the 64 lanes of a k_step wave).  A build without history gives
        # every wave the chunks of the starting guess (w0 / 8); a wave whose longest list outgrows them is given fresh rows of what that
        # list needs -- at most the chunks of the longest list of all -- and the abandoned rows stay taken: counted once
        waves = R * npad // 64
        upper = 1024 * waves * (max(w0 // 8, 1) + int(max(ch.max() for ch in chunks)))
        print(f"{label}: list_bytes {c.list_bytes} in [{lower}, {upper}] ({waves} waves, guess {max(w0 // 8, 1)} chunks, longest {max(ch.max() for ch in chunks)})")
        assert lower <= c.list_bytes <= upper, (c.list_bytes, lower, upper)
    else:
        # generic lists: uniform rows of list_W entries of 4 bytes for every slot of every replica
        W = generic_width(w0, max(cr.n_all.max() for cr in cen))
        print(f"{label}: list_bytes {c.list_bytes}, uniform rows of {W}: {W * R * npad * 4}")
        assert c.list_bytes == W * R * npad * 4, (c.list_bytes, W, R, npad)
    return cen


def ab_gas(lib, n, R, box=None):
    s = g.System(lib, n, R, box=box)
    s.set_bead_params(a=(np.arange(n) % 2).astype(float), b=((np.arange(n) + 1) % 2).astype(float), mobility=np.ones(n))
    s.set_pair_softcore(2.0, 0.3, 2.0, 0.24)
    return s


def gas_positions(n=6000):
    """Two replicas at different densities: 48 and 17 beads per unit volume (26 and 10 list entries per bead)."""
    rng = np.random.default_rng(31)
    return np.stack([(rng.random((n, 3)) - 0.5) * 5.0, (rng.random((n, 3)) - 0.5) * 7.0])


# ---- 1. open gas, tiled (16-bit entries) and generic

@pytest.mark.parametrize("path,near_fraction", [(2, 0.65), (2, 0.3), (1, 0.65)])
def test_open_gas_two_densities(hip, path, near_fraction):
    """Per-replica counts differ and each equals its own census (the lcount[r] / lcount[R + r] indexing)."""
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, near_fraction)
    x, ws = clear_all(gas_positions(), None, rv, rn)
    s = ab_gas(hip, x.shape[1], 2)
    s.set_tuning(skin=SKIN, near_fraction=near_fraction, kernel_path=path)
    s.set_positions(x)
    s.forces()
    assert path == 1 or s.context().tile_capacity <= 4080          # (tiles of this class hold 16-bit byte offsets)
    cen = check_lists(s, x, None, ws, rv, rn, path, f"gas path {path} nf {near_fraction}")
    assert cen[0].list_entries > 2 * cen[1].list_entries and cen[0].near_entries > 2 * cen[1].near_entries
    s.close()


# ---- 2. scaled cutoff

def test_scaled_cutoff_two_bead_scales(hip):
    """The genome model with bead_scale 0.8 in replica 0 and 1.0 in replica 1.  The handle builds ONE list radius and ONE near radius
    for all its replicas, from the largest bead scale (cut_scale: cutoff x (max scale + skin)): both replicas are censused at that
    radius, and near_radius() checks that the look-ahead cutoff it was derived from is cutoff x 1.0."""
    n, R = 6000, 2
    s, _ = wl.genome_interphase(hip, n_beads=n, n_replicas=R)
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    x, ws = clear_all(s.positions(), None, rv, rn)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2)
    c1 = s.context(1)
    s.set_context(0, 0, 0.8, 0.8, list(c1.semiaxes))
    s.set_positions(x)
    s.forces()
    assert s.context(0).bead_scale == 0.8 and s.context(1).bead_scale == 1.0
    check_lists(s, x, None, ws, rv, rn, 2, "scaled cutoff")
    # both replicas at 0.8: the radius follows, rn = 0.24 + 0.65 x skin width
    s.set_context(1, 0, 0.8, 0.8, list(c1.semiaxes))
    rv8 = list_radius(0.3, 0.8)
    rn8 = near_radius(rv8, 0.3, 0.8, SKIN, 0.65)
    assert abs(rn8 - (0.24 + 0.65 * 0.225)) < 1e-6
    x8, ws8 = clear_all(x, None, rv8, rn8)
    s.set_positions(x8)
    s.forces()
    check_lists(s, x8, None, ws8, rv8, rn8, 2, "scaled cutoff 0.8")
    s.close()


# ---- 3. globule and gas in one handle

def globule_and_gas(seed, n_glob=3000, n_gas=9000):
    g0 = np.random.default_rng(seed)
    v = g0.normal(size=(n_glob, 3))
    glob = 1.0 * v / np.linalg.norm(v, axis=1)[:, None] * g0.random((n_glob, 1)) ** (1 / 3)       # ~700 beads per unit volume
    gas = (g0.random((n_gas, 3)) - 0.5) * 9.0 + np.array([7.0, 0.0, 0.0])                          # ~12 per unit volume, elsewhere
    return np.concatenate([glob, gas])


def test_globule_and_gas_in_one_handle(hip):
    """The state of test_ragged_rows_globule_and_gas_in_one_handle: exact counts where list lengths span 0 to several hundred, and
    the ragged-rows claim as a bound: the lists take at most (guess + longest list) per wave -- here a fraction of uniform rows.
    (The window is 16 ulps of the gas's coordinates, up to 11.5, and the globule holds 630 000 pairs inside the list radius: 180 of
    them lie in a window, 1.5 % of the 12 000 beads are moved -- the one case that passes the clearing a limit of 2 % instead of 1 %.
    The lengths asserted below show that the state is still the globule and the gas.)"""
    n, R = 12000, 2
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    x, ws = clear_all(np.stack([globule_and_gas(101), globule_and_gas(202)]), None, rv, rn, max_moved=0.02)
    s = ab_gas(hip, n, R)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2)
    s.set_positions(x)
    s.forces()
    cen = check_lists(s, x, None, ws, rv, rn, 2, "globule and gas")
    for c in cen:
        assert c.n_all[:3000].max() > 400 and c.n_all[:3000].mean() > 200 and c.n_all[3000:].min() <= 3 and c.n_all[3000:].mean() < 10
    longest = max(c.n_all.max() for c in cen)
    assert s.context().list_bytes < 0.5 * 2.0 * R * n * longest           # (uniform rows of 16-bit entries of the longest list)
    s.close()


# ---- 4. repair

def test_repaired_rows_open(hip):
    """test_rows_recover_from_a_first_guess_that_is_far_too_small: every wave outgrows the one-chunk rows of list_width = 8.  The first
    build also outgrows the pool sized from that guess and is built again from what the beads needed; the state is then listed a
    second time from the same guess (positions set again: no history) into the pool that has its size: that build's waves are
    repaired in place, and its counters must still equal the census."""
    n, R = 8000, 2
    s, _ = wl.genome_interphase(hip, n_beads=n, n_replicas=R)
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    x, ws = clear_all(s.positions(), None, rv, rn)
    for relisted in (False, True):
        s.set_positions(x)
        s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2, list_width=8)
        s.forces()
        print("repair, open: relisted", relisted, "row_repairs", s.context().row_repairs, "rebuilds", s.context().rebuilds)
    assert s.context().row_repairs > 0
    check_lists(s, x, None, ws, rv, rn, 2, "repair, open", w0=8)
    s.close()


def test_repaired_rows_periodic(hip):
    """The same in the periodic 1 kb model (test_rows_recover_from_a_first_guess_that_is_far_too_small_periodic)."""
    n, R = 3000, 2
    s, info = wl.chromatin_1kb(hip, n_beads=n, n_replicas=R, n_loops=30, n_glues=60)
    box = (float(info["box"]),) * 3
    rv = list_radius(1.5, 1.0)
    rn = near_radius(rv, 1.5, 1.0, SKIN, 0.65)
    x, ws = clear_all(s.positions(), box, rv, rn)
    for relisted in (False, True):
        s.set_positions(x)
        s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2, list_width=8)
        s.forces()
        print("repair, periodic: relisted", relisted, "row_repairs", s.context().row_repairs, "rebuilds", s.context().rebuilds)
    assert s.context().row_repairs > 0
    check_lists(s, x, box, ws, rv, rn, 2, "repair, periodic", w0=8)
    s.close()


# ---- 5. periodic boxes, images

def test_periodic_images_1kb(hip):
    """The 1 kb model with every bead shifted by whole periods, up to 3 either way: minimum-image counts and pair sets."""
    n, R = 3000, 2
    s, info = wl.chromatin_1kb(hip, n_beads=n, n_replicas=R, n_loops=30, n_glues=60)
    L = float(info["box"])
    rv = list_radius(1.5, 1.0)
    rn = near_radius(rv, 1.5, 1.0, SKIN, 0.65)
    x0 = s.positions()
    x0 -= L * np.floor(x0 / L)
    k = np.random.default_rng(3).integers(-3, 4, size=(R, n, 3))
    assert k.min() == -3 and k.max() == 3
    x, ws = clear_all(x0 + k * L, (L,) * 3, rv, rn)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2)
    s.set_positions(x)
    s.forces()
    cen = check_lists(s, x, (L,) * 3, ws, rv, rn, 2, "1 kb, images")
    # (a shift by whole periods changes no minimum-image distance: the census is that of the beads inside the box)
    back = census(x[0] - k[0] * L, (L,) * 3, rv, rn)
    assert cen[0].list_entries == back.list_entries and cen[0].near_entries == back.near_entries and np.array_equal(cen[0].n_all, back.n_all)
    s.close()


@pytest.mark.parametrize("cells_x,path", [(3.4, 2), (2.5, 1)])
def test_periodic_thin_boxes(hip, cells_x, path):
    """A periodic gas in a box whose x axis holds exactly three cells of the list radius (tiled lists: every cell's neighbours are the
    whole row) and in one of two cells, which the tile builder hands to the generic path (aliasing neighbours); beads lie up to
    3 periods outside the box."""
    n, R = 3000, 2
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    box = (cells_x * rv, 5.0, 6.0)
    assert int(box[0] / rv) == int(cells_x) and box[0] > 2 * rv
    rng = np.random.default_rng(41)
    x0 = rng.random((R, n, 3)) * np.array(box)
    x0[1, :, 1] *= 0.8                                              # (the second replica: a denser slab)
    x0 = x0 + np.array(box) * rng.integers(-3, 4, size=(R, n, 3))
    x, ws = clear_all(x0, box, rv, rn)
    s = ab_gas(hip, n, R, box=box)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2)
    s.set_positions(x)
    s.forces()
    check_lists(s, x, box, ws, rv, rn, path, f"periodic, {cells_x} cells")
    s.close()


# ---- 6. single-class lists

def test_dense_cluster_two_classes(hip):
    """test_dense_cluster_within_and_beyond_the_tiled_record at 360 beads: 359 near entries per bead of the ball, list_width 400."""
    n_core = 360
    rng = np.random.default_rng(11)
    n = n_core + 840
    v = rng.normal(size=(n_core, 3))
    core = 0.1 * v / np.linalg.norm(v, axis=1)[:, None] * rng.random((n_core, 1)) ** (1 / 3)
    x0 = np.concatenate([core, (rng.random((n - n_core, 3)) - 0.5) * 6.0])[None]
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    x, ws = clear_all(x0, None, rv, rn)
    s = ab_gas(hip, n, 1)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2, list_width=400)
    s.set_positions(x)
    s.forces()
    cen = check_lists(s, x, None, ws, rv, rn, 2, "dense cluster", w0=400)
    assert cen[0].n_near.max() >= 359 and 8 * ((cen[0].n_far.max() + 7) // 8) <= MAX_FAR
    s.close()


def test_far_class_beyond_the_record_single_class_lists(hip):
    """test_far_class_beyond_the_tiled_record_builds_single_class_lists: two balls of 600 beads 0.49 apart, every bead holds the other
    ball in its far class -- 600 entries where the record's field counts 504.  The handle builds single-class lists: every entry is
    a near entry (rn = rv), near_entries counts them all in fours, and each bead's chunks are those of its whole list."""
    rng = np.random.default_rng(5)
    nb, n = 600, 2 * 600 + 800

    def ball(c):
        v = rng.normal(size=(nb, 3))
        return c + 0.01 * v / np.linalg.norm(v, axis=1)[:, None] * rng.random((nb, 1)) ** (1 / 3)
    x0 = np.concatenate([ball(np.array([0.0, 0.0, 0.0])), ball(np.array([0.49, 0.0, 0.0])),
                         (rng.random((n - 2 * nb, 3)) - 0.5) * 6.0 + np.array([0.0, 0.0, 5.0])])[None]
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    x, ws = clear_all(x0, None, rv, rn)
    two = census(x[0], None, rv, rn)
    assert 8 * ((two.n_far.max() + 7) // 8) > MAX_FAR and two.n_all.max() <= 8184          # (the far class overflows its field, the list fits one class)
    s = ab_gas(hip, n, 1)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=2)
    s.set_positions(x)
    s.forces()
    cen = check_lists(s, x, None, ws, rv, near_radius(rv, 0.3, 1.0, SKIN, 0.65, single_class=True), 2, "single class", two_class=False)
    assert cen[0].near_entries == int((4 * ((two.n_all + 3) // 4)).sum()) > two.near_entries
    s.close()


# ---- 7. after a run

@pytest.mark.parametrize("path", [2, 1])
def test_counters_after_a_run(hip, path):
    """Case 1 stepped for 3 rebuild intervals of K = 5 steps at T = 1, one gd_run per interval.  begin_phase drops the list, so every
    run starts with a build -- on the positions read just before it, with rows predicted from the build before -- and steps K times on
    that list: gd_timing.list_entries_visited (the sum over the run's step launches of the directed entries stored, all replicas)
    is K x the sum of list_entries after the run, exactly.  The first build lists the cleared input: its counters equal the census.
    The later builds list positions the device produced, which cannot be moved off the windows: their counters lie between the
    censuses at radius - w and radius + w (equal in most runs; printed).  At the end the positions are read, cleared, set again
    and listed: exact once more."""
    K, dt, kT = 5, 1e-5, 1.0
    rv = list_radius(0.3, 1.0)
    rn = near_radius(rv, 0.3, 1.0, SKIN, 0.65)
    x, ws = clear_all(gas_positions(), None, rv, rn)
    R = x.shape[0]
    s = ab_gas(hip, x.shape[1], R)
    s.set_tuning(skin=SKIN, near_fraction=0.65, kernel_path=path, rebuild_interval=K, adapt_interval=0)
    s.set_positions(x)
    s.forces()
    check_lists(s, x, None, ws, rv, rn, path, f"before the run, path {path}")
    s.begin_phase()
    for i in range(3):
        xb = s.positions()
        rb = s.context().rebuilds
        t = s.run(K, dt, kT, seed=7 + i, replica_seeds=[11 + i, 21 + i])
        c = [s.context(r) for r in range(R)]
        assert c[0].rebuilds == rb + 1 and c[0].rollbacks == 0 and c[0].list_path == path and c[0].rebuild_interval == K
        assert t.step_launches == K and t.rebuild_launches == 1
        L = sum(cr.list_entries for cr in c)
        print(f"run {i}: list_entries_visited {t.list_entries_visited}, K x L {K * L}")
        assert t.list_entries_visited == K * L
        for r in range(R):
            w = boundary_window(xb[r].astype(np.float32), None)
            lo, hi = census(xb[r], None, rv - w, rn - w), census(xb[r], None, rv + w, rn + w)
            near = (lo.near_entries, hi.near_entries) if path == 2 else (0, 0)
            print(f"run {i} r{r}: list_entries device {c[r].list_entries} census [{lo.list_entries}, {hi.list_entries}]"
                  f" | near_entries device {c[r].near_entries} census [{near[0]}, {near[1]}]")
            assert lo.list_entries <= c[r].list_entries <= hi.list_entries
            assert near[0] <= c[r].near_entries <= near[1]
            if i == 0:
                assert lo.list_entries == hi.list_entries and near[0] == near[1]          # (the cleared input: exact)
    x1, ws1 = clear_all(s.positions(), None, rv, rn)
    assert np.abs(x1 - x).max() > 0.01
    s.set_positions(x1)
    s.forces()
    check_lists(s, x1, None, ws1, rv, rn, path, f"after the run, path {path}")
    s.close()
