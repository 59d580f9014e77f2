"""The stressed states of tests/stressed_states.py on the CPU oracle (no GPU needed).

1. Coverage: each state reaches what the device comparisons at it rely on -- every configured term is a sizeable part of the total
   force in every replica, and the branches kernels get wrong (both sides of rest lengths and radii, tiny and folded bending angles,
   both sides of the wall, pair distances from 0 to the cutoff, images across the box faces) are populated.  These keep
   tests/test_term_parity_gpu.py from going vacuous the way the golden states are (test_golden_states_leave_terms_idle).
2. Per-term finite differences of the fp64 oracle at those states: the reference the device is held to is -grad U term by term.
   The wall's axial reaction: the production-size initial states leave it at zero (the record of why pressed_genome exists), the pressed
   genome presses on the wall from both sides, and the oracle's reaction equals its numpy restatement (tests/wall_restatement.py) --
   the reference tests/test_wall_context_gpu.py holds the device to.
3. The softcore-bond rule (include/gdyn.h): mix / scale_by_bond_scale are rejected; the accepted form is k_a (1-(r/l_a)^p)^q.
4. The runtime-power states (any soft-core powers but (2, 3, 8, 3): another pair kernel on the device): the spindle driver's form is
   the specialised form's function, the runtime composite, 1 kb, excluded-core, blob and box states reach every configured term with
   the pair term a sizeable part, and their forces are -grad U."""
import numpy as np
import pytest

import stressed_states as ss
import wall_restatement as wr
from util import CASES, build, g


def _assert_covered(s, configured):
    assert ss.idle_terms(s, configured) == [], ss.term_ratios(s)


# ------------------------------------------------------------------------------------------------ coverage

@pytest.mark.parametrize("name", list(CASES))
def test_golden_states_leave_terms_idle(oracle, name):
    """Why the stressed states exist: at the workloads' initial states (the golden states) spindle bonds and bending and the 1 kb
    springs do not act at all -- a per-term comparison there cannot see an error in them."""
    s, *_ = build(oracle, name)
    idle = ss.idle_terms(s, ss.CONFIGURED[name])
    assert idle == {"genome": [], "spindle": ["bend", "bond"], "ab_box": [], "chromatin_1kb": ["bond"]}[name]


@pytest.mark.parametrize("name", list(CASES))
def test_perturbed_workloads_cover_every_term(oracle, name):
    s = ss.perturbed(oracle, name)
    _assert_covered(s, ss.CONFIGURED[name])
    x = s.positions()
    assert x.shape[0] == 2 and np.abs(x[0] - x[1]).max() > 0.05                      # the replicas hold different states
    assert np.array_equal(x, ss.f32(x))
    if name == "genome":
        assert (s.context(0).bead_scale, s.context(0).bond_scale) != (s.context(1).bead_scale, s.context(1).bond_scale)
    if name == "spindle":
        info = ss.g_wl().spindle(oracle, n_beads=300)[1]
        r = ss.separations(x, ss.chain_bonds(info["ranges"])) / 0.2 - 1
        assert (r < -0.01).any() and (r > 0.01).any()                                # the semispring bonds: both sides of 0.2
        first = [i for b0, b1 in info["ranges"] for i in range(b0, b1 - 2)]
        th, _, _ = ss.bend_geometry(x, first)
        assert th.max() > 0.3                                                         # the rods are bent
    if name == "chromatin_1kb":
        r = ss.separations(x, ss.chain_bonds([(0, s.N)])) - 1.0
        assert (r < -0.01).any() and (r > 0.01).any()                                # the springs: compressed and stretched


def test_composite_model_reaches_every_branch(oracle):
    s = ss.composite(oracle)
    _assert_covered(s, ss.TERM_NAMES)
    x = s.positions()
    assert np.array_equal(x, ss.f32(x)) and np.abs(x[0] - x[1]).max() > 0.1
    scales = [(s.context(r).bead_scale, s.context(r).bond_scale) for r in range(2)]
    assert scales == list(ss.COMPOSITE_SCALES) and scales[0] != scales[1]
    for r in range(2):
        xr = x[r:r + 1]
        # semispring chains: both sides of the rest length, some within 1 % of it on either side
        u = ss.separations(xr, ss.chain_bonds([ss._chain_range(k) for k in ss.SEMISPRING_CHAINS])) / ss.BOND_L - 1
        assert (u < -0.01).any() and (u > 0.01).any()
        assert ((u > -0.01) & (u < 0)).any() and ((u > 0) & (u < 0.01)).any()
        # spring chains: compressed and stretched
        u = ss.separations(xr, ss.chain_bonds([ss._chain_range(k) for k in ss.SPRING_CHAINS])) / ss.BOND_L - 1
        assert (u < -0.01).any() and (u > 0.01).any()
        # softcore bonds: some inside their range l_a, some beyond
        u = ss.separations(xr, ss.softcore_bond_pairs().astype(np.int64)) / ss.SOFTCORE_BOND.l_a
        assert (u < 0.9).any() and (u > 1).any()
        # bending: angles under 1e-3 rad and over 3.1 rad, with unequal bond lengths in those triplets
        th, l1, l2 = ss.bend_geometry(xr, ss.composite_triplets())
        th, unequal = th[0], np.abs(l1 - l2)[0] > 0.05 * ss.BOND_L
        assert (th < 1e-3).any() and (th > 3.1).any() and th.min() > 0
        assert (unequal & (th < 1e-3)).any() and (unequal & (th > 3.1)).any()
        # point sources: targets inside and outside the semispring radius and the spring's rest radius
        for kind, _, b, pt, tg in ss.POINT_SOURCES:
            if kind == g.POT_HARMONIC:
                continue
            idx = slice(None) if tg is None else ss.source_targets(tg)
            dist = np.linalg.norm(x[r][idx] - np.array(pt), axis=-1)
            assert (dist < b).any() and (dist > b).any(), (kind, b)
        # the wall: beads on both sides of the surface where it acts, the outside ones within 0.02 of it
        Fw = np.linalg.norm(s.forces(g.TERM_WALL)[r], axis=-1)
        C = np.sum((x[r] / np.array(ss.SEMI)) ** 2, axis=-1) - 1
        assert ((C < 0) & (Fw > 0)).sum() >= 5 and ((C > 0) & (Fw > 0)).sum() >= 5
        assert Fw[C > 0].max() <= ss.PACKING * 0.025
        assert ((C < 0) & (Fw == 0)).sum() > 100                                     # and most of the beads away from it
        # pairs: one coincident pair; AA, BB and AB pairs from 1e-3 or closer to within 3 % of the cutoff
        cut = ss.PAIR["sigma_a"] * scales[r][0]
        pairs = s.search_pairs(cut, replica=r).astype(np.int64)
        dist = ss.separations(xr, pairs)[0]
        assert (dist == 0).sum() == 1
        a, b, _ = ss._types(s.N)
        ss._composite_free_types(a, b)
        for ta, tb in (((1, 0), (1, 0)), ((0, 1), (0, 1)), ((1, 0), (0, 1))):
            ti, tj = np.stack([a, b], 1)[pairs[:, 0]], np.stack([a, b], 1)[pairs[:, 1]]
            sel = (np.all(ti == ta, 1) & np.all(tj == tb, 1)) | (np.all(ti == tb, 1) & np.all(tj == ta, 1))
            assert dist[sel].min() <= 1.001e-3 and dist[sel].max() > 0.97 * cut, (ta, tb)


@pytest.mark.parametrize("shape", [(1.0, 1.0, 1.0), (0.8, 1.0, 1.25)])
def test_1kb_images_straddle_the_box_faces(oracle, shape):
    base = ss.chromatin_1kb_images(oracle, shifted=False, shape=shape)
    _assert_covered(base, ss.CONFIGURED["1kb_images"])
    s = ss.chromatin_1kb_images(oracle, shifted=True, shape=shape)
    L = np.array(s.box)
    assert len(set(s.box)) == len(set(shape))
    x, x0 = s.positions(), base.positions()
    assert np.array_equal(x, ss.f32(x)) and np.array_equal(np.rint((x - x0) / L), (x - x0) / L)     # shifts by whole periods, exact
    assert ((x < 0) | (x >= L)).any(axis=-1).mean() > 0.2                             # many beads outside [0, L) in raw coordinates
    loops, glues = ss.kb_pairs(s.N, 5)
    for r in range(2):
        # pair-term neighbours and glue pairs whose raw separation spans a box face: the minimum image is what makes them act
        nb = s.search_pairs(1.5, replica=r).astype(np.int64)
        raw = x[r, nb[:, 0]] - x[r, nb[:, 1]]
        assert (np.abs(raw) > L / 2).any(axis=-1).sum() > 100
        gl = glues.astype(np.int64)
        graw = np.linalg.norm(x[r, gl[:, 0]] - x[r, gl[:, 1]], axis=-1)
        gimg = ss.separations(x[r:r + 1], gl, box=s.box)[0]
        assert ((graw > 1.5) & (gimg < 1.5)).sum() >= 5                              # glues acting only through the image
        # unflagged chain bonds that are long in raw coordinates (and short through the image)
        cb = ss.chain_bonds([(0, s.N)])
        assert (ss.separations(x[r:r + 1], cb)[0] > L.min() / 2).sum() > 100
    # the oracle: pair and glue forces are those of the unshifted state; the springs see the raw separations
    for term in (g.TERM_PAIR,):
        assert np.abs(s.forces(term) - base.forces(term)).max() <= 1e-9 * np.abs(base.forces(term)).max()
    assert np.abs(s.forces(g.TERM_BOND)).max() > 100 * np.abs(base.forces(g.TERM_BOND)).max()


# ------------------------------------------------------------------------------------------------ the runtime-power states

def _pair_share(s):
    """max|F_pair| / max|F_all| per replica"""
    return ss.term_ratios(s)["pair"]


def test_spindle_driver_form_is_the_specialised_form_on_the_oracle(oracle):
    """host/gd_spindle.cpp's pair form (2, 3, 2, 3) with eps_b = sigma_b = 0 against (2, 3, 8, 3) with eps_b = 0 at the same state: one
    function of the positions (the B channel carries no energy), 1e-12 on the oracle -- so a difference between the two on the device
    (test_term_parity_gpu.py) is a difference between two kernels."""
    s, t = ss.spindle_driver(oracle), ss.spindle_driver(oracle, specialised=True)
    x = s.positions()
    assert np.array_equal(x, t.positions()) and np.array_equal(x, ss.f32(x)) and x.shape[0] == 2 and np.abs(x[0] - x[1]).max() > 0.05
    _assert_covered(s, ss.CONFIGURED["spindle_driver"])
    assert np.all(_pair_share(s) >= 0.3)
    F, Ft = s.forces(g.TERM_PAIR), t.forces(g.TERM_PAIR)
    assert np.abs(F - Ft).max() <= 1e-12 * np.abs(Ft).max()
    E, Et = s.energy(g.TERM_PAIR), t.energy(g.TERM_PAIR)
    assert np.all(E > 0) and np.all(np.abs(E - Et) <= 1e-12 * np.abs(Et))
    assert np.isfinite(s.forces()).all() and np.isfinite(s.energy()).all()


@pytest.mark.parametrize("powers", ss.RUNTIME_POWERS)
def test_runtime_power_composite_reaches_every_term(oracle, powers):
    s, d = ss.composite(oracle, powers=powers), ss.composite(oracle)
    _assert_covered(s, ss.TERM_NAMES)
    assert np.all(_pair_share(s) >= 0.3)
    x = s.positions()
    assert np.array_equal(x, d.positions()) and np.array_equal(x, ss.f32(x)) and np.abs(x[0] - x[1]).max() > 0.1
    assert [(s.context(r).bead_scale, s.context(r).bond_scale) for r in range(2)] == list(ss.COMPOSITE_SCALES)
    # the powers are seen: pair and wall forces differ from the default model's by far more than any tolerance; the rest is untouched
    for t in ("pair", "wall"):
        Fs, Fd = s.forces(ss.TERM_BITS[t]), d.forces(ss.TERM_BITS[t])
        assert np.abs(Fs - Fd).max() > 0.05 * np.abs(Fd).max(), t
    for t in ("bond", "bend", "point", "dynamic"):
        assert np.array_equal(s.forces(ss.TERM_BITS[t]), d.forces(ss.TERM_BITS[t])), t
    # both channels and the mixing act: pairs of every kind (AA, BB, AB, uu, Au, Bu) inside the cutoff in each replica
    a, b, _ = ss._types(s.N)
    ss._composite_free_types(a, b)
    for r in range(2):
        pairs = s.search_pairs(ss.PAIR["sigma_b"] * ss.COMPOSITE_SCALES[r][0], replica=r).astype(np.int64)
        kinds = {tuple(sorted([(a[i], b[i]), (a[j], b[j])])) for i, j in pairs}
        assert len(kinds) == 6, kinds
    # the wall's soft inside acts on both channels (beads with a > 0 and with b > 0 inside the surface, under force)
    Fw = np.linalg.norm(s.forces(g.TERM_WALL), axis=-1)
    C = np.sum((x / np.array(ss.SEMI)) ** 2, axis=-1) - 1
    for r in range(2):
        assert ((C[r] < 0) & (Fw[r] > 0)).sum() >= 5 and ((C[r] > 0) & (Fw[r] > 0)).sum() >= 5


@pytest.mark.parametrize("term", ["pair", "wall"])
@pytest.mark.parametrize("powers", ss.RUNTIME_POWERS)
def test_runtime_power_composite_force_is_minus_gradient(oracle, powers, term):
    s = ss.composite(oracle, powers=powers)
    if term == "wall":      # on a sphere, as test_composite_force_is_minus_gradient_per_term
        for r, (bs, os_) in enumerate(ss.COMPOSITE_SCALES):
            s.set_context(r, 0, bs, os_, semiaxes=(ss.SEMI[1],) * 3)
    beads = list(range(ss.N_CHAINS * ss.CHAIN_LEN, ss.N_COMPOSITE)) + [5, 77, 200]
    if powers[3] == 1 and term == "pair":
        # Q = 1: the force jumps at r = sigma_b, and a central difference across the jump is not the derivative -- the probe beads
        # whose B-channel partner sits within 2 h of it are left out (none is expected: asserted to be few)
        x, keep = s.positions(), []
        a, b, _ = ss._types(s.N)
        ss._composite_free_types(a, b)
        for i in beads:
            d = np.linalg.norm(x[:, :, :] - x[:, i:i + 1, :], axis=-1)
            edge = np.stack([np.abs(d[r] - ss.PAIR["sigma_b"] * ss.COMPOSITE_SCALES[r][0]) < 1e-5 for r in range(2)])
            if not edge.any():
                keep.append(i)
        assert len(keep) >= len(beads) - 2
        beads = keep
    _fd_check(s, ss.TERM_BITS[term], beads)


@pytest.mark.parametrize("shape", [(1.0, 1.0, 1.0), (0.8, 1.0, 1.25)])
def test_runtime_power_1kb_images(oracle, shape):
    pw = ss.KB_RUNTIME_POWERS
    base = ss.chromatin_1kb_images(oracle, shifted=False, shape=shape, powers=pw)
    _assert_covered(base, ss.CONFIGURED["1kb_images"])
    assert np.all(_pair_share(base) >= 0.1)
    s, d = ss.chromatin_1kb_images(oracle, shape=shape, powers=pw), ss.chromatin_1kb_images(oracle, shape=shape)
    x = s.positions()
    assert np.array_equal(x, d.positions()) and np.array_equal(x, ss.f32(x)) and np.abs(x[0] - x[1]).max() > 0.05
    Fs, Fd = s.forces(g.TERM_PAIR), d.forces(g.TERM_PAIR)
    assert np.abs(Fs - Fd).max() > 0.05 * np.abs(Fd).max()
    # both channels act, with opposite signs, and pair neighbours straddle the faces (as test_1kb_images_straddle_the_box_faces)
    p = ss.kb_pair(pw)
    for ch, sign in (((p[0], p[1], 0.0, 0.0), 1), ((0.0, 0.0, p[2], p[3]), -1)):
        s.set_pair_softcore(*ch, *pw, mix=False)
        e = s.energy(g.TERM_PAIR)
        assert np.all(sign * e > 0) and np.all(np.abs(s.forces(g.TERM_PAIR)).max(axis=(1, 2)) >= 0.1 * np.abs(Fs).max(axis=(1, 2)))
    s.set_pair_softcore(*p, mix=False)
    L = np.array(s.box)
    for r in range(2):
        nb = s.search_pairs(1.5, replica=r).astype(np.int64)
        assert (np.abs(x[r, nb[:, 0]] - x[r, nb[:, 1]]) > L / 2).any(axis=-1).sum() > 100
    assert np.abs(Fs - base.forces(g.TERM_PAIR)).max() <= 1e-9 * np.abs(Fs).max()


def test_inner_sphere_state_presses_on_both_sides_of_the_core(oracle):
    s, d = ss.inner_sphere(oracle), ss.inner_sphere(oracle, powers=None)
    _assert_covered(s, ss.CONFIGURED["inner_sphere"])
    assert np.all(_pair_share(s) >= 0.3)
    x = s.positions()
    assert np.array_equal(x, ss.f32(x)) and x.shape[0] == 2 and np.abs(x[0] - x[1]).max() > 0.05
    rad = np.linalg.norm(x, axis=-1)
    Fw, Fd = s.forces(g.TERM_WALL), d.forces(g.TERM_WALL)
    reach = ss.INNER["radius"] + 0.5 * max(ss.INNER["sigma"])
    for r in range(2):
        inside, gap = rad[r] < ss.INNER["radius"], (rad[r] > ss.INNER["radius"]) & (rad[r] < reach)
        assert inside.sum() >= 50 and gap.sum() >= 50
        # in the gap the force is the soft cores' (runtime powers: it differs from the default's), pointing outwards
        acted = gap & (np.linalg.norm(Fw[r], axis=-1) > 0)
        assert acted.sum() >= 30 and np.all(np.sum(Fw[r][acted] * x[r][acted], axis=-1) > 0)
        assert np.abs(Fw[r][gap] - Fd[r][gap]).max() > 0.05 * np.abs(Fd[r][gap]).max()
        assert np.array_equal(Fw[r][inside], Fd[r][inside])                          # the harmonic core has no powers
        # ... and it is a sizeable part of the wall term (the outer wall is the other)
        assert np.abs(Fw[r][gap]).max() >= 0.05 * np.abs(Fw[r]).max()
    _fd_check(s, g.TERM_WALL, list(np.nonzero((rad[0] < reach) & (rad[1] < reach))[0][:12]))


@pytest.mark.parametrize("family,n_beads,compress,edge", [("runtime_blob", 1500, 0.7, 0.24), ("runtime_blob", 6000, 0.4, 0.24),
                                                          ("runtime_box", 3000, 0.6, 1.5), ("runtime_box", 6000, 0.4, 1.5)])
def test_dense_runtime_power_families(oracle, family, n_beads, compress, edge):
    """The blobs and boxes test_runtime_pair_gpu.py compresses into the tile classes: every configured term acts, density grows as
    compress^-3, and clear_of_edge leaves no pair where the (12, 1) channel's force jumps, moving a handful of beads by a few 1e-6."""
    make = getattr(ss, family)
    s = make(oracle, n_beads, compress)
    _assert_covered(s, ss.CONFIGURED[family])
    assert np.all(_pair_share(s) >= 0.3)
    x = s.positions()
    assert np.array_equal(x, ss.f32(x)) and x.shape[0] == 2 and np.abs(x[0] - x[1]).max() > 0.05
    loose = make(oracle, n_beads, 2 * compress)
    assert len(s.search_pairs(edge)) > 4 * len(loose.search_pairs(edge))
    grid = ss.GRID if family == "runtime_box" else None
    if grid:
        assert np.array_equal(x, ss.on_grid(x)) and min(s.box) < 8 * edge * 1.75      # a few list radii wide
    y = ss.clear_of_edge(s, edge, grid=grid)
    assert np.array_equal(y, s.positions()) and np.array_equal(y, ss.f32(y))
    moved = np.abs(y - x).max(axis=-1) > 0
    assert moved.sum() <= 40 and np.abs(y - x).max() <= max(16 * ss.EDGE_MARGIN * edge, 2 * (grid or 0))
    for r in range(2):
        n_in, n_out = (len(s.search_pairs(edge * f, replica=r)) for f in (1 - ss.EDGE_MARGIN, 1 + ss.EDGE_MARGIN))
        assert n_in == n_out > 0


def test_spindle_coarse_model_is_the_drivers(oracle):
    """ss.spindle_coarse against what host/gd_spindle.cpp configures: the pair form's energy and forces are those of the (2, 3, 8, 3),
    eps_b = 0 form; at the rods only the pair term and the spindle source act, 40 steps on bonds and bending do as well."""
    s = ss.spindle_coarse(oracle)
    x = s.positions()
    assert 300 <= s.N <= 1000 and np.array_equal(x, ss.f32(x)) and np.abs(x[0] - x[1]).max() > 0.05
    assert ss.idle_terms(s, ("pair", "point")) == [] and sorted(ss.idle_terms(s, ("bond", "bend"))) == ["bend", "bond"]
    F, E = s.forces(g.TERM_PAIR), s.energy(g.TERM_PAIR)
    s.set_pair_softcore(s.cfg["init_bead_repulsion"], s.cfg["init_bead_diameter"], 0.0, 0.0, 2, 3, 8, 3, mix=False)
    assert np.abs(F - s.forces(g.TERM_PAIR)).max() <= 1e-12 * np.abs(F).max() and np.all(np.abs(E - s.energy(g.TERM_PAIR)) <= 1e-12 * E)
    s.begin_phase()
    s.run(40, s.cfg["init_timestep"], s.cfg["init_temperature"], seed=20220101)
    assert ss.idle_terms(s, ("pair", "bond", "bend", "point")) == []


# ------------------------------------------------------------------------------------------------ the wall's axial reaction

@pytest.mark.parametrize("n_beads,bead_scale_init", [(30000, 0.9), (62178, 0.8)])
def test_production_size_initial_states_leave_the_wall_idle(oracle, n_beads, bead_scale_init):
    """Why pressed_genome exists (as test_golden_states_leave_terms_idle for the terms): in the initial states the large device tests
    run from (test_parity_gpu.py: the 944-block wall context test, the many-tiles trajectory, the full-size and split-step
    comparisons) no bead is within the wall's reach, the axial reaction is exactly zero and stays zero over the 12 noisy steps with
    wall dynamics those tests take -- their semiaxes are driven by the spring alone, and their reaction compares 0 with 0."""
    s, info = ss.g_wl().genome_interphase(oracle, n_beads=n_beads, bead_scale_init=bead_scale_init)
    assert np.linalg.norm(s.positions()[0], axis=-1).max() < info["wall_radius"]
    acted, _ = wr.on_the_wall(s)[0]
    assert acted.sum() == 0 and tuple(s.context().axial_reaction) == (0.0, 0.0, 0.0)
    s.begin_phase()
    s.run(12, info["timestep"], info["temperature"], seed=20220101, flags=g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS)
    assert tuple(s.context().axial_reaction) == (0.0, 0.0, 0.0)
    decay = (1 - info["timestep"] * ss.WALL_MOBILITY * ss.WALL_SPRING) ** 12          # the spring alone
    assert np.allclose(np.array(s.context().semiaxes), info["wall_radius"] * decay, rtol=1e-13, atol=0)


# What the pressed genome must reach, per replica, at 33 280 beads; the beads on the wall are a surface layer, so at n beads their number
# goes as (n / 33 280)^(2/3) and the reaction against spring * semiaxes (semiaxes ~ n^(1/3)) as (n / 33 280)^(1/3): the figures for
# 1 500 beads are these, scaled and rounded up
PRESSED_REACH = {33280: dict(on_wall=500, per_side=30, reaction=0.2), 1500: dict(on_wall=64, per_side=4, reaction=0.072)}


@pytest.mark.parametrize("n_beads", list(PRESSED_REACH))
def test_pressed_genome_presses_on_the_wall(oracle, n_beads):
    reach = PRESSED_REACH[n_beads]
    assert reach["on_wall"] >= 500 * (n_beads / 33280) ** (2 / 3) and reach["per_side"] >= 30 * (n_beads / 33280) ** (2 / 3)
    assert reach["reaction"] >= 0.2 * (n_beads / 33280) ** (1 / 3)
    s = ss.pressed_genome(oracle, n_beads, 2)
    x = s.positions()
    assert np.array_equal(x, ss.f32(x)) and np.abs(x[0] - x[1]).max() > 0.05
    react, S, reported = wr.oracle_reaction(s)
    semis = []
    for r, (acted, C) in enumerate(wr.on_the_wall(s)):
        semi = np.array(s.context(r).semiaxes)
        semis.append(semi)
        assert len(set(semi)) == 3                                                   # three unequal semiaxes
        assert (s.context(r).bead_scale, s.context(r).bond_scale) == ss.SCALES[r][:2]
        assert acted.sum() >= reach["on_wall"], (r, acted.sum())
        assert (acted & (C > 0)).sum() >= reach["per_side"] and (acted & (C < 0)).sum() >= reach["per_side"], r
        assert np.all(react[r] >= reach["reaction"] * ss.WALL_SPRING * semi), (r, react[r] / (ss.WALL_SPRING * semi))
        # every bead pushes every semiaxis outwards: the contributions share one sign, |react_k| is its own rounding scale
        assert np.all(np.abs(S[r] - react[r]) <= 1e-12 * react[r]), r
    assert np.all(semis[1] < semis[0])                                               # and a tighter wall for replica 1
    # the wall is a sizeable part of the total force (the coverage rule of every stressed state)
    _assert_covered(s, ss.CONFIGURED["genome"])


def _restated(oracle, state):
    if state == "golden_genome":
        s, *_ = build(oracle, "genome")
        assert len(set(s.context().semiaxes)) == 1                                   # a sphere: the closed form
        x, F = s.positions(), s.forces(g.TERM_WALL)
        return np.array([wr.reaction_on_a_sphere(x[0], F[0])]), np.array([tuple(s.context().axial_reaction)])
    s = ss.composite(oracle) if state == "composite" else ss.pressed_genome(oracle, int(state), 2)
    react, _, reported = wr.oracle_reaction(s)
    return react, reported


@pytest.mark.parametrize("state", ["1500", "33280", "composite", "golden_genome"])
def test_oracle_axial_reaction_equals_its_restatement(oracle, state):
    """The reference the device's reaction is held to, against -sum_i F_wall,ik q_ik / a_k formed in numpy from the oracle's wall forces
    and positions (tests/wall_restatement.py): 1e-12 of the reaction (a sum of up to 1 400 one-signed terms in another order)."""
    react, reported = _restated(oracle, state)
    assert np.all(np.abs(reported) > 0)
    assert np.all(np.abs(react - reported) <= 1e-12 * np.abs(reported)), (react - reported) / reported


# ------------------------------------------------------------------------------------------------ per-term finite differences

def _fd_check(s, mask, beads, h=1e-6):
    x0 = s.positions()
    F = s.forces(mask)
    scale = np.abs(F).max()
    for r in range(s.R):
        for i in beads:
            for k in range(3):
                xp = x0.copy(); xp[r, i, k] += h; s.set_positions(xp); ep = s.energy(mask)[r]
                xm = x0.copy(); xm[r, i, k] -= h; s.set_positions(xm); em = s.energy(mask)[r]
                assert F[r, i, k] == pytest.approx(-(ep - em) / (2 * h), rel=2e-5, abs=1e-6 * scale + 1e-9), (mask, r, i, k)
    s.set_positions(x0)


def _composite_probe_beads():
    beads = set()
    for k in range(ss.N_CHAINS):
        b0, _ = ss._chain_range(k)
        for j in list(ss._SPECIAL_ANGLES) + [2, 3, 6, 7, 12, 13, 46, 47]:         # folded / straight triplets, near-rest bonds, ends
            beads |= {b0 + j, b0 + j + 1, b0 + j + 2} if j + 2 < ss.CHAIN_LEN else {b0 + j}
    beads |= set(range(ss.N_CHAINS * ss.CHAIN_LEN, ss.N_COMPOSITE))                   # wall band and close pairs
    return sorted(b for b in beads if b < ss.N_COMPOSITE)


@pytest.mark.parametrize("term", ss.TERM_NAMES)
def test_composite_force_is_minus_gradient_per_term(oracle, term):
    s = ss.composite(oracle)
    if term == "wall":
        # the wall's force is -grad U only where the second-order nearest-surface construction is exact, on a sphere (the ellipsoid's
        # construction is pinned against the reference's own geometry module: test_wall_distance_matches_the_reference_geometry_module)
        for r, (bs, os_) in enumerate(ss.COMPOSITE_SCALES):
            s.set_context(r, 0, bs, os_, semiaxes=(ss.SEMI[1],) * 3)
        Fw, C = s.forces(g.TERM_WALL), np.sum(s.positions() ** 2, axis=-1) - ss.SEMI[1] ** 2
        assert ((np.abs(Fw).max(-1) > 0) & (C < 0)).sum() >= 5 and ((np.abs(Fw).max(-1) > 0) & (C > 0)).sum() >= 5
    _fd_check(s, ss.TERM_BITS[term], _composite_probe_beads())


@pytest.mark.parametrize("name", list(CASES))
def test_perturbed_force_is_minus_gradient_per_term(oracle, name):
    s = ss.perturbed(oracle, name)
    beads = np.random.default_rng(4).choice(s.N, 16, replace=False)
    for t in ss.CONFIGURED[name]:
        _fd_check(s, ss.TERM_BITS[t], beads)


def test_1kb_images_force_is_minus_gradient_per_term(oracle):
    s = ss.chromatin_1kb_images(oracle, shape=(0.8, 1.0, 1.25))
    loops, glues = ss.kb_pairs(s.N, 5)
    beads = sorted(set(glues[:8].ravel()) | set(loops[:4].ravel()) | set(np.random.default_rng(6).choice(s.N, 8, replace=False)))
    for t in ss.CONFIGURED["1kb_images"]:
        _fd_check(s, ss.TERM_BITS[t], beads)


# ------------------------------------------------------------------------------------------------ the softcore-bond rule

def _glue(**kw):
    return g.System.bond_params(g.POT_SOFTCORE, k_a=-1.0, l_a=0.5, p=8, q=3, **kw)


@pytest.mark.parametrize("flags", [dict(mix=True), dict(scale_by_bond_scale=True), dict(mix=True, scale_by_bond_scale=True)])
def test_softcore_bond_rejects_mix_and_scale(oracle, flags):
    s = g.System(oracle, 4, 1)
    pairs = np.array([[0, 2]], dtype=np.uint32)
    for call in (lambda: s.add_bond_range(_glue(**flags), 0, 4, 1), lambda: s.add_bond_pairs(_glue(**flags), pairs),
                 lambda: s.set_dynamic_pairs(1, _glue(**flags), pairs)):
        with pytest.raises(g.GdynError) as e:
            call()
        assert e.value.code == 1 and "softcore" in str(e.value)
    s.add_bond_range(g.System.bond_params(g.POT_SEMISPRING, k_a=5.0, l_a=0.2, **flags), 0, 4, 1)   # the other kinds keep both flags
    s.add_bond_pairs(_glue(), pairs)
    s.set_dynamic_pairs(1, _glue(minimum_image=True), pairs)


@pytest.mark.parametrize("bond_scale", [1.0, 0.8])
def test_softcore_bond_is_the_documented_formula(oracle, bond_scale):
    """U = k_a (1 - (r/l_a)^p)^q with k_a, l_a as given, at any bond_scale and next to bond sets that do scale."""
    k, l, P, Q = -1.3, 0.5, 8, 3
    for r in (0.1, 0.3, 0.45, 0.499, 0.6):
        s = g.System(oracle, 4, 1)
        s.set_bead_params(a=np.array([1.0, 0.0, 0.5, 1.0]), b=np.array([0.0, 1.0, 0.5, 0.0]))
        s.add_bond_pairs(g.System.bond_params(g.POT_SOFTCORE, k_a=k, l_a=l, p=P, q=Q), np.array([[0, 1]]))
        s.add_bond_pairs(g.System.bond_params(g.POT_SPRING, k_a=3.0, l_a=0.3, k_b=1.0, l_b=0.2, mix=True, scale_by_bond_scale=True),
                         np.array([[2, 3]]))
        s.set_scaling(1.0, 1.0, bond_scale, 1.0)
        s.set_positions(np.array([[0.0, 0, 0], [r, 0, 0], [5.0, 0, 0], [5.0, 0, 0.25]]))
        u = r / l
        e = k * (1 - u ** P) ** Q if u < 1 else 0.0
        f = k * P * Q / l * (1 - u ** P) ** (Q - 1) * u ** (P - 1) if u < 1 else 0.0      # -dU/dr on bead 1
        F = s.forces(g.TERM_BOND)[0]
        Kb, lb = (0.75 * 3.0 + 0.25 * 1.0) / bond_scale ** 2, (0.75 * 0.3 + 0.25 * 0.2) * bond_scale
        assert F[1, 0] == pytest.approx(f, rel=1e-12, abs=1e-14) and F[0, 0] == pytest.approx(-f, rel=1e-12, abs=1e-14)
        assert s.energy(g.TERM_BOND)[0] == pytest.approx(e + 0.5 * Kb * (0.25 - lb) ** 2, rel=1e-12, abs=1e-15)
