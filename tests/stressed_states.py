"""Stressed states: deterministic models at which every configured force term acts (a helper module of the suite).

The golden states (tests/golden/golden_small.npz) are the workloads' initial states, and in them several terms do not act: the spindle
rods are straight with every bond at its rest length, the 1 kb springs sit at theirs.  A per-term comparison there sees nothing.  The
builders here return configured :class:`System` handles for any library (hip or oracle) at states where each term is a sizeable part of
the total and the branches kernels get wrong are reached:

  perturbed(lib, name)   a util.CASES workload, R = 2, every replica jittered differently (and its scales set per replica)
  pressed_genome(lib, n_beads, n_replicas)
                         the perturbed genome inside a tighter wall with three unequal semiaxes per replica: hundreds of beads on the
                         wall, on both sides of the surface, and an axial reaction of the size of spring * semiaxes
  composite(lib)         an open-box model with all six terms (pair, bond, bend, point, wall, dynamic), R = 2; with `powers` the
                         pair term takes runtime soft-core powers (the kernels' runtime-power pair form) and the wall WALL_POWERS
  spindle_driver(lib)    perturbed(lib, "spindle") with the pair form as host/gd_spindle.cpp sets it: (2, 3, 2, 3), eps_b = sigma_b = 0
  inner_sphere(lib)      the excluded-core model of test_parity_gpu.py::test_inner_sphere_wall_matches_oracle, runtime inner-wall powers
  isolated_pairs(lib, form)
                         one handle of two-bead systems at known separations, for the closed-form soft-core answers of every (P, Q)
  runtime_blob(lib, n_beads, compress), runtime_box(lib, n_beads, compress)
                         dense blobs of chains (open) and the compressed 1 kb model (periodic) with runtime pair powers: local density,
                         and with it the tile class of the LDS-tiled lists, set by `compress`; clear_of_edge() conditions such a state
  spindle_coarse(lib)    the coarse model host/gd_spindle.cpp builds, through the Python API
  chromatin_1kb_images(lib, shifted, shape, powers)
                         the 1 kb force field with beads shifted by whole periods, so that pair neighbours and glue pairs straddle
                         the box faces in raw coordinates (and unflagged chain bonds become long: they must NOT be minimum-imaged);
                         also in a box with three different periods

Positions are fp32-exact, so the device and the fp64 oracle start from the same coordinates and the comparison measures force
arithmetic, not input rounding.  composite() takes `terms`, a term mask: only those terms are configured (the step-mode tests need
term-isolated copies).  tests/test_stressed_states.py asserts on the oracle that the states reach what they are built for.
"""
import numpy as np

from util import build, g

P = g.System.bond_params
ALL = g.TERM_ALL
TERM_NAMES = ("pair", "bond", "bend", "point", "wall", "dynamic")
TERM_BITS = dict(pair=g.TERM_PAIR, bond=g.TERM_BOND, bend=g.TERM_BEND, point=g.TERM_POINT, wall=g.TERM_WALL, dynamic=g.TERM_DYNAMIC)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the four workloads, perturbed

JITTER = 0.03
# genome, per replica: (bead_scale, bond_scale, wall semiaxes as a fraction of the initial ones -- a slightly tighter wall, so that
# at every size the jittered beads press on it from both sides); the other workloads keep their context
SCALES = ((0.83, 0.86, 0.99), (0.94, 0.9, 0.995))


def perturbed(lib, name, n_replicas=2, seed=7, **over):
    """util.CASES[name] (builder arguments `over` changed) with a Gaussian jitter of 0.03 on the initial positions, a different one per
    replica; genome replicas also get their own bead_scale, bond_scale and wall semiaxes through set_context."""
    s, *_ = build(lib, name, n_replicas=n_replicas, **over)
    x = s.positions()
    rng = np.random.default_rng(seed)
    x = f32(x + JITTER * rng.normal(size=x.shape))
    s.set_positions(x)
    if name == "genome":
        s.initial_semiaxes = [tuple(s.context(r).semiaxes) for r in range(n_replicas)]
        for r in range(n_replicas):
            bs, os_, w = SCALES[r % len(SCALES)]
            s.set_context(r, 0, bs, os_, semiaxes=[w * a for a in s.initial_semiaxes[r]])
    return s


# the pressed genome: replica r's semiaxes as fractions of the workload's initial radius -- unequal, and tight enough that hundreds
# of beads press on the wall from both sides and the axial reaction is a sizeable part of spring * semiaxes (the wall ODE's other term)
PRESSED = (0.985, 0.975, 0.965)
PRESSED_STEP = 0.003
WALL_SPRING, WALL_MOBILITY = 1.0e4, 1.0e-4       # workloads.genome_interphase and composite(): semiaxes_spring (each axis), mobility


def pressed_genome(lib, n_beads=1500, n_replicas=2, seed=7):
    """perturbed(lib, "genome") at `n_beads`, the wall of replica r set to PRESSED * (1 - PRESSED_STEP r) times the initial radius
    (the per-replica scales of SCALES kept): the state at which the wall's axial reaction and semiaxis ODE are compared."""
    s = perturbed(lib, "genome", n_replicas=n_replicas, seed=seed, n_beads=n_beads)
    for r in range(n_replicas):
        bs, os_, _ = SCALES[r % len(SCALES)]
        s.set_context(r, 0, bs, os_, semiaxes=[f * (1.0 - PRESSED_STEP * r) * a for f, a in zip(PRESSED, s.initial_semiaxes[r])])
    return s


def nudged(x, seed):
    """x (fp32-exact) with every coordinate moved by one fp32 ulp, up or down at random: the smallest change of the input a device that
    holds fp32 coordinates can see."""
    x32 = np.asarray(x).astype(np.float32)
    up = np.random.default_rng(seed).random(x32.shape) < 0.5
    return np.where(up, np.nextafter(x32, np.float32(np.inf)), np.nextafter(x32, np.float32(-np.inf))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the composite model

SEMI = (1.5, 1.3, 1.15)           # ellipsoid semiaxes
WALL_SIGMA = (0.3, 0.24)
PACKING = 400.0
PAIR = dict(eps_a=2.0, sigma_a=0.3, eps_b=2.0, sigma_b=0.24, p_a=2, q_a=3, p_b=8, q_b=3)
CHAIN_LEN, N_CHAINS, N_FREE = 48, 6, 48
N_COMPOSITE = CHAIN_LEN * N_CHAINS + N_FREE
BOND_L = 0.2                      # rest length of the semispring and spring chain bonds (unscaled)
SPRING_SRC_B, SEMI_SRC_B = 0.6, 0.9
COMPOSITE_SCALES = ((0.82, 0.88), (0.95, 1.07))      # (bead_scale, bond_scale) of replicas 0 and 1
MOBILITY = (0.5, 1.0, 1.75)
# chain k occupies beads [k L, (k+1) L)
SEMISPRING_CHAINS = (0, 1, 4, 5)
SPRING_CHAINS = (2, 3)


def _chain_range(k):
    return k * CHAIN_LEN, (k + 1) * CHAIN_LEN


def _types(n):
    """(a, b) factors of the three bead types A (1, 0), B (0, 1), u (.5, .5), in runs of 4 (fp16-exact: the tiled path holds them)."""
    t = (np.arange(n) // 4) % 3
    a = np.choose(t, [1.0, 0.0, 0.5])
    b = np.choose(t, [0.0, 1.0, 0.5])
    return a, b, t


def _inside(p, frac):
    return float(np.sum((p / (frac * np.array(SEMI))) ** 2)) < 1.0


def _perp(d, rng):
    v = rng.normal(size=3)
    v -= v.dot(d) * d
    return v / np.linalg.norm(v)


# bond lengths of the chain bonds, as multiples of the rest length: both sides, some within 1 % of it
_LEN_FACTORS = (0.6, 1.35, 0.995, 1.004, 0.8, 1.2, 0.9991, 1.008, 0.7, 1.45)
# bending angles (rad) placed at fixed positions of every chain: under 1e-3 and over 3.1, with unequal bond lengths around them
_SPECIAL_ANGLES = {6: 4e-4, 13: 3.13, 21: 8e-4, 30: 3.115, 38: 1.6}


def _chain(rng, start):
    x = np.empty((CHAIN_LEN, 3))
    x[0] = start
    d = _perp(np.array([0.0, 0.0, 1.0]), rng)
    for k in range(1, CHAIN_LEN):
        length = BOND_L * _LEN_FACTORS[k % len(_LEN_FACTORS)]
        if (k - 1) in _SPECIAL_ANGLES:      # angle between bond k-1 (x[k-1]-x[k-2]) and bond k (x[k]-x[k-1])
            th = _SPECIAL_ANGLES[k - 1]
            for _ in range(40):             # the turn's plane is free: one that stays inside the wall
                nd = np.cos(th) * d + np.sin(th) * _perp(d, rng)
                if _inside(x[k - 1] + length * nd, 0.9):
                    break
            d = nd
        else:
            for _ in range(40):             # a random turn that keeps the chain well inside the wall
                nd = rng.normal(size=3)
                nd /= np.linalg.norm(nd)
                if _inside(x[k - 1] + length * nd, 0.78):
                    break
            else:                           # none did: back towards the centre
                nd = -x[k - 1] / np.linalg.norm(x[k - 1])
            d = nd
        d /= np.linalg.norm(d)
        x[k] = x[k - 1] + length * d
    return x


def _surface_point(u):
    return u / np.sqrt(np.sum((u / np.array(SEMI)) ** 2))


def composite_positions(seed, replica):
    rng = np.random.default_rng(seed + 101 * replica)
    x = np.empty((N_COMPOSITE, 3))
    for k in range(N_CHAINS):
        c = rng.normal(size=3)
        c = 0.35 * np.array(SEMI) * c / np.linalg.norm(c)
        b0, b1 = _chain_range(k)
        x[b0:b1] = _chain(rng, c)
    free = np.arange(N_CHAINS * CHAIN_LEN, N_COMPOSITE)
    # 24 free beads in the wall's band: inside (depth up to ~0.12, the soft wall acts within 0.15 x bead_scale) and outside (up to 0.02)
    depths = np.concatenate([np.linspace(-0.12, -0.004, 16), np.linspace(0.002, 0.02, 8)])
    for i, dep in zip(free[:24], depths):
        u = rng.normal(size=3)
        q = _surface_point(u)
        x[i] = q + dep * q / np.linalg.norm(q)
    # 24 free beads in close pairs: coincident, 1e-4, 1e-3, ... apart; the pairs' types cycle through AA, BB, AB, uu, Au, Bu
    seps = (0.0, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.15, 0.2, 0.22, 0.235, 0.25, 0.28)
    for p, sep in enumerate(seps):
        i, j = free[24 + 2 * p], free[25 + 2 * p]
        c = 0.5 * np.array(SEMI) * rng.uniform(-1, 1, size=3)
        d = rng.normal(size=3)
        x[i] = c
        x[j] = c + sep * d / np.linalg.norm(d)
    return x


def _composite_free_types(a, b):
    """Pair beads: (A, A), (B, B), (A, B), (u, u), (A, u), (B, u) in turn."""
    kinds = [((1, 0), (1, 0)), ((0, 1), (0, 1)), ((1, 0), (0, 1)), ((.5, .5), (.5, .5)), ((1, 0), (.5, .5)), ((0, 1), (.5, .5))]
    free = np.arange(N_CHAINS * CHAIN_LEN, N_COMPOSITE)
    for p in range(12):
        (ai, bi), (aj, bj) = kinds[p % len(kinds)]
        i, j = free[24 + 2 * p], free[25 + 2 * p]
        a[i], b[i], a[j], b[j] = ai, bi, aj, bj


# bond parameter sets of the composite model
HARMONIC_MIXED = P(g.POT_HARMONIC, k_a=6.0, k_b=3.0, mix=True, scale_by_bond_scale=True)
SEMISPRING_MIXED = P(g.POT_SEMISPRING, k_a=70.0, l_a=BOND_L, k_b=45.0, l_b=BOND_L, mix=True)
SPRING = P(g.POT_SPRING, k_a=60.0, l_a=BOND_L)
SOFTCORE_BOND = P(g.POT_SOFTCORE, k_a=1.5, l_a=0.45, p=2, q=2)
LOOP = P(g.POT_SPRING, k_a=8.0, l_a=0.3, k_b=4.0, l_b=0.4, mix=True, scale_by_bond_scale=True)
GLUE = P(g.POT_SOFTCORE, k_a=-1.0, l_a=0.55, p=8, q=3)
POINT_SOURCES = (   # kind, K, b, point, targets ('chain k' or None = every bead)
    (g.POT_HARMONIC, 4.0, 0.0, (0.1, -0.2, 0.05), 0),
    (g.POT_SEMISPRING, 6.0, SEMI_SRC_B, (0.0, 0.0, 0.0), None),
    (g.POT_SPRING, 5.0, SPRING_SRC_B, (-0.3, 0.2, 0.1), 2),
    (g.POT_SPRING, 3.0, 0.8, (0.25, 0.3, -0.2), 5),
)


def source_targets(spec):
    if spec is None:
        return None
    b0, b1 = _chain_range(spec)
    return np.arange(b0, b1, dtype=np.uint32)


def loop_pairs():
    """slot 0: (i, i+5) within the first three chains"""
    out = []
    for k in range(3):
        b0, b1 = _chain_range(k)
        out += [(i, i + 5) for i in range(b0, b1 - 5, 3)]
    return np.array(out, dtype=np.uint32)


def glue_pairs():
    """slot 1: (i, i+3) within the last three chains (close in space along a chain, so most of them act)"""
    out = []
    for k in range(3, N_CHAINS):
        b0, b1 = _chain_range(k)
        out += [(i, i + 3) for i in range(b0, b1 - 3, 2)]
    return np.array(out, dtype=np.uint32)


def softcore_bond_pairs():
    out = []
    for k in (4, 5):
        b0, b1 = _chain_range(k)
        out += [(i, i + 2) for i in range(b0, b1 - 2)]
    return np.array(out, dtype=np.uint32)


RUNTIME_POWERS = ((4, 2, 12, 1), (6, 4, 2, 3))      # (p_a, q_a, p_b, q_b) of the runtime-power composite models
WALL_POWERS = (4, 2, 6, 4)                          # ... and the powers of their ellipsoid wall


def composite(lib, terms=ALL, seed=11, n_replicas=2, powers=None):
    """Open-box model in which all six terms act at once (only the terms in `terms` are configured).  powers = (p_a, q_a, p_b, q_b):
    the pair term with these soft-core powers instead of (2, 3, 8, 3) -- the runtime-power pair form of the kernels, still mixed,
    scaled and with fp16-exact factors, so the tiled path stays available -- and the wall with WALL_POWERS instead of the default.

    pair:    AB soft-core (p 2/8, q 3), mixed, scaled with bead_scale
    bond:    mixed and scaled harmonic (i, i+2) bonds, mixed semispring chains, spring chains, unmixed softcore (i, i+2) bonds
    bend:    constant-energy and per-bead bending, overlapping on chains 1 and 3
    point:   HARMONIC, SEMISPRING (every bead), two SPRING sources with target lists
    wall:    the ellipsoid wall (soft inside, harmonic outside)
    dynamic: slot 0 mixed, scaled spring loops; slot 1 softcore glue
    R = 2 replicas with their own positions and (bead_scale, bond_scale); non-uniform mobility."""
    n = N_COMPOSITE
    s = g.System(lib, n, n_replicas)
    a, b, t = _types(n)
    _composite_free_types(a, b)
    mob = np.array(MOBILITY)[np.arange(n) % 3]
    bend_e = 0.5 + (np.arange(n) % 5) * 0.25
    s.set_bead_params(a=a, b=b, mobility=mob, bending_energy=bend_e)
    if terms & g.TERM_PAIR:
        pair = dict(PAIR) if powers is None else dict(PAIR, **dict(zip(("p_a", "q_a", "p_b", "q_b"), powers)))
        s.set_pair_softcore(**pair, mix=True, scale_by_bead_scale=True)
    if terms & g.TERM_BOND:
        for k in SEMISPRING_CHAINS:
            s.add_bond_range(SEMISPRING_MIXED, *_chain_range(k), 1)
        for k in SPRING_CHAINS:
            s.add_bond_range(SPRING, *_chain_range(k), 1)
        for k in (0, 1, 2):
            s.add_bond_range(HARMONIC_MIXED, *_chain_range(k), 2)
        s.add_bond_pairs(SOFTCORE_BOND, softcore_bond_pairs())
    if terms & g.TERM_BEND:
        s.add_bending_range(*_chain_range(0), 1.2, per_bead=False)
        c1 = _chain_range(1)
        s.add_bending_range(c1[0], c1[1], 0.9, per_bead=False)
        s.add_bending_range(c1[0] + 20, c1[1], 0.0, per_bead=True)          # overlaps the constant range of chain 1
        c3 = _chain_range(3)
        s.add_bending_range(c3[0], c3[1], 0.0, per_bead=True)
        s.add_bending_range(c3[0], c3[0] + 30, 0.7, per_bead=False)         # and again on chain 3
        s.add_bending_range(*_chain_range(4), 1.0, per_bead=False)
    if terms & g.TERM_POINT:
        for kind, K, bb, pt, tg in POINT_SOURCES:
            s.add_point_source(kind, K, bb, pt, targets=source_targets(tg))
    if terms & g.TERM_WALL:
        wp = {} if powers is None else dict(zip(("p_a", "q_a", "p_b", "q_b"), WALL_POWERS))
        s.set_ellipsoid_wall(2.0, WALL_SIGMA[0], 2.0, WALL_SIGMA[1], wall_a_factor=1.0, wall_b_factor=1.0, packing_spring=PACKING,
                             semiaxes_spring=(1e4,) * 3, mobility=1e-4, init_semiaxes=SEMI, **wp)
    if terms & g.TERM_DYNAMIC:
        s.set_dynamic_pairs(0, LOOP, loop_pairs())
        s.set_dynamic_pairs(1, GLUE, glue_pairs())
    s.set_scaling(0.8, 1.0, 0.8, 1.0)
    s.set_positions(f32(np.stack([composite_positions(seed, r) for r in range(n_replicas)])))
    for r in range(n_replicas):
        bs, os_ = COMPOSITE_SCALES[r % len(COMPOSITE_SCALES)]
        s.set_context(r, 0, bs, os_)
    return s


# ------------------------------------------------------------------------------------------------ 1 kb across the box faces

GRID = 2.0 ** -16       # coordinates and periods on this grid: x + k L is exact in fp32 and fp64 alike while |x + k L| < 2^7


def on_grid(x):
    return np.round(np.asarray(x, dtype=np.float64) / GRID) * GRID


def chromatin_1kb_images(lib, shifted=True, shape=(1.0, 1.0, 1.0), n_beads=3000, n_replicas=2, seed=5, frac=0.3, powers=None):
    """The 1 kb force field of workloads.chromatin_1kb (repulsion + attraction, spring chain, per-bead bending, spring loops in dynamic
    slot 0, minimum-image softcore glue in slot 1) with the jittered random walk of its initial state, in a box of periods
    shape x L (L the workload's period, put on the 2^-16 grid).  shifted=True moves `frac` of the beads by whole periods per axis
    (+-L), after the rounding: pair neighbours and glue pairs then straddle the box faces in raw coordinates, and so do chain bonds and
    loops, which are NOT minimum-imaged (simulation.cpp:126-140: only the glue is) and so become long.  powers = (p_a, q_a, p_b, q_b)
    replaces the pair term's (2, 3, 8, 3): the runtime-power pair form, unmixed, with the attractive B channel."""
    s0, info = g_wl().chromatin_1kb(lib, n_beads=n_beads, n_replicas=1, n_loops=30, n_glues=60)
    x0 = s0.positions()[0]
    s0.close()
    box = tuple(float(on_grid(info["box"] * f)) for f in shape)
    s = g.System(lib, n_beads, n_replicas, box=box)
    s.set_bead_params(mobility=np.ones(n_beads), bending_energy=np.full(n_beads, 1.0))
    s.set_pair_softcore(*kb_pair(powers), mix=False)
    s.add_bond_range(P(g.POT_SPRING, k_a=100.0, l_a=1.0), 0, n_beads, 1)
    s.add_bending_range(0, n_beads, 0.0, per_bead=True)
    loops, glues = kb_pairs(n_beads, seed)
    s.set_dynamic_pairs(0, KB_LOOP, loops)
    s.set_dynamic_pairs(1, KB_GLUE, glues)
    rng = np.random.default_rng(seed)
    x = on_grid(x0[None] + JITTER * rng.normal(size=(n_replicas, n_beads, 3)))
    if shifted:
        sel = rng.random((n_replicas, n_beads)) < frac
        k = rng.integers(-1, 2, size=(n_replicas, n_beads, 3))
        k[~sel] = 0
        x = x + k * np.array(box)
    s.set_positions(x)
    s.box = box
    return s


KB_PAIR = (2.0, 1.0, -0.2, 1.5, 2, 3, 8, 3)          # (eps_a, sigma_a, eps_b, sigma_b, p_a, q_a, p_b, q_b) of chromatin_1kb
KB_RUNTIME_POWERS = (2, 1, 8, 4)
KB_LOOP = P(g.POT_SPRING, k_a=10.0, l_a=1.0)
KB_GLUE = P(g.POT_SOFTCORE, k_a=-1.0, l_a=1.5, p=8, q=3, minimum_image=True)


def kb_pair(powers=None):
    """KB_PAIR with its powers replaced"""
    return KB_PAIR if powers is None else KB_PAIR[:4] + tuple(powers)


def kb_pairs(n_beads, seed):
    """30 loops (i, i + 20..200) and 60 glues (j, j+3), as workloads.chromatin_1kb draws them"""
    rng = np.random.default_rng(seed + 17)
    i = rng.integers(0, n_beads - 200, size=30)
    loops = np.stack([i, i + rng.integers(20, 200, size=30)], axis=1).astype(np.uint32)
    j = rng.integers(0, n_beads - 4, size=60)
    return loops, np.stack([j, j + 3], axis=1).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ the spindle driver's pair form

SPINDLE_PAIR = (5.0, 0.2)         # workloads.spindle: init_bead_repulsion, init_bead_diameter


def spindle_driver(lib, specialised=False, **kw):
    """perturbed(lib, "spindle") with the pair form exactly as host/gd_spindle.cpp:80-83 sets it: (eps, sigma, 0, 0, 2, 3, 2, 3), unmixed
    -- an unused B channel with sigma_b = 0 and runtime powers, where workloads.spindle writes (2, 3, 8, 3).  specialised=True: the
    (2, 3, 8, 3), eps_b = 0 form of the same state -- the same function of the positions, evaluated by the specialised kernels."""
    s = perturbed(lib, "spindle", **kw)
    s.set_pair_softcore(*SPINDLE_PAIR, 0.0, 0.0, 2, 3, *((8, 3) if specialised else (2, 3)), mix=False)
    return s


# ------------------------------------------------------------------------------------------------ the excluded core

INNER = dict(radius=0.6, eps=3.0, sigma=(0.30, 0.24), spring=40.0, outer=1.7, fill=1.6)
INNER_POWERS = (6, 4, 4, 2)


def inner_sphere(lib, powers=INNER_POWERS, n_beads=3000, n_replicas=2, seed=11):
    """The model of test_parity_gpu.py::test_inner_sphere_wall_matches_oracle at its size (3 000 A or B beads uniform in a ball of
    radius 1.6 around an excluded core of radius 0.6, inside a fixed spherical wall of radius 1.7), every replica drawn on its own, the
    inner wall's soft cores with the runtime powers `powers` (None: the default (2, 3, 8, 3))."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n_replicas, n_beads, 3))
    x *= (rng.random((n_replicas, n_beads)) ** (1 / 3) * INNER["fill"] / np.linalg.norm(x, axis=-1))[..., None]
    a = (rng.random(n_beads) < 0.5).astype(float)
    s = g.System(lib, n_beads, n_replicas)
    s.set_bead_params(a=a, b=1.0 - a, mobility=np.ones(n_beads))
    s.set_pair_softcore(2.0, 0.30, 2.0, 0.24, 2, 3, 8, 3, mix=True)
    s.set_ellipsoid_wall(4.0, 0.30, 4.0, 0.24, 0.0, 1.0, 50.0, (0.0,) * 3, 0.0, (INNER["outer"],) * 3, scale_by_bead_scale=False)
    pw = {} if powers is None else dict(zip(("p_a", "q_a", "p_b", "q_b"), powers))
    s.set_inner_sphere_wall(INNER["radius"], INNER["eps"], INNER["sigma"][0], INNER["eps"], INNER["sigma"][1], 0.0, 1.0, INNER["spring"], **pw)
    s.set_positions(f32(x))
    return s


# ------------------------------------------------------------------------------------------------ isolated pairs: known answers

FORMS = tuple((p, q) for p in (2, 4, 6, 8, 12) for q in (1, 2, 3, 4))      # what valid_pq admits
# separations of the pairs as multiples of sigma_a: coincident, tiny, inside, just inside, on the edge, the next fp32 above it, outside
# (0.9 and 0.999 rounded to fp32, so that u sigma_a is a position fp32 holds)
U_GRID = tuple(float(np.float32(u)) for u in (0.0, 2.0 ** -10, 0.25, 0.5, 0.9, 0.999, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 1.5))
PAIR_KINDS = (((1, 0), (1, 0)), ((0, 1), (0, 1)), ((1, 0), (0, 1)), ((.5, .5), (.5, .5)), ((1, 0), (.5, .5)), ((0, 1), (.5, .5)))
# channel A carries the form under test at sigma_a = 2^-2 (u sigma_a is then exact in fp32 for every fp32 u); channel B a second
# form at sigma_b = 5/16: it reaches further than A, so A's edge u = 1 lies inside the pair cutoff, and B's own edge (u = 1.25) is
# not on the grid
ISO = dict(eps_a=2.5, sigma_a=0.25, eps_b=1.5, sigma_b=0.3125)
ISO_SPACING = 1.0                 # lattice spacing of the pairs: beyond any list radius (cutoff 0.3125; lists reach under twice that)


def second_form(form):
    """The form of channel B next to `form` in channel A: twelve places on in FORMS, so that (2, 3) meets (8, 3) -- that one handle is
    the specialised pair form, the other nineteen are runtime-power forms -- and every form serves once as the second."""
    return FORMS[(FORMS.index(tuple(form)) + 12) % len(FORMS)]


def isolated_pairs_layout():
    """(x (N, 3) fp32-exact, a, b, pairs (n, 2), u (n,), axis (n,)): one pair per (u, kind), bead 2k at a lattice point and bead 2k+1
    u sigma_a further along axis k % 3; the lattice point's coordinate on that axis is 0, so both positions are exact in fp32."""
    combos = [(u, kind) for u in U_GRID for kind in PAIR_KINDS]
    n = len(combos)
    x, a, b = np.zeros((2 * n, 3)), np.zeros(2 * n), np.zeros(2 * n)
    side = int(np.ceil(np.sqrt(n)))
    for k, (u, ((ai, bi), (aj, bj))) in enumerate(combos):
        ax = k % 3
        others = [c for c in range(3) if c != ax]
        x[2 * k, others] = x[2 * k + 1, others] = ISO_SPACING * (1 + k % side), ISO_SPACING * (1 + k // side)
        x[2 * k + 1, ax] = u * ISO["sigma_a"]
        a[2 * k], b[2 * k], a[2 * k + 1], b[2 * k + 1] = ai, bi, aj, bj
    assert np.array_equal(x, f32(x))
    pairs = np.arange(2 * n).reshape(n, 2)
    return x, a, b, pairs, np.array([u for u, _ in combos]), np.arange(n) % 3


def isolated_pairs(lib, form):
    """One handle (R = 1) of the isolated pairs: `form` in channel A, second_form(form) in channel B, mixed, non-uniform mobility."""
    x, a, b, *_ = isolated_pairs_layout()
    s = g.System(lib, len(x), 1)
    s.set_bead_params(a=a, b=b, mobility=np.array(MOBILITY)[np.arange(len(x)) % 3])
    s.set_pair_softcore(ISO["eps_a"], ISO["sigma_a"], ISO["eps_b"], ISO["sigma_b"], *form, *second_form(form), mix=True)
    s.set_positions(x[None])
    return s


def softcore_closed_form(eps, sigma, P, Q, r):
    """(U, -dU/dr) of U = eps (1 - (r/sigma)^P)^Q for r < sigma, 0 beyond, in numpy fp64 (tests/test_oracle_kat.py:61-62)."""
    u = np.asarray(r, dtype=np.float64) / sigma
    inside = u < 1
    ui = np.where(inside, u, 0.0)
    e = np.where(inside, eps * (1 - ui ** P) ** Q, 0.0)
    f = np.where(inside, eps * P * Q / sigma * (1 - ui ** P) ** (Q - 1) * ui ** (P - 1), 0.0)
    return e, f


def isolated_pairs_reference(form):
    """(F (N, 3), e (n,) per pair) of isolated_pairs(lib, form) from the closed form with the mixing weights (a_i + a_j) / 2, (b_i + b_j) / 2."""
    x, a, b, pairs, _, axis = isolated_pairs_layout()
    i, j = pairs[:, 0], pairs[:, 1]
    r = np.linalg.norm(x[j] - x[i], axis=-1)
    wa, wb = 0.5 * (a[i] + a[j]), 0.5 * (b[i] + b[j])
    ea, fa = softcore_closed_form(ISO["eps_a"], ISO["sigma_a"], *form, r)
    eb, fb = softcore_closed_form(ISO["eps_b"], ISO["sigma_b"], *second_form(form), r)
    f = wa * fa + wb * fb                                   # bead j is pushed along +axis, bead i along -axis
    F = np.zeros_like(x)
    F[j, axis] = f
    F[i, axis] = -f
    return F, wa * ea + wb * eb


# ------------------------------------------------------------------------------------------------ dense blobs: the tile classes

BLOB_POWERS = (4, 2, 12, 1)
BLOB_BOND = P(g.POT_SPRING, k_a=600.0, l_a=0.25)     # (the walks' bonds are 0.2 x compress long: compressed at every member of the family)


def runtime_blob(lib, n_beads, compress, powers=BLOB_POWERS, n_replicas=2, seed=3):
    """A uniform blob of chains (the genome workload's confined random walks, one draw per replica) scaled by `compress` about the
    origin: local density, and with it the size of the list tiles, grows as compress^-3 at a fixed bead count.  Mixed pair term with
    the runtime powers `powers` on the three fp16-exact types, spring chains, non-uniform mobility; open box."""
    wl = g_wl()
    lens = wl.chain_lengths(n_beads)
    radius = 0.27 * (n_beads / (8 * 0.30)) ** (1 / 3)
    x = np.stack([wl.confined_random_walks(lens, radius, 0.2, np.random.default_rng(seed + r)) for r in range(n_replicas)])
    s = g.System(lib, n_beads, n_replicas)
    a, b, _ = _types(n_beads)
    s.set_bead_params(a=a, b=b, mobility=np.array(MOBILITY)[np.arange(n_beads) % 3])
    s.set_pair_softcore(2.0, 0.30, 2.0, 0.24, *powers, mix=True)
    st = 0
    for n in lens:
        s.add_bond_range(BLOB_BOND, st, st + int(n), 1)
        st += int(n)
    s.set_positions(f32(x * compress))
    return s


def runtime_box(lib, n_beads, compress, powers=BLOB_POWERS, n_replicas=2, seed=5):
    """The periodic counterpart: the 1 kb force field (chromatin_1kb_images, unshifted) with positions and periods scaled by
    `compress`, pair term with the runtime powers `powers` and the attractive B channel, unmixed.  At compress well below 1 the box
    is a few list radii wide and a block's tile wraps around it."""
    s0 = chromatin_1kb_images(lib, shifted=False, n_beads=n_beads, n_replicas=n_replicas, seed=seed, powers=powers)
    box = tuple(float(on_grid(L * compress)) for L in s0.box)
    x = on_grid(s0.positions() * compress)
    s0.close()
    s = g.System(lib, n_beads, n_replicas, box=box)
    s.set_bead_params(mobility=np.ones(n_beads), bending_energy=np.full(n_beads, 1.0))
    s.set_pair_softcore(*kb_pair(powers), mix=False)
    s.add_bond_range(P(g.POT_SPRING, k_a=100.0, l_a=1.0), 0, n_beads, 1)
    s.add_bending_range(0, n_beads, 0.0, per_bead=True)
    loops, glues = kb_pairs(n_beads, seed)
    s.set_dynamic_pairs(0, KB_LOOP, loops)
    s.set_dynamic_pairs(1, KB_GLUE, glues)
    s.set_positions(x)
    s.box = box
    return s


EDGE_MARGIN = 2.0 ** -19


def clear_of_edge(so, sigma, margin=EDGE_MARGIN, grid=None):
    """Positions of the ORACLE handle `so` (left set on it) with no pair within margin x sigma of the separation sigma.

    A soft core with Q = 1 has a force that jumps at r = sigma (by eps P / sigma), and fp32 r^2 / sigma^2 may fall on either side of 1
    for a pair within a few 1e-7 sigma of it: there a device-oracle difference measures the conditioning of the state, not the
    kernel.  One bead of every such pair is moved along the pair's axis by 8 margin sigma (at least one step of `grid`), the
    result rounded to fp32 (to `grid`), until no pair is left in the band.  A function of the positions and the oracle's pair search
    alone."""
    x = so.positions()
    box = getattr(so, "box", None)
    step = max(8 * margin * sigma, grid or 0.0)
    for _ in range(10):
        found = 0
        for r in range(so.R):
            hi, lo = (so.search_pairs(sigma * f, replica=r).astype(np.int64) for f in (1 + margin, 1 - margin))
            code = lambda p: np.minimum(p[:, 0], p[:, 1]) * so.N + np.maximum(p[:, 0], p[:, 1])
            band = np.setdiff1d(code(hi), code(lo))
            found += len(band)
            for i, j in zip(band // so.N, band % so.N):
                d = x[r, j] - x[r, i]
                if box is not None:
                    d -= np.array(box) * np.rint(d / np.array(box))
                x[r, j] += step * d / np.linalg.norm(d)
        if not found:
            return x
        x = f32(x) if grid is None else on_grid(x)
        so.set_positions(x)
    raise AssertionError("pairs left on the edge")


# ------------------------------------------------------------------------------------------------ the spindle driver's coarse model

SPINDLE_COARSE = dict(n_fine=1500, coarse=2, init_bend_energy=1.0, init_start_stddev=0.5)


def spindle_coarse(lib, n_replicas=2, seed=2024):
    """The coarse model host/gd_spindle.cpp builds (setup_chains, setup_system, add_spindle_forcefield, run_initialization) through
    the Python API: the workloads' chain lengths at 1 500 fine beads coarse-grained by 2, default bead factors, uniform mobility,
    the pair form (eps, sigma, 0, 0, 2, 3, 2, 3) unmixed, semispring chains with bending, the harmonic spindle source on the three
    beads around every centromere, randomly directed straight rods around init_start_point -- one draw per replica."""
    wl = g_wl()
    cfg = dict(wl.DEFAULT_CONFIG)
    cfg.update({k: v for k, v in SPINDLE_COARSE.items() if k.startswith("init_")})
    chains, start = [], 0
    for n in wl.chain_lengths(SPINDLE_COARSE["n_fine"]):
        size = (int(n) + SPINDLE_COARSE["coarse"] - 1) // SPINDLE_COARSE["coarse"]
        chains.append((start, start + size, start + (int(n) // 2) // SPINDLE_COARSE["coarse"]))
        start += size
    n = start
    s = g.System(lib, n, n_replicas)
    s.set_bead_params(mobility=np.full(n, cfg["init_mobility"]))
    s.set_pair_softcore(cfg["init_bead_repulsion"], cfg["init_bead_diameter"], 0.0, 0.0, 2, 3, 2, 3, mix=False)
    bond = P(g.POT_SEMISPRING, k_a=cfg["init_bond_spring"], l_a=cfg["init_bond_length"])
    for c0, c1, _ in chains:
        s.add_bond_range(bond, c0, c1, 1)
        s.add_bending_range(c0, c1, cfg["init_bend_energy"])
    s.add_point_source(g.POT_HARMONIC, cfg["init_spindle_spring"], 0.0, cfg["init_spindle_point"],
                       targets=[c + d for (_, _, c) in chains for d in (-1, 0, 1)])
    x = np.empty((n_replicas, n, 3))
    for r in range(n_replicas):
        rng = np.random.default_rng(seed + r)
        for c0, c1, _ in chains:
            centroid = np.array(cfg["init_start_point"]) + cfg["init_start_stddev"] * rng.normal(size=3)
            d = rng.normal(size=3)
            d *= cfg["init_bond_length"] / np.linalg.norm(d)
            x[r, c0:c1] = centroid - d * (c1 - c0) / 2 + np.arange(c1 - c0)[:, None] * d
    s.set_positions(f32(x))
    s.cfg = cfg
    return s


# ------------------------------------------------------------------------------------------------ what the states reach

# the terms each builder configures
CONFIGURED = {"genome": ("pair", "bond", "wall"), "spindle": ("pair", "bond", "bend", "point"), "ab_box": ("pair", "bond"),
              "chromatin_1kb": ("pair", "bond", "bend", "dynamic"), "composite": TERM_NAMES, "1kb_images": ("pair", "bond", "bend", "dynamic"),
              "spindle_driver": ("pair", "bond", "bend", "point"), "inner_sphere": ("pair", "wall"), "runtime_blob": ("pair", "bond"),
              "runtime_box": ("pair", "bond", "bend", "dynamic")}
COVERAGE = 1e-2      # every configured term: max|F_t| >= COVERAGE * max|F_all|, in every replica


def term_ratios(s):
    """{term: (R,) max|F_t| / max|F_all| per replica}"""
    Fa = np.abs(s.forces()).max(axis=(1, 2))
    return {t: np.abs(s.forces(TERM_BITS[t])).max(axis=(1, 2)) / Fa for t in TERM_NAMES}


def idle_terms(s, configured):
    """The configured terms that fall below the coverage bound in some replica."""
    rat = term_ratios(s)
    return sorted(t for t in configured if not np.all(rat[t] >= COVERAGE))


def separations(x, pairs, box=None):
    d = x[:, pairs[:, 0]] - x[:, pairs[:, 1]]
    if box is not None:
        d -= np.array(box) * np.rint(d / np.array(box))
    return np.linalg.norm(d, axis=-1)


def chain_bonds(ranges, stride=1):
    return np.array([(i, i + stride) for b0, b1 in ranges for i in range(b0, b1 - stride)], dtype=np.int64)


def bend_geometry(x, first):
    """angle (rad) and the two bond lengths of the triplets (i, i+1, i+2), i in `first`; x is (R, N, 3)"""
    first = np.asarray(first)
    d1 = x[:, first + 1] - x[:, first]
    d2 = x[:, first + 2] - x[:, first + 1]
    l1, l2 = np.linalg.norm(d1, axis=-1), np.linalg.norm(d2, axis=-1)
    cs = np.clip(np.sum(d1 * d2, axis=-1) / (l1 * l2), -1.0, 1.0)
    return np.arccos(cs), l1, l2


def composite_triplets():
    """first beads of the triplets the composite model's bending ranges configure (overlaps counted once)"""
    first = set()
    for k in (0, 1, 3, 4):
        b0, b1 = _chain_range(k)
        first |= set(range(b0, b1 - 2))
    return np.array(sorted(first))


def g_wl():
    import importlib
    return importlib.import_module(g.__name__ + ".workloads")
