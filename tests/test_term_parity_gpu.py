"""Device against oracle, force term by force term, each on its own scale, at the stressed states of tests/stressed_states.py.

test_parity_gpu.py compares every term on the scale of the TOTAL force, at the golden states; there several terms do not act, and a
term that is 1e-3 of the total can be 2 % wrong unseen.  Here each term t is held to the DESIGN.md section 2 tolerances on its own
scale, per replica r, at states where every term acts (tests/test_stressed_states.py asserts that on the CPU):

    forces    |F_t(dev) - F_t(oracle)|_r  <=  5e-5 * max|F_t(oracle)|_r
    energies  |E_t(dev) - E_t(oracle)|_r  <=  2e-6 * S_t,r

S_t is |E_t| for a term whose contributions share one sign.  For a term with parts of opposite sign -- the 1 kb pair term (repulsive A
channel, attractive B channel) and the dynamic term of the 1 kb and composite models (positive spring loops in slot 0, negative-energy
glue in slot 1) -- S_t is the sum of the magnitudes of its one-signed parts, each evaluated on the oracle alone: a sum of cancelling
parts carries the rounding of the parts, not of their difference.

Both kernel paths (generic global-gather lists, LDS-tiled lists) run every comparison, and the test asserts which one ran.

The workloads all set the soft-core powers (2, 3, 8, 3), which the kernels specialise; the states named *_runtime, composite_P_Q_P_Q,
spindle_driver and inner_sphere carry other powers (pair term, ellipsoid wall, inner wall) and run the runtime-power forms."""
import numpy as np
import pytest

import stressed_states as ss
from util import ENERGY_RTOL, FORCE_RTOL, g

pytestmark = pytest.mark.gpu
PATHS = {"generic": 1, "tiled": 2}


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


# name -> (builder(lib), the terms it configures, {term: [modifiers that leave one one-signed part]} for the mixed-sign terms)
def _pair_channel(a, powers=None):
    def mod(s):
        p = ss.kb_pair(powers)
        s.set_pair_softcore(*((p[0], p[1], 0.0, 0.0) if a else (0.0, 0.0, p[2], p[3])), *p[4:], mix=False)
    return mod


def _only_slot(keep):
    return lambda s: s.set_dynamic_pairs(1 - keep, ss.KB_LOOP, np.zeros((0, 2), dtype=np.uint32))


KB_PARTS = {"pair": [_pair_channel(True), _pair_channel(False)], "dynamic": [_only_slot(0), _only_slot(1)]}
KB_RT = ss.KB_RUNTIME_POWERS
KB_PARTS_RT = {"pair": [_pair_channel(True, KB_RT), _pair_channel(False, KB_RT)], "dynamic": KB_PARTS["dynamic"]}
COMPOSITE_PARTS = {"dynamic": [_only_slot(0), _only_slot(1)]}


def _powers_id(powers):
    return "_".join(str(k) for k in powers)


STATES = {
    "genome": (lambda lib: ss.perturbed(lib, "genome"), ss.CONFIGURED["genome"], {}),
    "genome_30k": (lambda lib: ss.perturbed(lib, "genome", seed=8, n_beads=30000), ss.CONFIGURED["genome"], {}),
    "spindle": (lambda lib: ss.perturbed(lib, "spindle"), ss.CONFIGURED["spindle"], {}),
    "ab_box": (lambda lib: ss.perturbed(lib, "ab_box"), ss.CONFIGURED["ab_box"], {}),
    "chromatin_1kb": (lambda lib: ss.perturbed(lib, "chromatin_1kb"), ss.CONFIGURED["chromatin_1kb"], KB_PARTS),
    "composite": (ss.composite, ss.TERM_NAMES, COMPOSITE_PARTS),
    "1kb_images": (lambda lib: ss.chromatin_1kb_images(lib), ss.CONFIGURED["1kb_images"], KB_PARTS),
    "1kb_images_aniso": (lambda lib: ss.chromatin_1kb_images(lib, shape=(0.8, 1.0, 1.25)), ss.CONFIGURED["1kb_images"], KB_PARTS),
    # the runtime-power pair form (and runtime wall powers): tests/stressed_states.py, asserted in tests/test_stressed_states.py
    "spindle_driver": (ss.spindle_driver, ss.CONFIGURED["spindle_driver"], {}),
    "1kb_images_runtime": (lambda lib: ss.chromatin_1kb_images(lib, powers=KB_RT), ss.CONFIGURED["1kb_images"], KB_PARTS_RT),
    "1kb_images_aniso_runtime": (lambda lib: ss.chromatin_1kb_images(lib, shape=(0.8, 1.0, 1.25), powers=KB_RT), ss.CONFIGURED["1kb_images"],
                                 KB_PARTS_RT),
    "inner_sphere": (ss.inner_sphere, ss.CONFIGURED["inner_sphere"], {}),
}
for _pw in ss.RUNTIME_POWERS:
    STATES["composite_" + _powers_id(_pw)] = (lambda lib, pw=_pw: ss.composite(lib, powers=pw), ss.TERM_NAMES, COMPOSITE_PARTS)


def _energy_scale(oracle, make, term, parts):
    """S_t per replica (module docstring)"""
    if term not in parts:
        return np.abs(make(oracle).energy(ss.TERM_BITS[term]))
    S = 0.0
    for mod in parts[term]:
        s = make(oracle)
        mod(s)
        S = S + np.abs(s.energy(ss.TERM_BITS[term]))
    return S


def _energy_floor(so, term):
    """The one absolute floor, for the wall energy.  A bead's wall energy is U(delta), delta its distance to the surface, which the
    device forms in fp32 from coordinates of size |x_i|: delta carries a rounding error of order 2^-24 |x_i| however small it is, and
    E_wall one of up to sum_i |F_wall,i| 2^-24 |x_i| (the oracle's forces and positions).  It matters where few beads press on a large
    wall: in genome_30k (|x| ~ 6.2, E_wall 2.8 in replica 1) the device is 2.8e-6 of E_wall off, above the relative bound and at 5 % of
    this floor (1.7e-4); on the smaller walls of genome and composite the floor is 1e-6 to 3e-6 of E_wall.  No other term gets one: the
    bending of mutant M5 (1e-3 of E_bend) stays held to 2e-6 of E_bend."""
    if term != "wall":
        return 0.0
    x, F = so.positions(), so.forces(g.TERM_WALL)
    return np.sum(np.linalg.norm(F, axis=-1) * np.linalg.norm(x, axis=-1), axis=1) * 2.0 ** -24


def _compare_forces(Fh, Fo, what):
    for r in range(Fo.shape[0]):
        scale = np.abs(Fo[r]).max()
        err = np.abs(Fh[r] - Fo[r]).max()
        assert scale > 0 and err <= FORCE_RTOL * scale, (what, r, err / scale)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("state", list(STATES))
def test_every_term_on_its_own_scale(hip, oracle, state, path):
    make, terms, parts = STATES[state]
    sh, so = make(hip), make(oracle)
    sh.set_tuning(kernel_path=PATHS[path])
    for t in terms:
        m = ss.TERM_BITS[t]
        _compare_forces(sh.forces(m), so.forces(m), (state, t))
        eh, eo = sh.energy(m), so.energy(m)
        S = _energy_scale(oracle, make, t, parts)
        assert np.all(np.abs(eh - eo) <= ENERGY_RTOL * S + _energy_floor(so, t)), (state, t, (eh - eo) / S)
    _compare_forces(sh.forces(), so.forces(), (state, "all"))
    _assert_path(sh, path)


# (powers, path): the default model keeps the ids it had; the runtime-power models are named by their powers
MASK_CASES = [(None, p) for p in PATHS] + [(pw, p) for pw in ss.RUNTIME_POWERS for p in PATHS]
MASK_IDS = [p if pw is None else f"{_powers_id(pw)}-{p}" for pw, p in MASK_CASES]


@pytest.mark.parametrize("powers,path", MASK_CASES, ids=MASK_IDS)
def test_every_term_mask_on_the_composite_model(hip, oracle, powers, path):
    """All 63 masks: the per-bond-type term bits (static bonds vs dynamic pairs in one adjacency) and every section's skip logic."""
    sh, so = ss.composite(hip, powers=powers), ss.composite(oracle, powers=powers)
    sh.set_tuning(kernel_path=PATHS[path])
    for m in range(1, 64):
        _compare_forces(sh.forces(m), so.forces(m), m)
    _assert_path(sh, path)


# the kernel path is a property of the pair list: for the other terms in isolation there is no pair term, so no list whose tiles the
# bonded, bending, point and wall sections could share -- a path has no meaning for them, they run once with the library's choice
# and the path is not asserted
STEP_CASES = [("pair", "generic", None), ("pair", "tiled", None)] + [(t, None, None) for t in ss.TERM_NAMES if t != "pair"]
# ... and the terms the runtime powers reach, with them: the pair term on both paths, the wall
STEP_CASES += [c for pw in ss.RUNTIME_POWERS for c in (("pair", "generic", pw), ("pair", "tiled", pw), ("wall", None, pw))]
STEP_IDS = [f"{t}-{p}" + ("" if pw is None else "-" + _powers_id(pw)) for t, p, pw in STEP_CASES]


@pytest.mark.parametrize("term,path,powers", STEP_CASES, ids=STEP_IDS)
def test_step_mode_per_term(hip, oracle, term, path, powers):
    """k_step in STEP mode (what trajectories run) against the oracle's F_t: one zero-noise, T = 0, compensated step of a term-isolated
    copy of the composite model with non-uniform mobility and no scale or wall update; (x1 - x0) / (mu dt) is the force the step used."""
    m = ss.TERM_BITS[term]
    sh, so = ss.composite(hip, terms=m, powers=powers), ss.composite(oracle, terms=m, powers=powers)
    if path:
        sh.set_tuning(kernel_path=PATHS[path])
    x0 = so.positions()
    Fo = so.forces(m)
    assert np.array_equal(Fo, so.forces(g.TERM_ALL))                     # the isolated copy configures this term alone
    mu = np.array(ss.MOBILITY)[np.arange(sh.N) % 3][None, :, None]
    dt = 1e-5
    sh.run(1, dt, 0.0, noise=g.NOISE_ZERO, flags=g.RUN_COMPENSATED)
    assert sh.context().compensated == 1 and sh.context().step == 1
    _compare_forces((sh.positions() - x0) / (mu * dt), Fo, term)
    if path:
        _assert_path(sh, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_spindle_driver_form_against_the_specialised_kernels(hip, path):
    """The spindle driver's pair form, (2, 3, 2, 3) with eps_b = sigma_b = 0, runs the runtime-power pair kernels; (2, 3, 8, 3) with
    eps_b = 0 is the same function of the positions (1e-12 on the oracle: tests/test_stressed_states.py) and runs the specialised ones.
    Two kernels, one function: forces (evaluated, and as one compensated zero-noise step used them) and energies agree."""
    out = []
    for specialised in (False, True):
        s = ss.spindle_driver(hip, specialised=specialised)
        s.set_tuning(kernel_path=PATHS[path])
        F, E, x0 = s.forces(g.TERM_PAIR), s.energy(g.TERM_PAIR), s.positions()
        assert np.isfinite(F).all() and np.isfinite(E).all() and np.isfinite(s.forces()).all()
        _assert_path(s, path)
        t = ss.spindle_driver(hip, specialised=specialised)
        t.set_tuning(kernel_path=PATHS[path])
        dt = 1e-5
        t.run(1, dt, 0.0, noise=g.NOISE_ZERO, flags=g.RUN_COMPENSATED)
        assert t.context().compensated == 1 and t.context().step == 1
        _assert_path(t, path)
        out.append((F, E, (t.positions() - x0) / dt, s.forces()))
    (F, E, Fstep, Fall), (Fs, Es, Fstep_s, Fall_s) = out
    _compare_forces(F, Fs, "pair")
    _compare_forces(Fstep, Fstep_s, "step")
    _compare_forces(Fstep, Fall_s, "step vs forces")
    assert np.all(np.abs(E - Es) <= ENERGY_RTOL * np.abs(Es)), (E - Es) / Es


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", [(1.0, 1.0, 1.0), (0.8, 1.0, 1.25)])
def test_periodic_images_leave_pair_and_glue_forces_unchanged(hip, oracle, shape, path):
    """Beads shifted by whole periods: the pair term and the minimum-image glue see the same forces; the loop springs, not
    minimum-imaged, are dropped here (their forces do change, and are compared with the oracle's in test_every_term_on_its_own_scale)."""
    out = {}
    for shifted in (False, True):
        s = ss.chromatin_1kb_images(hip, shifted=shifted, shape=shape)
        _only_slot(1)(s)
        s.set_tuning(kernel_path=PATHS[path])
        out[shifted] = (s.forces(g.TERM_PAIR), s.forces(g.TERM_DYNAMIC))
        _assert_path(s, path)
    for k, what in enumerate(("pair", "glue")):
        _compare_forces(out[True][k], out[False][k], what)
    so = ss.chromatin_1kb_images(oracle, shifted=True, shape=shape)
    _only_slot(1)(so)
    _compare_forces(out[True][1], so.forces(g.TERM_DYNAMIC), "glue vs oracle")


def test_point_source_limits(hip, oracle):
    """At most four point sources on both libraries; a SPRING-kind source (accepted by both) against the oracle, inside and outside
    its rest radius."""
    for lib in (hip, oracle):
        s = g.System(lib, 8, 1)
        for k in range(4):
            s.add_point_source(g.POT_HARMONIC, 1.0, 0.0, (0.0, 0.0, float(k)))
        with pytest.raises(g.GdynError) as e:
            s.add_point_source(g.POT_SPRING, 1.0, 0.5, (0.0, 0.0, 0.0))
        assert e.value.code == 1
    n = 400
    rng = np.random.default_rng(3)
    u = rng.normal(size=(2, n, 3))
    x = ss.f32(u / np.linalg.norm(u, axis=-1, keepdims=True) * rng.uniform(0.05, 1.5, size=(2, n, 1)) + np.array([0.1, -0.2, 0.3]))
    out = []
    for lib in (hip, oracle):
        s = g.System(lib, n, 2)
        s.add_point_source(g.POT_SPRING, 7.0, 0.75, (0.1, -0.2, 0.3), targets=np.arange(0, n, 2))
        s.set_positions(x)
        out.append((s.forces(), s.energy()))
    d = np.linalg.norm(x - np.array([0.1, -0.2, 0.3]), axis=-1)[:, ::2]
    assert (d < 0.7).sum() > 50 and (d > 0.8).sum() > 50
    _compare_forces(out[0][0], out[1][0], "spring source")
    assert np.all(np.abs(out[0][1] - out[1][1]) <= ENERGY_RTOL * np.abs(out[1][1]))
    assert np.all(out[1][0][:, 1::2] == 0)                                 # beads off the target list feel nothing


def test_softcore_bond_rule_on_the_device(hip):
    """include/gdyn.h: mix / scale_by_bond_scale on a softcore bond are GD_EINVAL at all three entry points (as on the oracle,
    tests/test_stressed_states.py)."""
    s = g.System(hip, 4, 1)
    pairs = np.array([[0, 2]], dtype=np.uint32)
    for flags in (dict(mix=True), dict(scale_by_bond_scale=True)):
        p = g.System.bond_params(g.POT_SOFTCORE, k_a=-1.0, l_a=0.5, p=8, q=3, **flags)
        for call in (lambda: s.add_bond_range(p, 0, 4, 1), lambda: s.add_bond_pairs(p, pairs), lambda: s.set_dynamic_pairs(1, p, pairs)):
            with pytest.raises(g.GdynError) as e:
                call()
            assert e.value.code == 1


@pytest.mark.parametrize("path", list(PATHS))
def test_softcore_bonds_next_to_scaled_bond_sets(hip, oracle, path):
    """Softcore bonds (unmixed, unscaled: the accepted form) in a model whose every other bond set scales with bond_scale, at
    bond_scale != 1 in both replicas: the uniform "every bond set scales" shortcut of the kernels must not take the softcore bonds in."""
    n = 600
    rng = np.random.default_rng(12)
    a, b, _ = ss._types(n)
    steps = rng.normal(size=(2, n, 3))
    steps *= (0.2 * rng.uniform(0.7, 1.3, size=(2, n, 1))) / np.linalg.norm(steps, axis=-1, keepdims=True)
    x = ss.f32(np.cumsum(steps, axis=1) * 0.6)
    sc = np.array([[0, 2], [1, 3]]) + np.arange(0, n - 4, 3)[:, None, None]
    sc = sc.reshape(-1, 2).astype(np.uint32)
    glue = (np.arange(0, n - 4, 5)[:, None] + np.array([0, 4])).astype(np.uint32)
    out = []
    for lib in (hip, oracle):
        s = g.System(lib, n, 2)
        s.set_bead_params(a=a, b=b)
        s.set_pair_softcore(1.0, 0.25, 1.0, 0.2, 2, 3, 8, 3, mix=True)
        s.add_bond_range(g.System.bond_params(g.POT_SEMISPRING, k_a=30.0, l_a=0.2, k_b=20.0, l_b=0.2, mix=True, scale_by_bond_scale=True), 0, n)
        s.add_bond_range(g.System.bond_params(g.POT_HARMONIC, k_a=2.0, scale_by_bond_scale=True), 0, n, 2)
        s.add_bond_pairs(g.System.bond_params(g.POT_SOFTCORE, k_a=6.0, l_a=0.45, p=2, q=2), sc)
        s.set_dynamic_pairs(1, g.System.bond_params(g.POT_SOFTCORE, k_a=-4.0, l_a=0.6, p=8, q=3), glue)
        s.set_scaling(0.8, 1.0, 0.8, 1.0)
        s.set_positions(x)
        s.set_context(0, 0, 0.9, 0.75)
        s.set_context(1, 0, 0.9, 0.85)
        if lib is hip:
            s.set_tuning(kernel_path=PATHS[path])
        out.append([s.forces(m) for m in (g.TERM_BOND, g.TERM_DYNAMIC)] + [s.energy(g.TERM_BOND), s.energy(g.TERM_DYNAMIC)])
        if lib is hip:
            _assert_path(s, path)
    # the softcore bonds are a sizeable part of the bond term (an error in them is visible on its scale)
    so = g.System(oracle, n, 2)
    so.add_bond_pairs(g.System.bond_params(g.POT_SOFTCORE, k_a=6.0, l_a=0.45, p=2, q=2), sc)
    so.set_positions(x)
    assert np.all(np.abs(so.forces()).max(axis=(1, 2)) >= 0.1 * np.abs(out[1][0]).max(axis=(1, 2)))
    for k, what in enumerate(("bond", "glue")):
        _compare_forces(out[0][k], out[1][k], what)
        assert np.all(np.abs(out[0][2 + k] - out[1][2 + k]) <= ENERGY_RTOL * np.abs(out[1][2 + k])), what
