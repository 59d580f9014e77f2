"""The glue kinetics on the device (include/gdyn_glue.h, glue.py) against the numpy restatement of the rule
(tests/glue_restatement.py): exact equality of the sets update by update, the sets acting through the per-replica slot, the two analytic
statistics of the process, the uniform selection, determinism, arguments and state.

Exact equality needs no tolerance: every draw and comparison is on integers, and the one floating-point test, d2 < reach^2 in fp32,
is decided the same way on both sides as long as no pair lies within rounding of the boundary -- positions on the 2^-16 grid are exact
in fp32, which leaves the rounding of the sum of squares (2.4e-7 relative); the states here keep every pair 1e-6 away from it, asserted
on the restatement alone.  The statistical bounds are 5 sigma of the process's own distributions (probability 6e-7 of a correct
implementation falling outside; the seeds are fixed, so the outcome is reproducible)."""
import importlib

import numpy as np
import pytest

import glue_restatement as gr
import stressed_states as ss
from util import PKG, g

replica = importlib.import_module(PKG + ".replica")
glue = importlib.import_module(PKG + ".glue")

pytestmark = pytest.mark.gpu
PATHS = {"generic": 1, "tiled": 2}
EINVAL, ESTATE = 1, 5
EMPTY = np.zeros((0, 2), dtype=np.uint32)
REACH, DT = 1.25, 1.0
N_KB, R_KB, SEEDS = 3000, 3, [0x1234567890abcdef, 7, (1 << 64) - 3]
P_ON, P_OFF, MAX_1, MAX_2 = 0.05, 0.3, 400, 20000
N_ST, R_ST = 1200, 8
SEEDS_ST = [1000 + 17 * r for r in range(R_ST)]


def _device(hip, path, n_beads, n_replicas):
    """The 1 kb model across the box faces, its shared slots emptied, per-replica slot 1 = glue"""
    sh = ss.chromatin_1kb_images(hip, shifted=True, n_beads=n_beads, n_replicas=n_replicas)
    sh.set_dynamic_pairs(0, ss.KB_LOOP, EMPTY)
    sh.set_dynamic_pairs(1, ss.KB_GLUE, EMPTY)
    sh.set_tuning(kernel_path=PATHS[path])
    replica.define(sh, 1, ss.KB_GLUE)
    return sh


def _assert_path(s, path):
    assert s.context().list_path == PATHS[path], (s.context().list_path, path)


def _fetch_all(sh):
    return [glue.fetch(sh, r) for r in range(sh.R)]


def _straddles(x32, pairs, box):
    raw = np.abs(x32[pairs[:, 0]].astype(np.float64) - x32[pairs[:, 1]])
    return bool(np.any(raw > np.array(box) / 2))


# ------------------------------------------------------------------------------------------------ 1. exact equality

def moved_positions(x32, bound, box, seed=31):
    """What test 1 sets after the third update: the state re-jittered on the 2^-16 grid; per replica the first bead of five bound pairs
    moved 3 along x (more than REACH from its partner), the second bead of five others shifted by a whole period along y."""
    rng = np.random.default_rng(seed)
    x = ss.on_grid(x32.astype(np.float64) + 0.02 * rng.normal(size=x32.shape))
    for r, B in enumerate(bound):
        assert len(B) >= 10
        x[r, B[:5, 0], 0] += 3.0
        x[r, B[5:10, 1], 1] += box[1]
    return x


def exact_case(x32, box):
    """The restatement's side of test 1 from the initial fp32 positions (R, N, 3): the sets after each of six updates, the positions
    to set after the third, and what happened."""
    R = len(x32)
    rate_on, rate_off = gr.rates(P_ON, P_OFF, DT)
    thr_on, thr_off = gr.thresholds(rate_on, rate_off, DT)
    bound = [EMPTY] * R
    sets, infos, margins, straddle, x_new = [], [], [], False, None
    cand = [gr.candidates(x32[r], box, REACH) for r in range(R)]
    x_cur = x32
    for epoch in range(6):
        max_glues = MAX_1 if epoch < 4 else MAX_2
        out = [gr.update(bound[r], cand[r][0], x_cur[r], box, REACH, max_glues, thr_on, thr_off, epoch, SEEDS[r]) for r in range(R)]
        bound = [o[0] for o in out]
        sets.append(bound); infos.append([o[1] for o in out]); margins.append(min(c[1] for c in cand))
        straddle = straddle or any(_straddles(x_cur[r], bound[r], box) for r in range(R))
        if epoch == 2:
            x_new = moved_positions(x_cur, bound, box)
            x_cur = x_new.astype(np.float32)
            assert np.array_equal(x_cur.astype(np.float64), x_new)      # (on the grid, below 256: exact in fp32)
            cand = [gr.candidates(x_cur[r], box, REACH) for r in range(R)]
    return dict(sets=sets, infos=infos, margins=margins, straddle=straddle, x_new=x_new, rates=(rate_on, rate_off))


def assert_exact_case_preconditions(ref):
    infos = ref["infos"]
    assert min(ref["margins"]) >= 1e-6, ref["margins"]                                  # no pair within rounding of reach
    assert all(i["fired"] > i["free"] for i in infos[0]), infos[0]                      # the selection path, in every replica
    assert any(i["fired"] <= i["free"] for e in (4, 5) for i in infos[e])               # ... and everything binds, after the re-define
    assert sum(i["far"] for e in infos for i in e) >= 1                                 # a pair unbinds by distance
    assert all(i["far"] >= 5 for i in infos[3]), infos[3]                               # (the moved beads' pairs among them)
    assert ref["straddle"]                                                              # a bound pair across a box face, raw coordinates
    assert sum(i["rebound"] for e in infos for i in e) >= 1                             # released and bound again in one update


_exact = {}


def _exact_reference(sh):
    x32 = sh.positions_f32()
    if not _exact:
        _exact.update(exact_case(x32, sh.box), x0=x32)
    assert np.array_equal(_exact["x0"], x32)
    return _exact


@pytest.mark.parametrize("path", list(PATHS))
def test_sets_equal_the_restatement(hip, path):
    sh = _device(hip, path, N_KB, R_KB)
    ref = _exact_reference(sh)
    assert_exact_case_preconditions(ref)
    glue.define(sh, 1, MAX_1, REACH, *ref["rates"])
    for epoch in range(6):
        glue.update(sh, DT, epoch, SEEDS)
        got = _fetch_all(sh)
        for r in range(R_KB):
            want = ref["sets"][epoch][r]
            print(f"  epoch {epoch} r{r}: {len(got[r])} bound (restatement {len(want)}), {ref['infos'][epoch][r]}")
            assert np.array_equal(got[r], want), (epoch, r)
        assert list(glue.counts(sh)) == [len(b) for b in ref["sets"][epoch]]
        if epoch == 2:
            sh.set_positions(ref["x_new"])
            assert np.array_equal(sh.positions_f32(), ref["x_new"].astype(np.float32))
        if epoch == 3:
            glue.define(sh, 1, MAX_2, REACH, *ref["rates"])
    _assert_path(sh, path)


# ------------------------------------------------------------------------------------------------ 2. the lists act

@pytest.mark.parametrize("path", list(PATHS))
def test_the_sets_act_through_the_slot(hip, path):
    sh, twin = _device(hip, path, N_KB, R_KB), _device(hip, path, N_KB, R_KB)
    glue.define(sh, 1, MAX_1, REACH, *gr.rates(P_ON, P_OFF, DT))
    glue.update(sh, DT, 0, SEEDS)
    sets = _fetch_all(sh)
    assert all(len(b) == MAX_1 for b in sets)
    for r, b in enumerate(sets):
        replica.set_pairs(twin, 1, r, b)
    assert [replica.count(sh, 1, r) for r in range(R_KB)] == list(glue.counts(sh)) == [replica.count(twin, 1, r) for r in range(R_KB)]
    assert np.abs(sh.forces(g.TERM_DYNAMIC)).max() > 0
    for terms in (g.TERM_DYNAMIC, g.TERM_ALL):
        assert np.array_equal(sh.forces(terms), twin.forces(terms))
        assert np.array_equal(sh.energy(terms), twin.energy(terms))
    for s in (sh, twin):
        s.run(20, 1e-4, 1.0, seed=999, replica_seeds=[11, 12, 13])
    assert np.array_equal(sh.positions(), twin.positions())
    _assert_path(sh, path)
    _assert_path(twin, path)


# ------------------------------------------------------------------------------------------------ 3. / 4. the process

_frozen = {}


def _frozen_candidates(sh):
    """The candidates of the frozen 1200-bead state, per replica (restatement, once)"""
    x32 = sh.positions_f32()
    if not _frozen:
        _frozen.update(x=x32, cand=[gr.candidates(x32[r], sh.box, REACH)[0] for r in range(R_ST)])
    assert np.array_equal(_frozen["x"], x32)
    return _frozen["cand"]


def _keys(pairs):
    return (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1]


def test_stationary_occupancy_and_epoch_dependence(hip):
    p_on, p_off = 0.2, 0.3
    sh = _device(hip, "tiled", N_ST, R_ST)
    total = sum(len(c) for c in _frozen_candidates(sh))
    glue.define(sh, 1, 1 << 30, REACH, *gr.rates(p_on, p_off, DT))
    for epoch in range(40):
        glue.update(sh, DT, epoch, SEEDS_ST)
    s40 = _fetch_all(sh)
    glue.update(sh, DT, 40, SEEDS_ST)
    s41 = _fetch_all(sh)
    n40 = sum(len(b) for b in s40)
    both = sum(int(np.isin(_keys(a), _keys(b)).sum()) for a, b in zip(s40, s41))
    (m1, s1), (m2, s2) = gr.stationary(p_on, p_off, total)
    print(f"  candidates {total} ({total / (N_ST * R_ST):.2f} a bead): bound {n40} (mean {m1:.1f}, sigma {s1:.1f}), "
          f"at both epochs {both} (mean {m2:.1f}, sigma {s2:.1f})")
    assert abs(n40 - m1) <= 5 * s1, (n40, m1, s1)
    assert abs(both - m2) <= 5 * s2, (both, m2, s2)


def test_uniform_selection(hip):
    sh = _device(hip, "tiled", N_ST, R_ST)
    cand = _frozen_candidates(sh)
    n = min(len(c) for c in cand) // 4
    glue.define(sh, 1, n, REACH, *gr.rates(1.0, 0.0, DT))
    got = mean = var = 0.0
    for epoch in range(8):
        for r in range(R_ST):
            glue.set_pairs(sh, r, EMPTY)
        glue.update(sh, DT, epoch, SEEDS_ST)
        for r, b in enumerate(_fetch_all(sh)):
            half = cand[r][: len(cand[r]) // 2]
            assert len(b) == n and np.isin(_keys(b), _keys(cand[r])).all()
            got += int(np.isin(_keys(b), _keys(half)).sum())
            m, v = gr.hypergeometric(len(cand[r]), len(half), n)
            mean += m; var += v
    print(f"  selected in the first half: {got:.0f}, mean {mean:.1f}, sigma {var ** 0.5:.1f}")
    assert abs(got - mean) <= 5 * var ** 0.5, (got, mean, var ** 0.5)


# ------------------------------------------------------------------------------------------------ 5. determinism

def test_determinism_across_handles_and_paths(hip):
    def sequence(path):
        sh = _device(hip, path, N_ST, R_ST)
        glue.define(sh, 1, 300, REACH, *gr.rates(0.1, 0.3, DT))
        out = []
        for epoch in range(4):
            glue.update(sh, DT, epoch, SEEDS_ST)
            out.append(_fetch_all(sh))
        _assert_path(sh, path)
        return out
    a, b, c = sequence("tiled"), sequence("tiled"), sequence("generic")
    assert any(len(s) == 300 for s in a[-1]) and a[0][0].tolist() != a[0][1].tolist()
    for other in (b, c):
        for ea, eo in zip(a, other):
            for sa, so in zip(ea, eo):
                assert np.array_equal(sa, so)


# ------------------------------------------------------------------------------------------------ 6. arguments and state

def test_arguments_and_state(hip):
    dll = glue.load_glue_library()
    assert dll.gd_glue_abi_version() == glue.GLUE_ABI_VERSION
    sh = _device(hip, "tiled", N_ST, 2)
    rates = gr.rates(0.2, 0.3, DT)
    seeds = [5, 6]

    def code(call):
        with pytest.raises(g.GdynError) as e:
            call()
        return e.value.code

    # before gd_glue_define; a slot that was never declared
    assert code(lambda: glue.update(sh, DT, 0, seeds)) == ESTATE
    assert code(lambda: glue.set_pairs(sh, 0, EMPTY)) == ESTATE
    assert code(lambda: glue.fetch(sh, 0)) == ESTATE
    assert code(lambda: glue.counts(sh)) == ESTATE
    assert code(lambda: glue.define(sh, 2, 100, REACH, *rates)) == ESTATE
    assert code(lambda: glue.define(sh, 4, 100, REACH, *rates)) == EINVAL
    replica.set_pairs(sh, 1, 0, np.array([[0, 3]], np.uint32))           # (not managed yet: accepted as before)
    glue.define(sh, 1, 100, REACH, *rates)
    assert list(glue.counts(sh)) == [0, 0] and replica.count(sh, 1, 0) == 0      # the slot holds the sets from here on
    glue.update(sh, DT, 0, seeds)
    glue.set_pairs(sh, 1, np.array([[9, 2], [0, 5], [3, 2]], np.uint32))
    assert glue.fetch(sh, 1).tolist() == [[0, 5], [2, 3], [2, 9]]        # normalised and sorted
    before = _fetch_all(sh)
    F0 = sh.forces(g.TERM_DYNAMIC)
    assert len(before[0]) > 10 and np.abs(F0[0]).max() > 0
    replica.define(sh, 2, ss.KB_LOOP)
    inf, nan = float("inf"), float("nan")
    one = np.array([[0, 1]], dtype=np.uint32)
    n = glue.C.c_uint32()
    seeds_a = np.array(seeds, dtype=np.uint64)
    bad = [
        (EINVAL, lambda: dll.gd_glue_define(None, 1, None)),
        (EINVAL, lambda: dll.gd_glue_define(sh._h, 1, None)),
        (EINVAL, lambda: dll.gd_glue_update(None, DT, 0, seeds_a.ctypes.data)),
        (EINVAL, lambda: dll.gd_glue_update(sh._h, DT, 0, None)),
        (EINVAL, lambda: dll.gd_glue_set(sh._h, 0, None, 1)),
        (EINVAL, lambda: dll.gd_glue_fetch(sh._h, 0, None, 0, None)),
        (EINVAL, lambda: dll.gd_glue_fetch(sh._h, 0, None, 1, glue.C.byref(n))),
        (EINVAL, lambda: dll.gd_glue_counts(sh._h, None)),
        (ESTATE, lambda: code(lambda: glue.define(sh, 2, 100, REACH, *rates))),                  # one glue slot per handle
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, len(before[0]) - 1, REACH, *rates))),   # below a current set size
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, 0.0, *rates))),
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, -1.0, *rates))),
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, nan, *rates))),
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, REACH, -1.0, 1.0))),
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, REACH, 1.0, -1.0))),
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, REACH, inf, 1.0))),
        (EINVAL, lambda: code(lambda: glue.define(sh, 1, 100, REACH, 1.0, nan))),
        (EINVAL, lambda: code(lambda: glue.update(sh, 0.0, 1, seeds))),
        (EINVAL, lambda: code(lambda: glue.update(sh, -1.0, 1, seeds))),
        (EINVAL, lambda: code(lambda: glue.update(sh, nan, 1, seeds))),
        (EINVAL, lambda: code(lambda: glue.set_pairs(sh, 2, one))),                              # replica >= R
        (EINVAL, lambda: code(lambda: glue.set_pairs(sh, 0, np.array([[0, 1], [1, 0]], np.uint32)))),      # listed twice
        (EINVAL, lambda: code(lambda: glue.set_pairs(sh, 0, np.array([[0, 1], [7, 7]], np.uint32)))),
        (EINVAL, lambda: code(lambda: glue.set_pairs(sh, 0, np.array([[0, 1], [5, N_ST]], np.uint32)))),
        (EINVAL, lambda: code(lambda: glue.set_pairs(sh, 0, np.stack([np.arange(101), np.arange(101) + 1], axis=1)))),      # n > max_glues
        (EINVAL, lambda: code(lambda: glue.fetch(sh, 2))),
        (ESTATE, lambda: code(lambda: replica.set_pairs(sh, 1, 0, one))),                        # the managed slot
    ]
    for k, (want, call) in enumerate(bad):
        assert call() == want, k
        now = _fetch_all(sh)
        assert all(np.array_equal(a, b) for a, b in zip(now, before)), k
        assert np.array_equal(sh.forces(g.TERM_DYNAMIC), F0), k
    # the count-then-fetch idiom with a short buffer
    few = np.zeros((2, 2), np.uint32)
    assert dll.gd_glue_fetch(sh._h, 0, few.ctypes.data, 2, glue.C.byref(n)) == 0
    assert n.value == len(before[0]) and np.array_equal(few, before[0][:2])
    # define again: the sets are kept, the new parameters hold (no binding, certain release: the next update empties every set)
    glue.define(sh, 1, 100, REACH, 0.0, 1000.0)
    assert all(np.array_equal(a, b) for a, b in zip(_fetch_all(sh), before))
    glue.update(sh, DT, 1, seeds)
    assert list(glue.counts(sh)) == [0, 0] and np.all(sh.forces(g.TERM_DYNAMIC) == 0)
    replica.set_pairs(sh, 2, 0, one)                                     # another slot of the same handle: as before
    assert replica.count(sh, 2, 0) == 1
    sh.close()
    # a handle that never defines glues takes gd_replica_pairs_set on every slot as before
    s2 = _device(hip, "tiled", N_ST, 2)
    replica.set_pairs(s2, 1, 1, one)
    assert replica.count(s2, 1, 1) == 1
    assert code(lambda: glue.counts(s2)) == ESTATE                       # (nothing carried over)
    s2.close()
