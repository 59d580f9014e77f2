"""A handle with every feature's buffers alive when it is destroyed, built twice (csrc/gdyn_system.hpp: the droplet term, the
per-replica pair upload, the glue kinetics, the search cache and the contact tables each own their device and pinned blocks, and
gd_destroy only waits and deletes).  Each owned block is released once and allocated afresh, so the second handle computes what the
first did: equal handles are deterministic, hence equality bit for bit and no tolerance."""
import importlib

import numpy as np
import pytest

from util import PKG, g

replica = importlib.import_module(PKG + ".replica")
glue = importlib.import_module(PKG + ".glue")

pytestmark = pytest.mark.gpu
N, R = 300, 2


def _model():
    """Two random walks of 300 steps of 0.25 (open box), 40 droplet targets, ten per-replica pairs a replica"""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(R, N, 3))
    x = np.cumsum(0.25 * d / np.linalg.norm(d, axis=-1, keepdims=True), axis=1)
    targets = np.sort(rng.choice(N, size=40, replace=False))
    pairs = []
    for _ in range(R):
        i = rng.choice(N - 20, size=10, replace=False)
        pairs.append(np.stack([i, i + rng.integers(5, 20, size=10)], axis=1).astype(np.uint32))
    return x, targets, pairs


def _one_life(hip, x, targets, pairs):
    s = g.System(hip, N, R)
    s.set_bead_params(a=np.ones(N), b=np.zeros(N))
    s.set_pair_softcore(5.0, 0.3)
    s.add_bond_range(g.System.bond_params(g.POT_SPRING, 100.0, 0.25), 0, N)
    s.set_positions(x)
    s.set_pair_softwell(0.8, 0.2, 0.4, targets)                       # the droplet term
    link = g.System.bond_params(g.POT_SPRING, 50.0, 0.3)
    replica.define(s, 0, link)                                         # a per-replica pair slot
    for r in range(R):
        replica.set_pairs(s, 0, r, pairs[r])
    replica.define(s, 1, link)                                         # the glue slot
    glue.define(s, 1, max_glues=200, reach=0.4, binding_rate=2.0, unbinding_rate=0.5)
    s.run(20, 1e-4, 1.0, seed=5)
    glue.update(s, 0.5, 0, [3, 4])
    s.contacts_update(0.4)
    out = dict(glues=[glue.fetch(s, r) for r in range(R)], contacts=[s.contacts(r) for r in range(R)],
               pairs=[s.search_pairs(0.45, r) for r in range(R)], x=s.positions_f32(), x64=s.positions())
    s.close()
    return out


def test_a_handle_with_every_feature_alive_is_destroyed_and_built_again(hip):
    model = _model()
    first = _one_life(hip, *model)
    second = _one_life(hip, *model)
    assert np.isfinite(first["x"]).all() and not np.array_equal(first["x"], model[0].astype(np.float32))      # the run moved the beads
    for r in range(R):
        assert len(first["glues"][r]) > 0 and len(first["contacts"][r]) > 0 and len(first["pairs"][r]) > 0, r
    for key in ("x", "x64"):
        assert np.array_equal(first[key], second[key]), key
    for key in ("glues", "contacts", "pairs"):
        for r in range(R):
            assert np.array_equal(first[key][r], second[key][r]), (key, r)
