"""The glue rule of include/gdyn_glue.h restated in numpy: Philox4x32-10, the integer thresholds, brute-force
candidates with the fp32 minimum image of the pair search, and one update of one replica's set.  The device must reproduce `update`
exactly wherever no pair sits within rounding of `reach` (`margin` measures that)."""
import math

import numpy as np

M32 = np.uint64(0xffffffff)
KEY_TAG = 0x474C5545


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two; returns the four output words as uint64 arrays holding 32-bit values"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in ctr]
    k = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return c


def threshold(p):
    return min(1 << 32, math.floor(p * 2.0 ** 32))


def thresholds(binding_rate, unbinding_rate, dt):
    """(thr_on, thr_off)"""
    return threshold(-math.expm1(-binding_rate * dt)), threshold(-math.expm1(-unbinding_rate * dt))


def draws(pairs, epoch, seed):
    """release word, fire word, sel of every pair (n, 2)"""
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    if len(pairs) == 0:
        z = np.zeros(0, dtype=np.uint64)
        return z, z, z
    w = philox4x32_10((pairs[:, 0], pairs[:, 1], epoch & 0xffffffff, epoch >> 32), (seed & 0xffffffff, ((seed >> 32) & 0xffffffff) ^ KEY_TAG))
    return w[0], w[1], (w[2] << np.uint64(32)) | w[3]


def _image(d, box):
    b = np.asarray(box, dtype=np.float32)
    inv = (1.0 / np.asarray(box, dtype=np.float64)).astype(np.float32)
    return d - b * np.rint(d * inv)


def dist2(x32, pairs, box):
    """fp32 squared minimum-image distances of the pairs (n, 2), as the pair search forms them"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    d = _image(x32[pairs[:, 0]] - x32[pairs[:, 1]], box)
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def candidates(x32, box, reach, rows=256):
    """All pairs i < j with fp32 d2 < fp32(reach^2), ascending, and the smallest |d2 / reach^2 - 1| over ALL pairs (the margin by which
    the nearest pair misses the boundary: above 1e-6 the fp32 rounding of d2, ~2.4e-7, cannot change the set)."""
    x32 = np.asarray(x32, dtype=np.float32)
    n = len(x32)
    r2 = np.float32(reach * reach)
    out, margin = [], np.inf
    for a in range(0, n, rows):
        d = _image(x32[a:a + rows, None, :] - x32[None, :, :], box)
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        upper = np.arange(n)[None, :] > np.arange(a, min(a + rows, n))[:, None]
        margin = min(margin, float(np.abs(d2[upper].astype(np.float64) / (reach * reach) - 1.0).min()))
        i, j = np.nonzero((d2 < r2) & upper)
        out.append(np.stack([i + a, j], axis=1))
    return np.concatenate(out).astype(np.uint32), margin


def _keys(pairs):
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return (pairs[:, 0] << np.uint64(32)) | pairs[:, 1]


def update(bound, cand, x32, box, reach, max_glues, thr_on, thr_off, epoch, seed):
    """One update of one replica.  bound: (n, 2) sorted set; cand: the candidates (any order).  Returns the new sorted set and what
    happened: pairs removed by distance, released, fired, the free capacity, pairs released and bound again."""
    bound = np.asarray(bound, dtype=np.uint32).reshape(-1, 2)
    cand = np.asarray(cand, dtype=np.uint32).reshape(-1, 2)
    far = ~(dist2(x32, bound, box) < np.float32(reach * reach))
    rel, _, _ = draws(bound, epoch, seed)
    released = ~far & (rel < np.uint64(thr_off))
    kept = bound[~far & ~released]
    unbound = ~np.isin(_keys(cand), _keys(kept))
    pool = cand[unbound]
    _, fire, sel = draws(pool, epoch, seed)
    fired, fsel = pool[fire < np.uint64(thr_on)], sel[fire < np.uint64(thr_on)]
    free = max_glues - len(kept)
    if len(fired) > free:
        order = np.lexsort((fired[:, 1], fired[:, 0], fsel))      # by sel, ties by (i, j)
        fired = fired[order[:free]]
    new = np.concatenate([kept, fired])
    new = new[np.argsort(_keys(new), kind="stable")]
    info = dict(far=int(far.sum()), released=int(released.sum()), fired=int((fire < np.uint64(thr_on)).sum()), free=int(free),
                rebound=int(np.isin(_keys(bound[released]), _keys(fired)).sum()))
    return new.astype(np.uint32), info


# ------------------------------------------------------------------------------------------------ what a correct process satisfies

def rates(p_on, p_off, dt):
    """(binding_rate, unbinding_rate) whose probabilities over dt are p_on and p_off; p = 1: a rate at which exp(-rate dt) is 0"""
    rate = lambda p: 1000.0 / dt if p >= 1 else -math.log1p(-p) / dt
    return rate(p_on), rate(p_off)


def stationary(p_on, p_off, n_pairs):
    """Frozen positions, no capacity limit: every candidate pair is a two-state chain of its own.  Returns (mean, sigma) of the bound
    count in the stationary state, and (mean, sigma) of the count of pairs bound at two successive epochs (a bound pair stays unless it
    releases and does not fire again in the same update)."""
    pi = p_on / (p_on + p_off * (1.0 - p_on))
    both = pi * (1.0 - p_off + p_off * p_on)
    return (pi * n_pairs, math.sqrt(pi * (1 - pi) * n_pairs)), (both * n_pairs, math.sqrt(both * (1 - both) * n_pairs))


def hypergeometric(population, marked, draws_):
    """(mean, variance) of the marked items among `draws_` drawn without replacement"""
    f = marked / population
    return draws_ * f, draws_ * f * (1 - f) * (population - draws_) / (population - 1)


def random_state(n_beads, box, seed):
    """n_beads uniform points in the periodic box, on the 2^-16 grid (exact in fp32)"""
    rng = np.random.default_rng(seed)
    return (np.rint(rng.random((n_beads, 3)) * box * 65536.0) / 65536.0).astype(np.float32)
