"""Inputs that take the compartment kernels (csrc/gdyn_hic.hip) past one block: a pixel table of seven
chromosomes with planted bins (A), tables whose pixels collide in a cell (B) and matrices for the solver at every size where its
grids, its loops or its split rule change (C).  Plain numpy, no device; tests/test_compartment_host.py asserts that every input is
what it claims to be, tests/test_compartment_edges_gpu.py feeds them to the device."""
import functools
from types import SimpleNamespace

import numpy as np

import compartment_restatement as R

# ---- A: seven chromosomes, 1 019 bins

SIZES = (300, 1, 64, 65, 257, 2, 330)      # code = position; code 6 is excluded from the profile and is the largest
EXCLUDED_CODE = 6
COUNTED = tuple(c for c in range(len(SIZES)) if c != EXCLUDED_CODE)
ONLY_FAR, EMPTY, NAN_WEIGHT, PARTNER = 40, 41, 280, 42      # local bins of chromosome 0, see table_a


@functools.lru_cache(maxsize=None)
def table_a():
    """Per chromosome a cis pair (i <= j) at separation d is kept with probability min(1, 12 / (d + 1)), and every pair at
    d >= 250 with probability 0.5 besides; counts in [1, 900]; weights uniform in [0.4, 1.6].  Planted in chromosome 0, every
    other pixel of the named bins removed:
      bin 40   only the pixel (40, 299): its row's one cell lies beyond column 256
      bin 41   no pixel
      bin 280  only the pixel (42, 280), and w[280] = NaN: with weights row 42 is finite but for one NaN in column 280
    The pixels are sorted by (bin1, bin2) as a cooler's are."""
    rng = np.random.default_rng(20224)      # a seed with every distance below 300 populated (the host test asserts it)
    chrom = np.repeat(np.arange(len(SIZES), dtype=np.int32), SIZES)
    first = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    b1, b2 = [], []
    for beg, n in zip(first, SIZES):
        i, j = np.triu_indices(n)
        d = j - i
        keep = (rng.random(len(d)) < np.minimum(1.0, 12.0 / (d + 1))) | ((d >= 250) & (rng.random(len(d)) < 0.5))
        if beg == 0:
            planted = (ONLY_FAR, EMPTY, NAN_WEIGHT)
            keep &= ~np.isin(i, planted) & ~np.isin(j, planted)
        b1.append(i[keep] + beg)
        b2.append(j[keep] + beg)
    b1 = np.concatenate(b1 + [[ONLY_FAR, PARTNER]]).astype(np.int64)
    b2 = np.concatenate(b2 + [[SIZES[0] - 1, NAN_WEIGHT]]).astype(np.int64)
    order = np.lexsort((b2, b1))
    b1, b2 = b1[order], b2[order]
    count = rng.integers(1, 901, len(b1)).astype(np.int32)
    weight = rng.uniform(0.4, 1.6, len(chrom))
    weight[NAN_WEIGHT] = np.nan
    return SimpleNamespace(chrom=chrom, first=first, bin1=b1, bin2=b2, count=count, weight=weight,
                           excluded=(chrom == EXCLUDED_CODE).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def expected_a(norm):
    """The restatement's matrices, profile, enrichment (codes 0, 4, 6) and valid bins of table A; computed once, not to be written to."""
    t = table_a()
    matrices = R.dense_fast(t.bin1, t.bin2, t.count, t.chrom, None if norm == "RAW" else t.weight)
    contacts, counts, mean = R.profile(matrices, COUNTED)
    k = {code: np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) for code, n in enumerate(SIZES)}
    with np.errstate(all="ignore"):
        enrichment = {code: matrices[code].astype(np.float64) / mean[k[code]] for code in (0, 4, 6)}      # R.enrichment, held to it on the host
    valid = np.concatenate([R.valid(matrices[code]) for code in range(len(SIZES))])
    return SimpleNamespace(matrices=matrices, contacts=contacts, counts=counts, mean=mean, enrichment=enrichment, valid=valid, distance=k)


def shuffled_ids(b1, b2, every=3):
    flip = np.arange(len(b1)) % every == 0
    return np.where(flip, b2, b1), np.where(flip, b1, b2)


CUTS_A = (0, 1501, 20003)      # the pixels go over in three calls; no cut is a multiple of 4 (a lane takes 4 pixels)

# ---- B: pixels that collide in a cell

CHROM_B = np.array([0] * 8 + [1] * 3, np.int32)
REPEATS = 6000
WEIGHT_B = np.array([0.7, 1.3, 0.9, 1.1, 0.6, 1.7, 1.9, 0.3, 1.0, 1.0, 1.0])      # not dyadic
COUNT_WEIGHTED = 3


def split_counts():
    """(one, two): 200 pixels over the 8 x 8 block of chromosome 0 (it has 36 cells i <= j, so cells repeat), and the same
    contacts as 400 pixels, every count c handed over as c1 + c2 = c, shuffled.  Every cell total stays below 2^24, so float32
    adds them exactly in any order."""
    rng = np.random.default_rng(8)
    i, j = rng.integers(0, 8, 200), rng.integers(0, 8, 200)
    i, j = np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)
    c = rng.integers(2, 40001, 200).astype(np.int32)
    c1 = (rng.integers(1, c)).astype(np.int32)
    order = rng.permutation(400)
    two = (np.concatenate([i, i])[order], np.concatenate([j, j])[order], np.concatenate([c1, c - c1])[order])
    return (i, j, c), two


CHROM_ZERO = np.array([0] * 5 + [1] * 3, np.int32)
WEIGHT_ZERO = np.array([0.7, 1.3, 0.0, 1.1, 0.6, 0.9, 1.2, 0.8])
ZERO_BIN, ZERO_PARTNERS = 2, (1, 4)
# bin 2 (w = 0) has the pixels (1, 2) and (2, 4): infinite cells at the distances 1 and 2, beside finite cells at both
PIXELS_ZERO = (np.array([0, 0, 1, 1, 2, 3, 0, 5, 5, 6], np.int64), np.array([0, 1, 2, 3, 4, 4, 3, 5, 7, 7], np.int64),
               np.array([5, 7, 3, 2, 5, 4, 6, 9, 2, 8], np.int32))

# ---- C: the solver across its boundaries

PCA_SIZES = (9, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 600, 1030)      # m, the valid bins
PCA_UNSYMMETRIC = (65, 513)
PCA_TWICE = (513, 1030)
LAYERS = ((1.0, 7), (0.6, 11), (0.35, 5), (0.2, 3))


def layered(n, seed, unmappable=(), sym=True):
    """Ones, plus a s s^T for (a, period) in LAYERS with s the +-1 checkerboard of that period, plus 0.01 N(0, 1) noise,
    symmetrised unless sym is False; the rows and columns of `unmappable` are zero."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    m = np.ones((n, n))
    for a, period in LAYERS:
        s = np.where((k // period) % 2 == 0, 1.0, -1.0)
        m += a * s[:, None] * s[None, :]
    m += 0.01 * rng.standard_normal((n, n))
    if sym:
        m = (m + m.T) / 2
    m[list(unmappable), :] = 0
    m[:, list(unmappable)] = 0
    return m


def pca_case(m, sym=True):
    """(matrix, mask) with m valid bins: n = m + 3 and the bins 0, n // 2, n - 1 unmappable when n > 20."""
    n = m + 3 if m + 3 > 20 else m
    unmappable = (0, n // 2, n - 1) if n > 20 else ()
    matrix = layered(n, 1000 + m, unmappable, sym)
    mask = np.ones(n, bool)
    mask[list(unmappable)] = False
    return matrix, mask


@functools.lru_cache(maxsize=None)
def pca_reference(m, sym=True):
    """(matrix, mask, R.pca(matrix, None, 3)); computed once per size, not to be written to."""
    matrix, mask = pca_case(m, sym)
    return matrix, mask, R.pca(matrix, None, 3)


def conditioning(singular, m, k):
    """(the block's convergence ratio lam[k + 8] / lam[k - 1], 0 where the block min(m, k + 8) is the whole space; the smallest
    gap_j / lam_0 of the first k components)."""
    lam = np.asarray(singular, np.float64) ** 2
    ratio = lam[k + 8] / lam[k - 1] if k + 8 < m else 0.0
    gap = min(np.abs(np.delete(lam, j) - lam[j]).min() for j in range(k)) / lam[0]
    return ratio, gap
