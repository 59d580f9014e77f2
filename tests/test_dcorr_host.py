"""The restatement of the displacement correlation (tests/dcorr_restatement.py) against closed forms, and the pure-Python helpers of
dcorr.py against the restatement.  No device."""
import importlib
import math

import numpy as np

import dcorr_restatement as dr
import rdf_restatement as R

dcorr = importlib.import_module("2022a-genome-dynamics_amd.dcorr")


def lattice_frame(rng, n, span=32, step=8):
    """n beads on a 1/step lattice in [0, span / step)^3: every coordinate and every difference is exact in float32."""
    return rng.integers(0, span, size=(n, 3)).astype(np.float64) / step


def test_class_index_enumerates_the_classes():
    for K in range(1, 9):
        seen = [int(dr.class_index(np.int64(a), np.int64(b), K)) for a in range(K) for b in range(a, K)]
        assert seen == list(range(K * (K + 1) // 2)) == [dcorr.class_index(b, a, K) for a in range(K) for b in range(a, K)]
        assert dr.n_classes(K, True) == 2 * len(seen) == dcorr.n_classes(K, True) == len(dcorr.class_labels(K, True))
        both = [dcorr.class_index(a, b, K, c) for a, b, c in dcorr.class_labels(K, True)]
        assert both == list(range(2 * len(seen)))
        assert int(dr.class_index(np.int64(K - 1), np.int64(0), K, True)) == 2 * (K - 1) + 1


def test_rigid_translation():
    """every bead moves by d: every dot equals t2 = |d|^2, so every class and bin with pairs has sum = count rint(|d|^2 2^S)"""
    rng = np.random.default_rng(1)
    x0 = lattice_frame(rng, 300)
    d = np.array([0.375, -1.25, 2.0])
    x = np.stack([x0, x0 + d, x0 + 2 * d])
    label, chain = rng.integers(-1, 3, size=300), rng.integers(0, 4, size=300)
    t2 = float(d @ d)
    for box in (None, (4.0, 4.0, 4.0)):
        for lag, scale in ((1, 0), (2, 0), (1, 7), (1, "unit")):
            count, total, self_count, self_sum, S = dr.pairs(x, lag, 0.125, 1.0, box, label, 3, chain, scale)
            n_sel = int((label >= 0).sum())
            assert S == (0 if scale == "unit" else scale or dr.auto_scale(n_sel, lag * lag * t2))
            q = int(np.rint(lag * lag * t2 * 2.0 ** S))
            assert count.shape == (3 - lag, 12, 8) and count.sum() > 0
            assert np.array_equal(total, count.astype(np.int64) * q)
            assert np.array_equal(self_sum, self_count.astype(np.int64) * q)
            assert np.array_equal(self_count[0], np.bincount(label[label >= 0], minlength=3))
            assert count.sum(axis=(1, 2)).tolist() == [R.counts_self(x0[label >= 0], box or (1e6,) * 3, 0.125, 1.0).sum()] * (3 - lag)


def test_uniform_dilation_is_exact_and_signed():
    """integer lattice about the origin, x -> k x with an integer k: dot = (k - 1)^2 x_i . x_j, exact integers at S = 0"""
    rng = np.random.default_rng(2)
    x0 = rng.integers(-6, 7, size=(250, 3)).astype(np.float64)
    k = 3
    x = np.stack([x0, k * x0]).astype(np.float32)
    md, bw = 9.0, 1.0
    count, total, self_count, self_sum, S = dr.pairs(x, 1, bw, md, None, None, 1, None, "unit")
    assert S == 0
    xi = x0.astype(np.int64)
    want_n, want_s = np.zeros(9, np.int64), np.zeros(9, np.int64)
    neg = pos = 0
    for i in range(len(xi)):
        for j in range(i + 1, len(xi)):
            r2 = int(((xi[i] - xi[j]) ** 2).sum())
            if r2 < 81:
                dot = (k - 1) ** 2 * int(xi[i] @ xi[j])
                want_n[math.isqrt(r2)] += 1
                want_s[math.isqrt(r2)] += dot
                neg, pos = neg + (dot < 0), pos + (dot > 0)
    assert neg > 100 and pos > 100
    assert np.array_equal(count[0, 0], want_n.astype(np.uint64)) and np.array_equal(total[0, 0], want_s)
    assert self_sum[0, 0] == (k - 1) ** 2 * int((xi * xi).sum()) and self_count[0, 0] == 250


def test_counts_equal_the_rdf_restatement():
    rng = np.random.default_rng(3)
    x = (rng.uniform(size=(2, 400, 3)) * (3.0, 5.0, 7.5)).astype(np.float32)
    for box, md in (((3.0, 5.0, 7.5), 1.0), ((3.0, 5.0, 7.5), 1.7), (None, 1.3)):
        count = dr.pairs(x, 1, 0.1, md, box)[0]
        assert np.array_equal(count[0, 0], R.counts_self(x[0], box or (1e6,) * 3, 0.1, md)) and count.sum() > 0


def test_guard_and_automatic_scale():
    """n = 62 178 beads, M = 4.0: n (n - 1) / 2 = 1 933 020 753 pairs, just under 2^31 (2^30.85).  A call is legal when
    pairs (4 * 2^S + 1) < 2^62.  S = 29: 4 * 2^29 + 1 = 2^31 + 1, times pairs = 4.151e18 < 2^62 = 4.612e18: legal.
    S = 30: 2^32 + 1, times pairs = 8.30e18 > 2^62: not legal.  So the automatic S is 29."""
    n, M = 62178, 4.0
    pairs = n * (n - 1) // 2
    assert pairs == 1933020753 and pairs * (4 * 2 ** 29 + 1) < 2 ** 62 < pairs * (4 * 2 ** 30 + 1)
    assert dr.legal(n, M, 29) and not dr.legal(n, M, 30) and dr.auto_scale(n, M) == 29 == dcorr.automatic_scale(n, M)
    for n, M in ((2, 1e-30), (700, 0.0), (700, 3.7e-3), (10, 1e12), (100, 3e12), (5, 4.6e18), (2, 1e19), (1, 1e7), (0, 0.0), (3000, 5e-324)):
        assert dr.auto_scale(n, M) == dcorr.automatic_scale(n, M), (n, M)
        for S in (0, 1, 20, 40):
            assert dr.legal(n, M, S) == dcorr.scale_is_legal(n, M, S), (n, M, S)
    assert dr.auto_scale(700, 0.0) == 40 and dr.auto_scale(2, 1e19) is None and not dr.legal(5, math.inf, 0)


def test_curves_divide_in_the_headers_order():
    count = np.array([[[2, 0]], [[1, 0]]], np.uint64)
    total = np.array([[[-6, 0]], [[3, 0]]], np.int64)
    c = dcorr.curves(count, total, np.array([[4], [4]], np.uint64), np.array([[16], [16]], np.int64), 1, 1, False, 0.5, 1.0)
    assert c.dot[0, 0] == -0.5 and np.isnan(c.dot[0, 1]) and c.normalised[0, 0] == -0.25 and c.r.tolist() == [0.25, 0.75]
    assert dcorr.bin_edges(0.4, 1.0).tolist() == [0.0, 0.4, 0.8, 1.0]


def test_library_and_binding_mirror_the_header():
    """the symbols, the ABI version and the macros of include/gdyn_dcorr.h, without a device"""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "gdyn_dcorr.h")).read()
    macro = lambda name: re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1)
    assert int(macro("GD_DCORR_ABI_VERSION")) == dcorr.DCORR_ABI_VERSION and int(macro("GD_DCORR_LDS_BINS")) == dcorr.LDS_BINS
    assert int(macro("GD_DCORR_MAX_LABELS")) == dcorr.MAX_LABELS and int(macro("GD_DCORR_MAX_SCALE_BITS")) == dcorr.MAX_SCALE_BITS == dr.MAX_SCALE_BITS
    assert int(macro("GD_DCORR_SCALE_UNIT")) == dcorr.SCALE_UNIT
    for name in dcorr.DCORR_SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
    d = dcorr.load_dcorr_library()      # checks every symbol and the version
    assert d.gd_dcorr_bins(0.02, 1.0) == 50 == dr.n_bins(0.02, 1.0) == dcorr.n_bins(0.02, 1.0)
    assert d.gd_dcorr_bins(0.0, 1.0) == 0 and d.gd_dcorr_bins(1e-9, 1.0) == 0 and d.gd_dcorr_classes(None) == 0
