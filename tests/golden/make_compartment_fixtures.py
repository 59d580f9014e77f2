#!/usr/bin/env python3
"""Generates tests/golden/compartment_fixtures.npz by IMPORTING the reference's own 2-signal/src/hic_analysis/cool.py in this
container and recording what load_contact_matrices, compute_enrichment_matrices and compute_contact_pca return for a toy cooler.
Only arrays are stored.  The image has no h5py, so a stand-in is placed in sys.modules for the import (the pattern of
make_hic_fixtures.py): its h5t.check_dtype reads the enum from the dtype's metadata.  Nothing of the reference is changed.

The toy cooler (resolutions/1000): chromosomes "1" (96 bins) and "2" (61 bins) with a planted checkerboard (period 12 and 7) on a
power-law decay and a few unmappable bins each, "X" (20 bins, left out of the profile), "3" (one bin); no pixel at 90 bins or more
apart, so the mean contact is NaN there and the far corners of the 96-bin enrichment matrix are NaN; trans pixels; a weight
column with NaNs; unique pairs in cooler order; every diagonal's raw sum below 2^24.
The principal components are recorded with the sign rule of DESIGN.md section 7f applied to the reference's output.
Run here:  python tests/golden/make_compartment_fixtures.py"""
import importlib.machinery
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import compartment_restatement as R      # noqa: E402

REFERENCE = "/root/reference"
BINSIZE = 1000
NAMES = ["1", "2", "X", "3"]
SIZES = [96, 61, 20, 1]
PERIODS = [12, 7, 5, 1]
REACH = 90            # no pixel at this distance or beyond
K = 3


class Dataset:
    def __init__(self, data):
        self.data, self.dtype, self.shape = data, data.dtype, data.shape

    def __getitem__(self, key):
        return self.data[key]


class Group(dict):
    def __getitem__(self, key):
        node = self
        for part in key.split("/"):
            node = dict.__getitem__(node, part)
        return node


def _load_reference():
    h5py = types.ModuleType("h5py")
    h5py.h5t = types.SimpleNamespace(check_dtype=lambda enum: enum.metadata["enum"])
    h5py.check_dtype = h5py.h5t.check_dtype
    sys.modules["h5py"] = h5py
    loader = importlib.machinery.SourceFileLoader("ref_cool", REFERENCE + "/2-signal/src/hic_analysis/cool.py")
    module = importlib.util.module_from_spec(importlib.util.spec_from_loader("ref_cool", loader))
    loader.exec_module(module)
    return module


def toy_cooler(rng):
    chrom = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    n_bins = len(chrom)
    first = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    within = np.arange(n_bins) - first[chrom]
    starts = within * BINSIZE
    ends = np.minimum(starts + BINSIZE, np.array(SIZES)[chrom] * BINSIZE - 137)
    mappable = np.ones(n_bins, bool)
    mappable[[17, 18, 40, 77]] = False                       # chromosome 1
    mappable[first[1] + np.array([9, 30, 31])] = False        # chromosome 2
    mappable[first[2] + 4] = False                            # X
    state = np.where((within // np.array(PERIODS)[chrom]) % 2 == 0, 1.0, -1.0)
    pairs = {}
    for i in np.flatnonzero(mappable):
        for j in np.flatnonzero(mappable):
            if j < i:
                continue
            d = j - i
            if chrom[i] == chrom[j]:
                if d >= REACH:
                    continue
                pairs[(i, j)] = 1 + rng.poisson(20000.0 / (d + 1) * (1 + 0.6 * state[i] * state[j]))
            elif rng.random() < 0.02:
                pairs[(i, j)] = 1 + rng.poisson(0.5)
    keys = np.array(sorted(pairs), np.int64)
    count = np.array([pairs[tuple(k)] for k in keys], np.int32)
    weights = rng.uniform(0.5, 1.5, n_bins)
    weights[~mappable] = np.nan
    weights[[5, 50, first[1] + 20]] = np.nan
    return chrom, starts.astype(np.int32), ends.astype(np.int32), keys[:, 0].copy(), keys[:, 1].copy(), count, weights


def signed(pcs, variances, axes, mask, k):
    """The leading k of compute_contact_pca's output with the sign rule applied."""
    pcs, axes = pcs[:, :k].copy(), axes[:k].copy()
    for j in range(k):
        row = axes[j][mask]
        if row[np.argmax(np.abs(row))] < 0:
            pcs[:, j], axes[j] = -pcs[:, j], -axes[j]
    return pcs, variances[:k].copy(), axes


def main():
    np.seterr(all="ignore")
    warnings.simplefilter("ignore")
    ref = _load_reference()
    rng = np.random.default_rng(20220607)
    chrom, starts, ends, bin1, bin2, count, weights = toy_cooler(rng)
    enum = np.dtype(np.int32, metadata={"enum": {n: k for k, n in enumerate(NAMES)}})
    datasets = Group(bins=Group(chrom=Dataset(chrom.astype(enum)), start=Dataset(starts), end=Dataset(ends), weight=Dataset(weights)),
                     pixels=Group(bin1_id=Dataset(bin1), bin2_id=Dataset(bin2), count=Dataset(count)))
    assert len(set(zip(bin1.tolist(), bin2.tolist()))) == len(bin1) and (bin1 <= bin2).all() and (chrom[bin1] != chrom[bin2]).any()
    out = {"chrom": chrom, "start": starts, "end": ends, "weight": weights, "bin1": bin1, "bin2": bin2, "count": count, "binsize": np.array(BINSIZE)}
    counted = [n for n in NAMES if n != "X"]
    enrich = {}
    for norm, w in (("RAW", None), ("weight", weights)):
        matrices, _ = ref.load_contact_matrices(datasets, norm)
        assert list(matrices) == NAMES and all(m.dtype == np.float32 for m in matrices.values())
        mine = R.dense(bin1, bin2, count, chrom, w)
        for code, name in enumerate(NAMES):
            assert np.array_equal(matrices[name], mine[code], equal_nan=True), (norm, name)      # the rule of the device: float32 adds
            if w is None:
                for d in range(matrices[name].shape[0]):
                    assert np.diag(matrices[name], k=d).astype(np.float64).sum() < 2 ** 24
        enrichment, mean = ref.compute_enrichment_matrices(matrices, counted)
        contacts, counts, my_mean = R.profile({c: mine[c] for c, n in enumerate(NAMES) if n != "X"})
        assert len(mean) == max(SIZES) and np.array_equal(np.isnan(mean), counts == 0) and np.isnan(mean[REACH:]).all() and not np.isnan(mean[:REACH]).any()
        if w is None:
            assert contacts.max() < 2 ** 24 and np.array_equal(mean, my_mean, equal_nan=True)
        for code, name in enumerate(NAMES):
            out[f"contact_{norm}_{code}"] = matrices[name]
            out[f"enrichment_{norm}_{code}"] = enrichment[name]
            assert enrichment[name].dtype == np.float64
        out[f"mean_{norm}"], out[f"counts_{norm}"] = mean, counts
        enrich[norm] = enrichment

    e1, e2 = enrich["RAW"]["1"], enrich["RAW"]["2"]
    assert np.isnan(e1[0, 95]) and not np.isnan(e2).any()
    mask_b = R.valid(out["contact_RAW_0"])
    mask_b[:SIZES[0] - REACH] = False          # bins that lie REACH or more from another bin: their rows of the enrichment hold NaN
    mask_b[REACH:] = False
    cases = {"a": (e2, None), "b": (e1, mask_b)}
    for key, (matrix, mask) in cases.items():
        pcs, variances, axes = ref.compute_contact_pca(matrix, mask)
        used = np.any(matrix != 0, axis=1) if mask is None else mask
        assert 2 < used.sum() < len(matrix)
        singular = np.sqrt(variances)
        p, v, a = signed(pcs, variances, axes, used, K)
        for j, (rel, absolute) in enumerate(R.pca_bounds(singular, K)):
            assert absolute <= 1e-8 and rel <= 1e-8, (key, j, rel, absolute)
            top = np.sort(np.abs(a[j][used]))[-2:]
            assert top[1] - top[0] > 1e-6, (key, j, top)                                       # the sign rule is stable
        mine = R.pca(matrix, mask, K)
        assert np.allclose(mine[0], p, rtol=0, atol=1e-12, equal_nan=True) and np.allclose(mine[2], a, rtol=0, atol=1e-12, equal_nan=True)
        out[f"pca_{key}_mask"], out[f"pca_{key}_singular"] = used, singular
        out[f"pca_{key}_pcs"], out[f"pca_{key}_variances"], out[f"pca_{key}_axes"] = p, v, a
        print("case", key, "m", int(used.sum()), "variances", v, "bounds", R.pca_bounds(singular, K))
    try:                                                                                        # (c): the default mask keeps the rows with NaN
        ref.compute_contact_pca(e1, None)
        raise SystemExit("the reference was expected to raise LinAlgError for the 96-bin enrichment with its default mask")
    except np.linalg.LinAlgError:
        pass
    path = os.path.join(HERE, "compartment_fixtures.npz")
    np.savez_compressed(path, **out)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "compartment_fixtures.npz")
    assert os.path.getsize(path) <= largest, (os.path.getsize(path), largest)
    print("ok", len(chrom), "bins,", len(bin1), "pixels,", os.path.getsize(path), "bytes; the largest other fixture has", largest)


if __name__ == "__main__":
    main()
