#!/usr/bin/env python3
"""Generates tests/golden/hic_fixtures.npz and hic_fixtures.json by IMPORTING the reference's own
2-signal/src/compute_interactions/compute_interactions.py, 2-signal/src/compute_local_alpha/command.py,
5-sim-genome/scripts/hic_power_law and 2-signal/src/downsample/__main__.py in this container and recording what their
functions and their run() return and print for a toy cooler.  Only arrays and recorded output text are stored (for downsample
also the unrounded values of its downsample(), which its text rounds to six digits).  The image has scipy and pandas but
neither h5py nor numba, so stand-ins are placed in sys.modules for the import: an `h5py` whose File()
hands out the in-memory store below and whose check_dtype reads the enum from the dtype's metadata, and a `numba` whose jit
is the identity, with or without keyword arguments.  Nothing of the reference is changed.

The toy cooler (resolutions/1000): chromosome names without a chr prefix, in an order that by_std_chrom_order changes; one
chromosome of a single bin; two of 2 (W - 1) <= n < 10 bins for W = 4; X, Y and MT, MT with 4 bins (below 2 (W - 1): the
reference's compute_local_decays asserts there, MT is the one chromosome compute_interactions skips, so its run() completes and
MT's signals are held against the restatement only); bins without any pixel; trans pixels; a weight column with NaNs; counts
below 2^24; unique pairs with bin1 <= bin2, sorted by (bin1, bin2).
Run here:  python tests/golden/make_hic_fixtures.py"""
import contextlib
import importlib.machinery
import importlib.util
import io
import json
import os
import runpy
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hic_restatement as R      # noqa: E402

REFERENCE = "/root/reference"
STORES = {}


class Dataset:
    def __init__(self, data, chunks=None):
        self.data = data
        self.chunks = chunks
        self.dtype = data.dtype
        self.shape = data.shape

    def __len__(self):
        return len(self.data)

    def __getitem__(self, key):
        return self.data[key]


class Group(dict):
    def __getitem__(self, key):
        node = self
        for part in key.split("/"):
            node = dict.__getitem__(node, part)
        return node

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _install_stand_ins():
    h5py = types.ModuleType("h5py")
    h5py.check_dtype = lambda enum: enum.metadata["enum"]
    h5py.File = lambda name, mode="r": STORES[name]
    h5py.Group, h5py.Dataset = Group, Dataset
    numba = types.ModuleType("numba")
    numba.jit = lambda *args, **kwargs: args[0] if args and callable(args[0]) else (lambda f: f)
    sys.modules["h5py"], sys.modules["numba"] = h5py, numba


def _load(name, path):
    loader = importlib.machinery.SourceFileLoader(name, path)
    spec = importlib.util.spec_from_loader(name, loader)
    module = importlib.util.module_from_spec(spec)
    loader.exec_module(module)
    return module


_install_stand_ins()
ref_ci = _load("ref_compute_interactions", REFERENCE + "/2-signal/src/compute_interactions/compute_interactions.py")
ref_alpha = _load("ref_compute_local_alpha", REFERENCE + "/2-signal/src/compute_local_alpha/command.py")
ref_pl = _load("ref_hic_power_law", REFERENCE + "/5-sim-genome/scripts/hic_power_law")

BINSIZE = 1000
NAMES = ["1", "2", "3", "10", "4", "5", "X", "Y", "MT"]
SIZES = [110, 90, 60, 8, 1, 45, 40, 7, 4]
WIDTHS = (10, 50)
DOWNSAMPLE_CASES = [(2, None), (5, None), (2, 5), (3, 2)]      # (rate, window)


def toy_cooler(rng):
    chrom = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    n_bins = len(chrom)
    first = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    within = np.arange(n_bins) - first[chrom]
    starts = within * BINSIZE
    ends = np.minimum(starts + BINSIZE, np.array(SIZES)[chrom] * BINSIZE - 137)      # the last bin of a chromosome is shorter
    mappable = rng.random(n_bins) > 0.08
    mappable[first[3]:first[3] + 8] = [True, True, False, True, True, True, True, True]
    mappable[first[4]] = True
    mappable[first[8]:] = True
    pairs = {}
    for i in np.flatnonzero(mappable):
        for j in np.flatnonzero(mappable):
            if j < i:
                continue
            d = j - i
            if chrom[i] == chrom[j]:
                p = 1.0 if d == 0 else min(1.0, 2.5 / d ** 0.8)
                if d == 0 and rng.random() < 0.03:
                    continue                                  # a mappable bin without a diagonal pixel
                if rng.random() < p:
                    pairs[(i, j)] = 1 + rng.poisson(3000.0 / (d + 1) ** 1.1)
            elif rng.random() < 0.02:
                pairs[(i, j)] = 1 + rng.poisson(0.5)          # trans
    keys = np.array(sorted(pairs), np.int64)
    count = np.array([pairs[tuple(k)] for k in keys], np.int32)
    weights = rng.uniform(0.5, 1.5, n_bins)
    weights[~mappable] = np.nan
    weights[rng.random(n_bins) < 0.05] = np.nan
    return chrom, starts.astype(np.int32), ends.astype(np.int32), keys[:, 0].copy(), keys[:, 1].copy(), count, weights, mappable


def store_of(chrom, starts, ends, bin1, bin2, count, weights):
    enum = np.dtype(np.int32, metadata={"enum": {n: k for k, n in enumerate(NAMES)}})
    bins = Group(chrom=Dataset(chrom.astype(enum)), start=Dataset(starts), end=Dataset(ends), weight=Dataset(weights))
    pixels = Group(bin1_id=Dataset(bin1, chunks=(4096,)), bin2_id=Dataset(bin2, chunks=(4096,)), count=Dataset(count, chunks=(4096,)))
    root = Group(resolutions=Group({str(BINSIZE): Group(bins=bins, pixels=pixels)}))
    assert bins["chrom"][:].dtype.metadata["enum"]["MT"] == 8
    return root


def captured(fn, **kwargs):
    out = io.StringIO()
    with contextlib.redirect_stdout(out), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        captured.value = fn(**kwargs)
    return out.getvalue()


def main():
    rng = np.random.default_rng(20220214)
    chrom, starts, ends, bin1, bin2, count, weights, mappable = toy_cooler(rng)
    n_bins = len(chrom)
    STORES["toy.mcool"] = store_of(chrom, starts, ends, bin1, bin2, count, weights)
    datasets = STORES["toy.mcool"][f"resolutions/{BINSIZE}"]
    assert count.max() < 2 ** 24 and len(set(zip(bin1.tolist(), bin2.tolist()))) == len(bin1) and (bin1 <= bin2).all()
    assert (chrom[bin1] != chrom[bin2]).any() and np.isnan(weights).any() and not mappable.all()
    out = {"chrom": chrom, "start": starts, "end": ends, "weight": weights, "bin1": bin1, "bin2": bin2, "count": count,
           "binsize": np.array(BINSIZE), "widths": np.array(WIDTHS)}
    text = {"names": NAMES}

    # compute_interactions: the bands and the signals of every chromosome the reference can process, W = 4 (run) and W = 6
    np.seterr(all="ignore")
    warnings.simplefilter("ignore")
    for W in (4, 6):
        tracks = ref_ci.extract_forward_bands(datasets, W)
        assert list(tracks) == ["1", "2", "3", "4", "5", "10", "X", "Y"]
        band = np.zeros((n_bins, W), np.int64)
        D, I = np.full((n_bins, W - 1), np.nan), np.full((n_bins, W - 2), np.nan)
        held = np.zeros(n_bins, bool)
        for name, track in tracks.items():
            rows = chrom == NAMES.index(name)
            band[rows] = np.nan_to_num(track.forward_bands, nan=0.0).astype(np.int64)
            n = int(rows.sum())
            if 1 < n < 2 * (W - 1):
                try:
                    ref_ci.compute_local_decays(track.forward_bands)
                    raise SystemExit("the reference was expected to assert for this chromosome")
                except AssertionError:
                    continue
            decays = ref_ci.compute_local_decays(track.forward_bands)
            D[rows], I[rows] = decays[:, 1:], ref_ci.compute_insulation_ratios(decays)[:, 1:]
            held[rows] = True
        mine = R.band(bin1, bin2, count, chrom, W)
        assert np.array_equal(mine[chrom != 8], band[chrom != 8])
        band[chrom == 8] = mine[chrom == 8]                   # MT: the reference drops its track
        out[f"band{W}"], out[f"decay{W}"], out[f"insulation{W}"], out[f"held{W}"] = band, D, I, held
    assert out["held4"][chrom != 8].all() and not out["held6"][chrom == 3].any() and not out["held6"][chrom == 7].any()
    text["compute_interactions_w4"] = captured(ref_ci.run, mcoolfile="toy.mcool", band_width=4, binsize=BINSIZE)

    # compute_local_alpha: the reference as it stands (float32 W and log W), and the float32 gap against the same formulas in fp64
    for width in WIDTHS:
        contact_band, codes, coords = ref_alpha.load_contact_band(datasets, band_width=width)
        w_sym = ref_alpha.compute_W(contact_band, ref_alpha.enumerate_runs(codes))
        alpha_ref = -ref_alpha.estimate_slope(np.log(np.arange(1, w_sym.shape[1])), np.log(w_sym[:, 1:]))
        band = np.nan_to_num(contact_band, nan=0.0).astype(np.int64)
        assert np.array_equal(band, R.band(bin1, bin2, count, chrom, width + 1))
        alpha_fp64 = R.local_alpha(band, chrom)
        assert np.array_equal(np.isnan(alpha_ref), np.isnan(alpha_fp64)) and np.isnan(alpha_ref).any() and (~np.isnan(alpha_ref)).sum() > 300
        gap = float(np.nanmax(np.abs(alpha_ref - alpha_fp64)))
        out[f"alpha_band{width}"], out[f"alpha_ref{width}"], out[f"alpha_fp32_gap{width}"] = band, np.asarray(alpha_ref, np.float64), np.array(gap)
        text[f"compute_local_alpha_w{width}"] = captured(ref_alpha.run, mcoolfile="toy.mcool", width=width, binsize=BINSIZE)
        print("alpha width", width, "fp32 gap", gap, "range", np.nanmin(alpha_ref), np.nanmax(alpha_ref))

    # hic_power_law: RAW and weighted
    size = max(SIZES)
    excluded = np.isin(chrom, [NAMES.index(n) for n in ("X", "Y", "MT")])
    for norm, w in (("RAW", None), ("weight", weights)):
        mean = ref_pl.collect_mean_contacts(datasets, norm)
        total, n = R.profile(bin1, bin2, count, chrom, excluded, w, size)
        assert len(mean) == size and np.array_equal(np.isnan(mean), n == 0)
        if w is None:
            assert np.array_equal(mean[n > 0], (total / np.maximum(n, 1))[n > 0])
        else:
            print("weighted P(s): restatement against the reference, max rel", np.nanmax(np.abs(total / n - mean) / mean))
        out[f"profile_mean_{norm}"], out[f"profile_n_{norm}"] = mean, n
        text[f"hic_power_law_{norm}"] = captured(ref_pl.run, mcool="toy.mcool", binsize=BINSIZE, normalize=norm)
    assert (out["profile_n_weight"] < out["profile_n_RAW"]).any()

    # downsample: main() runs on import
    script = REFERENCE + "/2-signal/src/downsample/__main__.py"
    text["downsample"] = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "signals.tsv")
        with open(path, "w") as f:
            f.write(text["compute_interactions_w4"])
        for rate, window in DOWNSAMPLE_CASES:
            argv = ["downsample", "--rate", str(rate)] + (["--window", str(window)] if window else []) + [path]
            saved = sys.argv
            sys.argv = argv
            try:
                result = captured(lambda: runpy.run_path(script, run_name="downsample_main"))
            finally:
                sys.argv = saved
            text["downsample"].append({"rate": rate, "window": window, "output": result})
            # the unrounded values of the reference's downsample() for every chromosome of the table, one after the other
            rows = [line.split("\t") for line in text["compute_interactions_w4"].splitlines()[1:]]
            parts = []
            for name in dict.fromkeys(r[0] for r in rows):
                values = np.array([[float(v) for v in r[3:]] for r in rows if r[0] == name])
                parts.append(captured.value["downsample"](values, rate=rate, window=window))
            out[f"downsample_{rate}_{window or 0}"] = np.concatenate(parts)
            assert len(out[f"downsample_{rate}_{window or 0}"]) == len(result.splitlines()) - 1

    np.savez_compressed(os.path.join(HERE, "hic_fixtures.npz"), **out)
    with open(os.path.join(HERE, "hic_fixtures.json"), "w") as f:
        json.dump(text, f, indent=0)
    print("ok", n_bins, "bins,", len(bin1), "pixels,", os.path.getsize(os.path.join(HERE, "hic_fixtures.npz")), "+",
          os.path.getsize(os.path.join(HERE, "hic_fixtures.json")), "bytes")


if __name__ == "__main__":
    main()
