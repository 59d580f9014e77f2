#!/usr/bin/env python3
"""Generates tests/golden/cmap_fixtures.npz by IMPORTING the reference's own 5-sim-genome/src/{contact_map, gw_contact_matrix,
nad_profile, power_law} in this container and recording the outputs of collect_contact_matrix, determine_rebin_map,
load_contact_matrix_into / collect_contacts, collect_nucleolus_contacts, compute_contact_profile / collect_contact_profile and
fit_power_law for a toy genome.  Only arrays are stored.  The image has scipy and sklearn but neither h5py nor numba, so
stand-ins are placed in sys.modules for the import: an `h5py` with enum_dtype / check_dtype (the enum travels in the dtype's
metadata) and a File() that hands out the in-memory stores below, and a `numba` whose jit is the identity.  The stores are
dict-like groups that resolve "a/b" paths and have .file; their datasets are numpy arrays with .chunks, .shape, .attrs, .dtype
and __len__.  Nothing of the reference is changed.
Run here:  python tests/golden/make_cmap_fixtures.py"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

STORES = {}


class Dataset:
    def __init__(self, data, chunks=None, attrs=None, dtype=None):
        self.data = np.asarray(data)
        self.chunks = chunks
        self.attrs = attrs or {}
        self.dtype = dtype if dtype is not None else self.data.dtype
        self.shape = self.data.shape

    def __len__(self):
        return len(self.data)

    def __getitem__(self, key):
        return self.data[key]

    def __iter__(self):
        return iter(self.data)


class Group(dict):
    file = None

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
    h5py.enum_dtype = lambda names, basetype: np.dtype(basetype, metadata={"enum": dict(names)})
    h5py.check_dtype = lambda enum: enum.metadata["enum"]
    h5py.File = lambda name, mode="r": STORES[name]
    numba = types.ModuleType("numba")
    numba.jit = lambda f: f
    sys.modules["h5py"], sys.modules["numba"] = h5py, numba
    return h5py


H5PY = _install_stand_ins()
sys.path.insert(0, "/root/reference/5-sim-genome/src")
from contact_map import contact_map as ref_map          # noqa: E402
from gw_contact_matrix import command as ref_gw         # noqa: E402
from nad_profile import nad_profile as ref_nad          # noqa: E402
from power_law import power_law as ref_pl               # noqa: E402

TYPE_ENUM = {"active_NOR": 5, "silent_NOR": 6, "centromere": 4, "A": 1, "B": 2, "u": 3, "nucleolus": 7}
# three homolog pairs of equal sizes, two beads between the first and the second pair that belong to no chromosome, and twelve
# nucleolar beads after the chromatin
NAMES = ["chr1:a", "chr1:b", "chr2:a", "chr2:b", "chr3:a", "chr3:b"]
RANGES = np.array([(0, 40), (40, 80), (82, 112), (112, 142), (142, 165), (165, 188)], np.int32)
N_CHROMATIN, N_PARTICLES = 188, 200
STEPS = [0, 10, 20, 30, 40, 50, 60, 70]
WITH_MAP = [{10, 20, 40, 60, 70}, {0, 20, 30, 50, 70}, {20, 40, 60}]           # per file
WINDOWS = [(-1, -1), (50, -1), (-1, 20), (50, 20), (45, 25)]                      # (before, after); -1: None
FRAME_RANGES = [(0, 0, 0), (1, 1, 0), (1, -3, 0), (2, 1, 4), (2, 0, -1), (2, -5, -2)]      # (tokens, a, b): 0 tokens = whole
REBIN_RATES = [1, 4, 7]


def _frame_rows(rng, m):
    """m unique rows (i, j, count), sorted by i then j: mostly near the diagonal, either order of i and j, a few i == j, and
    rows that touch the gap beads and the nucleolar ones."""
    i = rng.integers(0, N_PARTICLES, size=4 * m)
    near = rng.random(4 * m) < 0.7
    j = np.where(near, np.clip(i + rng.integers(-6, 7, size=4 * m), 0, N_PARTICLES - 1), rng.integers(0, N_PARTICLES, size=4 * m))
    nuc = rng.random(4 * m) < 0.15
    j = np.where(nuc, rng.integers(N_CHROMATIN, N_PARTICLES, size=4 * m), j)
    pairs = np.unique(np.stack([i, j], axis=1), axis=0)
    pairs = pairs[np.sort(rng.choice(len(pairs), size=m, replace=False))]
    flip = rng.random(m) < 0.2
    pairs[flip] = pairs[flip][:, ::-1]
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return np.concatenate([pairs, rng.integers(1, 6, size=(m, 1))], axis=1).astype(np.uint32)


def _store(name, frames, chunks):
    types_ = np.full(N_PARTICLES, 1, np.int8)
    types_[::3] = 2
    types_[80:82] = 3
    types_[N_CHROMATIN:] = TYPE_ENUM["nucleolus"]
    root = Group()
    meta = Group()
    meta["particle_types"] = Dataset(types_, dtype=H5PY.enum_dtype(TYPE_ENUM, np.int8))
    meta["chromosome_ranges"] = Dataset(RANGES, attrs={"keys": json.dumps({n: k for k, n in enumerate(NAMES)})})
    phase = Group()
    phase.file = root
    phase[".steps"] = [str(s) for s in STEPS]
    for s in STEPS:
        snap = Group()
        snap["positions"] = Dataset(np.zeros((N_PARTICLES, 3), np.float32))
        if s in frames:
            rows = frames[s]
            snap["contact_map"] = Dataset(rows, chunks=chunks(len(rows)))
        phase[str(s)] = snap
    root["metadata"] = meta
    root["snapshots"] = Group(interphase=phase)
    STORES[name] = root
    return root


def _none(v):
    return None if v < 0 else int(v)


def main():
    rng = np.random.default_rng(20220406)
    out = {"ranges": RANGES, "n_particles": np.array(N_PARTICLES), "steps": np.array(STEPS), "windows": np.array(WINDOWS),
           "frame_ranges": np.array(FRAME_RANGES), "rebin_rates": np.array(REBIN_RATES), "n_files": np.array(len(WITH_MAP)),
           "nucleolus_value": np.array(TYPE_ENUM["nucleolus"])}
    frames = []
    for f, with_map in enumerate(WITH_MAP):
        frames.append({s: _frame_rows(rng, 500 + 40 * f) for s in sorted(with_map)})
        out[f"map_steps{f}"] = np.array(sorted(with_map))
        for s, rows in frames[f].items():
            out[f"rows{f}_{s}"] = rows
    # three layouts of the same data: HDF5 chunks of 128 rows, one row per chunk, and contiguous (the reference then reads
    # 1024 * 1024 rows at a time)
    chunked = [_store(f"chunked{f}", frames[f], lambda m: (128, 3)) for f in range(len(frames))]
    by_row = [_store(f"by_row{f}", frames[f], lambda m: (1, 3)) for f in range(len(frames))]
    whole = [_store(f"whole{f}", frames[f], lambda m: None) for f in range(len(frames))]
    out["particle_types"] = chunked[0]["metadata/particle_types"][:]

    # contact_map: collect_contact_matrix per (file, chromosome, window)
    for f, store in enumerate(chunked):
        for c, (beg, end) in enumerate(RANGES):
            for w, (before, after) in enumerate(WINDOWS):
                m = ref_map.collect_contact_matrix(store["snapshots/interphase"], before=_none(before), after=_none(after), chain=(beg, end))
                m = np.asarray(m)
                assert m.shape == (end - beg, end - beg) and np.array_equal(m, m.T)
                assert np.array_equal(m, np.asarray(ref_map.collect_contact_matrix(whole[f]["snapshots/interphase"], before=_none(before),
                                                                                    after=_none(after), chain=(beg, end))))
                out[f"region{f}_{c}_{w}"] = m.astype(np.int64)

    # nad_profile: with one row per chunk the fancy-index += of the reference is the true sum; with larger chunks it keeps
    # one row per repeated index
    differ = 0
    for f in range(len(frames)):
        for c, (beg, end) in enumerate(RANGES):
            for w, (before, after) in enumerate(WINDOWS):
                args = dict(before=_none(before), after=_none(after), chain=(beg, end))
                true = ref_nad.collect_nucleolus_contacts(by_row[f]["snapshots/interphase"], **args)
                lossy = ref_nad.collect_nucleolus_contacts(whole[f]["snapshots/interphase"], **args)
                assert true.dtype == np.int32 and (true >= lossy).all()
                differ += int((true != lossy).any())
                out[f"nad{f}_{c}_{w}"] = true
                out[f"nad_default_chunks{f}_{c}_{w}"] = lossy
    assert differ > 0

    # gw_contact_matrix: determine_rebin_map of the first input, load_contact_matrix_into over every input
    inputs = [f"chunked{f}" for f in range(len(frames))]
    for rate in REBIN_RATES:
        rebin, binned = ref_gw.determine_rebin_map(chunked[0], rate)
        assert binned.dtype.metadata["enum"] == {n: k for k, n in enumerate(NAMES)}
        out[f"rebin_map{rate}"], out[f"binned_ranges{rate}"] = rebin, np.asarray(binned, np.int32)
        n_bins = binned.max()
        for r, (tokens, a, b) in enumerate(FRAME_RANGES):
            frame_range = None if tokens == 0 else (int(a), None) if tokens == 1 else (int(a), int(b))
            matrix = np.zeros((n_bins, n_bins), dtype=np.int32)
            assert list(ref_gw.load_contact_matrix_into(inputs, matrix, rebin, frame_range=frame_range)) == [0, 1, 2]
            out[f"gw{rate}_{r}"] = matrix

    # power_law: the profile of the last frame with a map, per file
    for f, store in enumerate(chunked):
        profile = ref_pl.compute_contact_profile(store)
        assert profile.dtype == np.int32 and len(profile) == 40
        out[f"separation{f}"] = profile

    # the fit needs separations up to 1500: one chain of 1600 beads and 60 nucleolar ones, contact counts falling as a power
    # of the separation
    n_chain = 1600
    sep = np.minimum((rng.pareto(0.9, size=40000) + 1).astype(np.int64), n_chain - 1)
    i = rng.integers(0, n_chain - sep)
    pairs = np.unique(np.stack([i, i + sep], axis=1), axis=0)
    other = np.stack([rng.integers(0, n_chain + 60, size=300), rng.integers(n_chain, n_chain + 60, size=300)], axis=1)
    pairs = np.unique(np.concatenate([pairs, other]), axis=0)
    rows = np.concatenate([pairs, rng.integers(1, 4, size=(len(pairs), 1))], axis=1).astype(np.uint32)
    long_store = Group()
    long_store["metadata"] = Group(particle_types=Dataset(np.zeros(n_chain + 60, np.int8)), chromosome_ranges=Dataset(np.array([(0, n_chain)], np.int32)))
    long_phase = Group({".steps": ["5", "15"], "5": Group(contact_map=Dataset(rows, chunks=(1000, 3))), "15": Group()})
    long_store["snapshots"] = Group(interphase=long_phase)
    profile = ref_pl.compute_contact_profile(long_store)
    distances = np.arange(len(profile))
    exponents = [ref_pl.fit_power_law(distances[a:b], profile[a:b])[0] for a, b in (ref_pl.NEAR_RANGE, ref_pl.LONG_RANGE, ref_pl.FAR_RANGE)]
    assert len(profile) == n_chain and (profile[100:1500] == 0).any() and (profile[100:1500] > 0).sum() > 50
    out["long_rows"], out["long_profile"], out["long_exponents"] = rows, profile, np.array(exponents, np.float64)
    out["long_n_particles"] = np.array(n_chain + 60)
    out["fit_ranges"] = np.array([ref_pl.NEAR_RANGE, ref_pl.LONG_RANGE, ref_pl.FAR_RANGE])

    np.savez_compressed(os.path.join(HERE, "cmap_fixtures.npz"), **out)
    print("ok", len(out), "arrays,", differ, "NAD profiles that depend on the chunk layout, exponents", exponents,
          os.path.getsize(os.path.join(HERE, "cmap_fixtures.npz")), "bytes")


if __name__ == "__main__":
    main()
