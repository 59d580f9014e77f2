#!/usr/bin/env python3
"""Generates tests/golden/lamina_fixtures.npz by IMPORTING the reference's own 5-sim-genome/src/analyze_lamina in this
container -- geometry.py (Ellipsoid.distance_from_surface) and command.py (analyze_distances_history) -- and recording
their outputs for fixed inputs.  Only arrays are stored.  geometry.py was written for numpy < 1.24 (`np.float`): the alias
is provided for the import.  command.py imports h5py, which this image lacks: an empty stand-in module is placed in
sys.modules for the import only; analyze_distances_history itself touches no h5py name and is run over small dict-like
snapshot objects.  analyze_contact_uniform needs a real HDF5 file, so its three lines (`<`, the float32 `+=`, `/=`) are
restated here with numpy on the reference's distances.  Nothing of the reference is changed.
Run here:  python tests/golden/make_lamina_fixtures.py"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if not hasattr(np, "float"):
    np.float = float          # the numpy the reference was written for had this alias
sys.path.insert(0, "/root/reference/5-sim-genome/src")
_stand_in = "h5py" not in sys.modules
if _stand_in:
    sys.modules["h5py"] = types.ModuleType("h5py")
from analyze_lamina import command, geometry      # noqa: E402
if _stand_in:
    del sys.modules["h5py"]

SEMIAXES = [(5.0, 5.0, 5.0), (6.15, 5.2, 4.47), (8.0, 8.0, 1.5), (1.3, 0.7, 1.1)]      # sphere, the nucleus, strongly oblate, small


class _Scalar:          # dataset[()] of a scalar string dataset
    def __init__(self, value):
        self.value = value

    def __getitem__(self, key):
        assert key == ()
        return self.value


def _points(rng, semi, n):
    """float32 points inside, near, on and outside the wall, the origin, and far ones (NaN for anisotropic walls)."""
    semi = np.asarray(semi)
    v = rng.normal(size=(6 * n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    scale = np.concatenate([rng.uniform(0.0, 0.9, n), rng.uniform(0.98, 1.02, n), np.ones(n), rng.uniform(1.05, 1.4, n),
                            rng.uniform(2.0, 12.0, 2 * n)])
    pts = v * semi[None, :] * scale[:, None]
    axes = np.concatenate([np.diag(semi), -np.diag(semi), np.zeros((1, 3)), np.diag(semi) * 0.5])
    return np.concatenate([axes, pts]).astype(np.float32)


def _snapshots(frames, semiaxes):
    snaps = {".steps": [str(100 * f) for f in range(len(frames))]}
    for f, (x, s) in enumerate(zip(frames, semiaxes)):
        context = {"time": 0.1 * f, "bead_scale": 1.0, "bond_scale": 1.0, "wall_semiaxes": [float(t) for t in s], "mean_energy": 0.0,
                   "wall_energy": 0.0}
        snaps[str(100 * f)] = {"context": _Scalar(json.dumps(context)), "positions": x}
    return snaps


def main():
    rng = np.random.default_rng(20220405)
    out = {}
    nan_total = 0
    for k, semi in enumerate(SEMIAXES):
        pts = _points(rng, semi, 40)
        with np.errstate(invalid="ignore"):
            d32 = geometry.Ellipsoid(semi).distance_from_surface(pts)
            pts64 = pts.astype(np.float64) + rng.normal(scale=1e-9, size=pts.shape)       # not representable in float32
            pts64[6] = 0.0                                                                 # the origin again
            d64 = geometry.Ellipsoid(semi).distance_from_surface(pts64)
        assert d32.dtype == np.float64 and d32[6] == 0.0 and d64[6] == 0.0 and not pts[6].any()
        nan_total += int(np.isnan(d32).sum())
        out[f"semi{k}"] = np.array(semi)
        out[f"points{k}"], out[f"dist{k}"] = pts, d32
        out[f"points64_{k}"], out[f"dist64_{k}"] = pts64, d64
    assert nan_total > 0, "no point gives NaN"
    out["n_sets"] = np.array(len(SEMIAXES))

    # histories through command.py: semiaxes that change from frame to frame, three trajectories of one shape
    F, N = 6, 50
    hists = []
    for t in range(3):
        semis = np.array([(6.15 - 0.07 * f, 5.2 + 0.05 * f * (t + 1), 4.47 - 0.02 * f) for f in range(F)])
        frames = np.stack([_points(rng, semis[f], 8)[:N] for f in range(F)])
        with np.errstate(invalid="ignore"):
            dist, scales = command.analyze_distances_history(_snapshots(frames, semis))
        assert dist.shape == (F, N) and dist.dtype == np.float64 and scales.shape == (F,)
        out[f"hist_semi{t}"], out[f"hist_points{t}"], out[f"hist_dist{t}"] = semis, frames, dist
        hists.append(dist.astype(np.float32))      # `dataset[...] = distances_history` into a float32 dataset
    out["n_hist"] = np.array(len(hists))

    # the contact lines of analyze_contact_uniform, restated: thresholds below every stored value but 0, at stored values
    # (strict <), typical and above everything
    finite = np.sort(hists[0][np.isfinite(hists[0])])
    thresholds = np.array([0.0, float(finite[len(finite) // 3]), float(hists[1][2, 20]), 0.3, 1.0, float(finite[-1]), 1e9])
    out["thresholds"] = thresholds
    for j, D in enumerate(thresholds):
        D = float(D)
        average = None
        for t, distances_history in enumerate(hists):
            with np.errstate(invalid="ignore"):
                contacts_history = distances_history < D
            out[f"contact{j}_{t}"] = contacts_history
            if average is None:
                average = np.zeros(contacts_history.shape, dtype=np.float32)
            average += contacts_history
        average /= len(hists)
        out[f"average{j}"] = average
    np.savez_compressed(os.path.join(HERE, "lamina_fixtures.npz"), **out)
    print("ok", len(out), "arrays,", nan_total, "NaN distances, EPSILON", geometry.EPSILON,
          os.path.getsize(os.path.join(HERE, "lamina_fixtures.npz")), "bytes")


if __name__ == "__main__":
    main()
