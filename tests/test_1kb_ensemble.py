"""`gd_1kb --seeds s0,s1,...`: an ensemble of 1 kb trajectories as the replicas of one handle, each with its own generator, kinetics,
per-replica loop / glue lists (include/gdyn_replica.h), output file and trace.  Replica r must be the trajectory `-s s_r` starts: its
host-side draws are compared byte for byte with the oracle-linked single run's, its frames and energies with a call-by-call replay
of its trace on the oracle (tests/test_1kb_driver.py's).  The oracle library has no per-replica lists: linked against it the program
still builds, runs single seeds unchanged and refuses an ensemble."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_1kb_driver import LENGTHS, N, STEPS, _config, _replay
from test_host_driver import _env, _make, _make_oracle, _tool

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")
SEEDS = [3, 4, 5]


def _write_config(tmp):
    cfg = _config(tmp)
    (tmp / "config.json").write_text(json.dumps(cfg, indent=1))
    return cfg


def _run(driver, cwd, *args, env=None):
    cwd.mkdir(exist_ok=True)
    return subprocess.run([str(driver), *map(str, args)], capture_output=True, text=True, env=env, cwd=cwd)


def _dataset(file, path, scratch):
    shape = [int(v) for v in _tool("dataset", file, path, scratch).split()]
    return np.fromfile(scratch, dtype="<f8").reshape(shape)


def _layout(file):
    """Datasets, shapes and types of an output file: h5dump's header without the line that names the file"""
    return subprocess.check_output(["/opt/conda/bin/h5dump", "-H", str(file)], text=True).splitlines()[1:]


def _dump(file):
    """The whole content of an output file as h5dump prints it, without the line that names the file"""
    out = subprocess.check_output(["/opt/conda/bin/h5dump", str(file)], text=True).splitlines()[1:]
    assert any("positions_history" in ln for ln in out) and len(out) > 1000
    return out


@pytest.mark.gpu
def test_ensemble_of_three_seeds_on_gpu(tmp_path, hip, oracle):
    cfg = _write_config(tmp_path)
    drv = _make("gd_1kb", ".", "../csrc", "gdyn")
    ens = tmp_path / "ens"
    r = _run(drv, ens, "--seeds", ",".join(map(str, SEEDS)), "--trace", ens / "trace", "-o", "out-{seed}.h5", tmp_path / "config.json")
    assert r.returncode == 0, r.stderr
    odrv = _make_oracle("gd_1kb", tmp_path)
    oenv = _env(os.path.join(ROOT, "oracle"))
    kb2 = 0.5 * cfg["loop"]["bond_spring"] * cfg["chain"]["repulsive_diameter"] ** 2
    for s in SEEDS:
        # the host path of `-s s`: initial positions, integrator seed and the preloaded loops, byte for byte
        one = tmp_path / f"single-{s}"
        (one / "trace").mkdir(parents=True)
        r1 = _run(odrv, one, "-s", s, "--trace", one / "trace", "-o", f"out-{s}.h5", tmp_path / "config.json", env=oenv)
        assert r1.returncode == 0, r1.stderr
        tdir = ens / "trace" / f"seed-{s}"
        assert (tdir / "init.f64").read_bytes() == (one / "trace" / "init.f64").read_bytes()
        trace = (tdir / "trace.txt").read_text().splitlines()
        single = (one / "trace" / "trace.txt").read_text().splitlines()
        for key in ("seed ", "loops -1 "):
            mine, ref = [ln for ln in trace if ln.startswith(key)], [ln for ln in single if ln.startswith(key)]
            assert len(ref) == 1 and mine == ref, (s, key)
        # the single-run layout of the output file
        assert _layout(ens / f"out-{s}.h5") == _layout(one / f"out-{s}.h5"), s
        # frames and energies against the replay of this seed's trace on the oracle
        x0 = np.fromfile(tdir / "init.f64", dtype="<f8").reshape(N, 3)
        frames, energies, events = _replay(oracle, cfg, x0, trace)
        pos = _dataset(ens / f"out-{s}.h5", "/positions_history", tmp_path / "ds.f64")
        loops = _dataset(ens / f"out-{s}.h5", "/loops_history", tmp_path / "ds.f64").astype(np.int64)
        assert pos.shape == (STEPS // 20 + 1, N, 3) and loops.shape == (STEPS // 20 + 1, 24, 3)
        for k, want in enumerate(frames):
            err = np.abs(pos[k] - want.astype(np.float64)).max()
            assert err <= 5e-4, (s, k, err)
        logs = [ln[len(f"[seed {s}] "):].split("\t") for ln in r.stderr.splitlines() if ln.startswith(f"[seed {s}] ")]
        assert [int(f[0]) for f in logs] == list(range(0, STEPS + 1, 10)), s
        for k in range(loops.shape[0]):
            step = 20 * k
            active = loops[k][loops[k][:, 2] > 0][:, :2]
            zero = int((active[:, 0] == active[:, 1]).sum())
            f = [f for f in logs if int(f[0]) == step][0]
            assert float(f[1][3:]) == pytest.approx(energies[step] + zero * kb2 / N, rel=2e-2, abs=1e-3), (s, step)
            assert float(f[2][3:]) == pytest.approx(len(active) / N, rel=1e-5)
        assert max(len(p) for st in events for w, p in events[st] if w == "glues") > 0          # glues formed in this trajectory
    # the trajectories differ
    a = _dataset(ens / "out-3.h5", "/positions_history", tmp_path / "ds.f64")
    b = _dataset(ens / "out-4.h5", "/positions_history", tmp_path / "ds.f64")
    assert np.abs(a - b).max() > 1e-2
    assert sum(LENGTHS) == N


def test_seeds_option_on_the_oracle_linked_program(tmp_path):
    """Linked against a library without gd_replica_*: builds, one seed is -s, several are refused, bad lists exit 1 with a message."""
    _write_config(tmp_path)
    drv = _make_oracle("gd_1kb", tmp_path)
    env = _env(os.path.join(ROOT, "oracle"))
    config = tmp_path / "config.json"
    r = _run(drv, tmp_path / "a", "--seeds", "3,4", "-o", "out-{seed}.h5", config, env=env)
    assert r.returncode == 1 and "per-replica dynamic pair lists" in r.stderr and "gd_replica_pairs" in r.stderr, r.stderr
    assert not list((tmp_path / "a").iterdir())                                     # refused before any output
    r1 = _run(drv, tmp_path / "b", "--seeds", "3", "-o", "out-{seed}.h5", config, env=env)
    r2 = _run(drv, tmp_path / "c", "-s", "3", "-o", "out-3.h5", config, env=env)
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert r1.stderr == r2.stderr and r1.stderr.startswith("0\tE: ")
    # byte for byte: every dataset's type, shape and values in h5dump's full dump.  (The raw files differ in the object modification
    # times the HDF5 library stamps, in seconds, whenever the clock ticks between the two runs.)
    assert _dump(tmp_path / "b" / "out-3.h5") == _dump(tmp_path / "c" / "out-3.h5")
    for args, message in ((["--seeds", "3,3", "-o", "out-{seed}.h5"], "listed twice"),
                          (["--seeds", "", "-o", "out-{seed}.h5"], "--seeds takes"),
                          (["--seeds", "3,x", "-o", "out-{seed}.h5"], "--seeds takes"),
                          (["--seeds", "3,4", "-o", "plain.h5"], "must contain {seed}"),
                          (["--seeds", "3,4"], "must contain {seed}"),               # the config's own output name has no placeholder
                          (["--seeds", "3", "-s", "3", "-o", "out-{seed}.h5"], "exclude each other")):
        r = _run(drv, tmp_path / "d", *args, config, env=env)
        assert r.returncode == 1 and message in r.stderr, (args, r.stderr)
        assert not list((tmp_path / "d").iterdir()), args
