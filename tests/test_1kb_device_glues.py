"""`gd_1kb --seeds ... --device-glues`: the glue kinetics of every trajectory of an ensemble in one device call per update
(include/gdyn_glue.h) instead of the host binder.  The traced glue lists are well-formed sets within the capacity, glues form, the
stored frames are the oracle's replay of each trajectory's trace (tests/test_1kb_driver.py's replay, the tolerance of
tests/test_1kb_ensemble.py), and two runs write the same traces byte for byte.  Without --seeds, or linked against a library without
the gd_glue_* symbols, the option is refused before any file exists."""
import os

import numpy as np
import pytest

from conftest import ROOT
from test_1kb_driver import N, STEPS, _config, _replay
from test_1kb_ensemble import _dataset, _run, _write_config
from test_host_driver import _env, _make, _make_oracle

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")
SEEDS = [3, 4]


@pytest.mark.gpu
def test_device_glues_on_gpu(tmp_path, hip, oracle):
    cfg = _write_config(tmp_path)
    max_glues = cfg["glue"]["max_glues"]
    drv = _make("gd_1kb", ".", "../csrc", "gdyn")
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = _run(drv, d, "--seeds", ",".join(map(str, SEEDS)), "--device-glues", "--trace", d / "trace", "-o", "out-{seed}.h5", tmp_path / "config.json")
        assert r.returncode == 0, r.stderr
        runs.append((d, r))
    d, r = runs[0]
    for s in SEEDS:
        tdir = d / "trace" / f"seed-{s}"
        trace = (tdir / "trace.txt").read_text().splitlines()
        assert (runs[1][0] / "trace" / f"seed-{s}" / "trace.txt").read_bytes() == (tdir / "trace.txt").read_bytes(), s      # two runs, one trace
        x0 = np.fromfile(tdir / "init.f64", dtype="<f8").reshape(N, 3)
        frames, energies, events = _replay(oracle, cfg, x0, trace)
        glues = [p for st in sorted(events) for w, p in events[st] if w == "glues"]
        assert len(glues) == STEPS // cfg["sampling"]["glue_update_interval"] + 1
        for p in glues:
            keys = (p[:, 0].astype(np.int64) << 32) | p[:, 1]
            assert len(p) <= max_glues and np.all(p[:, 0] < p[:, 1]) and np.all(np.diff(keys) > 0)      # i < j, sorted, unique
        assert max(len(p) for p in glues) > 0                                        # glues formed in this trajectory
        assert len({tuple(map(tuple, p)) for p in glues}) > 2                        # and turned over
        pos = _dataset(d / f"out-{s}.h5", "/positions_history", tmp_path / "ds.f64")
        assert pos.shape == (STEPS // 20 + 1, N, 3)
        for k, want in enumerate(frames):
            err = np.abs(pos[k] - want.astype(np.float64)).max()
            assert err <= 5e-4, (s, k, err)
        # the G: figure of the log is the size of the list uploaded before
        logs = [ln[len(f"[seed {s}] "):].split("\t") for ln in r.stderr.splitlines() if ln.startswith(f"[seed {s}] ")]
        assert [int(f[0]) for f in logs] == list(range(0, STEPS + 1, 10)), s
        sizes = {st: len(p) for st in events for w, p in events[st] if w == "glues"}
        for f in logs[1:]:
            assert float(f[3][3:]) == pytest.approx(sizes[int(f[0]) - 10] / N, rel=1e-5), (s, f)
    a = (d / "trace" / "seed-3" / "trace.txt").read_text().splitlines()
    b = (d / "trace" / "seed-4" / "trace.txt").read_text().splitlines()
    assert [ln for ln in a if ln.startswith("glues")] != [ln for ln in b if ln.startswith("glues")]      # the seeds' sets differ
    # one seed is allowed, and runs through the same path
    one = tmp_path / "one"
    r1 = _run(drv, one, "--seeds", "3", "--device-glues", "--trace", one / "trace", "-o", "out-{seed}.h5", tmp_path / "config.json")
    assert r1.returncode == 0, r1.stderr
    assert (one / "out-3.h5").exists() and any(ln.startswith("glues") for ln in (one / "trace" / "seed-3" / "trace.txt").read_text().splitlines())
    # without --seeds: refused, nothing written
    r2 = _run(drv, tmp_path / "none", "--device-glues", "-o", "out.h5", tmp_path / "config.json")
    assert r2.returncode == 1 and "--device-glues needs --seeds" in r2.stderr, r2.stderr
    assert not list((tmp_path / "none").iterdir())


def test_device_glues_option_on_the_oracle_linked_program(tmp_path):
    """Linked against a library without gd_glue_*: the program builds, and the option is refused with a message, before any output."""
    _write_config(tmp_path)
    drv = _make_oracle("gd_1kb", tmp_path)
    env = _env(os.path.join(ROOT, "oracle"))
    config = tmp_path / "config.json"
    for k, seeds in enumerate(("3,4", "3")):
        r = _run(drv, tmp_path / f"a{k}", "--seeds", seeds, "--device-glues", "--trace", tmp_path / f"a{k}" / "trace", "-o", "out-{seed}.h5", config, env=env)
        assert r.returncode == 1 and "device glue kinetics" in r.stderr and "gd_glue_" in r.stderr, r.stderr
        assert not list((tmp_path / f"a{k}").iterdir())
    r = _run(drv, tmp_path / "b", "--device-glues", "-o", "out.h5", config, env=env)
    assert r.returncode == 1 and "--device-glues needs --seeds" in r.stderr, r.stderr
    assert not list((tmp_path / "b").iterdir())
    r = _run(drv, tmp_path / "c", "-h", env=env)
    assert r.returncode == 0 and "--device-glues" in r.stderr
    # without the option the program runs as before
    r = _run(drv, tmp_path / "d", "--seeds", "3", "-o", "out-{seed}.h5", config, env=env)
    assert r.returncode == 0 and (tmp_path / "d" / "out-3.h5").exists(), r.stderr
