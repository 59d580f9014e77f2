"""bench.py's run shapes: a plain run times the steps and prints the line, --full adds the rest of the measurement row,
--dump-outputs writes the state the timed steps left (float32 / float64 .npy, at most 64 MB, identical from run to run)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from util import g

FULL_ONLY_CONFIG = ("steady_state_bead_steps_per_s", "steady_state_steps", "bead_steps_per_s_with_reference_cadence_rank0")
SMALL = ["--beads", "3000", "--replicas", "8", "--equil", "200", "--warmup", "10", "--steps", "40"]


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _FakeSystem:
    """What dump_outputs reads of a handle: R, N, positions() and context(r)."""

    def __init__(self, R, N):
        self.R, self.N = R, N
        self.x = np.random.default_rng(5).normal(size=(R, N, 3))

    def positions(self):
        return self.x.copy()

    def context(self, r):
        c = g.Context()
        c.step, c.time, c.bead_scale, c.bond_scale = 100 + r, 1e-3 * r, 0.5, 0.75
        for k in range(3):
            c.semiaxes[k], c.axial_reaction[k] = 6.0 + r + k, -1.0 * k
        return c


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_replica_in_float32_and_the_contexts(tmp_path):
    bench = _bench_module()
    s = _FakeSystem(4, 500)
    bench.dump_outputs(str(tmp_path), s)
    d = _load_dir(tmp_path)
    assert set(d) == {"positions", "step_time", "bead_bond_scale", "semiaxes", "axial_reaction"}
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert d["positions"].dtype == np.float32 and np.array_equal(d["positions"], s.x.astype(np.float32))
    assert d["step_time"][:, 0].tolist() == [100, 101, 102, 103] and d["semiaxes"][3].tolist() == [9.0, 10.0, 11.0]
    assert d["bead_bond_scale"].tolist() == [[0.5, 0.75]] * 4 and d["axial_reaction"][0].tolist() == [0.0, -1.0, -2.0]


def test_dump_outputs_samples_a_fixed_set_of_rows_above_the_size_limit(tmp_path, monkeypatch):
    bench = _bench_module()
    assert bench.DUMP_LIMIT_BYTES <= 64 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8192)
    s = _FakeSystem(3, 2000)
    sizes, runs = [], []
    for k in range(2):
        out = tmp_path / str(k)
        bench.dump_outputs(str(out), s)
        sizes.append(sum(os.path.getsize(out / f) for f in os.listdir(out)))
        runs.append(_load_dir(out))
    a, b = runs
    assert np.array_equal(a["positions_index"], b["positions_index"]) and np.array_equal(a["positions"], b["positions"])
    idx = a["positions_index"].astype(np.int64)
    assert len(idx) > 100 and np.all(np.diff(idx) > 0) and idx[-1] < 3 * 2000
    assert np.array_equal(a["positions"], s.x.reshape(-1, 3)[idx].astype(np.float32))
    assert max(sizes) <= 8192 + 6 * 128          # (each .npy adds its 128-byte header)


def _bench(*args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                         timeout=timeout, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_every_time(hip, tmp_path):
    lines = [_bench(*SMALL, "--dump-outputs", str(tmp_path / str(k))) for k in range(2)]
    for line in lines:
        assert line["steps"] == 40 and line["warmup"] == 10 and line["unit"] == "bead-steps/s" and line["dtype"] == "f32"
        assert line["value"] == pytest.approx(3000 * 8 * 1e3 / line["ms_per_step"], rel=1e-9)
        assert not {"checked", "cpu_baseline"} & set(line) and not {"other_workloads", *FULL_ONLY_CONFIG} & set(line["config"])
    a, b = _load_dir(tmp_path / "0"), _load_dir(tmp_path / "1")
    assert a["positions"].shape == (8, 3000, 3) and a["positions"].dtype == np.float32 and np.isfinite(a["positions"]).all()
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in os.listdir(tmp_path / "0")) <= 64 << 20
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
def test_full_run_adds_the_steady_state_and_cadence_figures(hip):
    line = _bench(*SMALL, "--full", "--no-cpu-baseline", "--no-extra")
    assert line["steps"] == 40 and all(line["config"][k] > 0 for k in FULL_ONLY_CONFIG)
