"""gd_interphase on files whose A/B factors differ (a model and two copies of one control): the libgdyn-linked program batches them as
the replicas of one handle, replica r under file r's factors (include/gdyn_ensemble.h), against the ORACLE-linked one-file program on
a copy of every file; --ensemble-matrix pools per model.  The bounds are test_batched_driver_on_gpu's: positions 2e-4, semiaxes 1e-7."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cmap_gpu import _dataset, needs_h5, progs      # noqa: F401  (progs: the fixture that builds the programs)
from test_ensemble_ab import permute_ab
from test_host_driver import _env, _frames, _inputs, _make_oracle

pytestmark = pytest.mark.gpu


@needs_h5
def test_driver_batches_a_model_and_its_controls(progs, tmp_path, hip, oracle):
    drv_o = _make_oracle("gd_interphase", tmp_path)
    batch, solo = [], []
    for k in range(3):      # their own seeds and initial structures; files 1 and 2 under ONE permutation of file 0's factors
        d = tmp_path / "batch" / f"run{k}"
        d.mkdir(parents=True)
        _, a, b, *_ = _inputs(d, seed=12345 + k, walk_seed=8 + k)
        if k > 0:
            pa, pb = permute_ab(d, 3)
            assert np.mean((pa != a) | (pb != b)) >= 0.25
        s = tmp_path / "solo" / f"run{k}"
        s.mkdir(parents=True)
        shutil.copy(d / "traj.h5", s / "traj.h5")
        batch.append(d)
        solo.append(s)
    for s in solo:
        subprocess.run([str(drv_o), str(s / "traj.h5")], check=True, capture_output=True, env=_env(os.path.join(ROOT, "oracle")))
    files = [str(d / "traj.h5") for d in batch]
    r = subprocess.run([progs["gd_interphase"], "--device", "0", "--ensemble-matrix", "4", str(tmp_path / "gw-{model}.h5"), *files],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    models = [ln for ln in r.stderr.splitlines() if ln.startswith("[model ")]
    assert models == [f"[model 0] file {files[0]}", f"[model 1] file {files[1]} file {files[2]}"], models
    for ds, db in zip(solo, batch):
        fs, fb = _frames(ds), _frames(db)
        assert fs.keys() == fb.keys() and len(fs) == 7
        for key in fs:
            dx = np.abs(fs[key][0] - fb[key][0]).max()
            print(f"  {db.name} {key}: |dx| {dx:.2e}")
            assert dx <= 2e-4, (db.name, key, dx)
            assert np.allclose(fs[key][1]["wall_semiaxes"], fb[key][1]["wall_semiaxes"], rtol=0, atol=1e-7), (db.name, key)
    # (on the oracle alone: factors that were ignored could not pass -- file 1's structure and seed under file 0's factors end ten
    # bounds away from file 1's own run)
    wrong = tmp_path / "wrong"
    wrong.mkdir()
    _inputs(wrong, seed=12345 + 1, walk_seed=8 + 1)
    subprocess.run([str(drv_o), str(wrong / "traj.h5")], check=True, capture_output=True, env=_env(os.path.join(ROOT, "oracle")))
    assert np.abs(_frames(wrong)[("interphase", 60)][0] - _frames(solo[1])[("interphase", 60)][0]).max() > 10 * 2e-4
    # one matrix per model, each what gd_gw_contact_matrix writes from the stored maps of the model's files
    assert sorted(p for p in os.listdir(tmp_path) if p.startswith("gw-")) == ["gw-0.h5", "gw-1.h5"]
    for k, members in enumerate(([files[0]], files[1:])):
        want = tmp_path / f"want-{k}.h5"
        r = subprocess.run([progs["gd_gw_contact_matrix"], "--rebin-rate", "4", "-o", str(want), *members], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for path in ("/contact_matrix", "/metadata/chromosome_ranges", "/metadata/rebin_map"):
            got, exp = _dataset(progs, tmp_path, tmp_path / f"gw-{k}.h5", path), _dataset(progs, tmp_path, want, path)
            assert got.shape == exp.shape and np.array_equal(got, exp), (k, path)
        assert _dataset(progs, tmp_path, want, "/contact_matrix").any()
    assert not np.array_equal(_dataset(progs, tmp_path, tmp_path / "gw-0.h5", "/contact_matrix"),
                              _dataset(progs, tmp_path, tmp_path / "gw-1.h5", "/contact_matrix"))
