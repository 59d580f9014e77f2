"""The C++ host side above the C-ABI: trajectory store in the reference's HDF5 layout and
the drivers `gd_interphase` (relaxation + interphase phases, logging cadence, contact map), `gd_spindle`
(coarse-grained spindle + packing phases) and `gd_fine_sampling` (deterministic continuation).  The driver is
backend-agnostic C++; the CPU test links it against the oracle library, the GPU test against libgdyn, and both
compare the files it writes with the same sequence of ABI calls issued from Python."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from util import Mt64 as _Mt64, g, mt64 as _mt64, wl

HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
H5DUMP = "/opt/conda/bin/h5dump"
pytestmark = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")

N, RELAX, INTER = 600, 40, 60


def _make(name, outdir, libdir, lib):
    """Builds the tools; `outdir` may lie outside the product tree (the oracle-linked test binaries)."""
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool"])
    subprocess.check_call(["make", "-s", "-C", HOST, f"{outdir}/{name}", f"OUTDIR={outdir}", f"GDYN_LIBDIR={libdir}", f"GDYN_LIB={lib}"])
    return os.path.join(HOST, outdir, name)


def _make_oracle(name, tmp):
    return _make(name, str(tmp), os.path.join(ROOT, "oracle"), "oracle")


def _env(*libdirs):
    return dict(os.environ, LD_LIBRARY_PATH=":".join([os.path.join(HOST, "h5lib"), *map(str, libdirs), os.environ.get("LD_LIBRARY_PATH", "")]))


def _config(radius):
    c = dict(wl.DEFAULT_CONFIG)
    c.update(a_core_diameter=0.30, b_core_diameter=0.24, a_core_bond_spring=70.0, a_core_bond_length=0.2,
             b_core_bond_spring=70.0, b_core_bond_length=0.2, a_core_2nd_bond_spring=5.0, b_core_2nd_bond_spring=5.0,
             wall_init_semiaxes=[radius] * 3, bead_scale_init=0.8, bond_scale_init=0.9,
             relaxation_steps=RELAX, relaxation_sampling_interval=20, relaxation_logging_interval=10,
             interphase_steps=INTER, interphase_sampling_interval=20, interphase_logging_interval=10,
             contactmap_update_interval=10, contactmap_thinning_rate=1, interphase_seed=12345)
    return c


NUC = (540, 600)           # nucleolar particles of the droplet variant: the last 60 beads; bonded to "NOR" beads 100..159


def _inputs(tmp, droplet=False, seed=None, walk_seed=8):
    rng = np.random.default_rng(7)
    lens = wl.chain_lengths(N)
    a, b = wl.ab_types(N, rng)
    radius = 0.27 * (N / (8 * 0.3)) ** (1 / 3)
    x0 = wl.confined_random_walks(lens, radius, 0.2, np.random.default_rng(walk_seed))
    cfg = _config(radius)
    if seed is not None:
        cfg["interphase_seed"] = seed
    if droplet:
        cfg.update(nucleolus_droplet_energy=0.6, nucleolus_droplet_decay=0.2, nucleolus_droplet_cutoff=0.4, nucleolus_mobility=0.7,
                   nucleolus_bond_spring=5.0, nucleolus_bond_length=0.1)
    (tmp / "config.json").write_text(json.dumps(cfg))
    st = 0
    rows, ranges = [], []
    for k, n in enumerate(lens):
        rows.append(f"chr{k + 1} {st} {st + n} {st + n // 2} {st + n // 2 + 1}")
        ranges.append((st, st + int(n)))
        st += int(n)
    (tmp / "chroms.tsv").write_text("\n".join(rows) + "\n")
    np.stack([a, b], axis=1).astype("<f8").tofile(tmp / "ab.f64")
    x0.astype("<f8").tofile(tmp / "pos.f64")
    extra = []
    if droplet:     # the nucleolar beads are not part of any chromosome: shorten the last chains' table entries accordingly
        rows2, ranges2 = [], []
        for row, (b0, b1) in zip(rows, ranges):
            if b0 >= NUC[0]:
                continue
            b1 = min(b1, NUC[0])
            f = row.split()
            rows2.append(f"{f[0]} {b0} {b1} {b0 + (b1 - b0) // 2} {b0 + (b1 - b0) // 2 + 1}")
            ranges2.append((b0, b1))
        rows, ranges = rows2, ranges2
        (tmp / "chroms.tsv").write_text("\n".join(rows) + "\n")
        bonds = np.array([[100 + k, NUC[0] + k] for k in range(NUC[1] - NUC[0])], dtype="<u4")
        bonds.tofile(tmp / "nbonds.u32")
        np.array([NUC], dtype="<u4").tofile(tmp / "nranges.u32")
        extra = [str(tmp / "nbonds.u32"), str(tmp / "nranges.u32")]
    subprocess.check_call([os.path.join(HOST, "gd_h5tool"), "make-input", str(tmp / "traj.h5"), str(tmp / "config.json"),
                           str(tmp / "chroms.tsv"), str(tmp / "ab.f64"), str(tmp / "pos.f64"), *extra])
    return cfg, a, b, x0, ranges, radius


def _tool(*args):
    return subprocess.check_output([os.path.join(HOST, "gd_h5tool"), *map(str, args)], text=True)


def _positions(tmp, phase, step):
    _tool("positions", tmp / "traj.h5", phase, step, tmp / "out.f64")
    return np.fromfile(tmp / "out.f64", dtype="<f8").reshape(-1, 3)


def test_async_writer_and_thread_pool_selftest():
    """gd_async_io.hpp: jobs run in submission order behind a bounded queue, drain() fences, a job's exception reaches the
    submitting thread and the writer stays usable; the pool runs every index exactly once and rethrows a task's exception."""
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool"])
    assert _tool("io-selftest").startswith("io-selftest ok")


@pytest.mark.parametrize("rows", [0, 1, 5000, 87381, 87382, 400001])
def test_hand_packed_chunks_read_back_like_the_library_pipeline(tmp_path, rows):
    """Batched drivers deflate their chunks on a thread pool and hand them to the file as they are (H5Dwrite_chunk): the datasets
    must read back exactly like ones written through the library's shuffle + deflate pipeline, with the same chunking and filter
    list -- empty, one row, one partial chunk, exactly one 1 MiB chunk, one row more, several chunks with a padded last one."""
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool"])
    out = _tool("packed-check", tmp_path / "p.h5", rows)
    assert out.startswith("packed-check ok")
    if rows == 400001 and os.path.exists("/opt/conda/bin/h5dump"):
        hdr = subprocess.check_output(["/opt/conda/bin/h5dump", "-H", "-p", str(tmp_path / "p.h5")], text=True)
        assert hdr.count("COMPRESSION DEFLATE { LEVEL 6 }") == 4 and hdr.count("PREPROCESSING SHUFFLE") == 4


def _python_driver(lib, oracle, cfg, a, b, x0q, ranges, droplet=False):
    """The same ABI call sequence as gd_interphase.cpp, issued from Python; returns {(phase, step): (positions, context)}."""
    s = g.System(lib, N, 1)
    mob = np.full(N, cfg["chromatin_mobility"])
    if droplet:
        mob[NUC[0]:] = 1.0                          # particles outside every chromosome keep the default mobility ...
        mob[NUC[0]:NUC[1]] = cfg["nucleolus_mobility"]      # ... nucleolar ones get theirs (simulation_driver_particles.cc:28-35)
    s.set_bead_params(a=a, b=b, mobility=mob)
    s.set_pair_softcore(cfg["a_core_repulsion"], cfg["a_core_diameter"], cfg["b_core_repulsion"], cfg["b_core_diameter"], 2, 3, 8, 3,
                        mix=True, scale_by_bead_scale=True)
    chain = g.System.bond_params(g.POT_SEMISPRING, k_a=cfg["a_core_bond_spring"], l_a=cfg["a_core_bond_length"],
                                 k_b=cfg["b_core_bond_spring"], l_b=cfg["b_core_bond_length"], mix=True, scale_by_bond_scale=True)
    loop = g.System.bond_params(g.POT_HARMONIC, k_a=cfg["a_core_2nd_bond_spring"], k_b=cfg["b_core_2nd_bond_spring"], mix=True,
                                scale_by_bond_scale=True)
    for (b0, b1) in ranges:
        s.add_bond_range(chain, b0, b1, 1)
        s.add_bond_range(loop, b0, b1, 2)
    if droplet:
        nuc = g.System.bond_params(g.POT_SEMISPRING, k_a=cfg["nucleolus_bond_spring"], l_a=cfg["nucleolus_bond_length"], scale_by_bond_scale=True)
        s.add_bond_pairs(nuc, np.array([[100 + k, NUC[0] + k] for k in range(NUC[1] - NUC[0])], dtype=np.uint32))
        s.set_pair_softwell(cfg["nucleolus_droplet_energy"], cfg["nucleolus_droplet_decay"], cfg["nucleolus_droplet_cutoff"],
                            np.arange(NUC[0], NUC[1], dtype=np.uint32))
    semi = np.array(cfg["wall_init_semiaxes"], dtype=float)
    s.set_ellipsoid_wall(cfg["a_core_repulsion"], cfg["a_core_diameter"], cfg["b_core_repulsion"], cfg["b_core_diameter"],
                         cfg["wall_a_factor"], cfg["wall_b_factor"], cfg["wall_packing_spring"], cfg["wall_semiaxes_spring"],
                         cfg["wall_mobility"], semi)
    s.set_scaling(cfg["bead_scale_init"], cfg["bead_scale_tau"], cfg["bond_scale_init"], cfg["bond_scale_tau"])
    out = {}
    ctx = dict(time=0.0, bead_scale=cfg["bead_scale_init"], bond_scale=cfg["bond_scale_init"], semi=semi.copy())

    def snap(phase, step):
        # mean_energy as the reference's callback computes it: under the context the previous callback left
        # (simulation_driver_interphase.cc:20-22 comes before :42-43)
        out[(phase, step)] = (s.positions_f32(quantize=True)[0].astype(np.float64),
                              dict(ctx, semi=ctx["semi"].copy(), mean_energy=float(s.energy()[0]) / N))

    # relaxation
    s.set_positions(x0q)
    s.begin_phase(semi)
    seed_relax, seed_inter = _mt64(oracle, cfg["interphase_seed"], 1), _mt64(oracle, cfg["interphase_seed"], 2)
    snap("relaxation", 0)
    step = 0
    while step < RELAX:
        nxt = min(RELAX, (step // 10 + 1) * 10)
        s.run(nxt - step, cfg["relaxation_timestep"], cfg["relaxation_temperature"], seed=seed_relax)
        step = nxt
        if step % 20 == 0:
            snap("relaxation", step)
    # interphase
    dt = cfg["interphase_timestep"]
    s.begin_phase(ctx["semi"])
    react = np.array(s.context().axial_reaction)
    snap("interphase", 0)
    ctx["semi"] = ctx["semi"] + dt * cfg["wall_mobility"] * (react - np.array(cfg["wall_semiaxes_spring"]) * ctx["semi"])
    s.set_context(0, 0, ctx["bead_scale"], ctx["bond_scale"], ctx["semi"])
    flags = g.RUN_UPDATE_SCALES | g.RUN_WALL_DYNAMICS
    contacts, dist = {}, cfg["contactmap_distance"] * ctx["bead_scale"]
    saved_contacts = {}
    step = 0
    while step < INTER:
        nxt = min(INTER, (step // 10 + 1) * 10)
        # callback(nxt): observation on the state callback(nxt - 1) left, then the state updates
        s.run(nxt - step, dt, cfg["interphase_temperature"], seed=seed_inter, flags=flags | g.RUN_DEFER_CALLBACK)
        c = s.context()
        assert c.callback_pending == 1 and c.step == nxt - 1
        ctx.update(bead_scale=c.bead_scale, bond_scale=c.bond_scale, semi=np.array(c.semiaxes))
        dist = cfg["contactmap_distance"] * c.bead_scale            # set by update_bead_scale() of callback(nxt - 1)
        step = nxt
        ctx["time"] = step * dt
        if step % 20 == 0:
            snap("interphase", step)
        for p in s.search_pairs(dist):
            contacts[tuple(int(v) for v in p)] = contacts.get(tuple(int(v) for v in p), 0) + 1
        if step % 20 == 0:
            saved_contacts[step] = dict(contacts)
            contacts = {}
        s.apply_callback()
        assert s.context().callback_pending == 0 and s.context().step == nxt
    return out, saved_contacts


def _check_run(tmp, lib, oracle, driver, atol, env=None, droplet=False):
    cfg, a, b, x0, ranges, radius = _inputs(tmp, droplet)
    x0q = _positions(tmp, "relaxation", 0)
    assert np.array_equal(x0q, (np.rint(x0.astype(np.float32) * np.float32(65536)) / np.float32(65536)).astype(np.float64))
    log = subprocess.run([str(driver), str(tmp / "traj.h5")], capture_output=True, text=True, env=env)
    assert log.returncode == 0, log.stderr
    lines = [ln for ln in log.stderr.splitlines() if ln.startswith("[")]
    assert sum(ln.startswith("[relax]") for ln in lines) == RELAX // 10 + 1        # logging interval 10, steps 0..40
    assert sum(ln.startswith("[inter]") for ln in lines) == INTER // 10 + 1
    assert "\tt: " in lines[-1] and "\tR: " in lines[-1] and "\tE: " in lines[-1]
    assert _tool("steps", tmp / "traj.h5", "relaxation").split() == ["0", "20", "40"]
    assert _tool("steps", tmp / "traj.h5", "interphase").split() == ["0", "20", "40", "60"]
    ref, ref_contacts = _python_driver(lib, oracle, cfg, a, b, x0q, ranges, droplet)
    for (phase, step), (pos, ctx) in ref.items():
        got = _positions(tmp, phase, step)
        assert np.abs(got - pos).max() <= atol, (phase, step)
        c = json.loads(_tool("context", tmp / "traj.h5", phase, step))
        assert c["time"] == pytest.approx(ctx["time"], abs=1e-15)
        assert c["bead_scale"] == pytest.approx(ctx["bead_scale"], rel=1e-12)
        assert np.allclose(c["wall_semiaxes"], ctx["semi"], rtol=0, atol=max(atol * 1e-3, 1e-12))
        if atol == 0:
            assert c["mean_energy"] == ctx["mean_energy"], (phase, step)          # bit-equal: same context, same positions
        else:
            assert c["mean_energy"] == pytest.approx(ctx["mean_energy"], rel=1e-4, abs=1e-4)
    for step, cm in ref_contacts.items():
        rows = [tuple(map(int, ln.split())) for ln in _tool("contacts", tmp / "traj.h5", "interphase", step).splitlines()]
        assert rows == sorted(rows)                                      # row-major (i, j) order, i < j
        assert all(i < j for i, j, _ in rows)
        if atol == 0:
            assert {(i, j): v for i, j, v in rows} == cm
        else:
            assert abs(len(rows) - len(cm)) <= 0.02 * len(cm) + 2
    return tmp / "traj.h5"


def test_store_layout_and_driver_on_oracle(tmp_path, oracle):
    drv = _make_oracle("gd_interphase", tmp_path)     # test-only binary: the same driver source linked against the oracle
    path = _check_run(tmp_path, oracle, oracle, drv, atol=0, env=_env(os.path.join(ROOT, "oracle")))
    if os.path.exists(H5DUMP):      # the on-disk layout the reference's readers rely on
        hdr = subprocess.check_output([H5DUMP, "-H", "-p", str(path)], text=True)
        pos = hdr[hdr.index('GROUP "interphase"'):]
        pos = pos[pos.index('DATASET "positions"'):][:1200]
        assert "H5T_IEEE_F32LE" in pos and f"( {N}, 3 )" in pos
        assert "SHUFFLE" in pos and "DEFLATE { LEVEL 6 }" in pos and "CHUNKED" in pos
        assert 'DATASET ".steps"' in hdr and 'DATASET "context"' in hdr and 'DATASET "contact_map"' in hdr
        assert "H5T_STD_U32LE" in hdr[hdr.index('DATASET "contact_map"'):][:600]
        meta = hdr[hdr.index('GROUP "metadata"'):]
        for name in ("config", "ab_factors", "chromosome_ranges", "centromere_ranges", "nucleolus_ranges", "nucleolus_bonds"):
            assert f'DATASET "{name}"' in meta
        assert 'ATTRIBUTE "keys"' in meta


def test_driver_with_nucleolar_droplet_on_oracle(tmp_path, oracle):
    """nucleolus_droplet_energy != 0: nucleolar side beads, their bonds and mobility, and the droplet attraction among them."""
    drv = _make_oracle("gd_interphase", tmp_path)
    _check_run(tmp_path, oracle, oracle, drv, atol=0, env=_env(os.path.join(ROOT, "oracle")), droplet=True)


def test_missing_config_key_is_an_error(tmp_path, oracle):
    drv = _make_oracle("gd_interphase", tmp_path)
    cfg, *_ = _inputs(tmp_path)
    del cfg["wall_mobility"]
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    subprocess.check_call([os.path.join(HOST, "gd_h5tool"), "make-input", str(tmp_path / "bad.h5"), str(tmp_path / "config.json"),
                           str(tmp_path / "chroms.tsv"), str(tmp_path / "ab.f64"), str(tmp_path / "pos.f64")])
    r = subprocess.run([str(drv), str(tmp_path / "bad.h5")], capture_output=True, text=True, env=_env(os.path.join(ROOT, "oracle")))
    assert r.returncode == 1 and "wall_mobility is not configured" in r.stderr      # simulation_config.cc:32


@pytest.mark.gpu
@pytest.mark.parametrize("droplet", [False, True])
def test_driver_on_gpu(tmp_path, hip, oracle, droplet):
    _check_run(tmp_path, oracle, oracle, _make("gd_interphase", ".", "../csrc", "gdyn"), atol=2e-4, droplet=droplet)


def _batch_case(tmp):
    """Three prepared trajectory files of one ensemble: same model, their own seeds and initial structures."""
    dirs = []
    for k in range(3):
        d = tmp / f"run{k}"
        d.mkdir()
        _inputs(d, seed=12345 + k, walk_seed=8 + k)
        dirs.append(d)
    return dirs


def _frames(d):
    out = {}
    for phase in ("relaxation", "interphase"):
        for step in _tool("steps", d / "traj.h5", phase).split():
            out[(phase, int(step))] = (_positions(d, phase, step), json.loads(_tool("context", d / "traj.h5", phase, step)),
                                       _tool("contacts", d / "traj.h5", phase, step) if phase == "interphase" else "")
    return out


def test_batched_driver_equals_solo_runs_on_oracle(tmp_path, oracle):
    """gd_interphase run0.h5 run1.h5 run2.h5 (three replicas of one handle, reference ensemble model:
    5-sim-genome/scripts/run_simulation:8-25) writes into every file exactly what the one-file program writes: each
    replica draws its own run's noise stream (gd_run_desc.replica_seeds).  On the fp64 oracle: bit for bit."""
    drv = _make_oracle("gd_interphase", tmp_path)
    env = _env(os.path.join(ROOT, "oracle"))
    solo = _batch_case(tmp_path / "solo") if (tmp_path / "solo").mkdir() is None else None
    batch = _batch_case(tmp_path / "batch") if (tmp_path / "batch").mkdir() is None else None
    for d in solo:
        subprocess.run([str(drv), str(d / "traj.h5")], check=True, capture_output=True, env=env)
    log = subprocess.run([str(drv), *[str(d / "traj.h5") for d in batch]], check=True, capture_output=True, text=True, env=env)
    assert sum(ln.startswith("[inter:2]") for ln in log.stderr.splitlines()) == INTER // 10 + 1
    for ds, db in zip(solo, batch):
        fs, fb = _frames(ds), _frames(db)
        assert fs.keys() == fb.keys() and len(fs) == 7
        for key in fs:
            assert np.array_equal(fs[key][0], fb[key][0]), key
            assert fs[key][1] == fb[key][1] and fs[key][2] == fb[key][2], key
    assert not np.array_equal(_frames(batch[0])[("interphase", 60)][0], _frames(batch[1])[("interphase", 60)][0])


def test_farm_launcher_splits_files_over_gpus(tmp_path):
    subprocess.check_call(["make", "-s", "-C", HOST, "gd_farm"])
    files = [f"out-{k}.h5" for k in range(5)]
    r = subprocess.run([os.path.join(HOST, "gd_farm"), "--gpus", "2", "--dry-run", "gd_interphase", *files], capture_output=True, text=True)
    assert r.returncode == 0
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[farm]")]
    assert lines == ["[farm] gpu 0: gd_interphase --device 0 out-0.h5 out-1.h5 out-2.h5", "[farm] gpu 1: gd_interphase --device 1 out-3.h5 out-4.h5"]
    # a real launch: two groups, the children run and their status comes back
    ok = subprocess.run([os.path.join(HOST, "gd_farm"), "--gpus", "2", "true", "a", "b"], capture_output=True, text=True)
    bad = subprocess.run([os.path.join(HOST, "gd_farm"), "--gpus", "2", "false", "a", "b"], capture_output=True, text=True)
    assert ok.returncode == 0 and bad.returncode == 1


def test_farm_of_two_driver_processes_on_oracle(tmp_path, oracle):
    """gd_farm --gpus 2 <driver> f0 f1 f2 as it runs on a node with two GPUs, rehearsed with oracle-linked drivers (which ignore
    --device): two processes (two files batched in one, one in the other), each bound to its share of the launcher's CPUs, one
    summary line per device, and every file holds exactly what a solo run writes."""
    subprocess.check_call(["make", "-s", "-C", HOST, "gd_farm"])
    drv = _make_oracle("gd_interphase", tmp_path)
    env = _env(os.path.join(ROOT, "oracle"))
    (tmp_path / "solo").mkdir(); (tmp_path / "farm").mkdir()
    solo, farm = _batch_case(tmp_path / "solo"), _batch_case(tmp_path / "farm")
    for d in solo:
        subprocess.run([str(drv), str(d / "traj.h5")], check=True, capture_output=True, env=env)
    r = subprocess.run([os.path.join(HOST, "gd_farm"), "--gpus", "2", str(drv), *[str(d / "traj.h5") for d in farm]],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    summary = [ln for ln in r.stderr.splitlines() if ln.startswith("[farm] gpu") and "file(s)" in ln]
    assert len(summary) == 2 and summary[0].startswith("[farm] gpu 0: 2 file(s), status 0,") and summary[1].startswith("[farm] gpu 1: 1 file(s), status 0,")
    if len(os.sched_getaffinity(0)) >= 2:
        shares = [tuple(int(v) for v in re.search(r"cpus (\d+)-(\d+)", ln).groups()) for ln in summary]
        assert shares[0][1] < shares[1][0]                       # disjoint, contiguous shares
    for ds, df in zip(solo, farm):
        fs, ff = _frames(ds), _frames(df)
        assert fs.keys() == ff.keys() and len(fs) == 7
        for key in fs:
            assert np.array_equal(fs[key][0], ff[key][0]) and fs[key][1] == ff[key][1] and fs[key][2] == ff[key][2], key


@pytest.mark.gpu
def test_batched_driver_on_gpu(tmp_path, hip, oracle):
    """The libgdyn-linked program batching three files on the MI355X against the ORACLE-linked one-file program."""
    drv_o = _make_oracle("gd_interphase", tmp_path)
    drv_h = _make("gd_interphase", ".", "../csrc", "gdyn")
    (tmp_path / "solo").mkdir(); (tmp_path / "batch").mkdir()
    solo, batch = _batch_case(tmp_path / "solo"), _batch_case(tmp_path / "batch")
    for d in solo:
        subprocess.run([str(drv_o), str(d / "traj.h5")], check=True, capture_output=True, env=_env(os.path.join(ROOT, "oracle")))
    subprocess.run([str(drv_h), "--device", "0", *[str(d / "traj.h5") for d in batch]], check=True, capture_output=True)
    for ds, db in zip(solo, batch):
        fs, fb = _frames(ds), _frames(db)
        assert fs.keys() == fb.keys()
        for key in fs:
            assert np.abs(fs[key][0] - fb[key][0]).max() <= 2e-4, key
            assert np.allclose(fs[key][1]["wall_semiaxes"], fb[key][1]["wall_semiaxes"], rtol=0, atol=1e-7)


@pytest.mark.gpu
def test_farm_runs_batched_drivers_on_gpu(tmp_path, hip):
    """gd_farm --gpus 1 gd_interphase f0 f1 f2: the launcher starts one driver process for GPU 0 with all three files (three
    replicas of one handle); every file gets its relaxation and interphase frames.  (With G GPUs the same command line starts
    G processes, `--device g` each; this box has one.)"""
    subprocess.check_call(["make", "-s", "-C", HOST, "gd_farm"])
    drv = _make("gd_interphase", ".", "../csrc", "gdyn")
    dirs = _batch_case(tmp_path)
    r = subprocess.run([os.path.join(HOST, "gd_farm"), "--gpus", "1", str(drv), *[str(d / "traj.h5") for d in dirs]],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[farm] gpu 0:" in r.stderr and "--device 0" in r.stderr
    frames = [_frames(d) for d in dirs]
    for f in frames:
        assert len(f) == 7 and ("interphase", 60) in f
    assert not np.array_equal(frames[0][("interphase", 60)][0], frames[1][("interphase", 60)][0])


# ---------------------------------------------------------------------------------------------- gd_spindle

SP_COARSE, SP_STEPS, SP_PACK = 2, 40, 30


def _spindle_inputs(tmp):
    lens = wl.chain_lengths(N)
    cfg = dict(wl.DEFAULT_CONFIG)
    cfg.update(init_coarse_graining=SP_COARSE, init_bend_energy=1.0, init_packing_spring=0.5, init_packing_radius=1.0,
               init_spindle_steps=SP_STEPS, init_packing_steps=SP_PACK, init_sampling_interval=20, init_logging_interval=10,
               init_start_stddev=0.5, spindle_seed=2024)
    (tmp / "config.json").write_text(json.dumps(cfg))
    st, rows, fine = 0, [], []
    for k, n in enumerate(lens):
        cen = st + int(n) // 2
        rows.append(f"chr{k + 1} {st} {st + n} {cen} {cen + 1}")
        fine.append((st, st + int(n), cen, cen + 1))
        st += int(n)
    (tmp / "chroms.tsv").write_text("\n".join(rows) + "\n")
    np.zeros((N, 2), dtype="<f8").tofile(tmp / "ab.f64")
    np.zeros((N, 3), dtype="<f8").tofile(tmp / "pos.f64")
    subprocess.check_call([os.path.join(HOST, "gd_h5tool"), "make-input", str(tmp / "traj.h5"), str(tmp / "config.json"),
                           str(tmp / "chroms.tsv"), str(tmp / "ab.f64"), str(tmp / "pos.f64")])
    chains, start = [], 0
    for (b0, b1, c0, c1) in fine:                                  # simulation_spindle/simulation_driver.cc:46-68
        size, cen = b1 - b0, (c0 + c1) // 2
        csize, ccen = (size + SP_COARSE - 1) // SP_COARSE, (cen - b0) // SP_COARSE
        chains.append((start, start + csize, start + ccen))
        start += csize
    return cfg, chains, start


def _python_spindle(lib, oracle, cfg, chains, n):
    rnd = _Mt64(oracle, cfg["spindle_seed"])
    x = np.zeros((n, 3))
    for (c0, c1, _) in chains:
        z = rnd.normals(6)
        centroid = np.array([cfg["init_start_point"][k] + cfg["init_start_stddev"] * z[k] for k in range(3)])
        d = np.array(z[3:])
        norm = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        step = cfg["init_bond_length"] * (d * (1 / norm))
        pos = centroid - step * float(c1 - c0) / 2
        for i in range(c0, c1):
            x[i] = pos
            pos = pos + step
    s = g.System(lib, n, 1)
    s.set_bead_params(mobility=np.full(n, cfg["init_mobility"]))
    s.set_pair_softcore(cfg["init_bead_repulsion"], cfg["init_bead_diameter"], 0.0, 0.0, 2, 3, 2, 3, mix=False)
    bond = g.System.bond_params(g.POT_SEMISPRING, k_a=cfg["init_bond_spring"], l_a=cfg["init_bond_length"])
    for (c0, c1, _) in chains:
        s.add_bond_range(bond, c0, c1, 1)
        s.add_bending_range(c0, c1, cfg["init_bend_energy"])
    s.set_positions(x)
    out, energies = {}, {}
    for phase, steps in (("spindle", SP_STEPS), ("packing", SP_PACK)):
        if phase == "spindle":
            s.add_point_source(g.POT_HARMONIC, cfg["init_spindle_spring"], 0.0, cfg["init_spindle_point"],
                               targets=[c + d for (_, _, c) in chains for d in (-1, 0, 1)])
        else:
            s.add_point_source(g.POT_SEMISPRING, cfg["init_packing_spring"], cfg["init_packing_radius"], cfg["init_spindle_point"])
        s.begin_phase()
        seed = rnd.draw()
        step = 0
        out[(phase, 0)] = s.positions_f32(quantize=True)[0].astype(np.float64)
        energies[(phase, 0)] = float(s.energy()[0]) / n
        while step < steps:
            s.run(10, cfg["init_timestep"], cfg["init_temperature"], seed=seed)
            step += 10
            energies[(phase, step)] = float(s.energy()[0]) / n
            if step % 20 == 0:
                out[(phase, step)] = s.positions_f32(quantize=True)[0].astype(np.float64)
    s.close()
    return out, energies


def _check_spindle(tmp, lib, oracle, driver, atol, env=None):
    cfg, chains, n = _spindle_inputs(tmp)
    log = subprocess.run([str(driver), str(tmp / "traj.h5")], capture_output=True, text=True, env=env)
    assert log.returncode == 0, log.stderr
    lines = [ln for ln in log.stderr.splitlines() if ln.startswith("[")]
    assert [ln.split("]")[0][1:] for ln in lines] == ["spindle"] * (SP_STEPS // 10 + 1) + ["packing"] * (SP_PACK // 10 + 1)
    assert _tool("steps", tmp / "traj.h5", "spindle").split() == ["0", "20", "40"]
    assert _tool("steps", tmp / "traj.h5", "packing").split() == ["0", "20"]
    ref, energies = _python_spindle(lib, oracle, cfg, chains, n)
    for (phase, step), pos in ref.items():
        got = _positions(tmp, phase, step)
        assert got.shape == (n, 3)
        assert np.abs(got - pos).max() <= atol, (phase, step)
    # "[phase] date time \t step \t E: energy-per-bead" (simulation_driver.cc:275-292)
    for ln in lines:
        phase = ln.split("]")[0][1:]
        _, step, e = ln.split("\t")
        assert e.startswith("E: ")
        assert float(e[3:]) == pytest.approx(energies[(phase, int(step))], rel=1e-5 if atol == 0 else 2e-2, abs=atol * 10)
    if os.path.exists(H5DUMP):          # the coarse chain table of each phase (save_chains, :295-309)
        for phase in ("spindle", "packing"):
            d = subprocess.check_output([H5DUMP, "-d", f"/snapshots/{phase}/metadata/chromosome_ranges", "-y", "-w", "200", str(tmp / "traj.h5")], text=True)
            body = d[d.index("DATA {") + 6:]
            vals = [int(v) for v in body[:body.index("}")].replace(",", " ").split()]
            assert vals == [v for (c0, c1, _) in chains for v in (c0, c1)]


def test_spindle_driver_on_oracle(tmp_path, oracle):
    drv = _make_oracle("gd_spindle", tmp_path)
    _check_spindle(tmp_path, oracle, oracle, drv, atol=0, env=_env(os.path.join(ROOT, "oracle")))


# (the driver's pair form (2, 3, 2, 3) runs the runtime-power pair kernels; its forces are held to the oracle at FORCE_RTOL on both list
# paths by tests/test_runtime_pair_gpu.py::test_spindle_driver_model_forces_match_oracle -- here: the program, end to end)
@pytest.mark.gpu
def test_spindle_driver_on_gpu(tmp_path, hip, oracle):
    _check_spindle(tmp_path, oracle, oracle, _make("gd_spindle", ".", "../csrc", "gdyn"), atol=2e-4)


# ---------------------------------------------------------------------------------------- gd_fine_sampling

FINE_STEPS = 250


def _python_fine(lib, oracle, cfg, a, b, ranges, x_restart, ctx_restart):
    """The ABI call sequence of gd_fine_sampling.cpp from Python."""
    s = g.System(lib, N, 1)
    s.set_bead_params(a=a, b=b, mobility=np.full(N, cfg["chromatin_mobility"]))
    s.set_pair_softcore(cfg["a_core_repulsion"], cfg["a_core_diameter"], cfg["b_core_repulsion"], cfg["b_core_diameter"], 2, 3, 8, 3,
                        mix=True, scale_by_bead_scale=True)
    chain = g.System.bond_params(g.POT_SEMISPRING, k_a=cfg["chromatin_bond_spring"], l_a=cfg["chromatin_bond_length"],
                                 scale_by_bond_scale=True)
    for (b0, b1) in ranges:
        s.add_bond_range(chain, b0, b1, 1)
    semi = np.array(ctx_restart["wall_semiaxes"], dtype=float)
    s.set_ellipsoid_wall(cfg["a_core_repulsion"], cfg["a_core_diameter"], cfg["b_core_repulsion"], cfg["b_core_diameter"],
                         cfg["wall_a_factor"], cfg["wall_b_factor"], cfg["wall_packing_spring"], cfg["wall_semiaxes_spring"],
                         cfg["wall_mobility"], np.array(cfg["wall_init_semiaxes"], dtype=float))
    s.set_scaling(cfg["bead_scale_init"], cfg["bead_scale_tau"], cfg["bond_scale_init"], cfg["bond_scale_tau"])
    s.set_positions(x_restart)
    dt = 1e-5 / 100
    s.begin_phase(semi)
    react = np.array(s.context().axial_reaction)
    s.set_context(0, 0, 1.0, 1.0, semi)
    out = {0: (s.positions_f32(quantize=True)[0].astype(np.float64), semi.copy(), float(s.energy()[0]) / N)}
    semi = semi + dt * cfg["wall_mobility"] * (react - np.array(cfg["wall_semiaxes_spring"]) * semi)
    s.set_context(0, 0, 1.0, 1.0, semi)
    seed = _mt64(oracle, cfg["interphase_seed"] ^ 700000, 1)
    step = 0
    while step < FINE_STEPS:
        nxt = min(FINE_STEPS, (step // 100 + 1) * 100)
        s.run(nxt - step, dt, 0.0, seed=seed, flags=g.RUN_WALL_DYNAMICS | g.RUN_DEFER_CALLBACK)
        semi = np.array(s.context().semiaxes)            # left by callback(nxt - 1); the energy is evaluated with them
        step = nxt
        if step % 100 == 0:
            out[step] = (s.positions_f32(quantize=True)[0].astype(np.float64), semi.copy(), float(s.energy()[0]) / N)
        s.apply_callback()
    assert s.context().bead_scale == 1.0 and s.context().bond_scale == 1.0
    s.close()
    return out


def _check_fine(tmp, lib, oracle, interphase_driver, fine_driver, atol, env=None):
    cfg, a, b, x0, ranges, radius = _inputs(tmp)
    r = subprocess.run([str(interphase_driver), str(tmp / "traj.h5")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    x_restart = _positions(tmp, "interphase", INTER)
    ctx_restart = json.loads(_tool("context", tmp / "traj.h5", "interphase", INTER))
    r = subprocess.run([str(fine_driver), "--steps", str(FINE_STEPS), str(tmp / "traj.h5"), "0", str(INTER)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[fine]")]
    assert len(lines) == FINE_STEPS // cfg["interphase_logging_interval"] + 1
    assert _tool("steps", tmp / "traj.h5", "fine_sampling").split() == ["0", "100", "200"]    # sampling interval forced to 100
    ref = _python_fine(lib, oracle, cfg, a, b, ranges, x_restart, ctx_restart)
    quantum = 2.0 ** -16       # the store rounds positions to 2^-16 (simulation_store.cc:403-407): both sides are on that grid
    for step, (pos, semi, e) in ref.items():
        got = _positions(tmp, "fine_sampling", step)
        if atol == 0:
            assert np.array_equal(got, pos), step
        else:
            # The device against the fp64 oracle from the same restart, at dt = 1e-7 and T = 0.  What this run outputs IS the small
            # displacement since the restart (flow fields, analyze_particle_flow), so the check is on the displacement, in units of
            # the storage quantum: the two trajectories agree to ~1e-7 (compensated fp32 positions, gdyn.h), so a saved coordinate
            # differs from the oracle's only where its value sits within that of a rounding boundary -- by one quantum, in under
            # 3 % of the coordinates.  A stepper that loses part of mu F dt to the rounding of x + dx fails both bounds, and one
            # that does not move the beads at all is off by the whole motion (checked to be >= 8 quanta for the median coordinate).
            diff = np.abs(got - pos)
            assert diff.max() <= quantum * (1 + 1e-9), (step, diff.max() / quantum)
            assert (diff == 0).mean() >= 0.97, (step, (diff == 0).mean())
            if step > 0:
                moved = np.abs(pos - x_restart)
                assert np.median(moved) >= 8 * quantum, (step, np.median(moved) / quantum)      # the test has the power to see motion
        c = json.loads(_tool("context", tmp / "traj.h5", "fine_sampling", step))
        assert c["time"] == pytest.approx(step * 1e-7, abs=1e-18)
        assert c["bead_scale"] == 1.0 and c["bond_scale"] == 1.0               # simulation_driver.cc:55-56
        assert np.allclose(c["wall_semiaxes"], semi, rtol=0, atol=max(atol * 1e-3, 1e-12))
        if atol == 0:
            assert c["mean_energy"] == e, step
        else:
            assert c["mean_energy"] == pytest.approx(e, rel=1e-3)
    # T = 0: deterministic descent, the energy does not increase between samples
    es = [ref[k][2] for k in sorted(ref)]
    assert all(e1 <= e0 + 1e-9 for e0, e1 in zip(es, es[1:]))


def test_fine_sampling_driver_on_oracle(tmp_path, oracle):
    env = _env(os.path.join(ROOT, "oracle"))
    _check_fine(tmp_path, oracle, oracle, _make_oracle("gd_interphase", tmp_path), _make_oracle("gd_fine_sampling", tmp_path), atol=0, env=env)


@pytest.mark.gpu
def test_fine_sampling_driver_on_gpu(tmp_path, hip, oracle):
    _check_fine(tmp_path, oracle, oracle, _make("gd_interphase", ".", "../csrc", "gdyn"), _make("gd_fine_sampling", ".", "../csrc", "gdyn"), atol=2e-4)
