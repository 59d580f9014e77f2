"""Host side of the Hi-C signal analyses (no GPU): the restatement (tests/hic_restatement.py) and hic.py's numpy functions against
the reference's own outputs (tests/golden/hic_fixtures.npz and .json, made by make_hic_fixtures.py) by the rules of DESIGN.md
section 7e, the gd_hic_* symbols of libgdyn against include/gdyn_hic.h, the command lines of the four programs, gd_h5tool
put-cool, and gd_downsample against the reference's output."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hic_restatement as R
from conftest import ROOT

PKG = "2022a-genome-dynamics_amd"
hic = importlib.import_module(PKG + ".hic")
HOST = os.path.join(ROOT, PKG, "host")
Z = np.load(os.path.join(ROOT, "tests", "golden", "hic_fixtures.npz"))
with open(os.path.join(ROOT, "tests", "golden", "hic_fixtures.json")) as _f:
    T = json.load(_f)
NAMES = T["names"]
CHROM, BIN1, BIN2, COUNT, WEIGHT = Z["chrom"], Z["bin1"], Z["bin2"], Z["count"], Z["weight"]
BINSIZE = int(Z["binsize"])
WIDTHS = [int(w) for w in Z["widths"]]
PROGRAMS = ["gd_compute_interactions", "gd_compute_local_alpha", "gd_hic_power_law", "gd_downsample"]
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")


def same_signal(got, want, ulps, what):
    """Identical NaN pattern and finite values within `ulps` units of the last place."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    d = R.ulp_distance(want, got)
    print(what, "ulp distance", d)
    assert d <= ulps, (what, d)


def test_fixtures_cover_the_cases():
    sizes = dict(zip(NAMES, np.bincount(CHROM).tolist()))
    assert not any(n.startswith("chr") for n in NAMES) and {"X", "Y", "MT"} < set(NAMES)
    assert 1 in sizes.values()                                                          # a chromosome of a single bin
    assert any(6 <= n < 10 for n in sizes.values()) and 1 < sizes["MT"] < 6            # 2 (W - 1) = 6 for the default band
    assert sorted(NAMES, key=hic.std_chrom_order) != NAMES                              # the output order differs from the file's
    touched = np.zeros(len(CHROM), bool)
    touched[BIN1] = touched[BIN2] = True
    assert (~touched).any()                                                             # unmappable bins
    assert (CHROM[BIN1] != CHROM[BIN2]).any() and np.isnan(WEIGHT).any() and COUNT.max() < 2 ** 24
    pairs = np.stack([BIN1, BIN2], axis=1)
    assert (BIN1 <= BIN2).all() and len(np.unique(pairs, axis=0)) == len(pairs)
    assert np.array_equal(pairs, pairs[np.lexsort((BIN2, BIN1))])                       # cooler order
    assert Z["held4"][CHROM != NAMES.index("MT")].all() and not Z["held4"][CHROM == NAMES.index("MT")].any()
    assert not Z["held6"].all() and Z["held6"].any()


@pytest.mark.parametrize("W", [4, 6] + [w + 1 for w in WIDTHS])
def test_band_restatements_equal_the_reference(W):
    want = Z[f"band{W}"] if W in (4, 6) else Z[f"alpha_band{W - 1}"]
    assert want.dtype == np.int64 and want.any() and (want == 0).any()
    assert np.array_equal(R.band(BIN1, BIN2, COUNT, CHROM, W), want)
    assert np.array_equal(R.band_fast(BIN1, BIN2, COUNT, CHROM, W), want)
    got = hic.band_matrix(BIN1, BIN2, COUNT, CHROM, W)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # either order of the two ids, and ids outside the table are ignored
    flip = np.arange(len(BIN1)) % 3 == 0
    b1, b2 = np.where(flip, BIN2, BIN1), np.where(flip, BIN1, BIN2)
    b1 = np.concatenate([b1, [-1, 5, len(CHROM), 2 ** 40]])
    b2 = np.concatenate([b2, [3, len(CHROM), 7, 0]])
    c = np.concatenate([COUNT, [9, 9, 9, 9]])
    assert np.array_equal(hic.band_matrix(b1, b2, c, CHROM, W), want) and np.array_equal(R.band(b1, b2, c, CHROM, W), want)


@pytest.mark.parametrize("W", [4, 6])
def test_decay_and_insulation_equal_the_reference(W):
    """Rule 2: identical NaN pattern and finite values within 4 ulp wherever the reference runs; elsewhere (1 < n < 2 (W - 1))
    hic.py is held against the restatement."""
    held = Z[f"held{W}"]
    for name, fn in (("restatement", R.decay_insulation), ("hic.py", hic.decay_insulation)):
        D, I = fn(Z[f"band{W}"], CHROM)
        assert D.shape == (len(CHROM), W - 1) and I.shape == (len(CHROM), W - 2)
        same_signal(D[held], Z[f"decay{W}"][held], 4, f"{name} D, W = {W}")
        same_signal(I[held], Z[f"insulation{W}"][held], 4, f"{name} I, W = {W}")
    (Dr, Ir), (Dh, Ih) = R.decay_insulation(Z[f"band{W}"], CHROM), hic.decay_insulation(Z[f"band{W}"], CHROM)
    same_signal(Dh, Dr, 4, "hic.py against the restatement, D")
    same_signal(Ih, Ir, 4, "hic.py against the restatement, I")
    assert np.isfinite(Dr[~held]).any()                                                 # the rule gives values where the reference asserts
    single = CHROM == NAMES.index("4")
    assert single.sum() == 1 and np.isnan(Dr[single]).all() and np.isnan(Z[f"decay{W}"][single]).all()


def test_short_chromosome_follows_the_rule():
    """n = 7, W = 6: the case the reference's assert len(sym_decay) == len(bands) rejects."""
    rng = np.random.default_rng(7)
    band = rng.integers(1, 500, size=(7, 6)).astype(np.int64)
    band[3, 0] = 0
    for k in range(1, 6):
        band[7 - k:, k] = 0                                                             # forward contacts end at the chromosome's end
    chrom = np.zeros(7, np.int32)
    D, I = R.decay_insulation(band, chrom)
    x = np.where(band == 0, np.nan, band.astype(float))
    f = lambda i, k: x[i, k] / np.sqrt(x[i, 0] * x[i + k, 0])
    assert D[0, 4] == f(0, 5) and D[6, 4] == f(1, 5) and np.isnan(D[2:5, 4]).all()      # k = 5: bins 0, 1 forward, 5, 6 backward
    assert D[1, 3] == f(1, 4) and D[5, 3] == f(1, 4) and D[4, 3] == f(0, 4)              # k = 4
    assert np.isnan(D[3, 3]) and np.isnan(D[6, 2])                                       # through the unmappable bin 3
    Dh, Ih = hic.decay_insulation(band, chrom)
    same_signal(Dh, D, 0, "hic.py D, n = 7") and same_signal(Ih, I, 0, "hic.py I, n = 7")


@pytest.mark.parametrize("width", WIDTHS)
def test_local_alpha_equals_the_reference_within_its_float32_gap(width):
    """Rule 3: fp64 from the integer band; the reference keeps W and log W in float32, so its recorded output is matched within
    4 x the gap the generator recorded between the reference and the same formulas in fp64."""
    band, ref, gap = Z[f"alpha_band{width}"], Z[f"alpha_ref{width}"], float(Z[f"alpha_fp32_gap{width}"])
    assert 0 < gap < 1e-4 and np.isnan(ref).any() and np.nanmax(ref) - np.nanmin(ref) > 1
    mine, got = R.local_alpha(band, CHROM), hic.local_alpha(band, CHROM)
    for name, a in (("restatement", mine), ("hic.py", got)):
        assert np.array_equal(np.isnan(a), np.isnan(ref)), name
        print(name, "width", width, "max |alpha - reference|", np.nanmax(np.abs(a - ref)), "allowed", 4 * gap)
        assert np.nanmax(np.abs(a - ref)) <= 4 * gap, name
    np.testing.assert_allclose(got, mine, rtol=1e-10, atol=0)


def test_distance_profile_equals_the_reference():
    """Rule 4: RAW sums are integers and the means equal the reference's bit for bit; weighted sums at rtol N * 2^-52."""
    size = hic.largest_chromosome(CHROM)
    excluded = hic.excluded_bins(CHROM, {n: k for k, n in enumerate(NAMES)})
    assert size == 110 and excluded.sum() == sum(np.bincount(CHROM)[NAMES.index(n)] for n in ("X", "Y", "MT"))
    assert np.array_equal(excluded, hic.excluded_bins(CHROM, {"chr" + n: k for k, n in enumerate(NAMES)}))
    total, n, mean = hic.distance_profile(BIN1, BIN2, COUNT, CHROM, excluded, None, size)
    assert total.dtype == np.int64 and np.array_equal(n, Z["profile_n_RAW"])
    assert np.array_equal(mean, Z["profile_mean_RAW"], equal_nan=True) and np.isnan(mean).any()
    rt, rn = R.profile(BIN1, BIN2, COUNT, CHROM, excluded, None, size)
    assert np.array_equal(rt, total) and np.array_equal(rn, n)
    total, n, mean = hic.distance_profile(BIN1, BIN2, COUNT, CHROM, excluded, WEIGHT, size)
    want = Z["profile_mean_weight"]
    assert np.array_equal(n, Z["profile_n_weight"]) and np.array_equal(np.isnan(mean), np.isnan(want))
    rtol = int(Z["profile_n_weight"].max()) * 2.0 ** -52
    print("weighted P(s): max relative difference", np.nanmax(np.abs(mean - want) / want), "allowed", rtol)
    np.testing.assert_allclose(mean, want, rtol=rtol, atol=0)
    with pytest.raises(ValueError):
        hic.distance_profile(BIN1, BIN2, COUNT, CHROM, excluded, None, 50)


def _signal_table():
    rows = [line.split("\t") for line in T["compute_interactions_w4"].splitlines()[1:]]
    names = list(dict.fromkeys(r[0] for r in rows))
    return names, {n: np.array([[float(v) for v in r[3:]] for r in rows if r[0] == n]) for n in names}, rows


@pytest.mark.parametrize("case", range(len(T["downsample"])))
def test_downsample_equals_the_reference(case):
    """Rule 5 at rtol 1e-12 against the unrounded values of the reference's downsample()."""
    rate, window = T["downsample"][case]["rate"], T["downsample"][case]["window"]
    names, tracks, _ = _signal_table()
    want = Z[f"downsample_{rate}_{window or 0}"]
    for fn in (R.downsample, hic.downsample):
        got = np.concatenate([fn(tracks[n], rate, window) for n in names])
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert np.isnan(want).any() and np.isfinite(want).any()


def test_library_exports_hic_symbols(gdyn):
    d = C.CDLL(gdyn.LIBGDYN_PATH)
    for name in hic.HIC_SYMBOLS:
        assert hasattr(d, name), name
    d.gd_hic_abi_version.restype = C.c_int
    assert d.gd_hic_abi_version() == hic.HIC_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "gdyn_hic.h")).read()
    assert set(re.findall(r"^int\s+(gd_hic_\w+)\(", hdr, flags=re.M)) == set(hic.HIC_SYMBOLS)
    assert f"#define GD_HIC_ABI_VERSION {hic.HIC_ABI_VERSION}" in hdr
    exported = subprocess.check_output(["nm", "-D", "--defined-only", gdyn.LIBGDYN_PATH], text=True)
    assert set(re.findall(r"\bT (gd_hic_\w+)", exported)) == set(hic.HIC_SYMBOLS)
    hic.load_hic_library()


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", *PROGRAMS])
    return {k: os.path.join(HOST, k) for k in ["gd_h5tool", *PROGRAMS]}


def _run(program, *args):
    return subprocess.run([program, *map(str, args)], capture_output=True, text=True)


@needs_h5
def test_command_line_errors(programs, tmp_path):
    out = tmp_path / "out.tsv"
    cases = {"gd_compute_interactions": [([], "required: -b"), (["a.mcool"], "required: -b"), (["-b", "1000"], "required: mcoolfile"), (["-b"], "expected one argument"),
                                         (["-b", "x", "a.mcool"], "invalid int value: 'x'"), (["-b1000", "-w", "1", "a.mcool"], "argument -w"),
                                         (["-b", "1000", "a.mcool", "b.mcool"], "unrecognized arguments: b.mcool"), (["-b", "1000", "--binsize=5", "a.mcool"], "unrecognized arguments: --binsize=5"),
                                         (["-b", "0", "-o", out, "a.mcool"], "at least 1")],
             "gd_compute_local_alpha": [([], "required: mcoolfile"), (["-w", "0", "a.mcool"], "argument -w"), (["-w", "1.5", "a.mcool"], "invalid int value: '1.5'"),
                                        (["-o"], "expected one argument"), (["--normalize", "RAW", "a.mcool"], "unrecognized arguments: --normalize")],
             "gd_hic_power_law": [([], "required: mcool"), (["--binsize", "x", "a.mcool"], "invalid int value: 'x'"), (["-b", "1000", "a.mcool"], "unrecognized arguments: -b"),
                                  (["--normalize"], "expected one argument"), (["--binsize=1000", "a.mcool", "more"], "unrecognized arguments: more")],
             "gd_downsample": [([], "required: infile"), (["--rate", "0", "a.tsv"], "at least 1"), (["--rate=x", "a.tsv"], "invalid int value: 'x'"),
                               (["--window"], "expected one argument"), (["-b", "5", "a.tsv"], "unrecognized arguments: -b")]}
    for prog, table in cases.items():
        for args, what in table:
            r = _run(programs[prog], *args)
            assert r.returncode == 2 and r.stderr.startswith(f"usage: {prog}") and what in r.stderr, (prog, args, r.stderr)
            assert f"{prog}: error:" in r.stderr and r.stdout == ""
    assert not out.exists()


@needs_h5
def test_dry_run(programs, tmp_path):
    out = tmp_path / "out.tsv"
    r = _run(programs["gd_compute_interactions"], "--dry-run", "-b", "50000", "-o", out, "a.mcool")
    assert r.returncode == 0, r.stderr
    lines = [l.split("\t") for l in r.stdout.splitlines()]
    assert lines[:2] == [["binsize", "50000"], ["band_width", "4"]] and lines[2][:2] == ["read", "a.mcool"] and "/resolutions/50000/bins/" in lines[2][2]
    assert lines[-1] == ["write", str(out), "chrom", "start", "end", "D1", "D2", "D3", "I1", "I2"]
    r = _run(programs["gd_compute_local_alpha"], "--dry-run", "-w50", "a.mcool")
    assert r.returncode == 0 and r.stdout.splitlines()[:2] == ["binsize\t100000", "width\t50"] and r.stdout.splitlines()[-1] == "write\tstdout\tchrom\tstart\tend\talpha"
    r = _run(programs["gd_hic_power_law"], "--dry-run", "--normalize=weight", "a.mcool")
    assert r.returncode == 0 and r.stdout.splitlines()[:2] == ["binsize\t100000", "normalize\tweight"]
    assert "read\ta.mcool\t/resolutions/100000/bins/{chrom,weight}" in r.stdout and r.stdout.splitlines()[-1] == "write\tstdout\tdistance\tcontacts"
    r = _run(programs["gd_downsample"], "--dry-run", "--rate", "5", "a.tsv")
    assert r.returncode == 0 and r.stdout.splitlines() == ["rate\t5", "window\t5", "read\ta.tsv", "write\tstdout"]
    assert not out.exists()


@needs_h5
def test_runtime_errors_exit_1(programs, tmp_path):
    """A missing input or a missing part of the file is `error: <what>` and exit 1 before any device work."""
    out = tmp_path / "out.tsv"
    for prog, args in [("gd_compute_interactions", ["-b", BINSIZE, "-o", out, tmp_path / "missing.mcool"]), ("gd_compute_local_alpha", [tmp_path / "missing.mcool"]),
                       ("gd_hic_power_law", [tmp_path / "missing.mcool"]), ("gd_downsample", [tmp_path / "missing.tsv"])]:
        r = _run(programs[prog], *args)
        assert r.returncode == 1 and r.stderr.startswith("error: ") and r.stdout == "", (prog, r.stderr)
    cool = tmp_path / "toy.mcool"
    assert R.put_cool(programs["gd_h5tool"], tmp_path, cool, BINSIZE, NAMES, CHROM, Z["start"], Z["end"], BIN1, BIN2, COUNT).returncode == 0
    for prog, args, what in [("gd_compute_interactions", ["-b", 5000, cool], "resolutions/5000"), ("gd_compute_local_alpha", ["-b", 5000, cool], "resolutions/5000"),
                             ("gd_hic_power_law", ["--binsize", BINSIZE, "--normalize", "KR", cool], "bins/KR")]:
        r = _run(programs[prog], *args)
        assert r.returncode == 1 and r.stderr.startswith("error: ") and what in r.stderr and r.stdout == "", (prog, r.stderr)
    named = tmp_path / "named.mcool"      # a name by_std_chrom_order has no rank for
    assert R.put_cool(programs["gd_h5tool"], tmp_path, named, BINSIZE, ["1", "scaffold_7"], [0, 0, 1], [0, 1000, 0], [1000, 2000, 1000], [0], [1], [5]).returncode == 0
    r = _run(programs["gd_compute_interactions"], "-b", BINSIZE, named)
    assert r.returncode == 1 and "scaffold_7" in r.stderr and r.stdout == ""
    (tmp_path / "bad.tsv").write_text("chrom\tstart\tend\tD1\nchr1\t0\t10\tabc\n")
    r = _run(programs["gd_downsample"], tmp_path / "bad.tsv")
    assert r.returncode == 1 and "abc" in r.stderr
    assert not out.exists()


@needs_h5
def test_put_cool_round_trip(programs, tmp_path):
    tool = programs["gd_h5tool"]
    cool = tmp_path / "toy.mcool"
    r = R.put_cool(tool, tmp_path, cool, BINSIZE, NAMES, CHROM, Z["start"], Z["end"], BIN1, BIN2, COUNT, WEIGHT)
    assert r.returncode == 0, r.stderr
    r = R.put_cool(tool, tmp_path, cool, 5 * BINSIZE, NAMES[:2], [0, 1], [0, 0], [5000, 5000], [0, 0], [0, 1], [3, 1])      # a second resolution
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in subprocess.check_output([tool, "cool-bins", str(cool), str(BINSIZE)], text=True).splitlines()]
    assert [r[0] for r in rows] == [NAMES[c] for c in CHROM]
    assert [int(r[1]) for r in rows] == Z["start"].tolist() and [int(r[2]) for r in rows] == Z["end"].tolist()
    for path, want in [("pixels/bin1_id", BIN1), ("pixels/bin2_id", BIN2), ("pixels/count", COUNT), ("bins/weight", WEIGHT)]:
        out = tmp_path / "column.f64"
        shape = subprocess.check_output([tool, "dataset", str(cool), f"/resolutions/{BINSIZE}/{path}", str(out)], text=True)
        assert shape.split() == [str(len(want))]
        assert np.array_equal(np.fromfile(out, "<f8"), want.astype(np.float64), equal_nan=True)
    assert subprocess.check_output([tool, "cool-bins", str(cool), str(5 * BINSIZE)], text=True).split() == ["1", "0", "5000", "2", "0", "5000"]
    (tmp_path / "short.bin").write_bytes(b"\0" * 12)      # three counts for two pixels
    r = _run(tool, "put-cool", cool, BINSIZE, tmp_path / "cool_names.txt", tmp_path / "cool_chrom.bin", tmp_path / "cool_start.bin", tmp_path / "cool_end.bin",
             tmp_path / "cool_bin1.bin", tmp_path / "cool_bin2.bin", tmp_path / "short.bin")
    assert r.returncode == 1 and "disagree" in r.stderr


@needs_h5
@pytest.mark.parametrize("case", range(len(T["downsample"])))
def test_gd_downsample_equals_the_reference(programs, tmp_path, case):
    """The rows, names and coordinates of the reference's output; every value is the %g of a number within rtol 1e-12 of the
    reference's unrounded one (its text rounds to six digits, where a last-bit difference of the running sum can show)."""
    c = T["downsample"][case]
    table = tmp_path / "signals.tsv"
    table.write_text(T["compute_interactions_w4"])
    args = ["--rate", c["rate"]] + (["--window", c["window"]] if c["window"] else [])
    r = _run(programs["gd_downsample"], *args, table)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), c["output"].splitlines()
    values = Z[f"downsample_{c['rate']}_{c['window'] or 0}"]
    assert len(got) == len(want) == len(values) + 1 and got[0] == want[0]
    assert "nan" in r.stdout and "-nan" not in r.stdout
    for g, w, v in zip(got[1:], want[1:], values):
        g, w = g.split("\t"), w.split("\t")
        assert g[:3] == w[:3] and len(g) == len(w)
        for text, x in zip(g[3:], v):
            assert text in {f"{x:g}", f"{x * (1 - 1e-12):g}", f"{x * (1 + 1e-12):g}"}, (g, w)
    out = tmp_path / "out.tsv"
    r2 = _run(programs["gd_downsample"], *args, "-o", out, table)
    assert r2.returncode == 0 and r2.stdout == "" and out.read_text() == r.stdout
