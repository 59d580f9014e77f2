"""The compartment analysis on the device (include/gdyn_hic.h: the dense target, its profile, enrichment and principal components)
against the reference's own outputs (tests/golden/compartment_fixtures.npz, made by make_compartment_fixtures.py) by the rules of
DESIGN.md section 7f, against the restatement (tests/compartment_restatement.py) for shapes the fixture lacks, bad arguments, and
gd_hic_compartments end to end on a file written by gd_h5tool put-cool."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import compartment_restatement as R
import hic_restatement as HR
from conftest import ROOT

pytestmark = pytest.mark.gpu
hic = importlib.import_module("2022a-genome-dynamics_amd.hic")
HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
Z = np.load(os.path.join(ROOT, "tests", "golden", "compartment_fixtures.npz"))
H = np.load(os.path.join(ROOT, "tests", "golden", "hic_fixtures.npz"))
NAMES = ["1", "2", "X", "3"]
CHROM, BIN1, BIN2, COUNT, WEIGHT, BINSIZE = Z["chrom"], Z["bin1"], Z["bin2"], Z["count"], Z["weight"], int(Z["binsize"])
EXCLUDED = (CHROM == NAMES.index("X")).astype(np.uint8)
EINVAL, EUNSUPPORTED = "GD_EINVAL", "GD_EUNSUPPORTED"


def shuffled_ids(b1, b2, every=3):
    flip = np.arange(len(b1)) % every == 0
    return np.where(flip, b2, b1), np.where(flip, b1, b2)


def in_three_calls(hs, b1, b2, count):
    cuts = [0, 1500, 1501, len(count)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        hs.accumulate(b1[a:b], b2[a:b], count[a:b])


@pytest.fixture(scope="module")
def toy():
    """One handle with the RAW and the weighted dense target after one pass, their profiles taken."""
    with hic.HicSignals(CHROM) as hs:
        raw, weighted = hs.add_dense(), hs.add_dense(WEIGHT)
        with pytest.raises(hic.GdynError, match="GD_ESTATE"):
            hs.fetch_dense(raw, 0, hic.DENSE_ENRICHMENT)                                # before a profile
        hs.accumulate(BIN1, BIN2, COUNT)
        profiles = {"RAW": hs.dense_profile(raw, EXCLUDED), "weight": hs.dense_profile(weighted, EXCLUDED)}
        yield hs, {"RAW": raw, "weight": weighted}, profiles


# ---- the reference's outputs

@pytest.mark.parametrize("batch", [0, 7, 1000])
def test_dense_matrices_equal_the_reference_byte_for_byte(batch):
    """RAW and weighted, ids exchanged in every third pixel, the pixels handed over in three calls; the same bytes on a second
    run; a band and a distance profile fed by the same pass still equal their fixtures."""
    b1, b2 = shuffled_ids(BIN1, BIN2)
    runs = []
    for _ in range(2):
        with hic.HicSignals(CHROM, max_pixels_per_launch=batch) as hs:
            band, prof = hs.add_band(4), hs.add_distance_profile(EXCLUDED, None, 96)
            targets = {"RAW": hs.add_dense(), "weight": hs.add_dense(WEIGHT)}
            in_three_calls(hs, b1, b2, COUNT)
            got = {(norm, code): hs.fetch_dense(t, code) for norm, t in targets.items() for code in range(len(NAMES))}
            assert np.array_equal(hs.fetch_band(band), HR.band(BIN1, BIN2, COUNT, CHROM, 4))
            want_total, want_n = HR.profile(BIN1, BIN2, COUNT, CHROM, EXCLUDED, None, 96)
            assert np.array_equal(hs.fetch_profile_raw(prof), want_total) and np.array_equal(hs.fetch_profile(prof)[1], want_n)
        for (norm, code), m in got.items():
            want = Z[f"contact_{norm}_{code}"]
            assert m.dtype == np.float32 and m.shape == want.shape
            assert m.tobytes() == want.tobytes() or np.array_equal(m, want, equal_nan=True), (norm, code)
        assert np.isnan(got["weight", 0]).any() and got["RAW", 3].shape == (1, 1)
        runs.append({k: np.nan_to_num(m, nan=-1.0).tobytes() for k, m in got.items()})
    assert runs[0] == runs[1]


def test_existing_targets_of_the_stage_2_fixture_are_unchanged_beside_a_dense_target():
    """The bands and profiles of tests/golden/hic_fixtures.npz fed in one pass with a dense target."""
    chrom, b1, b2, count = H["chrom"], H["bin1"], H["bin2"], H["count"]
    names = ["1", "2", "3", "10", "4", "5", "X", "Y", "MT"]
    excluded = np.isin(chrom, [names.index(n) for n in ("X", "Y", "MT")]).astype(np.uint8)
    with hic.HicSignals(chrom, max_pixels_per_launch=1000) as hs:
        b4, dense, b6, raw = hs.add_band(4), hs.add_dense(), hs.add_band(6), hs.add_distance_profile(excluded, None, 110)
        hs.accumulate(b1, b2, count)
        assert np.array_equal(hs.fetch_band(b4), H["band4"]) and np.array_equal(hs.fetch_band(b6), H["band6"])
        total, n, mean = hs.fetch_profile(raw)
        assert np.array_equal(n, H["profile_n_RAW"]) and np.array_equal(mean, H["profile_mean_RAW"], equal_nan=True)
        want = R.dense(b1, b2, count, chrom)
        for code in range(len(names)):
            assert np.array_equal(hs.fetch_dense(dense, code), want[code])


def test_raw_profile_and_enrichment_equal_the_reference_bit_for_bit(toy):
    hs, targets, profiles = toy
    contacts, counts, mean = profiles["RAW"]
    assert counts.dtype == np.int64 and np.array_equal(counts, Z["counts_RAW"])
    assert mean.tobytes() == Z["mean_RAW"].tobytes() or np.array_equal(mean, Z["mean_RAW"], equal_nan=True)
    assert np.array_equal(np.isnan(mean), np.isnan(Z["mean_RAW"])) and np.isnan(mean).any()
    assert np.array_equal(contacts, R.profile({c: Z[f"contact_RAW_{c}"] for c in (0, 1, 3)})[0])
    for code in range(len(NAMES)):
        got, want = hs.fetch_dense(targets["RAW"], code, hic.DENSE_ENRICHMENT), Z[f"enrichment_RAW_{code}"]
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True), code
    again = hs.dense_profile(targets["RAW"], EXCLUDED)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, profiles["RAW"]))      # a reduction of fixed shape


def test_weighted_profile_and_enrichment_within_float32_summation(toy):
    """Identical NaN pattern and counts; values at rtol L 2^-24, L the longest diagonal: the bound of float32 summation of
    positive terms in any order, which the reference does per diagonal and the device does not.  The enrichment: one ulp more."""
    hs, targets, profiles = toy
    contacts, counts, mean = profiles["weight"]
    want = Z["mean_weight"]
    assert np.array_equal(counts, Z["counts_weight"]) and np.array_equal(np.isnan(mean), np.isnan(want))
    rtol = 96 * 2.0 ** -24
    print("weighted mean: max rel", np.nanmax(np.abs(mean - want) / want), "allowed", rtol)
    np.testing.assert_allclose(mean, want, rtol=rtol, atol=0)
    for code in range(len(NAMES)):
        got, ref = hs.fetch_dense(targets["weight"], code, hic.DENSE_ENRICHMENT), Z[f"enrichment_weight_{code}"]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), code
        np.testing.assert_allclose(got, ref, rtol=rtol + 2.0 ** -52, atol=0)
    valid = hs.dense_valid(targets["weight"])
    assert np.array_equal(valid, np.concatenate([R.valid(Z[f"contact_weight_{c}"]) for c in range(len(NAMES))])) and valid.any() and not valid.all()


@pytest.mark.parametrize("case", ["a", "b"])
def test_principal_components_equal_the_reference(toy, case):
    """(a) the 61-bin enrichment with the default mask, (b) the 96-bin one with an explicit mask."""
    hs, targets, _ = toy
    code, mask = (1, None) if case == "a" else (0, Z["pca_b_mask"])
    got = hs.dense_pca(targets["RAW"], code, hic.DENSE_ENRICHMENT, mask, 3)
    print("case", case, "iterations", got[3], "variances", got[1])
    assert 0 < got[3] < 200
    R.check_pca(got, Z[f"pca_{case}_pcs"], Z[f"pca_{case}_variances"], Z[f"pca_{case}_axes"], Z[f"pca_{case}_singular"], Z[f"pca_{case}_mask"], f"case {case}")
    second = hs.dense_pca(targets["RAW"], code, hic.DENSE_ENRICHMENT, mask, 3)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, second))      # a fixed start block
    # the same matrix through the door for host matrices
    third = hs.pca_matrix(Z[f"enrichment_RAW_{code}"], mask, 3)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, third))


def test_non_finite_submatrix_is_einval(toy):
    """(c) the 96-bin enrichment with the default mask (numpy raises LinAlgError), and a weighted matrix with the default mask."""
    hs, targets, _ = toy
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.dense_pca(targets["RAW"], 0, hic.DENSE_ENRICHMENT, None, 3)
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.dense_pca(targets["weight"], 1, hic.DENSE_CONTACT, None, 3)
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.pca_matrix(Z["enrichment_RAW_0"], None, 1)


# ---- against the restatement

def planted(n, period, seed, unmappable=()):
    """A symmetric n x n matrix with a checkerboard on a power-law decay and noise; rows and columns of `unmappable` zero."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    state = np.where((k // period) % 2 == 0, 1.0, -1.0)
    m = (1 + 0.5 * state[:, None] * state[None, :]) * (1 + 0.3 / (1 + np.abs(k[:, None] - k[None, :]))) + 0.2 * rng.standard_normal((n, n))
    m = (m + m.T) / 2
    m[list(unmappable), :] = 0
    m[:, list(unmappable)] = 0
    return m


@pytest.fixture(scope="module")
def big():
    m = planted(300, 25, 3, unmappable=(0, 17, 18, 100, 199, 250, 299))
    return m, R.pca(m, None, 8)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_300_bins_equal_the_restatement(toy, big, k):
    """m = 293: beyond one block of 256 rows, no multiple of 16 or of 64."""
    hs = toy[0]
    m, (pcs, var, axes, singular) = big
    mask = np.any(m != 0, axis=1)
    assert mask.sum() == 293
    got = hs.pca_matrix(m, None, k)
    print("k", k, "iterations", got[3])
    R.check_pca(got, pcs[:, :k], var[:k], axes[:k], singular, mask, f"300 bins, k = {k}")


def test_smallest_matrices(toy):
    hs = toy[0]
    m2 = np.array([[3.0, 1.0, 0.0], [0.5, 2.0, 0.0], [0.0, 0.0, 0.0]])                  # m = 2 of n = 3
    want = R.pca(m2, None, 1)
    R.check_pca(hs.pca_matrix(m2, None, 1), *want[:3], want[3], np.array([True, True, False]), "m = 2, k = 1")
    m3 = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.3, 0.1, 2.0]])
    want = R.pca(m3, None, 2)
    R.check_pca(hs.pca_matrix(m3, None, 2), *want[:3], want[3], np.ones(3, bool), "m = 3, k = 2")
    # k = m = 3: the centred matrix has rank m - 1, its last singular value vanishes (numpy: 1e-16 of the first) and u = Xc v / s
    # is not defined; the rule for a vanishing wanted component holds
    assert want[3][2] <= 1e-14 * want[3][0]
    with pytest.raises(hic.GdynError, match=EUNSUPPORTED):
        hs.pca_matrix(m3, None, 3)
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.pca_matrix(m3, None, 4)                                                      # k > m
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.pca_matrix(m3, [True, False, False], 1)                                      # m < 2


def test_unsymmetric_matrix(toy):
    rng = np.random.default_rng(70)
    m = planted(70, 9, 4) + 0.3 * rng.standard_normal((70, 70))
    assert not np.allclose(m, m.T)
    want = R.pca(m, None, 3)
    R.check_pca(toy[0].pca_matrix(m, None, 3), *want[:3], want[3], np.ones(70, bool), "unsymmetric 70 x 70")


def test_vanishing_component_is_unsupported(toy):
    """Rank 2 after centring: the third component does not exist."""
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal((40, 2)), rng.standard_normal((2, 40))
    m = a @ b + 1.0
    want = R.pca(m, None, 2)
    R.check_pca(toy[0].pca_matrix(m, None, 2), *want[:3], want[3], np.ones(40, bool), "rank 2, k = 2")
    with pytest.raises(hic.GdynError, match=EUNSUPPORTED) as e:
        toy[0].pca_matrix(m, None, 3)
    assert "vanishing" in str(e.value)


def test_bad_arguments(toy):
    hs, targets, _ = toy
    for k in (0, 9):
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.dense_pca(targets["RAW"], 1, hic.DENSE_ENRICHMENT, None, k)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.pca_matrix(np.eye(12), None, k)
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.fetch_dense(targets["RAW"], 99)                                              # a code the table lacks
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.dense_pca(targets["RAW"], 99, hic.DENSE_ENRICHMENT, None, 1)
    with pytest.raises(hic.GdynError, match=EINVAL):
        hs.fetch_dense(targets["RAW"], 1, 7)                                            # neither contact nor enrichment
    with pytest.raises(ValueError):
        hs.dense_pca(targets["RAW"], 1, hic.DENSE_ENRICHMENT, np.ones(5, bool), 1)
    with hic.HicSignals(CHROM) as other:
        band = other.add_band(4)
        for call in (lambda: other.dense_profile(band), lambda: other.fetch_dense(band, 0), lambda: other.dense_valid(band),
                     lambda: other.dense_pca(band, 0, hic.DENSE_CONTACT, None, 1), lambda: other.dense_profile(5)):
            with pytest.raises(hic.GdynError, match=EINVAL):
                call()                                                                  # a wrong target kind, no such target
        dense = other.add_dense()
        with pytest.raises(hic.GdynError, match="GD_ESTATE"):
            other.dense_pca(dense, 0, hic.DENSE_ENRICHMENT, None, 1)                    # enrichment before a profile
        with pytest.raises(hic.GdynError, match=EINVAL):
            other.fetch_band(dense)
    with hic.HicSignals(np.array([0, 0, 1, 0], np.int32)) as split:
        with pytest.raises(hic.GdynError, match=EINVAL):
            split.add_dense()                                                           # code 0 in two runs


# ---- the program, end to end

def python_table(names, k, chroms=None, weights=None):
    """What gd_hic_compartments prints, by the Python path."""
    lines, rows = [], []
    with hic.HicSignals(CHROM) as hs:
        d = hs.add_dense(weights)
        hs.accumulate(BIN1, BIN2, COUNT)
        hs.dense_profile(d, EXCLUDED)
        valid = hs.dense_valid(d)
        for code, name in enumerate(names):
            if chroms is not None and name not in chroms:
                continue
            sel = CHROM == code
            pcs, var, _, it = hs.dense_pca(d, code, hic.DENSE_ENRICHMENT, valid[sel], k)
            lines.append(f"# {name} variances " + " ".join(f"{v:g}" for v in var) + f" iterations {it}")
            for b, p in zip(np.flatnonzero(sel), pcs):
                rows.append("\t".join([name, str(Z["start"][b]), str(Z["end"][b])] + [f"{x:g}" for x in p]))
    return "\n".join(lines + ["\t".join(["chrom", "start", "end"] + [f"PC{j + 1}" for j in range(k)])] + rows) + "\n"


def test_gd_hic_compartments_prints_what_the_python_path_prints(tmp_path):
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_hic_compartments"])
    cool = tmp_path / "toy.mcool"
    r = HR.put_cool(os.path.join(HOST, "gd_h5tool"), tmp_path, cool, BINSIZE, NAMES, CHROM, Z["start"], Z["end"], BIN1, BIN2, COUNT, WEIGHT)
    assert r.returncode == 0, r.stderr
    run = lambda *args: subprocess.run([os.path.join(HOST, "gd_hic_compartments"), *map(str, args)], capture_output=True, text=True)
    r = run("-b", BINSIZE, "-k", 2, "--chroms", "2,X", cool)
    assert r.returncode == 0, r.stderr
    assert r.stdout == python_table(NAMES, 2, ("2", "X")) and "nan" in r.stdout and "-nan" not in r.stdout
    assert "device start-up" in r.stderr
    # every chromosome: the corners of "1" lie beyond the longest observed distance, their enrichment is NaN and the mask of
    # gd_hic_dense_valid keeps those bins
    r = run("-b", BINSIZE, "-k", 1, cool)
    assert r.returncode == 1 and "error: chromosome 1" in r.stderr and "not finite" in r.stderr
    r = run("-b", BINSIZE, "-k", 1, "--chroms", "3", cool)                              # one bin
    assert r.returncode == 1 and "error: chromosome 3" in r.stderr
    # weighted: no bin of X has pixels and a NaN weight, so its matrix is finite and the rows of its unmappable bin are zero
    r = run("-b", BINSIZE, "-n", "weight", "-k", 1, "--chroms", "X", cool)
    assert r.returncode == 0, r.stderr
    assert r.stdout == python_table(NAMES, 1, ("X",), WEIGHT) and len(r.stdout.splitlines()) == 2 + 20 and "nan" in r.stdout
    # a bin of "2" has pixels and a NaN weight: v is NaN in its row and in its column, so every row of the chromosome holds a
    # non-finite cell and the rule of gd_hic_dense_valid leaves no bin; the program says so
    r = run("-b", BINSIZE, "-n", "weight", "-k", 1, "--chroms", "2", "--exclude", "X", cool)
    assert r.returncode == 1 and "error: chromosome 2" in r.stderr and "0 valid bins" in r.stderr and r.stdout == ""
