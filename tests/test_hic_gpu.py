"""The Hi-C signal analyses on the device (include/gdyn_hic.h, csrc/gdyn_hic.hip) against the reference's own outputs
(tests/golden/hic_fixtures.npz and .json, made by make_hic_fixtures.py) by the rules of DESIGN.md section 7e, against the
restatement (tests/hic_restatement.py) for short chromosomes and at the scale of a 100 kb human cooler, byte-identical integer
targets for every launch size and from run to run, ignored out-of-range bin ids, bad arguments, and the four programs end to end
on a file written by gd_h5tool put-cool."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import hic_restatement as R
from conftest import ROOT
from test_hic_host import BIN1, BIN2, BINSIZE, CHROM, COUNT, NAMES, T, WEIGHT, WIDTHS, Z, same_signal

pytestmark = pytest.mark.gpu
hic = importlib.import_module("2022a-genome-dynamics_amd.hic")
HOST = os.path.join(ROOT, "2022a-genome-dynamics_amd", "host")
EINVAL = "GD_EINVAL"
SIZE = hic.largest_chromosome(CHROM)
EXCLUDED = hic.excluded_bins(CHROM, {n: k for k, n in enumerate(NAMES)})


def shuffled_ids(b1, b2, every=3):
    """The same pixels with the two ids of every third one exchanged."""
    flip = np.arange(len(b1)) % every == 0
    return np.where(flip, b2, b1), np.where(flip, b1, b2)


# ---- the reference's outputs

@pytest.mark.parametrize("batch", [0, 7, 1000])
def test_every_target_in_one_pass_equals_the_reference(batch):
    """Bands of 4, 6, 11 and 51 columns and both distance profiles fed by one pass, the pixels handed over in three calls."""
    b1, b2 = shuffled_ids(BIN1, BIN2)
    with hic.HicSignals(CHROM, max_pixels_per_launch=batch) as hs:
        bands = {W: hs.add_band(W) for W in [4, 6] + [w + 1 for w in WIDTHS]}
        raw = hs.add_distance_profile(EXCLUDED, None, SIZE)
        weighted = hs.add_distance_profile(EXCLUDED, WEIGHT, SIZE)
        cuts = [0, 1500, 1501, len(COUNT)]
        for a, b in zip(cuts[:-1], cuts[1:]):
            hs.accumulate(b1[a:b], b2[a:b], COUNT[a:b])
        hs.accumulate(b1[:0], b2[:0], COUNT[:0])                                       # n == 0 is a no-op
        for W, t in bands.items():
            got = hs.fetch_band(t)
            want = Z[f"band{W}"] if W in (4, 6) else Z[f"alpha_band{W - 1}"]
            assert got.dtype == np.int64 and np.array_equal(got, want), W
        # rule 2: identical NaN pattern, finite values within 4 ulp, wherever the reference runs
        for W in (4, 6):
            D, I = hs.decay_insulation(bands[W])
            held = Z[f"held{W}"]
            same_signal(D[held], Z[f"decay{W}"][held], 4, f"device D, W = {W}")
            same_signal(I[held], Z[f"insulation{W}"][held], 4, f"device I, W = {W}")
            Dr, Ir = R.decay_insulation(Z[f"band{W}"], CHROM)                           # MT and, for W = 6, two more chromosomes
            assert np.isfinite(Dr[~held]).any()
            same_signal(D[~held], Dr[~held], 4, f"device D against the restatement, W = {W}")
            same_signal(I[~held], Ir[~held], 4, f"device I against the restatement, W = {W}")
        # rule 3, both layers
        for width in WIDTHS:
            alpha = hs.local_alpha(bands[width + 1])
            ref, gap = Z[f"alpha_ref{width}"], float(Z[f"alpha_fp32_gap{width}"])
            mine = R.local_alpha(Z[f"alpha_band{width}"], CHROM)
            assert np.array_equal(np.isnan(alpha), np.isnan(mine)) and np.array_equal(np.isnan(alpha), np.isnan(ref))
            print("width", width, "device against restatement, max rel", np.nanmax(np.abs(alpha - mine) / np.abs(mine)), "against the reference",
                  np.nanmax(np.abs(alpha - ref)), "allowed", 4 * gap)
            np.testing.assert_allclose(alpha, mine, rtol=1e-10, atol=0)
            assert np.nanmax(np.abs(alpha - ref)) <= 4 * gap
        # rule 4
        total, n, mean = hs.fetch_profile(raw)
        exact = hs.fetch_profile_raw(raw)
        want_total, want_n = R.profile(BIN1, BIN2, COUNT, CHROM, EXCLUDED, None, SIZE)
        assert exact.dtype == np.int64 and np.array_equal(exact, want_total) and np.array_equal(n, want_n) and np.array_equal(n, Z["profile_n_RAW"])
        assert np.array_equal(total, exact.astype(np.float64)) and np.array_equal(mean, Z["profile_mean_RAW"], equal_nan=True)
        total, n, mean = hs.fetch_profile(weighted)
        want = Z["profile_mean_weight"]
        assert np.array_equal(n, Z["profile_n_weight"]) and np.array_equal(np.isnan(mean), np.isnan(want))
        rtol = int(Z["profile_n_weight"].max()) * 2.0 ** -52
        print("weighted P(s): max relative difference", np.nanmax(np.abs(mean - want) / want), "allowed", rtol)
        np.testing.assert_allclose(mean, want, rtol=rtol, atol=0)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.fetch_profile_raw(weighted)
        # reset zeroes, the targets stay
        hs.reset()
        assert not hs.fetch_band(bands[4]).any() and not hs.fetch_profile(weighted)[1].any() and np.isnan(hs.fetch_profile(raw)[2]).all()
        hs.accumulate(BIN1, BIN2, COUNT)
        assert np.array_equal(hs.fetch_band(bands[6]), Z["band6"]) and np.array_equal(hs.fetch_profile_raw(raw), want_total)


def test_short_chromosome_follows_the_rule():
    """n = 7, W = 6 (where the reference asserts) beside a chromosome of one bin and one of two, against the restatement."""
    rng = np.random.default_rng(11)
    chrom = np.array([0] * 7 + [1] + [2] * 2 + [3] * 12, np.int32)
    i, j = np.triu_indices(len(chrom))
    keep = (chrom[i] == chrom[j]) & (i != 3) & (j != 3) & (rng.random(len(i)) < 0.85)
    i, j = i[keep], j[keep]
    count = rng.integers(1, 900, size=len(i)).astype(np.int32)
    with hic.HicSignals(chrom) as hs:
        t = hs.add_band(6)
        hs.accumulate(i, j, count)
        band = hs.fetch_band(t)
        assert np.array_equal(band, R.band(i, j, count, chrom, 6))
        D, I = hs.decay_insulation(t)
        Dr, Ir = R.decay_insulation(band, chrom)
        assert np.isfinite(Dr[:7]).any() and np.isnan(Dr[7]).all() and np.isfinite(Dr[8:10, 0]).any() and np.isnan(Dr[8:10, 1:]).all()
        same_signal(D, Dr, 4, "device D, short chromosomes")
        same_signal(I, Ir, 4, "device I, short chromosomes")
        alpha = hs.local_alpha(t)
        mine = R.local_alpha(band, chrom)
        assert np.array_equal(np.isnan(alpha), np.isnan(mine)) and np.isnan(mine[7]) and np.isfinite(mine[:7]).any()
        np.testing.assert_allclose(alpha, mine, rtol=1e-10, atol=0)


# ---- scale

def scale_cooler(seed=5):
    """About 30 000 bins in 24 chromosomes (the largest beyond the LDS budget of a profile) and a few million unique pixels in
    cooler order: contacts falling as a power of the distance, trans pixels, unmappable bins, weights with NaNs."""
    rng = np.random.default_rng(seed)
    sizes = np.array([5000, 2000, 1800, 1700, 1800, 1700, 1600, 1450, 1400, 1350, 1350, 1300, 1150, 1050, 1000, 900, 800, 800, 600, 650, 450, 500, 1000, 570])
    chrom = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    n = len(chrom)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    last = (first + sizes)[chrom]
    mappable = rng.random(n) > 0.05
    bins = np.arange(n)
    near_i, near_j = [], []
    for d in range(400):                                   # every separation up to 400 bins, thinning with the distance
        keep = (bins + d < last) & (rng.random(n) < min(1.0, 9.0 / (d + 1) ** 0.9))
        near_i.append(bins[keep])
        near_j.append(bins[keep] + d)
    m = 1_000_000                                          # and a heavy tail of long cis separations
    i = rng.integers(0, n, size=m)
    j = i + np.minimum(rng.pareto(0.35, size=m), 10.0 * n).astype(np.int64)
    cis = j < last[i]
    t = 900_000
    ti, tj = rng.integers(0, n, size=t), rng.integers(0, n, size=t)
    i, j = np.concatenate(near_i + [i[cis], np.minimum(ti, tj)]), np.concatenate(near_j + [j[cis], np.maximum(ti, tj)])
    ok = mappable[i] & mappable[j]
    key = np.unique(i[ok] * n + j[ok])
    i, j = key // n, key % n
    count = (1 + rng.poisson(np.where(chrom[i] == chrom[j], 400.0 / (j - i + 1.0), 0.3))).astype(np.int32)
    weights = rng.uniform(0.4, 1.6, n)
    weights[~mappable] = np.nan
    return chrom, sizes, i, j, count, weights


def test_scale_case_equals_the_restatement():
    chrom, sizes, b1, b2, count, weights = scale_cooler()
    assert len(sizes) == 24 and 29_000 < len(chrom) < 33_000 and len(count) > 2_500_000 and (chrom[b1] != chrom[b2]).sum() > 500_000
    size = int(sizes.max())
    assert size > 4096                                                                 # GD_HIC_LDS_BINS: LDS and global bins in one profile
    excluded = np.isin(chrom, [22, 23]).astype(np.uint8)
    f1, f2 = shuffled_ids(b1, b2, every=5)
    with hic.HicSignals(chrom) as hs:
        b4, b51 = hs.add_band(4), hs.add_band(51)
        raw, weighted = hs.add_distance_profile(excluded, None, size), hs.add_distance_profile(excluded, weights, size)
        hs.accumulate(f1, f2, count)
        band4, band51 = R.band_fast(b1, b2, count, chrom, 4), R.band_fast(b1, b2, count, chrom, 51)
        assert np.array_equal(hs.fetch_band(b4), band4) and np.array_equal(hs.fetch_band(b51), band51)
        D, I = hs.decay_insulation(b4)
        Dr, Ir = R.decay_insulation(band4, chrom)
        assert np.isnan(Dr).any() and np.isfinite(Dr).mean() > 0.7
        same_signal(D, Dr, 4, "device D, scale")
        same_signal(I, Ir, 4, "device I, scale")
        alpha = hs.local_alpha(b51)
        mine = R.local_alpha(band51, chrom)
        assert np.array_equal(np.isnan(alpha), np.isnan(mine)) and np.isfinite(mine).mean() > 0.9
        print("scale alpha: max rel", np.nanmax(np.abs(alpha - mine) / np.abs(mine)))
        np.testing.assert_allclose(alpha, mine, rtol=1e-10, atol=0)
        want_total, want_n = R.profile(b1, b2, count, chrom, excluded, None, size)
        assert np.array_equal(hs.fetch_profile_raw(raw), want_total) and np.array_equal(hs.fetch_profile(raw)[1], want_n)
        assert want_n[:4096].any() and want_n[4096:].any()
        want_total, want_n = R.profile(b1, b2, count, chrom, excluded, weights, size)
        total, n, mean = hs.fetch_profile(weighted)
        assert np.array_equal(n, want_n)
        rtol = int(want_n.max()) * 2.0 ** -52
        keep = want_n > 0
        print("scale weighted P(s): max rel", np.abs(total[keep] - want_total[keep]).max() / want_total[keep].min(), "N", want_n.max(), "allowed", rtol)
        np.testing.assert_allclose(total[keep], want_total[keep], rtol=rtol, atol=0)
        np.testing.assert_allclose(mean[keep], (want_total / np.maximum(want_n, 1))[keep], rtol=rtol, atol=0)
        assert np.isnan(mean[~keep]).all()


def test_integer_targets_are_the_same_bytes_for_every_launch_size_and_run():
    chrom, sizes, b1, b2, count, _ = scale_cooler(seed=6)
    size = int(sizes.max())
    results = []
    for batch in (1000, 65536, 0, 0):
        with hic.HicSignals(chrom, max_pixels_per_launch=batch) as hs:
            b4, b11 = hs.add_band(4), hs.add_band(11)
            first, second = hs.add_distance_profile(None, None, size), hs.add_distance_profile(None, None, size)      # LDS, then global only
            # a small launch size over every pixel would take thousands of launches: the first 200 000 pixels at 1000, all of
            # them otherwise, compared like for like below
            m = 200_000 if batch == 1000 else len(count)
            hs.accumulate(b1[:m], b2[:m], count[:m])
            results.append([hs.fetch_band(b4).tobytes(), hs.fetch_band(b11).tobytes(), hs.fetch_profile_raw(first).tobytes(), hs.fetch_profile(first)[1].tobytes(),
                            hs.fetch_profile_raw(second).tobytes(), hs.fetch_profile(second)[1].tobytes()])
            if batch == 65536:
                hs.reset()
                hs.accumulate(b1[:200_000], b2[:200_000], count[:200_000])
                head = [hs.fetch_band(b4).tobytes(), hs.fetch_band(b11).tobytes(), hs.fetch_profile_raw(first).tobytes(), hs.fetch_profile(first)[1].tobytes(),
                        hs.fetch_profile_raw(second).tobytes(), hs.fetch_profile(second)[1].tobytes()]
    assert results[0] == head                                                          # 1 000 against 65 536 per launch
    assert results[1] == results[2] == results[3]                                      # 65 536, automatic, automatic again
    assert results[2][2] == results[2][4] and results[2][3] == results[2][5]           # the LDS histogram and the global atomics agree
    assert np.frombuffer(results[2][0], np.int64).any()


def test_out_of_range_bin_ids_are_ignored():
    n = len(CHROM)
    bad1 = np.array([-1, 5, n, 2 ** 40, -2 ** 62, 3, 2 ** 31 + 4, n - 1], np.int64)
    bad2 = np.array([3, n, 7, 0, 1, -7, 4, 2 ** 32 + n - 1], np.int64)
    b1, b2, c = np.concatenate([bad1, BIN1, bad1]), np.concatenate([bad2, BIN2, bad2]), np.concatenate([np.full(8, 99, np.int32), COUNT, np.full(8, 77, np.int32)])
    with hic.HicSignals(CHROM, max_pixels_per_launch=999) as hs:
        band, raw = hs.add_band(4), hs.add_distance_profile(EXCLUDED, None, SIZE)
        hs.accumulate(b1, b2, c)
        assert np.array_equal(hs.fetch_band(band), Z["band4"])
        assert np.array_equal(hs.fetch_profile(raw)[2], Z["profile_mean_RAW"], equal_nan=True)


def test_bad_arguments():
    with pytest.raises(hic.GdynError, match=EINVAL):
        hic.HicSignals(CHROM, device=99)
    with pytest.raises(hic.GdynError, match=EINVAL):
        hic.HicSignals(np.zeros(0, np.int32))
    with hic.HicSignals(CHROM) as hs:
        with pytest.raises(hic.GdynError, match="GD_ESTATE"):
            hs.accumulate(BIN1[:4], BIN2[:4], COUNT[:4])                                # no target yet
        for W in (0, 4097):
            with pytest.raises(hic.GdynError, match=EINVAL):
                hs.add_band(W)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.add_distance_profile(EXCLUDED, None, 0)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.add_distance_profile(EXCLUDED, None, SIZE - 1)                           # chromosome 1 spans SIZE bins
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.add_distance_profile(None, None, 40)
        with pytest.raises(ValueError):
            hs.add_distance_profile(EXCLUDED[:-1], None, SIZE)
        with pytest.raises(ValueError):
            hs.accumulate(BIN1, BIN2[:-1], COUNT)
        assert hs._targets == []
        one, band, prof = hs.add_band(1), hs.add_band(2), hs.add_distance_profile(None, None, SIZE)
        hs.accumulate(BIN1, BIN2, COUNT)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.decay_insulation(one)                                                    # no D1 in a band of one column
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.local_alpha(one)
        D, I = hs.decay_insulation(band)
        assert D.shape == (len(CHROM), 1) and I.shape == (len(CHROM), 0) and np.isfinite(D).any()
        assert hs.local_alpha(band).shape == (len(CHROM),)                              # one separation: 0 / 0
        for call in (hs.fetch_band, hs.decay_insulation, hs.local_alpha):
            with pytest.raises(hic.GdynError, match=EINVAL):
                call(prof)                                                              # not a band
            with pytest.raises(hic.GdynError, match=EINVAL):
                call(9)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.fetch_profile(band)
        for _ in range(5):
            hs.add_band(1)
        with pytest.raises(hic.GdynError, match=EINVAL):
            hs.add_band(1)                                                              # GD_HIC_MAX_TARGETS
        hs.clear()
        with pytest.raises(hic.GdynError, match="GD_ESTATE"):
            hs.accumulate(BIN1[:4], BIN2[:4], COUNT[:4])
    d = hic.load_hic_library()
    assert d.gd_hic_destroy(None) == 0 and d.gd_hic_reset(None) != 0 and d.gd_hic_accumulate(None, None, None, None, 0) != 0


# ---- the programs, end to end

@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", "gd_h5tool", "gd_compute_interactions", "gd_compute_local_alpha", "gd_hic_power_law",
                           "gd_downsample"])
    d = tmp_path_factory.mktemp("hic")
    cool = d / "toy.mcool"
    r = R.put_cool(os.path.join(HOST, "gd_h5tool"), d, cool, BINSIZE, NAMES, CHROM, Z["start"], Z["end"], BIN1, BIN2, COUNT, WEIGHT)
    assert r.returncode == 0, r.stderr
    return d, cool


def _run(program, *args):
    return subprocess.run([os.path.join(HOST, program), *map(str, args)], capture_output=True, text=True)


def test_gd_compute_interactions_prints_the_reference_text(toy):
    d, cool = toy
    r = _run("gd_compute_interactions", "-b", BINSIZE, cool)
    assert r.returncode == 0, r.stderr
    assert r.stdout == T["compute_interactions_w4"]
    assert "read" in r.stderr and "device start-up" in r.stderr
    r2 = _run("gd_compute_interactions", "-b", BINSIZE, "-w", 4, "-o", d / "signals.tsv", cool)
    assert r2.returncode == 0 and r2.stdout == "" and (d / "signals.tsv").read_text() == T["compute_interactions_w4"]
    r3 = _run("gd_compute_interactions", "-b", BINSIZE, "-w", 6, cool)                  # where the reference asserts: rows by the rule
    assert r3.returncode == 0, r3.stderr
    lines = r3.stdout.splitlines()
    assert lines[0].split("\t") == ["chrom", "start", "end", "D1", "D2", "D3", "D4", "D5", "I1", "I2", "I3", "I4"]
    assert len(lines) == len(T["compute_interactions_w4"].splitlines()) and "-nan" not in r3.stdout


def test_signal_table_goes_through_gd_downsample(toy):
    d, cool = toy
    assert _run("gd_compute_interactions", "-b", BINSIZE, "-o", d / "table.tsv", cool).returncode == 0
    r = _run("gd_downsample", "--rate", 2, d / "table.tsv")
    assert r.returncode == 0 and r.stdout == T["downsample"][0]["output"]              # rate 2, window 2: no halfway digits in this table


@pytest.mark.parametrize("width", WIDTHS)
def test_gd_compute_local_alpha_matches_the_reference_text(toy, width):
    """Names, coordinates and rows are the reference's; the alpha column at the tolerance of rule 3 (plus the six digits of %g)."""
    d, cool = toy
    r = _run("gd_compute_local_alpha", "-w", width, "-b", BINSIZE, cool)
    assert r.returncode == 0, r.stderr
    got, want = [l.split("\t") for l in r.stdout.splitlines()], [l.split("\t") for l in T[f"compute_local_alpha_w{width}"].splitlines()]
    assert len(got) == len(want) == len(CHROM) + 1 and got[0] == want[0]
    assert [g[:3] for g in got] == [w[:3] for w in want]
    a, b = np.array([float(g[3]) for g in got[1:]]), np.array([float(w[3]) for w in want[1:]])
    assert np.array_equal(np.isnan(a), np.isnan(b)) and "-nan" not in r.stdout
    gap = float(Z[f"alpha_fp32_gap{width}"])
    # both columns are rounded to six significant digits: half a unit of the sixth digit each
    rounding = 2 * 0.5e-5 * np.maximum(np.abs(b), 1e-300)
    print("width", width, "max |alpha - reference| in the text", np.nanmax(np.abs(a - b)))
    assert (np.abs(a - b)[~np.isnan(b)] <= (4 * gap + rounding)[~np.isnan(b)]).all()


@pytest.mark.parametrize("normalize", ["RAW", "weight"])
def test_gd_hic_power_law_prints_the_reference_text(toy, normalize):
    d, cool = toy
    r = _run("gd_hic_power_law", "--binsize", BINSIZE, "--normalize", normalize, cool)
    assert r.returncode == 0, r.stderr
    assert r.stdout == T[f"hic_power_law_{normalize}"]
