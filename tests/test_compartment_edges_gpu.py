"""The compartment kernels (csrc/gdyn_hic.hip) past one block, against the restatement
(tests/compartment_restatement.py) on the inputs of tests/compartment_edge_cases.py:
  A  seven chromosomes of 300, 1, 64, 65, 257, 2 and 330 bins: the second block of distances and the one-row last row block of
     k_dense_profile, an excluded chromosome longer than every counted one, the second trip of k_row_flags;
  B  pixels that collide in a cell: the float32 atomic adds of k_hic_accumulate, infinite cells;
  C  the solver at every size where a grid, a loop or the split rule of k_pca_xty changes.
tests/test_compartment_host.py asserts on the CPU that every input reaches the branch it is here for."""
import importlib
import os
import time

import numpy as np
import pytest

import compartment_edge_cases as E
import compartment_restatement as R

pytestmark = pytest.mark.gpu
hic = importlib.import_module("2022a-genome-dynamics_amd.hic")
LIB = os.environ.get("GDYN_TEST_LIB") or None      # a developer build of csrc/ (conftest.py); the package itself reads no variable
NORMS = ("RAW", "weight")


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def worst(err, bound):
    """The largest err / bound where the bound is positive (elsewhere err must be 0: asserted by the caller)."""
    with np.errstate(all="ignore"):
        q = np.where(bound > 0, err / bound, 0.0)
    return float(np.nanmax(q)) if q.size else 0.0


# ---- A: seven chromosomes

@pytest.fixture(scope="module")
def seven():
    """One handle with the RAW and the weighted dense target of table A after one pass, their profiles taken."""
    t = E.table_a()
    with hic.HicSignals(t.chrom, path=LIB) as hs:
        targets = {"RAW": hs.add_dense(), "weight": hs.add_dense(t.weight)}
        hs.accumulate(t.bin1, t.bin2, t.count)
        profiles = {norm: hs.dense_profile(targets[norm], t.excluded) for norm in NORMS}
        yield hs, targets, profiles


@pytest.mark.parametrize("batch", [0, 7, 1000])
def test_dense_matrices_of_seven_chromosomes_byte_for_byte(batch):
    """Unique pixels: the same bytes as the restatement (NaN for NaN) for every launch size, with ids exchanged in every third
    pixel and the pixels handed over in three calls whose cuts are no multiples of 4."""
    t = E.table_a()
    b1, b2 = E.shuffled_ids(t.bin1, t.bin2)
    cuts = E.CUTS_A + (len(t.count),)
    with hic.HicSignals(t.chrom, max_pixels_per_launch=batch, path=LIB) as hs:
        targets = {"RAW": hs.add_dense(), "weight": hs.add_dense(t.weight)}
        for a, b in zip(cuts[:-1], cuts[1:]):
            hs.accumulate(b1[a:b], b2[a:b], t.count[a:b])
        for norm in NORMS:
            want = E.expected_a(norm).matrices
            for code, n in enumerate(E.SIZES):
                got = hs.fetch_dense(targets[norm], code)
                assert got.dtype == np.float32 and got.shape == (n, n)
                assert np.array_equal(got, want[code], equal_nan=True), (norm, code, int((~np.isclose(got, want[code], rtol=0, atol=0, equal_nan=True)).sum()))
    assert np.isnan(E.expected_a("weight").matrices[0]).sum() == 2 and not np.isnan(E.expected_a("RAW").matrices[0]).any()


def test_the_one_pass_handle_holds_the_same_matrices(seven):
    hs, targets, _ = seven
    for norm in NORMS:
        for code in range(len(E.SIZES)):
            assert np.array_equal(hs.fetch_dense(targets[norm], code), E.expected_a(norm).matrices[code], equal_nan=True), (norm, code)


def test_raw_profile_beyond_256_distances_is_exact(seven):
    """330 distances: two blocks of k_dense_profile; the 257-bin chromosome ends in a row block of one row; the excluded
    chromosome is the longest, so the distances from 300 on have no cell: counts 0, contacts 0, mean NaN."""
    hs, targets, profiles = seven
    x = E.expected_a("RAW")
    contacts, counts, mean = profiles["RAW"]
    assert len(mean) == 330 and counts.dtype == np.int64
    assert np.array_equal(counts, x.counts) and np.array_equal(contacts, x.contacts) and np.array_equal(mean, x.mean, equal_nan=True)
    assert np.array_equal(np.isnan(mean), np.isnan(x.mean))
    assert counts[256:300].any() and not counts[300:].any() and not contacts[300:].any() and np.isnan(mean[300:]).all() and not np.isnan(mean[:300]).any()
    again = hs.dense_profile(targets["RAW"], E.table_a().excluded)
    assert all(same_bytes(a, b) for a, b in zip(again, profiles["RAW"]))


def test_weighted_profile_within_the_order_of_an_fp64_sum(seven):
    """Counts and NaN pattern equal; contacts and mean at rtol counts[d] 2^-52, the bound between two orders of an fp64 sum of
    positive terms: both sides add the same float32 cells in fp64.  Measured on an MI355X: the error is 0, here and in the
    weighted enrichment (at most 300 float32 cells within a factor 2^20 of each other: their fp64 sum is exact in any order)."""
    hs, targets, profiles = seven
    x = E.expected_a("weight")
    contacts, counts, mean = profiles["weight"]
    assert np.array_equal(counts, x.counts) and np.array_equal(np.isnan(mean), np.isnan(x.mean)) and np.array_equal(np.isnan(contacts), np.isnan(x.contacts))
    assert not np.isnan(contacts).any() and np.isnan(mean[300:]).all() and not contacts[300:].any()
    bound = counts * 2.0 ** -52
    for name, got, want in (("contacts", contacts, x.contacts), ("mean", mean, x.mean)):
        live = counts > 0
        err = np.abs(got[live] - want[live]) / np.abs(want[live])
        print(f"weighted {name}: largest error over its bound {worst(err, bound[live]):.3g}")
        assert (err <= bound[live]).all(), (name, worst(err, bound[live]))
    again = hs.dense_profile(targets["weight"], E.table_a().excluded)
    assert all(same_bytes(a, b) for a, b in zip(again, profiles["weight"]))


@pytest.mark.parametrize("code", [0, 4, 6])
def test_enrichment_of_the_long_chromosomes(seven, code):
    """RAW exactly; weighted with the same NaN pattern at rtol counts[|i - j|] 2^-52 + 2^-52 (the mean's bound and one division);
    the excluded chromosome 6 is NaN exactly where |i - j| >= 300."""
    hs, targets, _ = seven
    for norm in NORMS:
        x = E.expected_a(norm)
        got, want = hs.fetch_dense(targets[norm], code, hic.DENSE_ENRICHMENT), x.enrichment[code]
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (norm, code)
        if norm == "RAW":
            assert np.array_equal(got, want, equal_nan=True), code
        else:
            bound = x.counts[x.distance[code]] * 2.0 ** -52 + 2.0 ** -52
            live = ~np.isnan(want) & (want != 0)
            err = np.abs(got[live] - want[live]) / np.abs(want[live])
            print(f"weighted enrichment of chromosome {code}: largest error over its bound {worst(err, bound[live]):.3g}")
            assert (err <= bound[live]).all() and np.array_equal(got == 0, want == 0), (code, worst(err, bound[live]))
        if code == 6:
            assert np.array_equal(np.isnan(got), x.distance[6] >= 300) and np.isnan(got).any()
        if code == 0 and norm == "RAW":
            assert not np.isnan(got).any()


def test_valid_bins_seen_only_by_the_second_trip(seven):
    """Bin 40's one cell is in column 299 and bin 42's one NaN is in column 280: a scan of the first 256 columns misses both."""
    hs, targets, _ = seven
    raw, weighted = hs.dense_valid(targets["RAW"]), hs.dense_valid(targets["weight"])
    assert np.array_equal(raw, E.expected_a("RAW").valid) and np.array_equal(weighted, E.expected_a("weight").valid)
    assert raw[E.ONLY_FAR] and weighted[E.ONLY_FAR]
    assert not raw[E.EMPTY] and not weighted[E.EMPTY]
    assert raw[E.PARTNER] and not weighted[E.PARTNER]
    assert raw[E.NAN_WEIGHT] and not weighted[E.NAN_WEIGHT]
    assert raw.sum() == len(raw) - 1 and weighted.sum() == len(raw) - 3


def test_default_mask_of_the_components_scans_the_whole_row(seven):
    """dense_pca on the RAW contact matrix of chromosome 0 with the default mask (k_row_flags<double>): bin 40 is kept, bin 41
    is dropped, and the components are the restatement's."""
    hs, targets, _ = seven
    matrix = E.expected_a("RAW").matrices[0].astype(np.float64)
    pcs, var, axes, singular = R.pca(matrix, None, 3)
    mask = np.any(matrix != 0, axis=1)
    assert mask[E.ONLY_FAR] and not mask[E.EMPTY] and mask.sum() == 299
    got = hs.dense_pca(targets["RAW"], 0, hic.DENSE_CONTACT, None, 3)
    print("chromosome 0, RAW contact matrix: iterations", got[3])
    assert 0 < got[3] < 1000
    assert not np.isnan(got[0][E.ONLY_FAR]).any() and np.isnan(got[0][E.EMPTY]).all()
    R.check_pca(got, pcs, var, axes, singular, mask, "chromosome 0, default mask")


# ---- B: colliding adds

def one_cell(batch, i, j, weights=None, c=1):
    with hic.HicSignals(E.CHROM_B, max_pixels_per_launch=batch, path=LIB) as hs:
        d = hs.add_dense(weights)
        hs.accumulate(np.full(E.REPEATS, i, np.int64), np.full(E.REPEATS, j, np.int64), np.full(E.REPEATS, c, np.int32))
        return hs.fetch_dense(d, 0), hs.fetch_dense(d, 1), hs.dense_profile(d)


@pytest.mark.parametrize("batch", [0, 64])
def test_identical_pixels_add_up_exactly(batch):
    """6 000 times the pixel (2, 5, 1) in one call: both cells are 6000.0; the diagonal pixel (3, 3, 1): 12000.0.  A read-add-write
    that is not atomic loses adds."""
    m, other, _ = one_cell(batch, 2, 5)
    want = np.zeros((8, 8), np.float32)
    want[2, 5] = want[5, 2] = E.REPEATS
    assert same_bytes(m, want) and not other.any(), (m[2, 5], m[5, 2])
    m, other, _ = one_cell(batch, 3, 3)
    want = np.zeros((8, 8), np.float32)
    want[3, 3] = 2 * E.REPEATS
    assert same_bytes(m, want) and not other.any(), m[3, 3]


@pytest.mark.parametrize("batch", [0, 64])
def test_split_counts_give_the_same_bytes(batch):
    """Integer cell totals below 2^24: c handed over as c1 + c2 in shuffled order over two calls is c."""
    one, two = E.split_counts()
    want = R.dense(*one, E.CHROM_B)[0]
    got = []
    for b1, b2, c in (one, two):
        with hic.HicSignals(E.CHROM_B, max_pixels_per_launch=batch, path=LIB) as hs:
            d = hs.add_dense()
            half = len(c) // 2 + 1
            hs.accumulate(b1[:half], b2[:half], c[:half])
            hs.accumulate(b1[half:], b2[half:], c[half:])
            got.append(hs.fetch_dense(d, 0))
    assert same_bytes(got[0], want) and same_bytes(got[1], want)


@pytest.mark.parametrize("batch", [0, 64])
def test_repeated_weighted_adds_round_once_each(batch):
    """The case whose last bits depend on the arrival order (section 7f, rule 1): no byte equality, but each float32 add of
    positive terms rounds once, so the cell is within 6000 2^-24 of the fp64 value 6000 c / (w_i w_j); the profile counts the
    cell once.  Measured on an MI355X: the error is 0.12 of the bound at either launch size."""
    m, _, (contacts, counts, mean) = one_cell(batch, 2, 5, E.WEIGHT_B, E.COUNT_WEIGHTED)
    exact = E.REPEATS * E.COUNT_WEIGHTED / (E.WEIGHT_B[2] * E.WEIGHT_B[5])
    bound = E.REPEATS * 2.0 ** -24
    err = abs(float(m[2, 5]) - exact) / exact
    print(f"{E.REPEATS} weighted adds, batch {batch}: error over its bound {err / bound:.4f}")
    assert m[2, 5] == m[5, 2] and err <= bound, (m[2, 5], exact, err / bound)
    assert np.count_nonzero(m) == 2
    assert counts.tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and contacts[3] == float(m[2, 5]) and mean[3] == float(m[2, 5])


@pytest.mark.parametrize("batch", [0, 64])
def test_a_zero_weight_gives_infinite_cells_that_count(batch):
    """Section 7f, rule 2: infinite cells count.  The bin with w = 0 has two pixels: +inf in the matrix, in contacts and in the
    mean at their distances; the enrichment there is 0 for finite cells and NaN for the infinite ones; the bin and its partners
    are not valid.  Everything equals the restatement."""
    b1, b2, c = E.PIXELS_ZERO
    want = R.dense(b1, b2, c, E.CHROM_ZERO, E.WEIGHT_ZERO)
    w_contacts, w_counts, w_mean = R.profile(want)
    with hic.HicSignals(E.CHROM_ZERO, max_pixels_per_launch=batch, path=LIB) as hs:
        d = hs.add_dense(E.WEIGHT_ZERO)
        hs.accumulate(b1, b2, c)
        got = {code: hs.fetch_dense(d, code) for code in (0, 1)}
        contacts, counts, mean = hs.dense_profile(d)
        enrichment = {code: hs.fetch_dense(d, code, hic.DENSE_ENRICHMENT) for code in (0, 1)}
        valid = hs.dense_valid(d)
    z = E.ZERO_BIN
    for code in (0, 1):
        assert np.array_equal(got[code], want[code], equal_nan=True) and not np.isnan(got[code]).any()
        assert np.array_equal(enrichment[code], R.enrichment(want[code], w_mean), equal_nan=True), code
    m = got[0]
    assert all(m[z, p] == np.inf and m[p, z] == np.inf for p in E.ZERO_PARTNERS) and np.isinf(m).sum() == 4
    assert np.array_equal(counts, w_counts) and np.array_equal(contacts, w_contacts) and np.array_equal(mean, w_mean, equal_nan=True)
    assert counts.tolist() == [2, 4, 3, 1, 0] and np.isinf(contacts[[1, 2]]).all() and np.isinf(mean[[1, 2]]).all() and np.isnan(mean[4])
    e = enrichment[0]
    assert np.isnan(e[1, 2]) and np.isnan(e[2, 4]) and e[0, 1] == 0 and e[3, 4] == 0 and e[1, 3] == 0 and e[0, 0] > 0
    assert np.array_equal(valid, np.concatenate([R.valid(want[0]), R.valid(want[1])]))
    assert valid.tolist() == [True, False, False, True, False, True, True, True]


# ---- C: the solver across its boundaries

@pytest.fixture(scope="module")
def solver():
    with hic.HicSignals(np.zeros(2, np.int32), path=LIB) as hs:
        yield hs


def run_solver(hs, m, k, sym):
    matrix, mask, (pcs, var, axes, singular) = E.pca_reference(m, sym)
    assert mask.sum() == m
    what = f"m = {m}, k = {k}" + ("" if sym else ", unsymmetric")
    t0 = time.perf_counter()
    got = hs.pca_matrix(matrix, None, k)
    print(f"{what}: iterations {got[3]}, {time.perf_counter() - t0:.3f} s")
    assert 0 < got[3] < 1000
    R.check_pca(got, pcs[:, :k], var[:k], axes[:k], singular, mask, what)
    if m in E.PCA_TWICE and sym:
        again = hs.pca_matrix(matrix, None, k)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again)), what


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("m", E.PCA_SIZES)
def test_solver_at_the_boundaries_of_its_grids(solver, m, k):
    """m = 9: the block is the whole space; 16 / 17: one and two splits; 64 / 65: one and two column stripes; 128 / 129 and
    256 / 257: the row blocks; 512: the last size of one trip of the wave loop; 513: 32 splits, the last one empty, a second
    trip of one row; 600: 19 rows a split; 1030: 33 rows a split, a third trip.  Measured on an MI355X: 4 iterations at every
    size (1 at m = 9), the largest error 3.3e-3 of its bound (m = 255 and 513, k = 3)."""
    run_solver(solver, m, k, True)


@pytest.mark.parametrize("m", E.PCA_UNSYMMETRIC)
def test_solver_on_unsymmetric_matrices(solver, m):
    matrix = E.pca_reference(m, False)[0]
    assert not np.array_equal(matrix, matrix.T)
    run_solver(solver, m, 3, False)
