"""The rules of the compartment analysis in plain numpy, written from the rules and not from hic.py: dense
cis matrices of a pixel table, the mean contact per distance, observed / expected, the validity of a bin, the leading principal
components with the sign rule, and the tolerances of the principal components that follow from the stopping residual."""
import numpy as np

RHO = 1e-12                     # the stopping residual of the block iteration, relative to the largest eigenvalue
LAPACK = 64 * 2.0 ** -52        # the allowance for the error of the SVD the values are compared with


def runs(chrom):
    chrom = np.asarray(chrom)
    cuts = [0] + [k for k in range(1, len(chrom)) if chrom[k] != chrom[k - 1]] + [len(chrom)]
    return list(zip(cuts[:-1], cuts[1:]))


def dense(bin1, bin2, count, chrom, weights=None):
    """{code: float32 (n, n)}: v = float32(c / (w[i] w[j])) added at [li, lj] and at [lj, li], pixel after pixel."""
    chrom = np.asarray(chrom)
    out = {int(chrom[b]): np.zeros((e - b, e - b), np.float32) for b, e in runs(chrom)}
    first = np.zeros(len(chrom), np.int64)
    for b, e in runs(chrom):
        first[b:e] = b
    with np.errstate(all="ignore"):
        for b1, b2, c in zip(np.asarray(bin1).tolist(), np.asarray(bin2).tolist(), np.asarray(count).tolist()):
            if not (0 <= b1 < len(chrom) and 0 <= b2 < len(chrom)):
                continue
            i, j = min(b1, b2), max(b1, b2)
            if chrom[i] != chrom[j] or first[i] != first[j]:
                continue
            v = np.float32(np.float64(c) / (np.float64(weights[i]) * np.float64(weights[j])) if weights is not None else np.float64(c))
            m = out[int(chrom[i])]
            m[i - first[i], j - first[i]] += v
            m[j - first[i], i - first[i]] += v
    return out


def dense_fast(bin1, bin2, count, chrom, weights=None):
    """dense() with np.add.at on float32 in the place of the loop: the same adds in the same order, so the same bytes (the host
    test holds the two together); for tables the loop would take seconds on."""
    chrom = np.asarray(chrom)
    b1, b2, c = np.asarray(bin1, np.int64), np.asarray(bin2, np.int64), np.asarray(count, np.float64)
    inside = (b1 >= 0) & (b1 < len(chrom)) & (b2 >= 0) & (b2 < len(chrom))
    i, j, c = np.minimum(b1, b2)[inside], np.maximum(b1, b2)[inside], c[inside]
    first = np.zeros(len(chrom), np.int64)
    for b, e in runs(chrom):
        first[b:e] = b
    cis = (chrom[i] == chrom[j]) & (first[i] == first[j])
    i, j, c = i[cis], j[cis], c[cis]
    with np.errstate(all="ignore"):
        v = (c if weights is None else c / (np.asarray(weights, np.float64)[i] * np.asarray(weights, np.float64)[j])).astype(np.float32)
        out = {}
        for b, e in runs(chrom):
            m = np.zeros((e - b, e - b), np.float32)
            mine = first[i] == b
            # one unbuffered pass over [li, lj], [lj, li], [li, lj], ...: the order of the loop
            rows = np.stack([i[mine] - b, j[mine] - b], axis=1).ravel()
            cols = np.stack([j[mine] - b, i[mine] - b], axis=1).ravel()
            np.add.at(m, (rows, cols), np.repeat(v[mine], 2))
            out[int(chrom[b])] = m
    return out


def profile(matrices, valid=None):
    """(contacts, counts, mean): fp64 sums of the float32 cells of the upper diagonals, zero and NaN cells skipped."""
    size = max(m.shape[0] for m in matrices.values())
    contacts, counts = np.zeros(size), np.zeros(size, np.int64)
    for key, m in matrices.items():
        if valid is not None and key not in valid:
            continue
        for d in range(m.shape[0]):
            diag = np.diag(m, k=d).astype(np.float64)
            keep = (diag != 0) & ~np.isnan(diag)
            contacts[d] += diag[keep].sum()
            counts[d] += keep.sum()
    with np.errstate(all="ignore"):
        return contacts, counts, contacts / counts


def enrichment(matrix, mean):
    n = matrix.shape[0]
    out = np.empty((n, n))
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(n):
                out[i, j] = np.float64(matrix[i, j]) / mean[abs(i - j)]
    return out


def valid(matrix):
    return np.array([bool((np.isfinite(r) & (r != 0)).any() and np.isfinite(r).all()) for r in matrix])


def pca(matrix, mask=None, k=3):
    """(pcs (n, k), variances (k), axes (k, n), every singular value) by np.linalg.svd and the sign rule."""
    matrix = np.asarray(matrix, np.float64)
    n = len(matrix)
    mask = np.any(matrix != 0, axis=1) if mask is None else np.asarray(mask, bool)
    x = matrix[mask, :][:, mask]
    m = len(x)
    xc = x - np.mean(x, axis=0)[None, :]
    u, s, vh = np.linalg.svd(xc)
    pcs, axes = np.full((n, k), np.nan), np.full((k, n), np.nan)
    for j in range(k):
        sign = -1.0 if vh[j][np.argmax(np.abs(vh[j]))] < 0 else 1.0
        axes[j, mask] = sign * vh[j]
        pcs[mask, j] = sign * u[:, j] * np.sqrt(m - 1)
    return pcs, s[:k] ** 2, axes, s


def split_rule(m):
    """The shape of the device solver at m valid bins (csrc/gdyn_hic.hip, pca_run), only to assert on the CPU which branch a size
    reaches: xblocks (stripes of 64 columns), splits = min(32, ceil(1024 / xblocks), ceil(m / 16)), rows_per_split, the rows
    (i0, i1) of every split (i0 > i1: the split starts past the last row and adds nothing), the trips of the wave loop (16 rows a
    trip) in the longest split, and the blocks of 128 and of 256 rows."""
    xblocks = -(-m // 64)
    splits = max(1, min(32, -(-1024 // xblocks), -(-m // 16)))
    rows_per_split = -(-m // splits)
    rows = [(s * rows_per_split, min((s + 1) * rows_per_split, m)) for s in range(splits)]
    return dict(xblocks=xblocks, splits=splits, rows_per_split=rows_per_split, rows=rows, trips=-(-rows_per_split // 16),
                rblocks=-(-m // 128), blocks256=-(-m // 256), ld=(m + 1) // 2 * 2)


def pca_bounds(singular, k):
    """Per component j < k: (relative bound of the variance, absolute bound of the axis and of pcs / sqrt(m - 1)).
    With lam = s^2 and a residual |A v - lam_j v| <= RHO lam_0: the eigenvalue moves by at most the residual (relative
    RHO lam_0 / lam_j, doubled for the rounding of the reference) and the vector by at most residual / gap (Davis-Kahan),
    gap = the distance of lam_j to its nearest other eigenvalue; LAPACK's own error enters with the same condition number."""
    lam = np.asarray(singular, np.float64) ** 2
    out = []
    for j in range(k):
        gap = np.abs(np.delete(lam, j) - lam[j]).min()
        out.append((2 * RHO * lam[0] / lam[j], (2 * RHO + LAPACK) * lam[0] / gap))
    return out


def check_pca(got, want_pcs, want_var, want_axes, singular, mask, what=""):
    """Asserts the rules of section 7f for one result of the device and prints the observed maxima."""
    pcs, var, axes = got[:3]
    k = len(want_var)
    m = int(np.asarray(mask).sum())
    assert pcs.shape == want_pcs.shape and axes.shape == want_axes.shape and var.shape == want_var.shape, what
    assert np.array_equal(np.isnan(pcs), np.repeat(~np.asarray(mask, bool)[:, None], k, axis=1)), what
    assert np.array_equal(np.isnan(axes), np.repeat(~np.asarray(mask, bool)[None, :], k, axis=0)), what
    for j, (rel, absolute) in enumerate(pca_bounds(singular, k)):
        dv = abs(var[j] - want_var[j]) / want_var[j]
        da = np.nanmax(np.abs(axes[j] - want_axes[j]))
        dp = np.nanmax(np.abs(pcs[:, j] - want_pcs[:, j])) / np.sqrt(m - 1)
        print(f"{what} component {j}: variance rel {dv:.3e} (allowed {rel:.3e}), axis abs {da:.3e}, pcs / sqrt(m - 1) abs {dp:.3e} (allowed {absolute:.3e})")
        assert dv <= rel and da <= absolute and dp <= absolute, (what, j, dv, rel, da, dp, absolute)
