"""The rules of DESIGN.md section 7e written out in fp64 numpy, one bin and one separation at a time where that is the clearest
form: what the device results and hic.py's vectorised functions are compared with where no recorded reference output exists
(chromosomes shorter than 2 (W - 1) bins, the scale case)."""
import numpy as np


def runs(chrom):
    out, start = [], 0
    for b in range(1, len(chrom) + 1):
        if b == len(chrom) or chrom[b] != chrom[start]:
            out.append((start, b))
            start = b
    return out


def band(bin1, bin2, count, chrom, W):
    """band[i, d] += c, pixel by pixel."""
    chrom = np.asarray(chrom)
    out = np.zeros((len(chrom), W), np.int64)
    for b1, b2, c in zip(np.asarray(bin1).tolist(), np.asarray(bin2).tolist(), np.asarray(count).tolist()):
        if not (0 <= b1 < len(chrom) and 0 <= b2 < len(chrom)):
            continue
        i, j = min(b1, b2), max(b1, b2)
        if chrom[i] == chrom[j] and j - i < W:
            out[i, j - i] += c
    return out


def band_fast(bin1, bin2, count, chrom, W):
    """The same sums with np.add.at, for the scale case."""
    chrom = np.asarray(chrom)
    b1, b2, c = np.asarray(bin1, np.int64), np.asarray(bin2, np.int64), np.asarray(count, np.int64)
    ok = (b1 >= 0) & (b1 < len(chrom)) & (b2 >= 0) & (b2 < len(chrom))
    i, j, c = np.minimum(b1, b2)[ok], np.maximum(b1, b2)[ok], c[ok]
    s = (chrom[i] == chrom[j]) & (j - i < W)
    out = np.zeros((len(chrom), W), np.int64)
    np.add.at(out, (i[s], (j - i)[s]), c[s])
    return out


def _mean_of_finite(values):
    kept = [v for v in values if not np.isnan(v)]
    if not kept:
        return np.nan
    return kept[0] if len(kept) == 1 else (kept[0] + kept[1]) / 2


def decay_full(band_, chrom):
    """D(i, k), k = 0 .. W-1, per run of equal codes."""
    band_ = np.asarray(band_)
    n_bins, W = band_.shape
    x = band_.astype(np.float64)
    x[band_ == 0] = np.nan
    D = np.full((n_bins, W), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for beg, end in runs(chrom):
            n = end - beg
            if n <= 1:
                continue
            r = x[beg:end]
            D[beg:end, 0] = 1.0
            for k in range(1, W):
                f = r[:max(n - k, 0), k] / np.sqrt(r[:max(n - k, 0), 0] * r[k:, 0])
                for i in range(n):
                    terms = []
                    if i < n - k:
                        terms.append(f[i])
                    if i >= k:
                        terms.append(f[i - k])
                    D[beg + i, k] = _mean_of_finite(terms)
    return D


def decay_insulation(band_, chrom):
    D = decay_full(band_, chrom)
    with np.errstate(invalid="ignore", divide="ignore"):
        return D[:, 1:].copy(), np.stack([D[:, k] / D[:, k + 1] for k in range(1, D.shape[1] - 1)], axis=1) if D.shape[1] > 2 else np.zeros((len(D), 0))


def local_alpha(band_, chrom):
    """estimate_slope's moments: mx and mxx over every s, my and mxy over the s with a finite log W.  Every moment is a running
    sum over s = 1, 2, ... in that order, one bin per lane of the arrays."""
    D = decay_full(band_, chrom)
    width = D.shape[1] - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        sx = sxx = 0.0
        sy, sxy, kept = np.zeros(len(D)), np.zeros(len(D)), np.zeros(len(D))
        for s in range(1, width + 1):
            x = np.log(float(s))
            sx, sxx = sx + x, sxx + x * x
            y = np.log(D[:, s])
            finite = ~np.isnan(y)
            sy = np.where(finite, sy + y, sy)
            sxy = np.where(finite, sxy + x * y, sxy)
            kept += finite
        mx, mxx = sx / width, sxx / width
        my, mxy = sy / kept, sxy / kept                      # 0 / 0: no finite W
        return -((mxy - mx * my) / (mxx - mx * mx))


def profile(bin1, bin2, count, chrom, excluded, weights, size):
    """(sum, n) per distance with np.bincount; int64 sums without weights."""
    chrom = np.asarray(chrom)
    b1, b2, c = np.asarray(bin1, np.int64), np.asarray(bin2, np.int64), np.asarray(count, np.int64)
    ok = (b1 >= 0) & (b1 < len(chrom)) & (b2 >= 0) & (b2 < len(chrom))
    i, j, c = np.minimum(b1, b2)[ok], np.maximum(b1, b2)[ok], c[ok]
    s = chrom[i] == chrom[j]
    if excluded is not None:
        ex = np.asarray(excluded).astype(bool)
        s &= ~ex[i] & ~ex[j]
    i, j, c = i[s], j[s], c[s]
    if weights is None:
        total = np.zeros(size, np.int64)
        np.add.at(total, j - i, c)
        return total, np.bincount(j - i, minlength=size).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = c / (np.asarray(weights)[i] * np.asarray(weights)[j])
    keep = ~np.isnan(v)
    return np.bincount((j - i)[keep], weights=v[keep], minlength=size), np.bincount((j - i)[keep], minlength=size).astype(np.int64)


def downsample(values, rate, window=None):
    v = np.asarray(values, np.float64)
    window = rate if window is None else window
    n = len(v)
    out = np.full(((n + rate - 1) // rate, v.shape[1]), np.nan)
    for m in range(len(out)):
        for col in range(v.shape[1]):
            kept = [v[r, col] for r in range(max(rate * (m + 1) - window + 1, 0), rate * (m + 1) + 1) if r < n and not np.isnan(v[r, col])]
            if kept:
                out[m, col] = sum(kept) / len(kept)
    return out


def ulp_distance(a, b):
    """The largest distance in units of the last place between two fp64 arrays with equal NaN masks (finite values of one sign)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    keep = ~np.isnan(a)
    if not keep.any():
        return 0
    ia, ib = a[keep].view(np.int64), b[keep].view(np.int64)
    return int(np.abs(ia - ib).max())


def put_cool(tool, directory, path, binsize, names, chrom, start, end, bin1, bin2, count, weights=None, weight_name="weight"):
    """Writes resolutions/<binsize> of a cooler file with gd_h5tool put-cool; returns the completed process."""
    import os
    import subprocess
    files = {}
    for key, data, dtype in [("chrom", chrom, "<i4"), ("start", start, "<i8"), ("end", end, "<i8"), ("bin1", bin1, "<i8"), ("bin2", bin2, "<i8"),
                             ("count", count, "<i4")] + ([("weights", weights, "<f8")] if weights is not None else []):
        files[key] = os.path.join(str(directory), f"cool_{key}.bin")
        np.asarray(data).astype(dtype).tofile(files[key])
    files["names"] = os.path.join(str(directory), "cool_names.txt")
    with open(files["names"], "w") as f:
        f.write("".join(n + "\n" for n in names))
    args = [tool, "put-cool", str(path), str(binsize), files["names"]] + [files[k] for k in ("chrom", "start", "end", "bin1", "bin2", "count")]
    if weights is not None:
        args += [weight_name, files["weights"]]
    return subprocess.run(args, capture_output=True, text=True)
