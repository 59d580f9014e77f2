"""An independent brute-force restatement of the reference's radial distribution analyses, 4-sim-ab/box/src/rdf_analysis and
rdf_analysis_hetero, for the tests of include/gdyn_rdf.h and gd_rdf_analysis[_hetero].  numpy, O(N^2) in chunks; it shares no
code with the package.  The rules the reference leaves to micromd (minimum image, strict cutoff, one count per unordered pair)
are the project's.

Line citations: rdf_analysis/{analysis.cc, distance_histogram.cc} and rdf_analysis_hetero/{analysis.cc, distance_histogram.cc}."""
import math

import numpy as np

PI = 3.1416                 # distance_histogram.cc:12 (both programs)


def n_bins(bin_width, max_distance):
    return int(math.ceil(max_distance / bin_width))          # distance_histogram.cc:25


def bin_volumes(bin_width, max_distance):
    vols = []
    for i in range(n_bins(bin_width, max_distance)):         # distance_histogram.cc:27-36
        r_min = bin_width * float(i)
        r_max = bin_width * float(i + 1)
        if r_max > max_distance:
            r_max = max_distance
        dr3 = r_max * r_max * r_max - r_min * r_min * r_min
        vols.append(4 * PI / 3 * dr3)
    return np.array(vols)


def select(ab, type_=None):
    """rdf_analysis/analysis.cc:31-52: A -> |a - 1| < 0.1, B -> |a - 0| < 0.1, anything else -> every bead."""
    a = np.asarray(ab, np.float64)[:, 0]
    if type_ == "A":
        return np.flatnonzero(np.abs(a - 1.0) < 0.1)
    if type_ == "B":
        return np.flatnonzero(np.abs(a - 0.0) < 0.1)
    return np.arange(len(a))


def select_hetero(ab, type_="A"):
    """rdf_analysis_hetero/analysis.cc:32-54: centres |a - c| < 1e-6, every other bead a target."""
    c = {"A": 1.0, "B": 0.0}.get(type_)
    if c is None:
        raise ValueError(f"invalid center type: '{type_}'")
    a = np.asarray(ab, np.float64)[:, 0]
    m = np.abs(a - c) < 1e-6
    return np.flatnonzero(m), np.flatnonzero(~m)


def _bins_of(d, box, bin_width, max_distance):
    """d (..., 3) raw displacements -> (bin, kept mask): minimum image per axis, strict cutoff on (dx^2 + dy^2) + dz^2,
    bin size_t(norm * (1 / bin_width)) below n_bins (distance_histogram.cc:50-55)."""
    box = np.asarray(box, np.float64)
    d = d - box * np.rint(d / box)
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore"):
        keep = r2 < max_distance * max_distance
        b = np.zeros(r2.shape, np.uint64)
        b[keep] = (np.sqrt(r2[keep]) * (1 / bin_width)).astype(np.uint64)
    keep &= b < n_bins(bin_width, max_distance)
    return b, keep


def pair_counts(a, b, pairs, box, bin_width, max_distance):
    """Counts of given candidate pairs (i into a, j into b), each taken once."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    bins, keep = _bins_of(np.asarray(a, np.float64)[pairs[:, 0]] - np.asarray(b, np.float64)[pairs[:, 1]], box, bin_width, max_distance)
    return np.bincount(bins[keep].astype(np.int64), minlength=n_bins(bin_width, max_distance)).astype(np.uint64)


def counts_self(points, box, bin_width, max_distance, chunk=256):
    """Unordered pairs i < j of one frame (distance_histogram.cc:46-57 of rdf_analysis)."""
    p = np.asarray(points, np.float64)
    out = np.zeros(n_bins(bin_width, max_distance), np.uint64)
    for i0 in range(0, len(p), chunk):
        i1 = min(len(p), i0 + chunk)
        bins, keep = _bins_of(p[i0:i1, None, :] - p[None, :, :], box, bin_width, max_distance)
        keep &= np.arange(i0, i1)[:, None] < np.arange(len(p))[None, :]
        out += np.bincount(bins[keep].astype(np.int64), minlength=len(out)).astype(np.uint64)
    return out


def counts_cross(centers, targets, box, bin_width, max_distance, chunk=256):
    """(centre, target) pairs of one frame (rdf_analysis_hetero/distance_histogram.cc:49-64)."""
    c, t = np.asarray(centers, np.float64), np.asarray(targets, np.float64)
    out = np.zeros(n_bins(bin_width, max_distance), np.uint64)
    for i0 in range(0, len(c), chunk):
        bins, keep = _bins_of(c[i0:i0 + chunk, None, :] - t[None, :, :], box, bin_width, max_distance)
        out += np.bincount(bins[keep].astype(np.int64), minlength=len(out)).astype(np.uint64)
    return out


def values(counts, bin_width, max_distance, box_size, n_center, n_target=None):
    """analysis.cc:106-114: frequency count * unit_weight (2/n or 1/n_center), density frequency / bin volume, over the
    expected density (n_selected or n_target) / box_size^3.  Empty selections give what 0/0 gives."""
    volume = box_size * box_size * box_size
    with np.errstate(divide="ignore", invalid="ignore"):
        if n_target is None:
            w, rho = np.float64(2) / np.float64(n_center), np.float64(n_center) / np.float64(volume)
        else:
            w, rho = np.float64(1) / np.float64(n_center), np.float64(n_target) / np.float64(volume)
        return np.asarray(counts, np.uint64).astype(np.float64) * w / bin_volumes(bin_width, max_distance) / rho


def fmt(v):
    """std::ostream << double at the default precision: printf's %g (glibc spells a NaN with its sign bit set "-nan")."""
    if math.isnan(v):
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return "%g" % v


def line(vals):
    return "\t".join(fmt(float(v)) for v in vals)


def analysis_lines(ab, box_size, frames, bin_width=0.1, max_distance=1.0, type_=None, hetero=False):
    """stdout of either program for the given frames (a list of (N, 3) arrays in .steps order)."""
    box = (box_size,) * 3
    out = []
    if hetero:
        ci, ti = select_hetero(ab, "A" if type_ is None else type_)
        for x in frames:
            x = np.asarray(x, np.float64)
            cnt = counts_cross(x[ci], x[ti], box, bin_width, max_distance)
            out.append(line(values(cnt, bin_width, max_distance, box_size, len(ci), len(ti))))
    else:
        si = select(ab, type_)
        for x in frames:
            x = np.asarray(x, np.float64)
            cnt = counts_self(x[si], box, bin_width, max_distance)
            out.append(line(values(cnt, bin_width, max_distance, box_size, len(si))))
    return out
