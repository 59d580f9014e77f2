"""numpy fp64 restatement of include/gdyn_dmap.h (a helper of test_dmap_host.py, test_dmap_gpu.py and tools/bench_dmap.py; not
collected).  The term of two beads i != j of a frame, every operation rounded on its own:

    d = double(X[f,i]) - double(X[f,j]) per axis;   with a box: d -= box * rint(d / box)   (np.rint rounds half to even)
    r2 = (dx*dx + dy*dy) + dz*dz;   r = sqrt(r2)   (np.sqrt is correctly rounded)

numpy neither contracts nor reassociates these, so r2, and with it every hit, is the device's bit for bit; the sums over frames
and beads are numpy's (pairwise), which the parity bound (2 count + 8) 2^-53 covers as it covers any order of non-negative terms."""
import numpy as np

EPS = 2.0 ** -53


def terms(xi, xj, box=None):
    """r2 of the beads xi (..., n, 1, 3) against xj (..., 1, m, 3), or any shapes that broadcast."""
    d = xi.astype(np.float64) - xj.astype(np.float64)
    if box is not None:
        b = np.asarray(box, dtype=np.float64)
        d = d - b * np.rint(d / b)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dmap(x, bins=None, first_frame=0, n_frames=None, box=None, thresholds=()):
    """sum1, sum2 (B, B) float64, hits (T, B, B) uint64 and count (B, B) uint64 of gd_dmap_map over all bins."""
    F, N, _ = x.shape
    bins = [(i, i + 1) for i in range(N)] if bins is None else [(int(a), int(b)) for a, b in bins]
    n_frames = F - first_frame if n_frames is None else n_frames
    w = x[first_frame:first_frame + n_frames]
    B, T = len(bins), len(thresholds)
    sum1, sum2 = np.zeros((B, B)), np.zeros((B, B))
    hits, count = np.zeros((T, B, B), np.uint64), np.zeros((B, B), np.uint64)
    thr2 = [np.float64(t) * np.float64(t) for t in thresholds]
    for I, (a0, a1) in enumerate(bins):
        for J, (b0, b1) in enumerate(bins):
            r2 = terms(w[:, a0:a1, None, :], w[:, None, b0:b1, :], box)      # (frames, |I|, |J|)
            if I == J:
                r2 = r2[:, ~np.eye(a1 - a0, dtype=bool)]      # j != i
            sum2[I, J] = r2.sum()
            sum1[I, J] = np.sqrt(r2).sum()
            for t in range(T):
                hits[t, I, J] = np.count_nonzero(r2 < thr2[t])
            count[I, J] = n_frames * ((a1 - a0) * (b1 - b0) - (a1 - a0 if I == J else 0))
    return sum1, sum2, hits, count


def bound(count, value):
    """The parity bound of the header: |device - restatement| <= (2 count + 8) 2^-53 restatement."""
    return (2.0 * count.astype(np.float64) + 8.0) * EPS * np.abs(value)


def bins_from_chains(chain_ranges, rate):
    """The rule of Dmap.bins_from_chains and gd_distance_map --rebin-rate: `rate` consecutive beads per bin within each chain, the last
    bin of a chain shorter, no bin across two chains."""
    out = []
    for start, end in chain_ranges:
        a = int(start)
        while a < int(end):
            out.append((a, min(a + int(rate), int(end))))
            a += int(rate)
    return out


def line_closed_form(n_beads, bins, n_frames, step2):
    """Beads at i * e with |e|^2 = step2 a perfect square, the same in every frame: r = sqrt(step2) |i - j|, so
    sum1[I, J] = n_frames sqrt(step2) sum |i - j| and sum2[I, J] = n_frames step2 sum (i - j)^2, in integers."""
    s = int(round(np.sqrt(step2)))
    assert s * s == step2
    B = len(bins)
    sum1, sum2 = np.zeros((B, B)), np.zeros((B, B))
    for I, (a0, a1) in enumerate(bins):
        for J, (b0, b1) in enumerate(bins):
            d = [abs(i - j) for i in range(a0, a1) for j in range(b0, b1)]
            sum1[I, J] = n_frames * s * sum(d)
            sum2[I, J] = n_frames * step2 * sum(v * v for v in d)
    return sum1, sum2
