"""The inputs of test_msd_edges_gpu.py, each from a fixed seed, with the restatement's results (msd_restatement.time / chain /
per_bead) and the path of csrc/gdyn_msd.hip each shape is there for (a helper, not collected).  test_msd_host.py holds, on the
CPU, the restatement of the integer flavour to int64 sums of the same terms and the shape facts below to the kernel's constants.

    A  long along time       F = 8200 frames: three origin ranges (4096 + 4096 + 7), N = 20: two bead tiles, the second of 4
    B  long along the chain  chains of 1, 4097 (one full range) and 8200 beads (three), 19 frames: two frame tiles, the second of 3
    C  many lags             201 lags: four trips of the 64 lag slots; N = 300: 19 bead tiles (the last of 12), two chunks of 256
    D  many sequences        7 chains x 40 frames = 280 sequences: two chunks with 256 % 7 = 4; three frame tiles, the last of 8

Every case comes in two flavours: "integer", iid coordinates in [0, 32), so t2 <= 2883, t4 <= 8.4e6 and every sum is far below
2^53 and exact in any order; and "walk", an offset of +-1e3 plus a random walk along the sequence, whose sums round."""
import functools
from types import SimpleNamespace

import numpy as np

import msd_restatement as mr

# kRange, kSlots, kSeqs, kChunk of csrc/gdyn_msd.hip, and the items of a window that fit in its 160 KiB of LDS (49 elements a row)
K_RANGE, K_SLOTS, K_SEQS, K_CHUNK = 4096, 64, 16, 256
FIT = {"float32": 160 * 1024 // (49 * 4), "float64": 160 * 1024 // (49 * 8)}      # 835, 417

CASES = ("A", "B", "C", "D")
FLAVOURS = ("integer", "walk")
DTYPES = (np.float32, np.float64)

_SHAPES = {
    "A": dict(axis="time", F=8200, N=20, n_groups=3, group=np.arange(20) % 3 - 1,
              lags=[1, 2, 416, 417, 418, 834, 835, 4095, 4096, 4097, 8191, 8192, 8193, 8199, 8200, 9000],
              alone=[2, 4097, 8193], per_bead=[1, 4096, 4097, 8199]),
    "B": dict(axis="chain", F=21, N=12310, window=(1, 19), chains=[(0, 1), (1, 4098), (4100, 12300)],
              lags=[1, 2, 417, 4095, 4096, 4097, 8191, 8192, 8199, 8200], alone=[2, 4097, 8192], tile_window=(1, 16)),
    "C": dict(axis="time", F=200, N=300, n_groups=4, group=np.arange(300) % 4 - 1, lags=list(range(1, 201)) + [250],
              alone=[1, 64, 65, 128, 199]),
    "D": dict(axis="chain", F=45, N=180, window=(3, 40), chains=[(0, 5), (5, 6), (6, 40), (40, 42), (50, 90), (90, 130), (130, 171)],
              lags=[1, 2, 4, 33, 34, 40, 41], alone=[1, 34, 40], subset=3),
}


def ranges_of(items):
    """The origin ranges of a sequence of `items` items (origins 0 .. items - 2)."""
    return (items - 1 + K_RANGE - 1) // K_RANGE if items > 1 else 0


def tiles_of(n):
    """(tiles of K_SEQS sequences, sequences of the last tile)."""
    return (n + K_SEQS - 1) // K_SEQS, (n - 1) % K_SEQS + 1


def c_orders():
    """The lag list of C ascending, reversed and in a fixed random permutation."""
    lags = _SHAPES["C"]["lags"]
    return [list(lags), lags[::-1], [lags[i] for i in np.random.default_rng(201).permutation(len(lags))]]


@functools.lru_cache(maxsize=None)
def _history(name, flavour):
    """(F, N, 3) float64: values that float32 holds exactly in the integer flavour."""
    s = _SHAPES[name]
    F, N = s["F"], s["N"]
    rng = np.random.default_rng([ord(name), FLAVOURS.index(flavour)])
    if flavour == "integer":
        x = rng.integers(0, 32, size=(F, N, 3)).astype(np.float64)
    elif s["axis"] == "time":
        x = rng.uniform(-1e3, 1e3, size=(1, N, 3)) + np.cumsum(rng.normal(scale=0.3, size=(F, N, 3)), axis=0)
    else:
        x = rng.uniform(-1e3, 1e3, size=(F, 1, 3)) + np.cumsum(rng.normal(scale=0.5, size=(F, N, 3)), axis=1)
    x.setflags(write=False)
    return x


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def case(name, flavour, dtype):
    """One case in one flavour and precision: its history x, groups or chains, lags (or separations), the frame window, and
    want = (sum2, sum4, count) of the restatement.  Computed once and shared: every array is read-only."""
    s = _SHAPES[name]
    dtype = np.dtype(dtype)
    x = np.ascontiguousarray(_history(name, flavour).astype(dtype))
    x.setflags(write=False)
    c = SimpleNamespace(name=name, flavour=flavour, dtype=dtype, x=x, fit=FIT[dtype.name], **s)
    if c.axis == "time":
        c.want = _frozen(mr.time(x, c.lags, c.group, c.n_groups))
    else:
        c.want = _frozen(mr.chain(x, c.chains, c.lags, *c.window))
    return c


@functools.lru_cache(maxsize=None)
def per_bead(name, flavour, dtype, lag):
    """The restatement's (m2, m4) of one lag along time."""
    return _frozen(mr.per_bead(case(name, flavour, dtype).x, lag))


@functools.lru_cache(maxsize=None)
def chain_window(name, flavour, dtype, first_frame, n_frames):
    """The restatement along the chain over another frame window of the case's history."""
    c = case(name, flavour, dtype)
    return _frozen(mr.chain(c.x, c.chains, c.lags, first_frame, n_frames))


def int_sums(name):
    """(sum2, sum4, count) of the integer flavour in Python-sized integers (int64, exact): the same terms as the restatement's,
    summed without a floating-point number anywhere, and the counts from their closed forms."""
    s = _SHAPES[name]
    x = _history(name, "integer").astype(np.int64)
    assert np.array_equal(x, _history(name, "integer")) and x.min() >= 0 and x.max() < 32
    lags = s["lags"]

    def t2_sums(a, b, axis):
        t2 = ((b - a) ** 2).sum(axis=-1)
        assert t2.max(initial=0) <= 2883
        return t2.sum(axis=axis), (t2 * t2).sum(axis=axis)

    if s["axis"] == "time":
        F, N, G = s["F"], s["N"], s["n_groups"]
        sum2, sum4, count = (np.zeros((G, len(lags)), np.int64) for _ in range(3))
        for l, lag in enumerate(lags):
            if lag < F:
                m2, m4 = t2_sums(x[:F - lag], x[lag:], 0)
                for g in range(G):
                    sum2[g, l], sum4[g, l] = m2[s["group"] == g].sum(), m4[s["group"] == g].sum()
            for g in range(G):
                count[g, l] = int((s["group"] == g).sum()) * max(0, F - lag)
        return sum2, sum4, count
    f0, nf = s["window"]
    w = x[f0:f0 + nf]
    sum2, sum4, count = (np.zeros((len(s["chains"]), len(lags)), np.int64) for _ in range(3))
    for c, (start, end) in enumerate(s["chains"]):
        for l, sep in enumerate(lags):
            if sep < end - start:
                sum2[c, l], sum4[c, l] = t2_sums(w[:, start:end - sep], w[:, start + sep:end], None)
            count[c, l] = nf * max(0, end - start - sep)
    return sum2, sum4, count


def assert_shape_facts():
    """Every case reaches the path of csrc/gdyn_msd.hip it is named after: arithmetic on the shapes and the kernel's constants."""
    a, b, c, d = (_SHAPES[k] for k in CASES)
    # A: three origin ranges (4096 + 4096 + 7 origins), two bead tiles with 4 beads in the second, one chunk; lags at, around and
    # beyond the window of either precision, one range, two ranges and the last origin; a walk through two windows (want > fit)
    assert ranges_of(a["F"]) == 3 and a["F"] - 1 - 2 * K_RANGE == 7 and tiles_of(a["N"]) == (2, 4) and a["N"] <= K_CHUNK
    for edge in (FIT["float64"], FIT["float32"], K_RANGE, 2 * K_RANGE):
        assert {edge - 1, edge, edge + 1} & set(a["lags"]) >= {edge - 1, edge}, edge
    assert {a["F"] - 1, a["F"]} <= set(a["lags"]) and max(a["lags"]) > a["F"] > FIT["float32"]
    assert set(a["alone"] + a["per_bead"]) <= set(a["lags"]) and max(a["per_bead"]) == a["F"] - 1
    # B: chains of one bead (no origin), exactly one full range, and three ranges; two frame tiles, 3 frames in the second
    lens = [end - start for start, end in b["chains"]]
    assert [ranges_of(n) for n in lens] == [0, 1, 3] and lens[1] - 1 == K_RANGE and lens[2] > FIT["float32"]
    assert tiles_of(b["window"][1]) == (2, 3) and tiles_of(b["tile_window"][1]) == (1, K_SEQS) and b["window"][0] + b["window"][1] < b["F"]
    assert b["chains"][1][1] < b["chains"][2][0] and b["chains"][2][1] < b["N"]      # uncovered beads between and after
    assert [b["window"][1] * max(0, lens[2] - s) for s in b["lags"][-4:]] == [171, 152, 19, 0]
    # C: 201 lags are four trips of the 64 slots, the whole sequence in one window; 19 bead tiles, 12 beads in the last; two chunks
    assert len(c["lags"]) == 201 and -(-len(c["lags"]) // K_SLOTS) == 4 and c["F"] <= FIT["float64"]
    assert tiles_of(c["N"]) == (19, 12) and -(-c["N"] // K_CHUNK) == 2
    assert sorted(c["lags"]) == c["lags"] and sum(lag >= c["F"] for lag in c["lags"]) == 2
    assert {K_SLOTS, K_SLOTS + 1, 2 * K_SLOTS} <= set(c["alone"])
    orders = c_orders()
    assert orders[1] == orders[0][::-1] and sorted(orders[2]) == orders[0] and orders[2] not in orders[:2]
    # D: 280 sequences in two chunks whose boundary no multiple of the 7 chains meets; three frame tiles, 8 frames in the last
    n_seqs = len(d["chains"]) * d["window"][1]
    assert n_seqs == 280 and -(-n_seqs // K_CHUNK) == 2 and K_CHUNK % len(d["chains"]) == 4 and tiles_of(d["window"][1]) == (3, 8)
    assert d["subset"] * d["window"][1] == 120 <= K_CHUNK
    assert [d["window"][1] * max(0, end - start - 1) for start, end in d["chains"]] == [160, 0, 1320, 40, 1560, 1560, 1600]
