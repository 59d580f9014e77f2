"""The lamina analysis restated operation by operation (the rules of include/gdyn_lamina.h), for
the tests: the wall distance of 5-sim-genome/src/analyze_lamina/geometry.py:13-28 in scalar float64 and in column-wise
numpy with the same operation order, and the contact / average lines of command.py:99-133."""
import math

import numpy as np

EPSILON = 1e-6


def distance_scalar(point, semiaxes):
    """One point, Python floats (IEEE double, one rounding per operation)."""
    x = [float(np.float64(t)) for t in point]
    inv = [math.pow(float(s), -2.0) for s in semiaxes]
    s1 = [inv[k] * x[k] for k in range(3)]
    s2 = [inv[k] * s1[k] for k in range(3)]
    s3 = [inv[k] * s2[k] for k in range(3)]
    a = (s3[0] * x[0] + s3[1] * x[1]) + s3[2] * x[2]
    b = (s2[0] * x[0] + s2[1] * x[1]) + s2[2] * x[2]
    c = ((s1[0] * x[0] + s1[1] * x[1]) + s1[2] * x[2]) - 1
    disc = b * b - a * c
    root = math.sqrt(disc) if disc >= 0 else math.nan
    den = a + EPSILON
    num = b - root
    u = num / den if den != 0 else (math.nan if num == 0 or num != num else math.copysign(math.inf, num))
    v = math.sqrt((s1[0] * s1[0] + s1[1] * s1[1]) + s1[2] * s1[2])
    return abs(u * v)


def distances(points, semiaxes):
    """(N, 3) float32 or float64 points of one frame -> (N,) float64, the scalar order evaluated column by column."""
    p = np.asarray(points)
    x = [p[:, k].astype(np.float64) for k in range(3)]
    inv = [np.float64(math.pow(float(s), -2.0)) for s in semiaxes]
    s1 = [inv[k] * x[k] for k in range(3)]
    s2 = [inv[k] * s1[k] for k in range(3)]
    s3 = [inv[k] * s2[k] for k in range(3)]
    a = (s3[0] * x[0] + s3[1] * x[1]) + s3[2] * x[2]
    b = (s2[0] * x[0] + s2[1] * x[1]) + s2[2] * x[2]
    c = ((s1[0] * x[0] + s1[1] * x[1]) + s1[2] * x[2]) - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (b - np.sqrt(b * b - a * c)) / (a + EPSILON)
        v = np.sqrt((s1[0] * s1[0] + s1[1] * s1[1]) + s1[2] * s1[2])
        return np.abs(u * v)


def history(frames, semiaxes):
    """(F, N, 3) frames, (F, 3) semiaxes -> (F, N) float64."""
    return np.stack([distances(x, s) for x, s in zip(frames, semiaxes)])


def contacts(distances_f32, contact_distance):
    """command.py:106: float32 distances against a Python float."""
    return np.asarray(distances_f32, dtype=np.float32).astype(np.float64) < float(contact_distance)


def average(contact_histories):
    """command.py:117-124: a float32 sum of the boolean histories, divided by their number."""
    total = np.zeros(contact_histories[0].shape, np.float32)
    for c in contact_histories:
        total += c
    total /= len(contact_histories)
    return total


def same(a, b):
    """Equal bit patterns, except that any NaN equals any NaN (the sign and payload of an invalid operation's NaN are the
    platform's)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)))) and \
        bool(np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])))
