"""The ellipsoid wall's axial reaction, restated in plain fp64 numpy (a helper module of the suite).

include/gdyn.h: the wall's semiaxes move by dt * mobility * (axial_reaction - semiaxes_spring (.) semiaxes), and

    axial_reaction_k = - sum_i F_wall,ik q_ik / a_k

with q_i the point of the surface the second-order nearest-surface construction assigns to bead i (the line through x_i along the
gradient of f(x) = sum_k (x_k / a_k)^2 - 1, intersected with f = 0) and a the semiaxes.  Here it is computed from the oracle's wall
FORCES and the positions alone -- none of the oracle's own reaction code -- together with

    S_k = sum_i |F_wall,ik q_ik| / a_k

the scale an fp32 evaluation of the sum is held to.  For equal semiaxes q_i = a x_i / |x_i|, and the reaction has the closed form
- sum_i F_ik x_ik / |x_i|.
"""
import numpy as np

from util import g


def contact_points(x, semi):
    """q (N, 3) and C = f(x) (N,) of positions x (N, 3) on the ellipsoid with semiaxes semi (3,)."""
    x, semi = np.asarray(x, dtype=np.float64), np.asarray(semi, dtype=np.float64)
    i2 = 1.0 / (semi * semi)
    s1 = x * i2
    C = np.sum(x * s1, axis=-1) - 1.0
    B = np.sum(s1 * s1, axis=-1)
    A = np.sum(s1 * s1 * i2, axis=-1)
    u = (B - np.sqrt(np.maximum(B * B - A * C, 0.0))) / np.where(A > 0, A, 1.0)
    return x - u[:, None] * s1, C


def reaction(x, F_wall, semi):
    """(react (3,), S (3,)) of one replica: positions (N, 3), the wall's forces on them (N, 3), semiaxes (3,)."""
    q, _ = contact_points(x, semi)
    w = F_wall * q / np.asarray(semi, dtype=np.float64)
    return -w.sum(axis=0), np.abs(w).sum(axis=0)


def reaction_on_a_sphere(x, F_wall):
    """The closed form for equal semiaxes."""
    return -(F_wall * x / np.linalg.norm(x, axis=-1, keepdims=True)).sum(axis=0)


def on_the_wall(s):
    """Per replica of an oracle handle: (acted (N,) bool, C (N,)) -- the beads the wall acts on and their side of the surface."""
    x, F = s.positions(), s.forces(g.TERM_WALL)
    out = []
    for r in range(s.R):
        _, C = contact_points(x[r], s.context(r).semiaxes)
        out.append((np.abs(F[r]).max(axis=-1) > 0, C))
    return out


def oracle_reaction(s):
    """(react, S, reported), each (R, 3): the restatement at the state of oracle handle s, and what the oracle itself reports after the
    same wall-force evaluation."""
    x, F = s.positions(), s.forces(g.TERM_WALL)
    rs = [reaction(x[r], F[r], s.context(r).semiaxes) for r in range(s.R)]
    return (np.array([a for a, _ in rs]), np.array([b for _, b in rs]),
            np.array([tuple(s.context(r).axial_reaction) for r in range(s.R)]))
