"""Yardstick of the nearest-neighbour tests: chunked numpy brute force in the arithmetic order the kernel promises --
d2 = (dx*dx + dy*dy) + dz*dz, every operation a separate fp64 rounding (numpy never contracts), dist = sqrt(min d2), index =
numpy.argmin (the first, i.e. lowest, index of the minimum) -- and the three data families the tests run on.  Plain numpy only."""
import numpy as np


def nn_ref(q, s, rows=256, return_counts=False):
    """q [nq, 3], s [ns, 3] float64 -> (dist [nq] float64, idx [nq] int64[, number of support points AT the minimum])."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)
    nq = len(q)
    dist, idx, cnt = np.empty(nq), np.empty(nq, dtype=np.int64), np.empty(nq, dtype=np.int64)
    sx, sy, sz = (np.ascontiguousarray(s[:, c])[None, :] for c in range(3))
    for a in range(0, nq, rows):
        b = min(nq, a + rows)
        dx, dy, dz = q[a:b, 0:1] - sx, q[a:b, 1:2] - sy, q[a:b, 2:3] - sz
        d2 = (dx * dx + dy * dy) + dz * dz
        i = np.argmin(d2, axis=1)
        m = d2[np.arange(b - a), i]
        dist[a:b], idx[a:b], cnt[a:b] = np.sqrt(m), i, (d2 == m[:, None]).sum(1)
    return (dist, idx, cnt) if return_counts else (dist, idx)


FAMILIES = ('gaussian', 'scan', 'lattice')


def make_cloud(family, n, rng):
    """gaussian: fp64 normal.  scan: anisotropic room-sized cloud with float32 VALUES (as the .npy vertices), cast to fp64.
    lattice: points on a quarter-unit grid of 12^3 cells -- exact ties and bitwise duplicates everywhere."""
    if family == 'gaussian':
        return rng.standard_normal((n, 3))
    if family == 'scan':
        return (rng.standard_normal((n, 3)) * np.array([4.0, 3.0, 0.8]) + np.array([1.0, -2.0, 0.5])).astype(np.float32).astype(np.float64)
    if family == 'lattice':
        return rng.integers(0, 12, size=(n, 3)).astype(np.float64) * 0.25
    raise ValueError(family)


def make_pair(family, nq, ns, seed, copied=500):
    """(queries, support); in the scan family `copied` of the queries are bitwise copies of support points (distance exactly 0)."""
    rng = np.random.default_rng(seed)
    s, q = make_cloud(family, ns, rng), make_cloud(family, nq, rng)
    if family == 'scan':
        k = min(copied, nq, ns)
        q[rng.choice(nq, k, replace=False)] = s[rng.choice(ns, k, replace=False)]
    return q, s
