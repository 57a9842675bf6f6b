"""NumPy yardstick and cases for the feature-space nearest-neighbour search (csrc/featnn.hip) and the registration from features
built on it (utils/registration.py).  Everything here is fp64 brute force on the host.

The error bound.  The kernel ranks the support rows of a query a by the fp32 score  s_j = n_j - 2 dot_j,  n_j = |b_j|^2 and dot_j = a . b_j
each an fp32 sum of C products.  With u = 2^-24 (round to nearest) and gamma_n = n u / (1 - n u), the standard result for a sum of n
products accumulated in ANY order, fused or not (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1), is
    |fl(dot_j) - dot_j| <= gamma_C sum_k |a_k b_jk|,        |fl(n_j) - n_j| <= gamma_C |b_j|^2.
Doubling fl(dot) is exact; the final subtraction multiplies the result by one more (1 + delta), |delta| <= u, which raises each factor to
at most gamma_(C+1).  gamma_(C+2) leaves one rounding to spare, so
    |fl(s_j) - s_j| <= E(i, j) = 2 gamma sum_k |a_ik b_jk| + gamma |b_j|^2,        gamma = (C + 2) u / (1 - (C + 2) u).
The true score is s_j = d2(i, j) - |a_i|^2.  If the kernel returns j' for query i while j* is the true nearest row, fl(s_j') <= fl(s_j*),
hence  d2(i, j') - d2(i, j*) = s_j' - s_j* <= E(i, j') + E(i, j*) <= 2 max_j E(i, j).  Zero columns appended to both rows add exact zeros and
leave the bound where it is."""
import numpy as np

U = 2.0 ** -24


def d2_matrix(q, s, block_bytes=32 << 20):
    """[nq, ns] fp64 squared distances, as sum_k (a_k - b_k)^2 of the rows widened to fp64 (exact for the integer lattice)."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)
    out = np.empty((len(q), len(s)))
    step = max(1, block_bytes // max(8 * len(s) * max(q.shape[1], 1), 1))
    for i in range(0, len(q), step):
        d = q[i:i + step, None, :] - s[None, :, :]
        out[i:i + step] = (d * d).sum(-1)
    return out


def seq_d2(a, b):
    """sum_k (double(a_k) - double(b_k))^2 in ascending k, every operation rounded on its own: cumsum is sequential, np.sum is pairwise."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.cumsum(d * d, axis=-1)[..., -1]


def nn_ref(q, s):
    """(idx int64, d2 float64): the fp64 arg-min, the lowest index among equal minima (numpy.argmin's rule); (-1, +inf) for an empty support.
    d2 is the sequential sum for the chosen row."""
    q, s = np.asarray(q), np.asarray(s)
    if len(s) == 0:
        return np.full(len(q), -1, dtype=np.int64), np.full(len(q), np.inf)
    if len(q) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0)
    idx = d2_matrix(q, s).argmin(axis=1)
    return idx, seq_d2(q, s[idx])


def error_bound(q, s):
    """E [nq, ns] of the module docstring, in fp64."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)
    c = q.shape[1]
    gamma = (c + 2) * U / (1.0 - (c + 2) * U)
    return 2.0 * gamma * (np.abs(q) @ np.abs(s).T) + gamma * (s * s).sum(1)[None, :]


def lattice_sets(sizes, c, seed, n_codes=None):
    """Integer feature rows in [-8, 8] as float32: every product and partial sum is exact in fp32 (c * 16^2 < 2^24).  All sets draw their
    rows from one small pool of codes, so duplicates -- exact ties -- are dense inside a support and queries hit support rows exactly."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(-8, 9, size=(n_codes or max(4, max(sizes) // 3), c)).astype(np.float32)
    return [pool[rng.integers(0, len(pool), size=n)] for n in sizes]


def gaussian_pair(nq, ns, c, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, c)).astype(np.float32), rng.standard_normal((ns, c)).astype(np.float32)


def pack(sets):
    """-> (packed [sum n, C], offsets [n_sets + 1] int64)."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return np.concatenate(sets), off


def mutual_filter(nn_fwd, nn_back):
    """The mutual rule: keep (i, j) iff nn_fwd[i] = j and nn_back[j] = i.  -> [m, 2] int64 sorted by i."""
    nn_fwd, nn_back = np.asarray(nn_fwd, dtype=np.int64), np.asarray(nn_back, dtype=np.int64)
    keep = [(i, j) for i, j in enumerate(nn_fwd) if j >= 0 and nn_back[j] == i]
    return np.asarray(keep, dtype=np.int64).reshape(-1, 2)


def match_ref(src_feats, ref_feats, mutual):
    fwd, _ = nn_ref(src_feats, ref_feats)
    if mutual:
        return mutual_filter(fwd, nn_ref(ref_feats, src_feats)[0])
    return np.stack([np.arange(len(fwd)), fwd], axis=1)[fwd >= 0]


def edge_length_ok(corr, samples, similarity=0.9):
    """Open3D's CorrespondenceCheckerBasedOnEdgeLength for triples of rows of corr [n, 6] (source xyz | reference xyz): a triple passes iff
    for each of its three point pairs d_src >= similarity * d_ref and d_ref >= similarity * d_src.  -> bool [H]."""
    corr, samples = np.asarray(corr, dtype=np.float64), np.asarray(samples)
    ok = np.ones(len(samples), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        d = corr[samples[:, a]] - corr[samples[:, b]]
        sq = d * d
        d_src, d_ref = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]), np.sqrt((sq[:, 3] + sq[:, 4]) + sq[:, 5])
        ok &= (d_src >= similarity * d_ref) & (d_ref >= similarity * d_src)
    return ok


def rigid(seed):
    """A proper rigid 4x4: a rotation by about one radian about a random axis, a translation of order one."""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    ang = 0.7 + 0.6 * rng.random()
    t = np.eye(4)
    t[:3, :3] = np.eye(3) + np.sin(ang) * k + (1.0 - np.cos(ang)) * (k @ k)
    t[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    return t


def planted_registration(seed, n_src=300, n_out=100, c=6):
    """A source cloud, the reference = the moved source, shuffled, plus outliers; descriptors = distinct integer codes (the base-7 digits of a
    code number, c columns) that true partners share and nobody else has.  -> dict(src, ref, src_feats, ref_feats, transform, perm) with
    ref[perm[i]] the partner of src[i]."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-2.0, 2.0, (n_src, 3))
    t = rigid(seed + 1)
    codes = rng.permutation(7 ** min(c, 5))[:n_src + n_out]
    digits = np.stack([(codes // 7 ** k) % 7 for k in range(c)], axis=1).astype(np.float32)
    order = rng.permutation(n_src + n_out)                      # reference row r holds candidate order[r]; candidates < n_src are partners
    cand = np.concatenate([src @ t[:3, :3].T + t[:3, 3], rng.uniform(-4.0, 4.0, (n_out, 3))])
    perm = np.empty(n_src + n_out, dtype=np.int64)
    perm[order] = np.arange(n_src + n_out)
    return {'src': src, 'ref': cand[order], 'src_feats': digits[:n_src], 'ref_feats': digits[order], 'transform': t, 'perm': perm[:n_src]}
