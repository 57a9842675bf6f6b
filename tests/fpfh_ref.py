"""NumPy fp64 yardstick and cases for the FPFH chain (csrc/fpfh.hip through utils/features.py): neighbour lists, normals, the SPFH
census, the FPFH weighting.  It restates the contract of include/sgaligner_hip.h; Open3D is not available to compare against, so that
contract -- not Open3D's output -- is what the kernels are held to.

Neighbour lists and the FPFH weighting are bit-equal yardsticks (pinned arithmetic: the d2 expression, explicit ascending loops).  The
normals (numpy.linalg.eigh) and the census (libm's atan2) are not, so this module also reports where a comparison is not meaningful:
  * an SPFH point is UNDECIDED when for one of its pairs ||a1| - |a2||, a non-zero |v|, or the distance of one of the three scaled features
    to an integer is below EPS: a rounding difference may then pick the other branch or the neighbouring bin;
  * a normal is ILL when (lambda1 - lambda0) < ILL_REL * lambda2: the smallest eigenvalue's eigenvector is then poorly determined;
  * a normal is SIGN-NEAR when |n . (v - p)| < SIGN_REL |v - p|: the orientation test is then a coin toss."""
import numpy as np

EPS = 1e-9
ILL_REL = 1e-3
SIGN_REL = 1e-6
BINS = 33


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def d2_matrix(p):
    """[n, n] squared distances, (dx*dx + dy*dy) + dz*dz with every operation rounded on its own."""
    p = np.asarray(p, dtype=np.float64)
    dx, dy, dz = (p[:, None, a] - p[None, :, a] for a in range(3))
    with np.errstate(invalid='ignore', over='ignore'):
        return (dx * dx + dy * dy) + dz * dz


def lists_ref(p, radius=None, max_nn=30):
    """One cloud -> (count [n] int32, idx [n, max_nn] int32 with -1 past count, d2 [n, max_nn] float64 with +inf past count): the first
    max_nn of { j : d2(i, j) <= r2 } by np.lexsort((j, d2)); r2 = float(radius) * float(radius), +inf for None.  NaN fails d2 <= r2."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    r2 = np.inf if radius is None else float(radius) * float(radius)
    count = np.zeros(n, dtype=np.int32)
    idx = np.full((n, max_nn), -1, dtype=np.int32)
    d2 = np.full((n, max_nn), np.inf)
    D = d2_matrix(p)
    for i in range(n):
        with np.errstate(invalid='ignore'):
            cand = np.flatnonzero(D[i] <= r2)
        cand = cand[np.lexsort((cand, D[i, cand]))][:max_nn]
        count[i] = len(cand)
        idx[i, :len(cand)] = cand
        d2[i, :len(cand)] = D[i, cand]
    return count, idx, d2


def lists_ref_packed(clouds, radius=None, max_nn=30):
    """Clouds packed back to back, indices cloud-local."""
    parts = [lists_ref(c, radius, max_nn) for c in clouds]
    return tuple(np.concatenate([q[a] for q in parts]) if parts else None for a in range(3))


def straddlers(lists_more, max_nn):
    """Points whose list is cut inside a run of equal d2: entry max_nn - 1 and entry max_nn of a list one entry longer are equal."""
    count, _, d2 = lists_more
    return (count > max_nn) & (d2[:, max_nn - 1] == d2[:, max_nn])


def normals_ref(p, lists, viewpoint=None):
    """-> dict(normals [n, 3], status [n], ill [n] bool, sign_near [n] bool).  numpy.linalg.eigh of the neighbours' covariance (divided
    by m); m < 3 or a non-finite coordinate: (0, 0, 1), status 1, not oriented."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    count, idx, _ = lists
    n, K = idx.shape
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    status = np.ones(n, dtype=np.int32)
    ill, sign_near = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    if n == 0:
        return dict(normals=normals, status=status, ill=ill, sign_near=sign_near)
    valid = np.arange(K)[None, :] < count[:, None]
    q = p[np.clip(idx, 0, n - 1)]                                           # [n, K, 3]
    fin = np.isfinite(p).all(1) & np.where(valid[..., None], np.isfinite(q), True).all((1, 2))
    good = (count >= 3) & fin
    w = valid[..., None].astype(np.float64)
    m = np.maximum(count, 1).astype(np.float64)[:, None]
    qz = np.where(valid[..., None], np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), 0.0)
    mu = qz.sum(1) / m
    c = (qz - mu[:, None, :]) * w
    cov = np.einsum('nka,nkb->nab', c, c) / m[:, :, None]
    lam, vec = np.linalg.eigh(np.where(good[:, None, None], cov, np.eye(3)))
    nr = vec[:, :, 0]
    if viewpoint is None:
        big = np.abs(nr).argmax(1)                                          # the first (lowest axis) of equal magnitudes
        flip = nr[np.arange(n), big] < 0
    else:
        to_v = np.asarray(viewpoint, dtype=np.float64).reshape(1, 3) - p
        s = _dot(nr, np.nan_to_num(to_v))
        flip = s < 0
        sign_near = good & (np.abs(s) < SIGN_REL * np.sqrt(_dot(np.nan_to_num(to_v), np.nan_to_num(to_v))))
    nr = np.where(flip[:, None], -nr, nr)
    normals[good] = nr[good]
    status[good] = 0
    ill = good & ((lam[:, 1] - lam[:, 0]) < ILL_REL * lam[:, 2])
    return dict(normals=normals, status=status, ill=ill, sign_near=sign_near)


def _scaled_features(p, nrm, lists):
    """The pair features of every list entry, scaled to bin coordinates: t [n, K, 3], `valid` [n, K] (entries 1 .. m-1 with an index inside
    the cloud), and the quantities the undecided test looks at."""
    p, nrm = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    count, idx, d2 = lists
    n, K = idx.shape
    k = np.arange(K)[None, :]
    valid = (k >= 1) & (k < count[:, None]) & (idx >= 0) & (idx < n)
    j = np.clip(idx, 0, max(n - 1, 0))
    n1, n2 = np.broadcast_to(nrm[:, None, :], (n, K, 3)), nrm[j]
    dp = p[j] - p[:, None, :]
    with np.errstate(all='ignore'):
        d = np.sqrt(np.where(valid, d2, 1.0))
        a1, a2 = _dot(n1, dp) / d, _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        m1, m2 = np.where(swap[..., None], n2, n1), np.where(swap[..., None], n1, n2)
        dq = np.where(swap[..., None], -dp, dp)
        v = _cross(dq, m1)
        vn = np.sqrt(_dot(v, v))
        live = valid & ~(d == 0) & ~(vn == 0)
        v = v / vn[..., None]
        w = _cross(m1, v)
        f1 = _dot(v, m2)
        f0 = np.arctan2(_dot(w, m2), _dot(m1, m2))
        f2 = np.where(swap, -a2, a1)
        f = np.where(live[..., None], np.stack([f0, f1, f2], axis=-1), 0.0)
        t = np.stack([11.0 * (f[..., 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[..., 1] + 1.0) / 2.0, 11.0 * (f[..., 2] + 1.0) / 2.0], axis=-1)
    return t, valid, d, a1, a2, vn, live


def bin_of(t):
    """floor(t) clamped to [0, 10]; NaN -> 0."""
    with np.errstate(invalid='ignore'):
        return np.where(t >= 0.0, np.where(t >= 10.0, 10, np.floor(np.where(np.isfinite(t), t, 0.0))), 0).astype(np.int64)


def spfh_ref(p, nrm, lists):
    """The census from GIVEN normals -> (counts [n, 33] int32, undecided [n] bool, number of pairs looked at)."""
    t, valid, d, a1, a2, vn, live = _scaled_features(p, nrm, lists)
    n = t.shape[0]
    counts = np.zeros((n, BINS), dtype=np.int32)
    rows = np.broadcast_to(np.arange(n)[:, None], valid.shape)[valid]
    b = bin_of(t)
    for g in range(3):
        np.add.at(counts, (rows, 11 * g + b[..., g][valid]), 1)
    with np.errstate(all='ignore'):
        pair = valid & ~(d == 0)
        near = (np.abs(np.abs(a1) - np.abs(a2)) < EPS) | (~(vn == 0) & (vn < EPS)) | (live & (np.abs(t - np.round(t)) < EPS).any(-1))
    undecided = (pair & near).any(1)
    return counts, undecided, int(valid.sum())


def fpfh_ref(counts, lists):
    """The weighting, in the contract's order: for k ascending, for j ascending within a bin group, val = s_{idx_k}[j] / d2_k; sum_g += val;
    acc_j += val -- explicit loops, never np.sum.  An entry that the contract skips (k >= m, d2_k == 0, an index outside the cloud)
    contributes an exact + 0.0.  -> out [n, 33] float64."""
    counts = np.asarray(counts)
    count, idx, d2 = lists
    n, K = idx.shape
    with np.errstate(divide='ignore'):
        scale = np.where(count > 1, 100.0 / (np.maximum(count, 2) - 1).astype(np.float64), 0.0)
    s = counts.astype(np.float64) * scale[:, None]
    acc, sums = np.zeros((n, BINS)), np.zeros((n, 3))
    for k in range(1, K):
        use = (k < count) & (idx[:, k] >= 0) & (idx[:, k] < n) & (d2[:, k] != 0.0)
        sj = s[np.clip(idx[:, k], 0, max(n - 1, 0))]
        dk = np.where(use, d2[:, k], 1.0)
        for g in range(3):
            for c in range(11):
                val = np.where(use, sj[:, 11 * g + c] / dk, 0.0)
                sums[:, g] = sums[:, g] + val
                acc[:, 11 * g + c] = acc[:, 11 * g + c] + val
    for g in range(3):
        nz = sums[:, g] != 0.0
        wgt = 100.0 / np.where(nz, sums[:, g], 1.0)
        for c in range(11):
            acc[:, 11 * g + c] = np.where(nz, acc[:, 11 * g + c] * wgt, acc[:, 11 * g + c])
    return acc + s


def fpfh_ref_packed(counts, lists, offsets):
    return np.concatenate([fpfh_ref(counts[a:b], tuple(q[a:b] for q in lists)) for a, b in zip(offsets[:-1], offsets[1:])])


def descriptor_ref(p, radius_normal, max_nn_normal, radius_feature, max_nn_feature, viewpoint):
    """The whole chain on the host for one cloud -> [n, 33] float32."""
    nr = normals_ref(p, lists_ref(p, radius_normal, max_nn_normal), viewpoint)['normals']
    lf = lists_ref(p, radius_feature, max_nn_feature)
    return fpfh_ref(spfh_ref(p, nr, lf)[0], lf).astype(np.float32)


# ---- clouds ------------------------------------------------------------------------------------------------------------------------------
def surface(n, seed, bump=False):
    """x, y uniform in [0, 1], z = 0.3 sin 2x cos 2y + uniform(-0.002, 0.002) -> (points [n, 3], given normals [n, 3]): the analytic normals
    plus 0.05 N(0, 1) per component, normalised.  (Estimated normals are not used for the census: points that share a neighbour set get
    normals equal to 1e-16, which puts |a1| = |a2| on a knife edge.)  bump: a fixed asymmetric bump added to z, so that no two parts of
    the surface look alike."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    z = 0.3 * np.sin(2 * x) * np.cos(2 * y) + rng.uniform(-0.002, 0.002, n)
    if bump:
        z = z + 0.15 * np.exp(-((x - 0.3) ** 2 + (y - 0.65) ** 2) / 0.02) - 0.1 * np.exp(-((x - 0.75) ** 2 + (y - 0.2) ** 2) / 0.01)
    nr = np.stack([-0.6 * np.cos(2 * x) * np.cos(2 * y), 0.6 * np.sin(2 * x) * np.sin(2 * y), np.ones(n)], axis=1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    nr = nr + 0.05 * rng.standard_normal((n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return np.stack([x, y, z], axis=1), nr


def lattice(n, seed):
    """n points with integer coordinates in [-4, 4], scaled by 1/8: 729 places, so duplicates and equal distances are dense, and every
    d2 is exact."""
    return np.random.default_rng(seed).integers(-4, 5, (n, 3)).astype(np.float64) / 8.0


def plane_lattice(axis):
    """The 81 points of the 9 x 9 lattice in the plane `axis` = 0."""
    g = np.arange(-4, 5, dtype=np.float64) / 8.0
    a, b = (v.reshape(-1) for v in np.meshgrid(g, g, indexing='ij'))
    cols = [a, b]
    cols.insert(axis, np.zeros_like(a))
    return np.stack(cols, axis=1)


def planted_pair(n=600, seed=11):
    """The end-to-end case: src = surface(n) with the bump; ref = a row-permuted copy moved by a rotation of 30 degrees about z and the
    translation (0.3, -0.2, 0.1).  -> (src, ref, transform 4x4 with ref ~ R src + t, viewpoint on the rotation axis, perm with ref[i] the
    partner of src[perm[i]])."""
    src, _ = surface(n, seed, bump=True)
    a = np.deg2rad(30.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.3, -0.2, 0.1]
    perm = np.random.default_rng(seed + 1).permutation(n)
    ref = (src @ T[:3, :3].T + T[:3, 3])[perm]
    return src, ref, T, np.array([0.0, 0.0, 1000.0]), perm
