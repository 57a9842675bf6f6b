"""Yardstick of the cross-cloud grid search (csrc/icp.hip, sga_nn_search_grid): the contract of include/sgaligner_hip.h restated in plain
numpy.  numpy never contracts a multiply and an add, so every operation below is a separate fp64 rounding, as the kernel promises:

    x' = ((m0 x + m1 y) + m2 z) + m9 ...        the moved query, m the row-major [R | t] of the job (None: the query as it is)
    d2 = (dx dx + dy dy) + dz dz                dx = x' - s.x ...
    result = the support point of minimal d2 among those with d2 <= r2, the LOWEST index among exactly equal minima; a NaN or +inf d2
             never wins; nothing within r2 (or an empty support): (+inf, -1)

No grid appears here: the grid decides how much of the support the kernel looks at, never what comes out."""
import numpy as np


def move(q, m):
    """q [n, 3] float64, m: 12 numbers (R row-major, then t) or None -> the moved points [n, 3], bit for bit the kernel's."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    if m is None:
        return q.copy()
    m = np.asarray(m, dtype=np.float64).reshape(12)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r] for r in range(3)], axis=1)


def rigid12(axis, degrees, t):
    """The 12-number model of a rotation by `degrees` about `axis` (Rodrigues) followed by the translation t."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(degrees)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
    return np.concatenate([R.reshape(9), np.asarray(t, dtype=np.float64)])


IDENTITY12 = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def nn_moved_ref(q, s, m=None, rows=256):
    """The unmasked search: (d2 [nq] float64, idx [nq] int64) of the moved queries against s [ns, 3]; (+inf, -1) where no d2 is below +inf."""
    qm, s = move(q, m), np.asarray(s, dtype=np.float64).reshape(-1, 3)
    nq = len(qm)
    d2o, idx = np.full(nq, np.inf), np.full(nq, -1, dtype=np.int64)
    if len(s) == 0:
        return d2o, idx
    sx, sy, sz = (np.ascontiguousarray(s[:, c])[None, :] for c in range(3))
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, nq, rows):
            b = min(nq, a + rows)
            dx, dy, dz = qm[a:b, 0:1] - sx, qm[a:b, 1:2] - sy, qm[a:b, 2:3] - sz
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(np.isnan(d2), np.inf, d2)                      # a NaN never wins
            i = np.argmin(d2, axis=1)                                    # the first, i.e. lowest, index of the minimum
            mn = d2[np.arange(b - a), i]
            d2o[a:b], idx[a:b] = mn, np.where(mn < np.inf, i, -1)
    return d2o, idx


def mask_r2(d2, idx, r2):
    """(d2, idx) of an unmasked search -> the same within r2: (+inf, -1) where d2 > r2."""
    keep = d2 <= r2
    return np.where(keep, d2, np.inf), np.where(keep, idx, -1)


def nn_grid_ref(q, s, m=None, r2=np.inf):
    return mask_r2(*nn_moved_ref(q, s, m), r2)


# ---- the ICP loop (sga_icp) ---------------------------------------------------------------------------------------------------------------
# The yardstick solvers are NOT the kernel's: SVD Kabsch for point-to-point, numpy.linalg.solve for point-to-plane.  Everything else -- the
# search, the counts, the order of the decisions -- restates the contract.
def kabsch12(a, b):
    """The least-squares proper rotation + translation with b ~ R a + t, by SVD -> 12 numbers."""
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return np.concatenate([R.reshape(9), cb - R @ ca])


def plane12(x, s, n, pivot):
    """One Gauss-Newton step of point-to-plane about `pivot`: r = (a - b) . n, J = [a x n, n], (sum J J^T) u = -sum J r by linalg.solve;
    R_U = Rz(u2) Ry(u1) Rx(u0), t_U = (u3, u4, u5) + pivot - R_U pivot.  None when the normal matrix is not positive definite."""
    a, b = x - pivot, s - pivot
    r = ((a - b) * n).sum(1)
    J = np.concatenate([np.cross(a, n), n], axis=1)
    A, g = J.T @ J, J.T @ r
    try:
        np.linalg.cholesky(A)
        u = np.linalg.solve(A, -g)
    except np.linalg.LinAlgError:
        return None
    ca, sa, cb, sb, cg, sg = np.cos(u[0]), np.sin(u[0]), np.cos(u[1]), np.sin(u[1]), np.cos(u[2]), np.sin(u[2])
    R = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                  [-sb, cb * sa, cb * ca]])
    return np.concatenate([R.reshape(9), u[3:] + pivot - R @ pivot])


def compose12(u, t):
    """U after T: R = R_U R_T, t = R_U t_T + t_U."""
    Ru, Rt = u[:9].reshape(3, 3), t[:9].reshape(3, 3)
    return np.concatenate([(Ru @ Rt).reshape(9), Ru @ t[9:] + u[9:]])


def update12(method, xm, ref, idx, normals, pivot):
    """The yardstick's update from a correspondence set (idx [nq], -1: none) of the moved queries xm -> 12 numbers or None."""
    has = idx >= 0
    if method == 0:
        return kabsch12(xm[has], ref[idx[has]])
    return plane12(xm[has], ref[idx[has]], normals[idx[has]], pivot)


def box_min(ref):
    """The pivot the Python layer passes: the minimum of the reference cloud's rows without a non-finite coordinate; 0 without one."""
    keep = np.isfinite(ref).all(1)
    return ref[keep].min(0) if keep.any() else np.zeros(3)


def icp_ref(src, ref, t0, max_distance, method=0, normals=None, max_iters=30, rel_fitness=1e-6, rel_rmse=1e-6, tau=None):
    """sga_icp for one job -> dict(transform [12], fitness, rmse, iters, status, trace [evaluations, 2], idx, d2 of the final transform,
    sum_d2 / count per evaluation, and with tau: near [evaluations] = the number of queries whose outcome a perturbation of tau could change --
    | sqrt(d2) - max_distance | <= 2 tau, or the two nearest reference points within 2 tau of each other in distance)."""
    src, ref = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    T, r2, pivot = np.asarray(t0, dtype=np.float64).reshape(12).copy(), max_distance * max_distance, box_min(ref)
    trace, sums, near, status, pf, pr = [], [], [], 0, 0.0, 0.0
    for k in range(max_iters + 1):
        xm = move(src, T)
        if tau is not None and len(ref) and len(src):
            e = xm[:, None, :] - ref[None, :, :]
            D = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            two = np.sqrt(np.partition(D, min(1, len(ref) - 1), axis=1)[:, :2])
            flag = np.abs(two[:, 0] - max_distance) <= 2 * tau
            if two.shape[1] > 1:
                flag |= (two[:, 1] - two[:, 0]) <= 2 * tau
            near.append(int(flag.sum()))
        d2, idx = mask_r2(*nn_moved_ref(xm, ref), r2)
        has = idx >= 0
        cnt = int(has.sum())
        fit = cnt / len(src) if len(src) else 0.0
        sd2 = float(d2[has].sum())
        rm = float(np.sqrt(sd2 / cnt)) if cnt else 0.0
        trace.append((fit, rm))
        sums.append((sd2, cnt))
        done = k == max_iters or (k >= 1 and abs(fit - pf) < rel_fitness and abs(rm - pr) < rel_rmse)
        pf, pr = fit, rm
        if done:
            break
        if cnt < (3 if method == 0 else 6):
            status = 1
            break
        U = update12(method, xm, ref, idx, normals, pivot)
        if U is None or not np.isfinite(U).all():
            status = 2
            break
        T = compose12(U, T)
    return {'transform': T, 'fitness': fit, 'rmse': rm, 'iters': k, 'status': status, 'trace': np.array(trace), 'idx': idx, 'd2': d2,
            'sums': sums, 'near': near}


def matrix44(m):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(m)[:9].reshape(3, 3), np.asarray(m)[9:]
    return T


def rre_rte(truth, est):
    """Rotation error in degrees and translation error of two 12-number models."""
    Rt, Re = truth[:9].reshape(3, 3), est[:9].reshape(3, 3)
    c = np.clip(0.5 * (np.trace(Re.T @ Rt) - 1.0), -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(truth[9:] - est[9:]))


def surface_case(n_src, n_ref, degrees, shift=0.0):
    """The whole-run case: src = fpfh_ref.surface(n_src, 11, bump), ref = surface(n_ref, 12, bump) moved by planted_pair's transform (30
    degrees about z, (0.3, -0.2, 0.1)), both shifted by `shift`; the start is the truth followed by a rotation of `degrees` about
    (0.2, -0.1, 1) through the reference's centroid and the translation (0.02, -0.01, 0.015).  The reference's normals are the surface's
    given ones, rotated.  -> dict(src, ref, normals, truth [12], start [12])."""
    import fpfh_ref as PR
    src = PR.surface(n_src, 11, bump=True)[0]
    base, nr = PR.surface(n_ref, 12, bump=True)
    T = PR.planted_pair(8, 11)[2]
    R, t = T[:3, :3], T[:3, 3]
    ref = base @ R.T + t + shift
    src = src + shift
    truth = np.concatenate([R.reshape(9), t + shift - R @ np.full(3, shift)])
    c = ref.mean(0)
    P = rigid12([0.2, -0.1, 1.0], degrees, [0.02, -0.01, 0.015])
    Rp = P[:9].reshape(3, 3)
    P = np.concatenate([P[:9], c - Rp @ c + P[9:]])                       # the rotation turns about the reference's centroid
    return {'src': src, 'ref': ref, 'normals': nr @ R.T, 'truth': truth, 'start': compose12(P, truth)}


WHOLE_RUNS = ((600, 700, 3.0), (2000, 2300, 5.0))
MAX_DISTANCE = 0.05
TAU = 1e-7 * MAX_DISTANCE
