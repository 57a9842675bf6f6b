"""numpy fp64 yardstick for the batched RANSAC rigid registration (csrc/ransac.hip, utils/registration.py).

Hypothesis = SVD Kabsch with the determinant fix on the three sampled pairs; count = #{i : |R s_i + t - r_i|^2 <= threshold^2}; selected = the
lowest index among the valid hypotheses with the maximal count; refinement = `refine_rounds` times (mask under the current transform, Kabsch
over the mask, recount, accept if the count did not drop, else stop).  Besides the result it reports where a comparison with another
implementation is not meaningful: `near` (some residual lies within 1e-7 x threshold of the threshold, so the last bits of the transform
decide a count) and `ill` (the sample's cross-covariance has a second singular value below 1e-3 of the first: a near-collinear triangle,
whose rotation about its own axis is not determined to working precision)."""
import numpy as np

FAMILIES = ('clean', 'loose', 'exact', 'far')
NOISE = {'clean': 0.005, 'loose': 0.02, 'exact': 0.0, 'far': 0.005}
INLIER_SHARE = 0.4
NEAR_REL = 1e-7
ILL_REL = 1e-3


def random_transform(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    return T


def make_case(family, n, seed):
    """-> (corr [n, 6], planted 4x4, planted inlier flags [n]).  Source points uniform in a 2 m box; inliers = moved source + uniform
    +-noise per axis; outliers get reference points uniform in the box; rows shuffled.  At least three inliers whenever n >= 3."""
    rng = np.random.default_rng(seed)
    T = random_transform(rng)
    src = rng.uniform(0.0, 2.0, (n, 3))
    ref = src @ T[:3, :3].T + T[:3, 3] + rng.uniform(-1.0, 1.0, (n, 3)) * NOISE[family]
    n_in = min(n, max(3, int(round(INLIER_SHARE * n))))
    planted = np.zeros(n, dtype=bool)
    planted[rng.permutation(n)[:n_in]] = True
    ref[~planted] = rng.uniform(0.0, 2.0, (int((~planted).sum()), 3))
    corr = np.concatenate([src, ref], axis=1)
    if family == 'far':
        v = rng.uniform(500.0, 1500.0, 6) * rng.choice([-1.0, 1.0], 6)          # one constant vector of order 1e3 on all six columns
        corr = corr + v
        T = T.copy()
        T[:3, 3] = T[:3, 3] - T[:3, :3] @ v[:3] + v[3:]
    return np.ascontiguousarray(corr), T, planted


def draw_samples(sizes, iters, seed):
    """The package's rule, restated: per job `iters` triples of distinct row indices (draw from n, n-1, n-2 and shift past the earlier
    picks), the generator restarted from `seed` for every job; none for a job with fewer than three rows.
    -> (samples [total, 3] int32, hyp_offsets [n_jobs + 1] int64)."""
    out, off = [], [0]
    for n in sizes:
        n = int(n)
        if n < 3 or iters <= 0:
            off.append(off[-1])
            continue
        rng = np.random.default_rng(seed)
        a = rng.integers(0, n, iters)
        b = rng.integers(0, n - 1, iters)
        c = rng.integers(0, n - 2, iters)
        b = b + (b >= a)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        c = c + (c >= lo)
        c = c + (c >= hi)
        out.append(np.stack([a, b, c], axis=1))
        off.append(off[-1] + iters)
    s = np.concatenate(out).astype(np.int32) if out else np.zeros((0, 3), dtype=np.int32)
    return s, np.asarray(off, dtype=np.int64)


def kabsch(src, ref):
    """Least-squares proper rigid transform ref ~ R src + t -> (4x4, singular values)."""
    cs, cr = src.mean(0), ref.mean(0)
    H = (src - cs).T @ (ref - cr)
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    D = np.diag([1.0, 1.0, d if d != 0 else 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = cr - R @ cs
    return T, S


def residual2(corr, T):
    d = corr[:, :3] @ T[:3, :3].T + T[:3, 3] - corr[:, 3:]
    return (d * d).sum(1)


def _near(r2, threshold):
    return bool((np.abs(np.sqrt(r2) - threshold) <= NEAR_REL * threshold).any())


def ransac_ref(corr, samples, threshold, refine_rounds=2):
    """One job.  -> dict(status, transform, count, mask, best, hyp_count, valid, near, ill, near_final, rounds_accepted, first_count)."""
    corr = np.asarray(corr, dtype=np.float64)
    samples = np.asarray(samples, dtype=np.int64).reshape(-1, 3)
    n, H = len(corr), len(samples)
    thr2 = threshold * threshold
    hyp_count = np.zeros(H, dtype=np.int32)
    valid = np.zeros(H, dtype=bool)
    near = np.zeros(H, dtype=bool)
    ill = np.zeros(H, dtype=bool)
    models = np.zeros((H, 4, 4))
    for h, (a, b, c) in enumerate(samples):
        if min(a, b, c) < 0 or max(a, b, c) >= n or a == b or a == c or b == c:
            continue
        rows = corr[[a, b, c]]
        T, S = kabsch(rows[:, :3], rows[:, 3:])
        if not np.isfinite(T).all():
            continue
        valid[h] = True
        models[h] = T
        ill[h] = not (S[1] >= ILL_REL * S[0]) or S[0] == 0
        r2 = residual2(corr, T)
        hyp_count[h] = int((r2 <= thr2).sum())
        near[h] = _near(r2, threshold)
    out = dict(status=1, transform=np.eye(4), count=0, mask=np.zeros(n, dtype=np.uint8), best=-1, hyp_count=hyp_count, valid=valid,
               near=near, ill=ill, near_final=False, rounds_accepted=0, first_count=0)
    if n < 3 or not valid.any():
        return out
    cand = np.where(valid, hyp_count, -1)
    best = int(np.argmax(cand))                       # argmax: the lowest index of the maximum
    if cand[best] < 3:
        return out
    T = models[best]
    r2 = residual2(corr, T)
    mask = r2 <= thr2
    count = int(mask.sum())
    near_final = _near(r2, threshold)
    first = count
    accepted = 0
    for _ in range(refine_rounds):
        T2, _ = kabsch(corr[mask, :3], corr[mask, 3:])
        if not np.isfinite(T2).all():
            break
        r2 = residual2(corr, T2)
        near_final = near_final or _near(r2, threshold)          # a round that is rejected still decided something
        m2 = r2 <= thr2
        if int(m2.sum()) >= count:
            T, mask, count = T2, m2, int(m2.sum())
            accepted += 1
        else:
            break
    out.update(status=0, transform=T, count=count, mask=mask.astype(np.uint8), best=best, near_final=near_final,
               rounds_accepted=accepted, first_count=first)
    return out


def ransac_ref_jobs(corrs, samples, hyp_offsets, threshold, refine_rounds=2):
    return [ransac_ref(c, samples[hyp_offsets[j]:hyp_offsets[j + 1]], threshold, refine_rounds) for j, c in enumerate(corrs)]


def compose_shift(T, shift):
    """T fits the rows minus `shift` (a 6-vector: source | reference columns); the transform of the unshifted rows, column convention:
    r = R (s - a) + t + b."""
    out = np.array(T, dtype=np.float64, copy=True)
    out[:3, 3] = T[:3, 3] - T[:3, :3] @ shift[:3] + shift[3:]
    return out


EXCLUDED_CAP = 0.02


def preconditions(ref):
    """What a case must satisfy before another implementation is compared with it exactly -> (compared [H] flags, list of violations).
    Hypotheses that are `near` or `ill` are left out of the count comparison, at most EXCLUDED_CAP of the case's; the final transform (every
    refinement round that decided something) must not be `near`; and no left-out hypothesis may reach the best compared count, or the
    selection itself would hang on it."""
    out = ref['near'] | ref['ill']
    bad = []
    if out.sum() > EXCLUDED_CAP * len(out):
        bad.append(f'{int(out.sum())} of {len(out)} hypotheses are near or ill (cap {EXCLUDED_CAP:.0%})')
    if ref['near_final']:
        bad.append('a residual of the final transform lies within 1e-7 x threshold of the threshold')
    keep = ~out & ref['valid']
    top = int(ref['hyp_count'][keep].max()) if keep.any() else 0
    if out.any() and top >= 3 and int(ref['hyp_count'][out].max()) >= top:
        bad.append('a near or ill hypothesis ties or beats the best compared one')
    return ~out, bad
