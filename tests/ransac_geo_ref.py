"""Yardstick of the geometrically scored feature-matching RANSAC (csrc/ransac_geo.hip, utils/registration.py): the contract of
include/sgaligner_hip.h restated in plain numpy, on top of icp_ref (the search), ransac_ref (SVD Kabsch, near / ill) and featnn_ref (the
planted case).  numpy never contracts a multiply and an add, so the residual below has the kernel's very roundings.

    resid2   = max over the three sampled rows of (dx dx + dy dy) + dz dz, dx = (((m0 x + m1 y) + m2 z) + m9) - r.x ...
    passing  = valid and resid2 <= threshold^2                       (Open3D's distance checker; the edge-length checker came before)
    validated = the first max_validation passing hypotheses in ascending index
    score    = (count, sum d2) of icp_ref.nn_grid_ref of ALL source points under the model at r = threshold
    selected = the largest count, then the smallest sum d2, then the lowest index; a best count below 3 is no model"""
import math

import numpy as np

import featnn_ref as FR
import icp_ref as IR
import ransac_ref as RR

THRESHOLD = 0.05
MAX_VALIDATION = (1, 7, 32, 1000)
SEEDS = (0, 1, 2)
N_SRC, N_OUT, N_HYP = 300, 100, 512
NOISE, REDIRECTED = 0.03, 0.4


def model12(T):
    T = np.asarray(T, dtype=np.float64)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def resid2_ref(models, corr, samples):
    """models [H, 12], corr [n, 6], samples [H, 3] (valid ones only are meaningful) -> [H] float64, bit for bit the kernel's resid2 of a
    valid hypothesis."""
    out = np.full(len(models), np.inf)
    n = len(corr)
    for h, (m, s) in enumerate(zip(models, np.asarray(samples, dtype=np.int64))):
        if s.min() < 0 or s.max() >= n or not np.isfinite(m).all():
            continue
        rows = corr[s]
        d = IR.move(rows[:, :3], m) - rows[:, 3:]
        out[h] = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
    return out


def score_ref(q, s, m, r2):
    """-> (count, math.fsum of the d2, d2 [nq], idx [nq]) of the moved queries against s within r2."""
    d2, idx = IR.nn_grid_ref(q, s, m, r2)
    has = idx >= 0
    return int(has.sum()), math.fsum(d2[has]), d2, idx


def validated_ref(valid, resid2, thr2, max_validation):
    """-> the indices of the validated hypotheses, ascending."""
    return np.flatnonzero((np.asarray(valid) != 0) & (np.asarray(resid2) <= thr2))[:max_validation]


def select_ref(hyp_count, hyp_sum_d2):
    """The lexicographic choice over the scored hypotheses (count >= 0): -> index, or -1 without one or with a best count below 3."""
    c = np.asarray(hyp_count, dtype=np.int64)
    if not (c >= 0).any() or c.max() < 3:
        return -1
    top = np.flatnonzero(c == c.max())
    s = np.asarray(hyp_sum_d2)[top]
    return int(top[np.flatnonzero(s == s.min())[0]])


def edge_length_ref(corr, samples, similarity=0.9):
    """registration.edge_length_filter for one job in numpy: a failing triple becomes its first index three times."""
    sm = np.asarray(samples, dtype=np.int64)
    rows = corr[sm]                                                       # [H, 3, 6]
    ok = np.ones(len(sm), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        d = rows[:, a] - rows[:, b]
        sq = d * d
        ds, dr = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]), np.sqrt((sq[:, 3] + sq[:, 4]) + sq[:, 5])
        ok &= (ds >= similarity * dr) & (dr >= similarity * ds)
    return np.where(ok[:, None], sm, sm[:, :1]).astype(np.int32)


def whole_case(seed):
    """featnn_ref.planted_registration(seed, 300, 100) with uniform +-0.03 noise per axis on the reference and 40 % of the correspondences
    redirected to random reference rows; 512 sample triples by draw_samples([300], 512, seed), through the edge-length checker.
    -> dict(src, ref, corr [300, 6], partner [300] (row i's reference row is src[i]'s true partner), samples [512, 3] int32, transform)."""
    c = FR.planted_registration(seed, N_SRC, N_OUT)
    rng = np.random.default_rng(1000 + seed)
    ref = c['ref'] + rng.uniform(-NOISE, NOISE, c['ref'].shape)
    to = c['perm'].copy()
    moved = rng.permutation(N_SRC)[:int(REDIRECTED * N_SRC)]
    to[moved] = rng.integers(0, len(ref), len(moved))
    corr = np.ascontiguousarray(np.concatenate([c['src'], ref[to]], axis=1))
    samples, _ = RR.draw_samples([N_SRC], N_HYP, seed)
    return {'src': c['src'], 'ref': ref, 'corr': corr, 'partner': to == c['perm'], 'samples': edge_length_ref(corr, samples),
            'transform': c['transform']}


def whole_case_census(case, threshold=THRESHOLD):
    """The case under SVD Kabsch: per hypothesis valid, ill, passing (both checkers), near (at the distance checker or in the geometric
    count: a distance within NEAR_REL x threshold of the threshold), and the geometric count / sum d2 of the passing ones (-1 / inf
    elsewhere)."""
    corr, samples, H = case['corr'], case['samples'], len(case['samples'])
    valid, ill, near, passing = (np.zeros(H, dtype=bool) for _ in range(4))
    count, sum_d2 = np.full(H, -1, dtype=np.int64), np.full(H, np.inf)
    for h, (a, b, c) in enumerate(samples):
        if a == b or a == c or b == c:
            continue
        rows = corr[[a, b, c]]
        T, S = RR.kabsch(rows[:, :3], rows[:, 3:])
        valid[h] = True
        ill[h] = not (S[1] >= RR.ILL_REL * S[0]) or S[0] == 0
        r = np.sqrt(RR.residual2(rows, T))
        near[h] = bool((np.abs(r - threshold) <= RR.NEAR_REL * threshold).any())
        passing[h] = r.max() <= threshold
        if passing[h]:
            d2, _ = IR.nn_moved_ref(case['src'], case['ref'], model12(T))
            near[h] |= bool((np.abs(np.sqrt(d2) - threshold) <= RR.NEAR_REL * threshold).any())
            count[h], sum_d2[h] = int((d2 <= threshold * threshold).sum()), float(d2[d2 <= threshold * threshold].sum())
    return {'valid': valid, 'ill': ill, 'near': near, 'passing': passing, 'count': count, 'sum_d2': sum_d2}
