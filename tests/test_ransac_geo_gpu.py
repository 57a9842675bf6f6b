"""GPU tier of csrc/ransac_geo.hip against tests/ransac_geo_ref.py.  The fused score (sga_score_transforms_grid): counts exactly those of
numpy and of the unfused search, sum d2 within the summation bound of math.fsum over that search's d2 and with identical bits across cell
sizes, calls and batchings.  The models (sga_ransac_models): valid exactly, moved sample points by the rule of test_ransac_gpu.py, resid2
bit for bit.  The whole path (ransac_geometric_batch, registration_with_ransac_from_feats(score='geometric')): every decision restated in
numpy from the device's own models, so that nothing hangs on the last bits of a solver."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fpfh_ref as PR  # noqa: E402
import icp_ref as IR  # noqa: E402
import ransac_geo_ref as GR  # noqa: E402
import ransac_ref as RR  # noqa: E402
from sgaligner_amd.utils.registration import hypothesis_models_batch, ransac_geometric_batch, score_transforms_batch  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GUARD = 16
SENT_C, SENT_S = -77, -77.5
RADII = (0.1, 0.25, np.inf)
QUERY_SIZES = (0, 1, 3, 1023, 1024, 1025, 2100)          # round the slice of 1024 rows, and three slices


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _cells(r):
    base = 0.1 if np.isinf(r) else r
    return (base / 4, base, 4 * base, 100.0, 1e-9)       # r / 4, r, 4 r, the whole cloud in one cell, far too fine for the key (status 2)


# ---- the scoring kernel -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _score_case():
    """-> (clouds, pairs, transforms [n, 12], live [n])."""
    support = PR.surface(2300, 12, bump=True)[0]
    q = PR.surface(2100, 11, bump=True)[0]
    clouds = [support] + [q[:n].copy() for n in QUERY_SIZES]             # 0; 1 .. 7
    copies = np.tile([[0.25, 0.5, 0.125]], (200, 1))                     # 8: 200 copies of one point
    bad_q = PR.surface(40, 2)[0]                                         # 9: a query row with a NaN, one with an inf
    bad_q[7] = [np.nan, 0.1, 0.0]
    bad_q[19] = [0.1, -np.inf, 0.0]
    bad_s = PR.surface(60, 9)[0]                                         # 10: support rows with a NaN and an inf
    bad_s[0] = [0.0, np.nan, 0.0]
    bad_s[33] = [np.inf, 0.0, 0.0]
    clouds += [copies, bad_q, bad_s, np.zeros((0, 3))]                   # 11: empty
    small = lambda k: IR.rigid12([0.2, -0.1, 1.0], 1.0 + 0.5 * k, [0.01 * k, -0.01, 0.005 * k])
    pairs, tr = [], []
    for k in range(len(QUERY_SIZES)):                                    # the slice edges against the surface
        pairs.append((1 + k, 0))
        tr.append(small(6 + k))                                          # 0.06 to 0.12 along x: r = 0.1 cuts through
    for k in range(5):                                                   # jobs that share both clouds: the hypothesis pattern
        pairs.append((7, 0))
        tr.append(small(3 + 2 * k))
    pairs += [(6, 11), (6, 8), (8, 8), (9, 0), (6, 10), (9, 10)]         # empty support, copies, NaN / inf rows on either side
    tr += [small(1), IR.IDENTITY12, small(2), small(1), small(2), IR.IDENTITY12]
    pairs += [(7, 0), (6, 0)]                                            # carried 1000 away; a NaN in the transform
    far = small(1).copy()
    far[9] += 1000.0
    nan = small(1).copy()
    nan[4] = np.nan
    tr += [far, nan]
    live = np.ones(len(pairs) + 3, dtype=np.int32)
    pairs += [(7, 0), (2, 0), (6, 10)]                                   # live = 0
    tr += [small(3), small(2), small(3)]                                 # job 20 is job 7 again
    live[-3:] = 0
    return clouds, pairs, np.stack(tr), live


@functools.lru_cache(maxsize=None)
def _score_reference():
    """The unmasked numpy search of every job, once: [(d2, idx), ...]."""
    clouds, pairs, tr, _ = _score_case()
    return [IR.nn_moved_ref(clouds[q], clouds[s], tr[p]) for p, (q, s) in enumerate(pairs)]


def _score(pts, off, pairs, G, tr, live, r2):
    """The C entry with guard rows round both outputs -> (count, sum_d2) host arrays."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    from sgaligner_amd.packed import upload, workspace
    h_off, h_pr = np.asarray(off, dtype=np.int32), np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    d_off, d_pr = upload([h_off, h_pr], pts.device)
    n = len(h_pr)
    cnt = torch.full((n + 2 * GUARD,), SENT_C, device=pts.device, dtype=torch.int32)
    sd2 = torch.full((n + 2 * GUARD,), SENT_S, device=pts.device, dtype=torch.float64)
    max_q = max(int(h_off[q + 1] - h_off[q]) for q, _ in pairs)
    L = _lib.lib()
    nbytes = int(L.sga_score_transforms_workspace_bytes(n, max_q))
    ws = workspace(nbytes, pts.device)
    ws.fill_(float('nan'))                                               # the workspace need not be zeroed
    rc = L.sga_score_transforms_grid(_p(pts), _p(d_off), len(h_off) - 1, int(pts.shape[0]), _p(d_pr), n, max_q, h_off.ctypes.data,
                                     h_pr.ctypes.data, _p(G.cell), _p(G.origin), _p(G.dims), _p(G.status), _p(G.order), _p(G.sorted_keys), _p(tr),
                                     _p(live) if live is not None else None, r2, _p(cnt[GUARD:]), _p(sd2[GUARD:]), _p(ws), nbytes, _stream())
    _lib.check(rc, 'sga_score_transforms_grid')
    cnt, sd2 = cnt.cpu().numpy(), sd2.cpu().numpy()
    assert (cnt[:GUARD] == SENT_C).all() and (cnt[GUARD + n:] == SENT_C).all()                   # the guard rows are untouched
    assert (sd2[:GUARD] == SENT_S).all() and (sd2[GUARD + n:] == SENT_S).all()
    return cnt[GUARD:GUARD + n], sd2[GUARD:GUARD + n]


@pytest.mark.parametrize('r', RADII)
def test_score_equals_numpy_and_the_unfused_search(r):
    from sgaligner_amd import ops
    from sgaligner_amd.utils import point_cloud as PC
    from sgaligner_amd.utils import voxel as V
    clouds, pairs, tr, live = _score_case()
    ref = _score_reference()
    n, r2 = len(pairs), r * r
    assert n == 23 and len(tr) == n
    pts, off = _dev(np.concatenate(clouds)), np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    d_tr, d_live = _dev(tr), _dev(live)
    # the unfused route: the parent's search with one job per transform, then host reductions
    was, ops.VALIDATE = ops.VALIDATE, False                              # the NaN and inf rows are the case
    try:
        ud, ui, uo = PC.nearest_neighbor_batch(pts, off, pairs, squared=True, search='grid', radius=None if np.isinf(r) else r, transforms=d_tr,
                                               cell=0.05)
        via_python = score_transforms_batch(pts, off, pairs, d_tr, r, d_live, cell=0.07)
    finally:
        ops.VALIDATE = was
    ud, ui = ud.cpu().numpy(), ui.cpu().numpy()
    want_c, want_s, bound = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
    for p in range(n):
        _, idx = IR.mask_r2(*ref[p], r2)
        d2, has = ud[uo[p]:uo[p + 1]], ui[uo[p]:uo[p + 1]] >= 0
        assert np.array_equal(has, idx >= 0), p                          # the unfused search agrees with numpy on who has a partner
        if live[p]:
            want_c[p], want_s[p] = int(has.sum()), math.fsum(d2[has])
            bound[p] = len(d2) * 2.0 ** -52 * want_s[p]
    assert want_c[:7].tolist() == [0, 1, 3, 1023, 1024, 1025, 2100] or not np.isinf(r)
    assert (want_c[18] == 0 or np.isinf(r)) and want_c[19] == 0 and want_c[12] == 0               # 1000 away, a NaN transform, an empty support
    nq = np.array([len(clouds[q]) for q, _ in pairs])
    assert (want_c[:n - 3] > 0).sum() >= 10 and (np.isinf(r) or ((want_c > 0) & (want_c < nq)).sum() >= 3)      # the radius cuts through the case
    first = None
    for cell in _cells(r):
        G = V.build_grid(pts, off, cell)
        got_c, got_s = _score(pts, off, pairs, G, d_tr, d_live, r2)
        assert got_c.dtype == np.int32 and np.array_equal(got_c, want_c), (r, cell, got_c, want_c)
        err = np.abs(got_s - want_s)
        print(f'r {r} cell {cell}: largest sum_d2 error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}')
        assert (err <= bound).all(), (r, cell, err, bound)
        assert (got_s[want_c == 0] == 0.0).all() and not np.signbit(got_s).any()
        if first is None:
            first = got_s
            assert _bits(_score(pts, off, pairs, G, d_tr, d_live, r2)[1]) == _bits(first)        # two calls
            for p in (3, 5, 6, 9, 16, 17):                                                       # a job alone against in the batch
                c1, s1 = _score(pts, off, [pairs[p]], G, d_tr[p:p + 1].contiguous(), None, r2)
                assert c1[0] == want_c[p] and _bits(s1) == _bits(first[p:p + 1]), (r, p)
            c0, s0 = _score(pts, off, pairs, G, d_tr, None, r2)                                   # no live array: every job is searched
            assert np.array_equal(c0[:n - 3], want_c[:n - 3]) and _bits(s0[:n - 3]) == _bits(first[:n - 3]) and c0[20] == want_c[7] and _bits(s0[20:21]) == _bits(first[7:8])
        assert _bits(got_s) == _bits(first), (r, cell)                   # every cell size
    assert np.array_equal(via_python[0].cpu().numpy(), want_c) and _bits(via_python[1].cpu().numpy()) == _bits(first)


# ---- the models ---------------------------------------------------------------------------------------------------------------------------------
M_THRESHOLD = 0.03
M_TOL = RR.NEAR_REL * M_THRESHOLD


@functools.lru_cache(maxsize=None)
def _model_case():
    corrs, parts, hoff = [], [], [0]
    for family in ('clean', 'far'):
        for n in (3, 64, 515):
            corr = RR.make_case(family, n, 1)[0]
            for H in (1, 65, 512):
                corrs.append(corr)
                parts.append(RR.draw_samples([n], H, 101)[0])
    corrs.append(RR.make_case('clean', 64, 1)[0])                        # planted bad samples: repeated and out-of-range indices
    parts.append(np.array([[5, 5, 6], [5, 6, 5], [7, 7, 7], [0, 1, 64], [-1, 2, 3], [2 ** 31 - 1, 0, 1], [3, 9, 27]], dtype=np.int32))
    for s in parts:
        hoff.append(hoff[-1] + len(s))
    return corrs, parts, np.asarray(hoff, dtype=np.int64)


def test_models_valid_residual_and_counts():
    from sgaligner_amd.utils import registration as RG
    corrs, parts, hoff = _model_case()
    off = np.concatenate([[0], np.cumsum([len(c) for c in corrs])])
    d_corr, d_samples = _dev(np.concatenate(corrs)), _dev(np.concatenate(parts))
    M = hypothesis_models_batch(d_corr, off, d_samples, hoff)
    assert M['models'].dtype == torch.float64 and M['valid'].dtype == torch.int32 and M['resid2'].dtype == torch.float64
    again = hypothesis_models_batch(d_corr, off, d_samples, hoff)
    assert all(_bits(M[k].cpu().numpy()) == _bits(again[k].cpu().numpy()) for k in M)
    models, valid, resid2 = M['models'].cpu().numpy(), M['valid'].cpu().numpy(), M['resid2'].cpu().numpy()
    counts = RG.score_hypotheses_batch(d_corr, off, d_samples, hoff, M_THRESHOLD).cpu().numpy()
    worst, left_out = 0.0, 0
    for j, (corr, s) in enumerate(zip(corrs, parts)):
        sl = slice(hoff[j], hoff[j + 1])
        ref = RR.ransac_ref(corr, s, M_THRESHOLD, 0)
        m, v = models[sl], valid[sl] != 0
        assert np.array_equal(v, ref['valid']), j                        # valid is exact
        assert np.isnan(m[~v]).all() and np.isposinf(resid2[sl][~v]).all() and np.isfinite(m[v]).all()
        assert _bits(resid2[sl]) == _bits(GR.resid2_ref(m, corr, s)), j  # bit for bit from the downloaded model
        for h in np.flatnonzero(v):
            rows = corr[s[h]]
            if not ref['ill'][h]:
                T, _ = RR.kabsch(rows[:, :3], rows[:, 3:])
                worst = max(worst, float(np.abs(IR.move(rows[:, :3], m[h]) - (rows[:, :3] @ T[:3, :3].T + T[:3, 3])).max()))
        # the count under the device model against ransac.hip's own count, on the hypotheses that are not near
        keep = v & ~ref['near']
        left_out += int((v & ref['near']).sum())
        R, t = m[:, :9].reshape(-1, 3, 3), m[:, 9:]
        with np.errstate(invalid='ignore'):
            d = np.einsum('hab,nb->hna', R, corr[:, :3]) + t[:, None, :] - corr[None, :, 3:]
            mine = ((d * d).sum(2) <= M_THRESHOLD * M_THRESHOLD).sum(1)
        assert np.array_equal(mine[keep], counts[sl][keep]), j
        assert (counts[sl][~v] == 0).all()
    print(f'models: moved sample points within {worst:.3e} of SVD Kabsch (allowed {M_TOL:.1e}); {left_out} near hypotheses left out of the counts')
    assert worst <= M_TOL
    assert valid[hoff[-2]:].tolist() == [0, 0, 0, 0, 0, 0, 1]


# ---- the whole path -----------------------------------------------------------------------------------------------------------------------------
FIELDS = ('transform', 'fitness', 'inlier_rmse', 'best_hyp', 'n_validated', 'status', 'hyp_count', 'hyp_sum_d2')


def _geo(cases, max_validation, cell=None):
    """ransac_geometric_batch on a list of dict(src, ref, corr, samples) -> (host dict, hyp_offsets)."""
    clouds = [c for k in cases for c in (k['src'], k['ref'])]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    coff = np.concatenate([[0], np.cumsum([len(k['corr']) for k in cases])])
    hoff = np.concatenate([[0], np.cumsum([len(k['samples']) for k in cases])])
    samples = np.concatenate([k['samples'].reshape(-1, 3) for k in cases]).astype(np.int32)
    res = ransac_geometric_batch(_dev(np.concatenate(clouds)), off, [(2 * p, 2 * p + 1) for p in range(len(cases))],
                                 _dev(np.concatenate([k['corr'] for k in cases])), coff, _dev(samples), hoff, GR.THRESHOLD, max_validation, cell)
    assert res['transform'].dtype == torch.float64 and res['hyp_sum_d2'].dtype == torch.float64
    assert all(res[k].dtype == torch.int32 for k in ('best_hyp', 'n_validated', 'status', 'hyp_count', 'valid'))
    return {k: v.cpu().numpy() for k, v in res.items()}, hoff


def _job_bits(out, hoff, j):
    return [_bits(out[k][hoff[j]:hoff[j + 1]] if k.startswith('hyp_') else out[k][j]) for k in FIELDS]


@pytest.mark.parametrize('seed', GR.SEEDS)
def test_whole_path_every_decision_restated(seed):
    case = GR.whole_case(seed)
    thr2 = GR.THRESHOLD * GR.THRESHOLD
    brute = {}
    for K in GR.MAX_VALIDATION:
        out, _ = _geo([case], K)
        models, valid, resid2 = out['models'], out['valid'], out['resid2']
        want = GR.validated_ref(valid, resid2, thr2, K)                  # the first K passing hypotheses, from the device's valid and resid2
        assert np.array_equal(np.flatnonzero(out['hyp_count'] >= 0), want) and len(want) == min(K, len(GR.validated_ref(valid, resid2, thr2, 10 ** 6)))
        assert int(out['n_validated'][0]) == len(want)
        assert np.isposinf(out['hyp_sum_d2'][out['hyp_count'] < 0]).all() and (out['hyp_count'] >= -1).all()
        for h in want:                                                   # brute-force numpy under the device's own model
            if h not in brute:
                brute[h] = GR.score_ref(case['src'], case['ref'], models[h], thr2)[:2]
            assert int(out['hyp_count'][h]) == brute[h][0], (K, h)
            assert abs(out['hyp_sum_d2'][h] - brute[h][1]) <= GR.N_SRC * 2.0 ** -52 * brute[h][1], (K, h)
        best = GR.select_ref(out['hyp_count'], out['hyp_sum_d2'])        # over the device's own scores
        assert int(out['best_hyp'][0]) == best >= 0 and int(out['status'][0]) == 0
        T = out['transform'][0]
        assert _bits(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])) == _bits(models[best]) and _bits(T[3]) == _bits(np.array([0.0, 0.0, 0.0, 1.0]))
        cnt = int(out['hyp_count'][best])
        assert out['fitness'][0] == cnt / GR.N_SRC and abs(out['inlier_rmse'][0] - math.sqrt(out['hyp_sum_d2'][best] / cnt)) <= 1e-15
        print(f'seed {seed} max_validation {K}: validated {len(want)}, best {best} count {cnt} rmse {out["inlier_rmse"][0]:.5f}')
        assert case['partner'][case['samples'][best]].all()              # the three sampled rows of the winner are true partners
        assert K < 1000 or cnt >= 280                                    # test_ransac_geo_cpu.py: the best of all passing ones has 294 to 296
    if seed == 0:                                                        # the cell is a speed choice only
        again, _ = _geo([case], 1000, cell=0.3)
        assert all(_bits(again[k]) == _bits(out[k]) for k in FIELDS)


def test_batch_equals_single_jobs_bitwise():
    from sgaligner_amd.utils import registration as RG
    cases = [GR.whole_case(s) for s in GR.SEEDS]
    c0 = cases[0]
    # the device's edge-length checker is the yardstick's
    raw = RR.draw_samples([GR.N_SRC], GR.N_HYP, 0)[0]
    assert np.array_equal(RG.edge_length_filter(_dev(c0['corr']), [0, GR.N_SRC], _dev(raw), [0, GR.N_HYP]).cpu().numpy(), c0['samples'])
    two = {'src': c0['src'], 'ref': c0['ref'], 'corr': c0['corr'][:2].copy(), 'samples': np.zeros((0, 3), dtype=np.int32)}       # two correspondences
    grown = c0['corr'].copy()
    grown[:, 3:] *= 2.0                                                  # a reference twice the size: no rigid model brings three pairs within 0.05
    none = {'src': c0['src'], 'ref': 2.0 * c0['ref'], 'corr': grown, 'samples': RR.draw_samples([GR.N_SRC], 65, 5)[0]}
    jobs = cases + [two, none]
    for K in (7, 1000):
        out, hoff = _geo(jobs, K)
        assert out['status'].tolist() == [0, 0, 0, 1, 1] and out['best_hyp'][3:].tolist() == [-1, -1] and out['n_validated'][3:].tolist() == [0, 0]
        assert np.array_equal(out['transform'][3], np.eye(4)) and np.array_equal(out['transform'][4], np.eye(4))
        assert out['fitness'][3:].tolist() == [0.0, 0.0] and out['inlier_rmse'][3:].tolist() == [0.0, 0.0]
        assert (out['valid'][hoff[4]:] != 0).any() and (out['hyp_count'][hoff[4]:] == -1).all()
        assert _geo(jobs, K)[0]['transform'].tobytes() == out['transform'].tobytes()
        for j, job in enumerate(jobs):
            single, h1 = _geo([job], K)
            assert _job_bits(out, hoff, j) == _job_bits(single, h1, 0), (K, j)


def test_public_entry_with_geometric_score():
    from sgaligner_amd.utils import registration as RG
    import featnn_ref as FR
    c = FR.planted_registration(1, GR.N_SRC, GR.N_OUT)
    ref = c['ref'] + np.random.default_rng(7).uniform(-GR.NOISE, GR.NOISE, c['ref'].shape)
    args = (c['src'], ref, c['src_feats'], c['ref_feats'])
    T, info = RG.registration_with_ransac_from_feats(*args, num_iterations=GR.N_HYP, val_iterations=32, seed=3, score='geometric', return_info=True)
    # the same stages by hand: every source row with its partner (the codes are distinct), the samples, the checker, the batch function
    corr = np.concatenate([c['src'], ref[c['perm']]], axis=1)
    samples = GR.edge_length_ref(corr, RR.draw_samples([GR.N_SRC], GR.N_HYP, 3)[0])
    out, _ = _geo([{'src': c['src'], 'ref': ref, 'corr': corr, 'samples': samples}], 32)
    assert int(out['status'][0]) == 0 and _bits(T) == _bits(out['transform'][0])
    assert info == {'status': 0, 'fitness': float(out['fitness'][0]), 'inlier_rmse': float(out['inlier_rmse'][0]), 'best_hyp': int(out['best_hyp'][0]),
                    'n_validated': 32}
    assert info['fitness'] > 0.9 and RG.compute_registration_error(c['transform'], T)[0] < 3.0
    pairs = RG.registration_with_ransac_from_feats_pairs([args, args], num_iterations=GR.N_HYP, val_iterations=32, seed=3, score='geometric')
    assert _bits(pairs[0]) == _bits(T) and _bits(pairs[1]) == _bits(T)
    # 'correspondence' is the path as it was, with or without the keyword
    plain = RG.registration_with_ransac_from_feats(*args, num_iterations=GR.N_HYP, seed=3)
    named, info = RG.registration_with_ransac_from_feats(*args, num_iterations=GR.N_HYP, seed=3, score='correspondence', return_info=True)
    assert _bits(plain) == _bits(named) and info['status'] == 0 and info['inlier_count'] >= 250 and set(info) == {'status', 'inlier_count', 'best_hyp'}
    with pytest.raises(ValueError, match='score must be one of'):
        RG.registration_with_ransac_from_feats(*args, score='fitness')


def test_both_tie_keys_decide():
    """One true triple four times -- twice as drawn, once with its rows in another order, once more as drawn: the repeats tie in count AND in
    sum d2 bit for bit, so the lowest index must win among them; the reordered triple is another model that competes on count, then sum d2."""
    case = GR.whole_case(0)
    t = case['samples'][int(_geo([case], 1000)[0]['best_hyp'][0])]       # a triple that passes both checkers
    job = dict(case, samples=np.array([t[[1, 0, 2]], t, t, t[[2, 1, 0]], t], dtype=np.int32))
    out, _ = _geo([job], 1000)
    c, s = out['hyp_count'], out['hyp_sum_d2']
    assert (c >= 0).all() and c[1] == c[2] == c[4] and _bits(s[1:2]) == _bits(s[2:3]) == _bits(s[4:5])
    best = GR.select_ref(c, s)
    assert int(out['best_hyp'][0]) == best and best in (0, 1, 3)
    print('tie keys: counts', c.tolist(), 'sum d2', s.tolist(), 'best', best)
