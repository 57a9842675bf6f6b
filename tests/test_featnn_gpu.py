"""GPU tier of the feature-space nearest-neighbour search (csrc/featnn.hip) and the registration from features built on it: exact on an
integer lattice with dense ties (indices equal to the fp64 yardstick, distances bit-equal), the same through the chunked form, packed
jobs with empty sets, continuous data inside the fp32 error bound of featnn_ref, a planted registration recovered from descriptors, the
edge-length checker, and the evaluator's two matcher paths."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import featnn_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu

Q_SIZES, S_SIZES = (1, 31, 32, 33, 129), (1, 31, 33, 64, 257)


def _search(sets, pairs, chunk=None):
    """feature_nn_batch on a list of float32 numpy sets -> [(idx int64, d2 float64), ...] per pair, on the host."""
    from sgaligner_amd.utils import registration as RG
    packed, off = FR.pack(sets)
    idx, d2, oo = RG.feature_nn_batch(torch.from_numpy(packed).cuda(), off, pairs, chunk=chunk)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and idx.is_cuda and d2.is_cuda and oo.dtype == np.int64
    idx, d2 = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()
    return [(idx[oo[p]:oo[p + 1]], d2[oo[p]:oo[p + 1]]) for p in range(len(pairs))]


def _assert_exact(got, q, s):
    want_idx, want_d2 = FR.nn_ref(q, s)
    assert np.array_equal(got[0], want_idx), (len(q), len(s), int((got[0] != want_idx).sum()))
    assert np.array_equal(got[1].view(np.int64), want_d2.view(np.int64)), (len(q), len(s))


@pytest.mark.parametrize('c', [4, 8, 36, 260, 1, 3, 33])
def test_lattice_is_exact(c):
    """Integer features in [-8, 8]: every product and partial sum is exact in fp32, so the kernel's scores tie exactly where the true
    distances do and the answer must equal the yardstick's everywhere.  4, 8, 36, 260 go to the entry as they are, 1, 3, 33 through the
    zero padding.  Every query size against every support size, all in one call; the supports are full of duplicated rows."""
    sets = FR.lattice_sets(Q_SIZES + S_SIZES, c, seed=100 + c)
    pairs = [(a, len(Q_SIZES) + b) for a in range(len(Q_SIZES)) for b in range(len(S_SIZES))]
    res = _search(sets, pairs)
    ties = 0
    for (a, b), got in zip(pairs, res):
        _assert_exact(got, sets[a], sets[b])
        d = FR.d2_matrix(sets[a], sets[b])
        ties += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 100                                            # the family exists for its ties


def test_chunked_equals_unchunked_and_the_lowest_index_wins(monkeypatch):
    from sgaligner_amd import _lib
    from sgaligner_amd.utils import registration as RG
    q, s257, s700 = FR.lattice_sets((130, 257, 700), 36, seed=7, n_codes=4000)           # few accidental ties: the planted ones decide
    s257[230], s700[600], s700[300] = s257[5], s700[17], s700[17]                        # the same row in the first and in later chunks
    q[0], q[129] = s257[5], s700[17]
    whole = _search([q, s257, s700], [(0, 1), (0, 2)])
    assert whole[0][0][0] == 5 and whole[1][0][129] == 17 and whole[0][1][0] == 0.0
    # chunks of the 257-row / 700-row support: 3 (57 rows in the last) / 7, 2 (1 row) / 3 (188 rows), 5 (1 row) / 11 (60 rows)
    for chunk, n_chunks in ((100, 7), (256, 3), (64, 11)):
        assert _lib.lib().sga_featnn_workspace_bytes(130 + 257 + 700, 260, 700, chunk) == (130 + 257 + 700) * 4 + 4 + 8 * n_chunks * 260
        monkeypatch.setattr(RG, 'FEATNN_CHUNK', chunk)
        split = _search([q, s257, s700], [(0, 1), (0, 2)])
        monkeypatch.setattr(RG, 'FEATNN_CHUNK', None)
        for w, g, s in zip(whole, split, (s257, s700)):
            assert np.array_equal(w[0], g[0]) and np.array_equal(w[1].view(np.int64), g[1].view(np.int64)), chunk
            _assert_exact(g, q, s)


def test_packed_jobs_with_empty_sets_and_a_self_match():
    a, d, e = FR.lattice_sets((50, 129, 70), 8, seed=21)
    empty = np.zeros((0, 8), dtype=np.float32)
    sets = [a, empty, d, e]
    pairs = [(0, 2), (0, 1), (1, 0), (2, 2), (3, 0), (2, 3)]
    res = _search(sets, pairs)
    assert (res[1][0] == -1).all() and np.isposinf(res[1][1]).all() and len(res[1][0]) == 50          # empty support
    assert len(res[2][0]) == 0                                                                         # empty query set
    assert (res[3][1] == 0.0).all()                                                                    # a set against itself: distance 0,
    assert np.array_equal(res[3][0], [int(np.flatnonzero((d == r).all(1))[0]) for r in d])             # at the first copy of each row
    for p in (0, 3, 4, 5):
        _assert_exact(res[p], sets[pairs[p][0]], sets[pairs[p][1]])
        alone, = _search(sets, [pairs[p]])                       # independent of which other jobs share the call
        assert np.array_equal(alone[0], res[p][0]) and np.array_equal(alone[1].view(np.int64), res[p][1].view(np.int64))


@pytest.mark.parametrize('c', [33, 256])
def test_continuous_data_stays_inside_the_fp32_bound(c):
    """Gaussian rows: the returned row is within 2 max_j E(i, j) of the true nearest (featnn_ref's bound for an fp32 score of length C in
    any order), and out_d2 is the sequential fp64 sum for the returned row, bit for bit."""
    q, s = FR.gaussian_pair(500, 700, c, seed=c)
    (idx, d2), = _search([q, s], [(0, 1)])
    true = FR.d2_matrix(q, s)
    excess = true[np.arange(500), idx] - true.min(1)
    bound = 2.0 * FR.error_bound(q, s).max(1)
    print(f'C={c}: {int((idx != true.argmin(1)).sum())} of 500 indices differ from the fp64 arg-min; max excess {excess.max():.3e}, '
          f'min bound {bound.min():.3e}')
    assert (idx >= 0).all() and (idx < 700).all()
    assert (excess <= bound).all(), (float(excess.max()), float(bound.min()))
    assert np.array_equal(d2.view(np.int64), FR.seq_d2(q, s[idx]).view(np.int64))


@pytest.fixture(scope='module')
def planted():
    return [FR.planted_registration(seed) for seed in (3, 4, 5)]


@pytest.mark.parametrize('mutual', [True, False])
def test_registration_from_features_recovers_the_planted_transform(planted, mutual):
    from sgaligner_amd.utils import registration as RG
    matches = RG.match_features_pairs([(c['src_feats'], c['ref_feats']) for c in planted], mutual=mutual)
    for c, (cij, d2) in zip(planted, matches):
        assert cij.dtype == torch.int64 and cij.is_cuda
        assert np.array_equal(cij.cpu().numpy(), np.stack([np.arange(300), c['perm']], axis=1))
        assert (d2.cpu().numpy() == 0.0).all()
    singles = [RG.registration_with_ransac_from_feats(c['src'], c['ref'], c['src_feats'], c['ref_feats'], num_iterations=2000, mutual=mutual,
                                                      seed=1) for c in planted]
    for c, t in zip(planted, singles):
        assert t.shape == (4, 4) and np.abs(t - c['transform']).max() < 1e-9
    many = RG.registration_with_ransac_from_feats_pairs([(c['src'], c['ref'], c['src_feats'], c['ref_feats']) for c in planted],
                                                        num_iterations=2000, mutual=mutual, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(singles, many))


def test_registration_from_features_without_a_model_is_the_identity():
    from sgaligner_amd.utils import registration as RG
    c = FR.planted_registration(9)
    t = RG.registration_with_ransac_from_feats(c['src'][:2], c['ref'], c['src_feats'][:2], c['ref_feats'], num_iterations=16)
    assert np.array_equal(t, np.eye(4))                          # two correspondences: no triple to draw


def test_edge_length_checker_zeroes_exactly_the_violating_triples():
    from sgaligner_amd.utils import registration as RG
    rng = np.random.default_rng(12)
    t = FR.rigid(13)
    src = rng.uniform(-1.0, 1.0, (60, 3))
    ref = src @ t[:3, :3].T + t[:3, 3]
    ref[50:] = 3.0 * ref[50:]                                    # rows 50..59: every edge among them is three times as long on the reference side
    corr = np.concatenate([src, ref], axis=1)
    good = np.stack([rng.permutation(50)[:3] for _ in range(40)])                       # rigid rows only: every edge keeps its length
    bad = np.stack([50 + rng.permutation(10)[:3] for _ in range(30)])                   # stretched rows only: every edge violates
    mixed = np.stack([rng.permutation(60)[:3] for _ in range(58)])
    samples = np.concatenate([good, bad, mixed]).astype(np.int32)
    ok = FR.edge_length_ok(corr, samples)
    assert ok[:40].all() and not ok[40:70].any() and ok[70:].any() and not ok[70:].all()
    # two jobs over the same rows, the second with the list reversed: the filter works on job-local indices
    corr2, off, hoff = np.concatenate([corr, corr]), [0, 60, 120], [0, 128, 256]
    both, ok2 = np.concatenate([samples, samples[::-1]]), np.concatenate([ok, ok[::-1]])
    d_corr, d_samples = torch.from_numpy(corr2).cuda(), torch.from_numpy(both).cuda()
    checked = RG.edge_length_filter(d_corr, off, d_samples, hoff)
    assert checked.dtype == torch.int32 and np.array_equal(checked.cpu().numpy()[ok2], both[ok2])
    assert np.array_equal(d_samples.cpu().numpy(), both)                                # the caller's list is left alone
    got = RG.score_hypotheses_batch(d_corr, off, checked, hoff, 0.05).cpu().numpy()
    plain = RG.score_hypotheses_batch(d_corr, off, d_samples, hoff, 0.05).cpu().numpy()
    assert (got[~ok2] == 0).all() and np.array_equal(got[ok2], plain[ok2])
    assert (plain[:40] >= 50).all()                                                     # a rigid triple brings all 50 rigid rows in


def _eval_scene(seed):
    """A pair with gt_transform = identity, as the reference's testers set it: the reference cloud is the source cloud in another order.
    Four objects; coordinates are multiples of 2^-10, exact in float32 (the descriptor is the point itself)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(-4096, 4096, (460, 3)) / 1024.0
    ids = np.repeat([1, 2, 3, 4], [100, 150, 30, 180])           # object 3 is below min_object_points
    order = rng.permutation(460)
    return {'src_points': src, 'ref_points': src[order], 'node_corrs': [(1, 11), (2, 12), (3, 13), (4, 14)],
            'src_plydata': {'objectId': ids}, 'ref_plydata': {'objectId': ids[order] + 10}, 'gt_transform': np.eye(4),
            'raw_points': src[order], 'gt_src_corr_points': src[::4], 'gt_ref_corr_points': src[::4]}


def test_evaluator_with_the_feature_matcher():
    from sgaligner_amd.registration_evaluator import FeatureMatcher, RegistrationEvaluator
    fm = FeatureMatcher(lambda p: p.astype(np.float32))
    d = _eval_scene(5)
    ev = RegistrationEvaluator(fm, ransac_iters=512, seed=2)
    plain = RegistrationEvaluator(lambda s, r, g: fm(s, r, g), ransac_iters=512, seed=2)      # no match_many: one call per node pair
    rows = ev.collect_correspondences(d)
    assert rows.shape == (100 + 150 + 180, 6) and np.array_equal(rows, plain.collect_correspondences(d))
    assert np.array_equal(rows[:, :3], rows[:, 3:])                                      # every point found its own copy
    one = fm(d['src_points'][:100], d['ref_points'], np.eye(4))
    assert set(one) == {'src_corr_points', 'ref_corr_points', 'corr_scores'} and (one['corr_scores'] == 1.0).all()
    normal, aligner = ev.run_registration(d)
    for res in (normal, aligner):
        assert set(res) == set(RegistrationEvaluator.RESULT_KEYS)
        assert res['RRE'] < 1e-6 and res['RTE'] < 1e-9 and res['IR'] == 1.0 and res['recall'] == 1.0 and res['FMR'] == 1.0
    est, score = ev.run_normal_registration(d, evaluate_registration=False)
    assert est.shape == (4, 4) and np.abs(est - np.eye(4)).max() < 1e-9 and score == 1.0
    big = dict(d, src_points=np.tile(d['src_points'], (30, 1)))                          # 13 800 rows: subsampled to 10 000, seeded
    a, b = ev.run_normal_registration(big, evaluate_registration=False), ev.run_normal_registration(big, evaluate_registration=False)
    assert np.array_equal(a[0], b[0]) and np.abs(a[0] - np.eye(4)).max() < 1e-9
