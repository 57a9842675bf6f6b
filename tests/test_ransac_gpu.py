"""GPU tier of the batched RANSAC rigid registration (csrc/ransac.hip) against the numpy yardstick (tests/ransac_ref.py).

One tolerance, derived and not tuned: a device transform that moves every source point to within 1e-7 x threshold (3e-9 m) of where the
yardstick's transform moves it cannot change any count outside the yardstick's `near` set.  So moved points are compared with that
tolerance, and counts, best index, status and masks EXACTLY, on the hypotheses that are neither `near` nor `ill` (at most 2 % of a case's;
tests/test_ransac_cpu.py checks the same preconditions without a device).

Measured on an MI355X over the 4 families x 30 (n, H) cases x 3 chunkings: no count mismatch among the compared hypotheses, at most 2 of 512
hypotheses left out (ill), moved points within 6.4e-15 m of the yardstick's on clean / loose / exact and 9.1e-13 m on far (coordinates of
order 1e3 m), against the 3e-9 m allowed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ransac_ref as RR  # noqa: E402
from sgaligner_amd.utils.registration import find_rigid_transform_batch, score_hypotheses_batch  # noqa: E402,F401  (the feature under test)

pytestmark = pytest.mark.gpu

THRESHOLD = 0.03
TOL = RR.NEAR_REL * THRESHOLD
GRID_N = (3, 4, 64, 257, 515, 1000)
GRID_H = (1, 63, 65, 257, 512)
OUTPUTS = ('transform', 'inlier_count', 'best_hyp', 'status', 'inlier_mask', 'hyp_count')


def _run(corrs, samples, hoff, threshold=THRESHOLD, rounds=2, chunk=None):
    """list of [n, 6] arrays + packed samples -> dict of numpy outputs."""
    from sgaligner_amd.utils import registration as RG
    off = np.concatenate([[0], np.cumsum([len(c) for c in corrs])]).astype(np.int64)
    packed = np.concatenate(corrs) if len(corrs) else np.zeros((0, 6))
    res = RG.find_rigid_transform_batch(torch.from_numpy(np.ascontiguousarray(packed)).cuda(), off,
                                        torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int32)).cuda(), hoff, threshold, rounds, chunk=chunk)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    assert out['transform'].dtype == np.float64 and out['inlier_mask'].dtype == np.uint8
    assert all(out[k].dtype == np.int32 for k in ('inlier_count', 'best_hyp', 'status', 'hyp_count'))
    out['offsets'], out['hyp_offsets'] = off, np.asarray(hoff, dtype=np.int64)
    return out


def _job(out, j):
    o, h = out['offsets'], out['hyp_offsets']
    return {'transform': out['transform'][j], 'inlier_count': out['inlier_count'][j], 'best_hyp': out['best_hyp'][j],
            'status': out['status'][j], 'inlier_mask': out['inlier_mask'][o[j]:o[j + 1]], 'hyp_count': out['hyp_count'][h[j]:h[j + 1]]}


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in OUTPUTS)


def _moved(corr, T):
    return corr[:, :3] @ T[:3, :3].T + T[:3, 3]


def _compare(tag, got, ref, corr):
    """One job of a device result against the yardstick, by the rules in the module docstring."""
    compared, bad = RR.preconditions(ref)
    assert not bad, (tag, bad)                                           # a precondition, never a skip
    diff = got['hyp_count'] != ref['hyp_count']
    dist = float(np.abs(_moved(corr, got['transform']) - _moved(corr, ref['transform'])).max()) if len(corr) else 0.0
    print(tag, 'hypotheses left out', int((~compared).sum()), 'of', len(compared), 'count mismatches among the compared', int(diff[compared].sum()),
          'best', int(got['best_hyp']), int(ref['best']), 'inliers', int(got['inlier_count']), int(ref['count']), 'moved points differ by', dist)
    assert np.isfinite(got['transform']).all(), tag
    assert np.array_equal(got['hyp_count'][compared], ref['hyp_count'][compared]), tag
    assert (got['hyp_count'][~ref['valid']] == 0).all(), tag
    assert int(got['status']) == ref['status'], tag
    assert int(got['best_hyp']) == ref['best'], tag
    assert dist <= TOL, (tag, dist)
    assert int(got['inlier_count']) == ref['count'] == int(got['inlier_mask'].sum()), tag
    assert np.array_equal(got['inlier_mask'], ref['mask']), tag
    assert np.array_equal(got['transform'][3], [0.0, 0.0, 0.0, 1.0]), tag
    if ref['status'] == 1:
        assert np.array_equal(got['transform'], np.eye(4)) and int(got['inlier_count']) == 0 and not got['inlier_mask'].any(), tag


@functools.lru_cache(maxsize=None)
def _grid(family):
    """The (n, H) grid of one family as a job list: (corrs, samples, hyp_offsets, yardstick results), computed once and never changed."""
    corrs, parts, hoff, refs = [], [], [0], []
    for n in GRID_N:
        corr, _, _ = RR.make_case(family, n, 1)
        for H in GRID_H:
            s, _ = RR.draw_samples([n], H, 101)
            corrs.append(corr)
            parts.append(s)
            hoff.append(hoff[-1] + len(s))
            refs.append(RR.ransac_ref(corr, s, THRESHOLD, 2))
    return corrs, np.concatenate(parts), np.asarray(hoff, dtype=np.int64), refs


# chunk None: the package's own rule (128 rows here: up to eight chunks); 192: n = 515 in three chunks (192, 192, 131) and n = 1000 in six
# (5 x 192 + 40), each with a ragged last one; 4096: everything in one chunk.
@pytest.mark.parametrize('chunk', (None, 192, 4096))
@pytest.mark.parametrize('family', RR.FAMILIES)
def test_every_output_equals_the_yardstick(family, chunk):
    from sgaligner_amd import _lib
    corrs, samples, hoff, refs = _grid(family)
    if chunk == 192:
        one = _lib.lib().sga_ransac_workspace_bytes(1, 512, 1000, 4096)
        assert _lib.lib().sga_ransac_workspace_bytes(1, 512, 1000, 192) == one + 5 * 512 * 4          # really six chunks
        assert _lib.lib().sga_ransac_workspace_bytes(1, 512, 515, 192) == \
            _lib.lib().sga_ransac_workspace_bytes(1, 512, 515, 4096) + 2 * 512 * 4                    # really three
    out = _run(corrs, samples, hoff, chunk=chunk)
    k = 0
    for n in GRID_N:
        for H in GRID_H:
            _compare(f'{family} n={n} H={H} chunk={chunk}', _job(out, k), refs[k], corrs[k])
            k += 1


def test_the_module_level_chunk_override_is_honoured():
    from sgaligner_amd.utils import registration as RG
    corrs, samples, hoff, refs = _grid('loose')
    base = _run(corrs, samples, hoff)
    assert RG.RANSAC_CHUNK is None
    RG.RANSAC_CHUNK = 192
    try:
        forced = _run(corrs, samples, hoff)
    finally:
        RG.RANSAC_CHUNK = None
    assert _same_bits(forced, _run(corrs, samples, hoff, chunk=192))
    assert _same_bits(forced, base)                     # integer folds: the chunking cannot show in any output


def test_a_mixed_job_list_equals_its_single_jobs_bit_for_bit():
    sizes, hyps = (0, 2, 3, 64, 1000, 257), (0, 0, 1, 65, 512, 257)
    corrs, parts, hoff = [], [], [0]
    for j, (n, H) in enumerate(zip(sizes, hyps)):
        corrs.append(RR.make_case('loose', n, 20 + j)[0])
        s = RR.draw_samples([n], H, 120 + j)[0] if H else np.zeros((0, 3), dtype=np.int32)
        parts.append(s)
        hoff.append(hoff[-1] + len(s))
    samples = np.concatenate(parts)
    out = _run(corrs, samples, hoff)
    assert out['status'][:2].tolist() == [1, 1] and out['best_hyp'][:2].tolist() == [-1, -1] and out['inlier_count'][:2].tolist() == [0, 0]
    assert np.array_equal(out['transform'][0], np.eye(4)) and np.array_equal(out['transform'][1], np.eye(4))
    assert not out['inlier_mask'][:2].any()
    for j in range(len(sizes)):
        single = _run([corrs[j]], parts[j], [0, len(parts[j])])
        assert _same_bits(_job(out, j), _job(single, 0)), j
        if sizes[j] >= 3:
            _compare(f'mixed job {j}', _job(out, j), RR.ransac_ref(corrs[j], parts[j], THRESHOLD, 2), corrs[j])
    assert out['status'][3:].tolist() == [0, 0, 0]


def test_invalid_and_degenerate_samples():
    corr, _, planted = RR.make_case('clean', 64, 1)
    corr = corr.copy()
    corr[10:13, :3] = corr[10, :3] + np.outer([0.0, 1.0, 2.0], [0.1, 0.2, -0.1])          # rows 10-12: collinear in the source ...
    corr[10:13, 3:] = corr[10, 3:] + np.outer([0.0, 1.0, 2.0], [0.2, -0.1, 0.1])          # ... and in the reference
    corr[20:23] = corr[20]                                                                  # rows 20-22: one point three times
    good = np.flatnonzero(planted & ~np.isin(np.arange(64), [10, 11, 12, 20, 21, 22]))[:3]
    samples = np.array([[5, 5, 6], [5, 6, 5], [7, 7, 7], [0, 1, 64], [-1, 2, 3], [2 ** 31 - 1, 0, 1], [10, 11, 12], [20, 21, 22],
                        list(good)], dtype=np.int32)
    out = _run([corr], samples, [0, len(samples)])
    got = _job(out, 0)
    ref = RR.ransac_ref(corr, samples, THRESHOLD, 2)
    print('hyp_count', got['hyp_count'].tolist(), 'yardstick', ref['hyp_count'].tolist(), 'best', int(got['best_hyp']))
    assert (got['hyp_count'][:6] == 0).all()                             # repeated / out-of-range indices: never a model
    assert np.isfinite(got['transform']).all() and (got['hyp_count'] >= 0).all() and (got['hyp_count'] <= 64).all()
    assert int(got['status']) == 0 and int(got['best_hyp']) == 8 == ref['best']
    assert int(got['hyp_count'][8]) == int(ref['hyp_count'][8])
    assert int(got['inlier_count']) == ref['count'] and np.array_equal(got['inlier_mask'], ref['mask'])
    # nothing but invalid and degenerate samples: still a normal return, either no model or a finite one
    out = _run([corr], samples[:8], [0, 8])
    got = _job(out, 0)
    assert np.isfinite(got['transform']).all() and int(got['status']) in (0, 1)
    if int(got['status']) == 1:
        assert np.array_equal(got['transform'], np.eye(4)) and int(got['inlier_count']) == 0 and not got['inlier_mask'].any()
    else:
        assert int(got['best_hyp']) in (6, 7) and int(got['inlier_count']) == int(got['inlier_mask'].sum()) >= 3
    # only invalid ones: no model
    out = _run([corr], samples[:6], [0, 6])
    assert int(out['status'][0]) == 1 and int(out['best_hyp'][0]) == -1 and np.array_equal(out['transform'][0], np.eye(4))
    assert not out['hyp_count'].any() and not out['inlier_mask'].any()


def test_ties_go_to_the_lowest_index():
    corr, _, planted = RR.make_case('clean', 257, 1)
    inl, outl = np.flatnonzero(planted), np.flatnonzero(~planted)
    rng = np.random.default_rng(4)
    samples = np.array([[rng.choice(inl), *rng.choice(outl, 2, replace=False)] for _ in range(64)], dtype=np.int32)      # one inlier, two outliers
    samples[5] = samples[40] = inl[[0, 7, 19]]
    ref = RR.ransac_ref(corr, samples, THRESHOLD, 2)
    others = np.delete(ref['hyp_count'], [5, 40])
    assert ref['hyp_count'][5] == ref['hyp_count'][40] > others.max() and ref['best'] == 5          # the case is what it claims to be
    got = _job(_run([corr], samples, [0, 64]), 0)
    assert int(got['hyp_count'][5]) == int(got['hyp_count'][40]) == int(ref['hyp_count'][5])
    assert int(got['best_hyp']) == 5
    _compare('ties', got, ref, corr)


def test_all_outliers():
    rng = np.random.default_rng(9)
    corr = rng.uniform(0.0, 2.0, (257, 6))
    samples, hoff = RR.draw_samples([257], 257, 109)
    ref = RR.ransac_ref(corr, samples, THRESHOLD, 2)
    got = _job(_run([corr], samples, hoff), 0)
    print('all outliers: status', int(got['status']), ref['status'], 'count', int(got['inlier_count']), ref['count'],
          'largest hypothesis count', int(got['hyp_count'].max()))
    assert int(got['status']) == 1 or int(got['inlier_count']) == ref['count']
    assert np.isfinite(got['transform']).all()
    _compare('all outliers', got, ref, corr)


def test_two_calls_give_the_same_bits():
    corr, _, _ = RR.make_case('loose', 1000, 3)
    samples, hoff = RR.draw_samples([1000], 512, 103)
    for chunk in (None, 192):
        a, b = _run([corr], samples, hoff, chunk=chunk), _run([corr], samples, hoff, chunk=chunk)
        assert _same_bits(a, b), chunk
        assert int(a['status'][0]) == 0 and int(a['inlier_count'][0]) > 300


def test_scoring_alone_gives_the_same_counts():
    from sgaligner_amd.utils import registration as RG
    corrs, samples, hoff, refs = _grid('clean')
    full = _run(corrs, samples, hoff)
    off = np.concatenate([[0], np.cumsum([len(c) for c in corrs])])
    counts = RG.score_hypotheses_batch(torch.from_numpy(np.concatenate(corrs)).cuda(), off, torch.from_numpy(samples).cuda(), hoff, THRESHOLD)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), full['hyp_count'])


def test_find_rigid_transform_shifts_and_composes():
    from sgaligner_amd.utils import registration as RG
    corr, planted_T, _ = RR.make_case('far', 1000, 2)
    shift = corr.min(0)
    samples, _ = RR.draw_samples([1000], 512, 7)
    ref = RR.ransac_ref(corr - shift, samples, THRESHOLD, 2)
    _, bad = RR.preconditions(ref)
    assert not bad and ref['status'] == 0, bad
    want = RR.compose_shift(ref['transform'], shift)
    T, info = RG.find_rigid_transform(corr, threshold=THRESHOLD, iters=512, seed=7)
    dist = float(np.abs(_moved(corr, T) - _moved(corr, want)).max())
    print('far, unshifted at the Python layer: moved points differ by', dist, 'inliers', info['inlier_count'], ref['count'])
    assert dist <= TOL
    assert info['inlier_count'] == ref['count'] and info['best_hyp'] == ref['best'] and info['status'] == 0
    assert np.array_equal(info['inlier_mask'], ref['mask'].astype(bool)) and np.array_equal(info['shift'], shift)
    rre, rte = RG.compute_registration_error(planted_T, T)
    assert rre < 0.11                                                     # the planted rotation, by the bound of the CPU tier
    # the open3d-style entry point: correspondences=None pairs row i with row i
    src, dst = corr[:, :3], corr[:, 3:]
    t_none = RG.registration_with_ransac_from_correspondences(src, dst, None, distance_threshold=0.05, ransac_n=3, num_iterations=512)
    ident = np.stack([np.arange(1000), np.arange(1000)], axis=1)
    t_ident = RG.registration_with_ransac_from_correspondences(src, dst, ident, distance_threshold=0.05, ransac_n=3, num_iterations=512)
    assert np.array_equal(t_none, t_ident)
    perm = np.random.default_rng(0).permutation(1000)                     # a real index pairing: the reference shuffled
    t_perm = RG.registration_with_ransac_from_correspondences(src, dst[perm], np.stack([np.arange(1000), np.argsort(perm)], axis=1),
                                                              distance_threshold=0.05, num_iterations=512)
    assert np.array_equal(t_perm, t_none)
    assert np.array_equal(t_none, RG.find_rigid_transform(corr, threshold=0.05, iters=512)[0])


# ---- RegistrationEvaluator with a synthetic matcher ------------------------------------------------------------------------------
OBJECTS = ((1, 200), (2, 300), (3, 30), (4, 120), (5, 400))          # (id, points): 3 is below min_object_points, 4 gets no match,
BUDGET = 1000 // len(OBJECTS)                                         # 2 and 5 are above the per-node cut of 200


def _matcher(src, ref, gt_transform):
    """Planted correspondences: row i with row i, a third of the reference rows swapped among themselves; scores distinct by construction."""
    if len(src) == 120:
        return None
    k = len(src)
    ref_c = ref.copy()
    wrong = np.arange(0, k, 3)
    ref_c[wrong] = ref[np.roll(wrong, 1)]
    scores = ((np.arange(k) * 0.6180339887498949) % 1.0)
    return {'src_corr_points': src, 'ref_corr_points': ref_c, 'corr_scores': scores}


def _scene(seed, objects=OBJECTS):
    rng = np.random.default_rng(seed)
    gt = RR.random_transform(rng)
    ids = np.concatenate([np.full(n, i) for i, n in objects])
    centres = {i: rng.uniform(0.0, 2.0, 3) for i, _ in objects}
    src = np.concatenate([centres[i] + rng.uniform(-0.3, 0.3, (n, 3)) for i, n in objects])
    ref = src @ gt[:3, :3].T + gt[:3, 3] + rng.uniform(-1.0, 1.0, src.shape) * 0.004
    return {'node_corrs': [(i, i + 10) for i, _ in objects], 'src_points': src, 'ref_points': ref,
            'src_plydata': {'objectId': ids}, 'ref_plydata': {'objectId': ids + 10}, 'gt_transform': gt,
            'raw_points': np.concatenate([ref, rng.uniform(-1.0, 3.0, (200, 3))]),
            'gt_src_corr_points': src[::5], 'gt_ref_corr_points': (src @ gt[:3, :3].T + gt[:3, 3])[::5]}


def _restated_rows(d):
    """What the evaluator must hand to RANSAC, written out again in numpy."""
    src_rows, ref_rows = [], []
    for i, n in OBJECTS:
        s = d['src_points'][d['src_plydata']['objectId'] == i]
        r = d['ref_points'][d['ref_plydata']['objectId'] == i + 10]
        if n < 50 or n == 120:
            continue
        m = _matcher(s, r, d['gt_transform'])
        sc, rc, score = m['src_corr_points'], m['ref_corr_points'], m['corr_scores']
        if n > BUDGET:
            top = np.argsort(-score)[:BUDGET]
            sc, rc = sc[top], rc[top]
        src_rows.append(sc)
        ref_rows.append(rc)
    return np.concatenate([np.concatenate(src_rows), np.concatenate(ref_rows)], axis=1)


def test_registration_evaluator_with_a_synthetic_matcher():
    from sgaligner_amd.registration_evaluator import RegistrationEvaluator
    from sgaligner_amd.utils import registration as RG
    ev = RegistrationEvaluator(_matcher, num_p2p_corrs=1000, ransac_threshold=THRESHOLD, ransac_iters=512, seed=3)
    d = _scene(31)
    rows = _restated_rows(d)
    assert rows.shape == (200 + 200 + 200, 6)                          # object 1 whole, 2 and 5 cut to the budget, 3 and 4 absent
    assert np.array_equal(ev.collect_correspondences(d), rows)
    shift = rows.min(0)
    samples, _ = RR.draw_samples([len(rows)], 512, 3)
    ref = RR.ransac_ref(rows - shift, samples, THRESHOLD, 2)
    _, bad = RR.preconditions(ref)
    assert not bad and ref['status'] == 0, bad
    want_T = RR.compose_shift(ref['transform'], shift)
    T = ev.run_aligner_registration(d, evaluate_registration=False)
    dist = float(np.abs(_moved(d['src_points'], T) - _moved(d['src_points'], want_T)).max())
    print('evaluator: moved points differ by', dist)
    assert dist <= TOL
    want = dict(zip(('CD', 'IR', 'RRE', 'RTE', 'recall', 'FMR'),
                    ev.evaluate_registration(d['src_points'], d['ref_points'], d['raw_points'], want_T, d['gt_transform'], rows[:, :3],
                                             rows[:, 3:], d['gt_src_corr_points'], d['gt_ref_corr_points'])))
    ir = RG.compute_inlier_ratio(rows[:, 3:], rows[:, :3], d['gt_transform'])
    assert want['IR'] == ir and want['FMR'] == float(ir >= 0.05) and want['recall'] in (0.0, 1.0)
    got = ev.run_aligner_registration(d)
    print('evaluator result', got, 'restated', want)
    assert tuple(got) == ('CD', 'IR', 'RRE', 'RTE', 'recall', 'FMR')
    assert got['IR'] == want['IR'] and got['FMR'] == want['FMR'] and got['recall'] == want['recall'] == 1.0
    for key in ('CD', 'RRE', 'RTE'):                                   # these move with the transform: the 3e-9 rule
        assert abs(got[key] - want[key]) <= TOL, (key, got[key], want[key])
    assert got['RRE'] < 0.2 and got['RTE'] < 0.01 and 0.6 < got['IR'] < 0.75
    # pairs without any usable object: None, alone and inside a batch; the batch equals the per-pair calls exactly
    empty = _scene(32, objects=((3, 30), (4, 120)))
    assert ev.run_aligner_registration(empty) is None
    scenes = [d, empty, _scene(33), _scene(34)]
    batch = ev.run_aligner_registration_batch(scenes)
    assert batch[1] is None and batch == [ev.run_aligner_registration(s) for s in scenes]
    t_batch = ev.run_aligner_registration_batch(scenes, evaluate_registration=False)
    assert t_batch[1] is None and all(np.array_equal(a, ev.run_aligner_registration(s, evaluate_registration=False))
                                      for a, s in zip(t_batch, scenes) if a is not None)
