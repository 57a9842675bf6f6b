"""CPU tier of the batched RANSAC rigid registration (csrc/ransac.hip, utils/registration.py, registration_evaluator.py): the numpy
yardstick recovers planted transforms, the sample rule is what it says, the C ABI is complete and refuses bad arguments without a device,
nothing falls back to the host, the kernels do not spill, and the shift composition gives a hand-computed transform."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import ransac_ref as RR  # noqa: E402
from sgaligner_amd.utils.registration import draw_samples, find_rigid_transform_batch  # noqa: E402,F401  (the feature under test)

THRESHOLD = 0.03
GRID_N = (3, 4, 64, 257, 515, 1000)
GRID_H = (1, 63, 65, 257, 512)


@pytest.mark.parametrize('family', RR.FAMILIES)
def test_yardstick_recovers_the_planted_transform(family):
    """n = 1000 rows (400 planted inliers), 512 hypotheses, seeds 1-3, two refinement rounds; RRE / RTE by the package's own
    compute_registration_error.

    Bound, from the data and not from the result: the final fit is a least-squares fit over m ~ 400 inliers whose noise is uniform
    +-noise per axis (sigma = noise / sqrt(3)).  Points uniform in a 2 m box have variance 1/3 per axis, so a rotation about any axis
    sees a squared lever arm of 2/3 per point: sigma_rot = sigma / sqrt(2 m / 3) per axis; the translation of the centroid has
    sigma / sqrt(m) per axis.  Six sigma of the three-axis norm bounds RRE; RTE is read at the ORIGIN, so it adds the rotation error
    times the distance of the inliers' centroid from it (about 1.7 m, and order 1e3 m for `far`, which is why `far` exists).  `exact` has
    no noise: there the bound is the resolution of acos near 1 (sqrt(2 eps) rad, taken as 1e-5 degrees) and rounding at the coordinates'
    magnitude.

    Measured (max over the three seeds; bounds 0.105 deg clean / far, 0.42 deg loose): clean 0.0205 deg / 0.52 mm, loose 0.0865 deg /
    2.3 mm, exact 2.4e-6 deg / 1.2e-15 m, far 0.0205 deg / 0.50 m (clean's rotation error, read about 1.5 km from the centroid)."""
    from sgaligner_amd.utils.registration import compute_registration_error
    worst = [0.0, 0.0]
    for seed in (1, 2, 3):
        corr, planted_T, planted = RR.make_case(family, 1000, seed)
        samples, _ = draw_samples([1000], 512, seed + 100)
        ref = RR.ransac_ref(corr, samples, THRESHOLD, 2)
        assert ref['status'] == 0
        rre, rte = compute_registration_error(planted_T, ref['transform'])
        m = int(planted.sum())
        sigma = RR.NOISE[family] / np.sqrt(3.0)
        rot_bound = 6.0 * np.sqrt(3.0) * sigma / np.sqrt(2.0 * m / 3.0) + np.radians(1e-5)
        lever = float(np.linalg.norm(corr[planted, :3].mean(0)))
        rte_bound = 6.0 * np.sqrt(3.0) * sigma / np.sqrt(m) + rot_bound * lever + 1e-12 * (1.0 + lever)
        print(family, seed, 'RRE deg', rre, 'bound', np.degrees(rot_bound), 'RTE m', rte, 'bound', rte_bound, 'count', ref['count'], 'of', m)
        assert np.radians(rre) <= rot_bound and rte <= rte_bound, (family, seed, rre, rte)
        if family != 'loose':
            assert ref['count'] >= m - 2                  # noise well inside the threshold: the planted set is found
        else:
            assert ref['count'] > ref['first_count']      # the family exists for its refinement
        worst = [max(worst[0], rre), max(worst[1], rte)]
    print(family, 'worst RRE deg', worst[0], 'worst RTE m', worst[1])


@pytest.mark.parametrize('family', RR.FAMILIES)
def test_comparison_cases_meet_their_preconditions(family):
    """The grid the GPU tier compares exactly (seed 1, sample seed 101): at most 2 % of a case's hypotheses are near or ill, no final
    transform is near, and the grid exercises what it is meant to: ties at the maximum, refinement that gains inliers, status 1."""
    ties = gained = no_model = 0
    for n in GRID_N:
        corr, _, _ = RR.make_case(family, n, 1)
        for H in GRID_H:
            samples, _ = draw_samples([n], H, 101)
            ref = RR.ransac_ref(corr, samples, THRESHOLD, 2)
            _, bad = RR.preconditions(ref)
            assert not bad, (family, n, H, bad)
            ties += int((ref['hyp_count'] == ref['hyp_count'].max()).sum() > 1 and ref['status'] == 0)
            gained += int(ref['count'] > ref['first_count'])
            no_model += int(ref['status'] == 1)
    print(family, 'cases with ties', ties, 'with gain in refinement', gained, 'without a model', no_model)
    assert ties >= 5
    if family == 'loose':
        assert gained >= 5


def test_draw_samples():
    sizes = [0, 2, 3, 4, 64, 1000]
    s, off = draw_samples(sizes, 200, 5)
    assert s.dtype == np.int32 and s.shape == (800, 3) and off.tolist() == [0, 0, 0, 200, 400, 600, 800]
    for j, n in enumerate(sizes):
        t = s[off[j]:off[j + 1]]
        assert ((t >= 0) & (t < max(n, 1))).all()
        assert ((t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])).all()
    assert len(np.unique(s[off[5]:off[6]], axis=0)) > 190                    # really random
    assert len(np.unique(np.sort(s[off[3]:off[4]], axis=1), axis=0)) == 4     # n = 4: all four triangles turn up
    s2, off2 = draw_samples(sizes, 200, 5)
    assert np.array_equal(s, s2) and np.array_equal(off, off2)
    assert not np.array_equal(draw_samples(sizes, 200, 6)[0], s)
    one, _ = draw_samples([1000], 200, 5)                                    # a job's samples do not depend on its neighbours
    assert np.array_equal(one, s[off[5]:off[6]])
    rs, roff = RR.draw_samples(sizes, 200, 5)                                # the yardstick's restatement of the rule
    assert np.array_equal(rs, s) and np.array_equal(roff, off)
    assert draw_samples([2, 1], 10, 0)[0].shape == (0, 3)


def test_abi_has_the_entry_points_and_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    for name in ('sga_ransac_rigid', 'sga_ransac_workspace_bytes'):
        assert name + '(' in hdr and name in _lib.SIGNATURES
    l = _lib.lib()
    need = l.sga_ransac_workspace_bytes(1, 8, 16, 128)
    assert need > 0 and need % 8 == 0
    assert l.sga_ransac_workspace_bytes(1, 8, 16, 4) == need + 3 * 8 * 4          # four chunks of counts instead of one
    assert l.sga_ransac_workspace_bytes(0, 8, 16, 128) == 0

    buf = np.zeros(64, dtype=np.float64)                  # host memory: never dereferenced, every call must stop before a launch
    p = buf.ctypes.data
    off = np.array([0, 16], dtype=np.int32)
    hoff = np.array([0, 8], dtype=np.int32)

    def call(corr=p, offsets=p, n_jobs=1, total_rows=16, samples=p, hyp_offsets=p, total_hyp=8, max_rows=16, max_hyp=8, chunk=128,
             offsets_host=off.ctypes.data, hyp_offsets_host=hoff.ctypes.data, threshold=0.03, rounds=2, transform=p, count=p, best=p,
             status=p, mask=p, hyp_count=p, ws=p, ws_bytes=need):
        rc = l.sga_ransac_rigid(corr, offsets, n_jobs, total_rows, samples, hyp_offsets, total_hyp, max_rows, max_hyp, chunk, offsets_host,
                                hyp_offsets_host, threshold, rounds, transform, count, best, status, mask, hyp_count, ws, ws_bytes, None)
        return rc, l.sga_last_error()

    for null in ('corr', 'offsets', 'samples', 'hyp_offsets', 'transform', 'count', 'best', 'status', 'mask', 'hyp_count'):
        rc, msg = call(**{null: None})
        assert rc != 0 and b'null pointer' in msg, (null, msg)
    for odd in ('corr', 'transform'):
        rc, msg = call(**{odd: p + 4})
        assert rc != 0 and b'misaligned' in msg, (odd, msg)
    for odd in ('offsets', 'samples', 'hyp_offsets', 'count', 'best', 'status', 'hyp_count'):
        rc, msg = call(**{odd: p + 2})
        assert rc != 0 and b'misaligned' in msg, (odd, msg)
    rc, msg = call(ws=p + 4)
    assert rc != 0 and b'misaligned' in msg
    for neg in ('n_jobs', 'total_rows', 'total_hyp', 'max_rows', 'max_hyp'):
        rc, msg = call(**{neg: -1})
        assert rc != 0 and b'negative count' in msg, (neg, msg)
    rc, msg = call(chunk=0)
    assert rc != 0 and b'chunk' in msg
    rc, msg = call(rounds=-2)
    assert rc != 0 and b'refine_rounds' in msg
    rc, msg = call(threshold=float('nan'))
    assert rc != 0 and b'threshold' in msg
    off3 = np.array([0, 12, 8, 16], dtype=np.int32)
    hoff3 = np.array([0, 4, 4, 8], dtype=np.int32)
    need3 = l.sga_ransac_workspace_bytes(3, 8, 16, 128)
    wide_buf = np.zeros(need3 // 8 + 1, dtype=np.float64)
    wide = wide_buf.ctypes.data
    rc, msg = call(n_jobs=3, offsets_host=off3.ctypes.data, hyp_offsets_host=hoff3.ctypes.data, ws=wide, ws_bytes=need3)
    assert rc != 0 and b'offsets decrease at job 1' in msg, msg
    off3 = np.array([0, 4, 8, 16], dtype=np.int32)
    hoff3 = np.array([0, 6, 4, 8], dtype=np.int32)
    rc, msg = call(n_jobs=3, offsets_host=off3.ctypes.data, hyp_offsets_host=hoff3.ctypes.data, ws=wide, ws_bytes=need3)
    assert rc != 0 and b'hyp_offsets decrease at job 1' in msg, msg
    short = np.array([0, 15], dtype=np.int32)
    rc, msg = call(offsets_host=short.ctypes.data)
    assert rc != 0 and b'offsets must run from 0 to total_rows' in msg
    rc, msg = call(ws=None, ws_bytes=0)
    assert rc != 0 and b'workspace' in msg
    rc, msg = call(ws_bytes=need - 8)
    assert rc != 0 and b'workspace' in msg
    assert call(n_jobs=0, offsets_host=None, hyp_offsets_host=None)[0] == 0          # nothing to do is not an error


def test_no_silent_fallback():
    from sgaligner_amd.registration_evaluator import RegistrationEvaluator
    from sgaligner_amd.utils import registration as RG
    corr = np.zeros((8, 6))
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        RG.find_rigid_transform_batch(torch.zeros((8, 6), dtype=torch.float64), [0, 8], torch.zeros((2, 3), dtype=torch.int32), [0, 2], 0.03)
    with pytest.raises(ValueError, match='ransac_n'):
        RG.registration_with_ransac_from_correspondences(corr[:, :3], corr[:, 3:], ransac_n=4)
    if torch.cuda.is_available():
        return                                             # the rest is about machines without a device
    ev = RegistrationEvaluator(lambda s, r, t: {'src_corr_points': s[:60], 'ref_corr_points': r[:60], 'corr_scores': np.ones(60)})
    data = {'node_corrs': [(1, 1)], 'src_points': np.zeros((60, 3)), 'ref_points': np.zeros((60, 3)),
            'src_plydata': {'objectId': np.ones(60, dtype=int)}, 'ref_plydata': {'objectId': np.ones(60, dtype=int)}, 'gt_transform': np.eye(4)}
    for fn in (lambda: RG.find_rigid_transform(corr), lambda: RG.find_rigid_transform_pairs([corr, corr]),
               lambda: RG.registration_with_ransac_from_correspondences(corr[:, :3], corr[:, 3:]),
               lambda: ev.run_aligner_registration(data), lambda: ev.run_aligner_registration_batch([data])):
        with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
            fn()


def test_ransac_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    _, res = kr.analyse(os.path.join(_build.CSRC, 'ransac.hip'))
    kernels = ('ransac_hyp_kernel', 'ransac_score_kernel', 'ransac_fold_kernel', 'ransac_select_kernel', 'ransac_accum_kernel',
               'ransac_step_kernel', 'ransac_mask_kernel')
    for tag in kernels:
        ks = [k for k in res if tag in k]
        assert ks, (tag, sorted(res))
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
            assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
    assert len(res) == len(kernels), sorted(res)           # every kernel of the file is named above


def test_shift_is_composed_back_into_the_transform(monkeypatch):
    """Four exact pairs: ref = Rz(90 deg) src + (5, -7, 100), the source near (10, 20, 30).  By hand: the column minima are
    a = (10, 20, 30) and b = (-17, 3, 130), so the estimator sees rows whose transform is [Rz | Rz a + t - b] = [Rz | (2, 0, 0)], and the
    function must hand back [Rz | (5, -7, 100)].  The device call is replaced by the yardstick."""
    from sgaligner_amd.utils import registration as RG
    rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([5.0, -7.0, 100.0])
    src = np.array([10.0, 20.0, 30.0]) + np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]])
    corr = np.concatenate([src, src @ rz.T + t], axis=1)
    assert np.array_equal(corr.min(0), [10.0, 20.0, 30.0, -17.0, 3.0, 130.0])
    seen = {}

    def fake(packed, off, samples, hoff, threshold, refine_rounds):
        seen['packed'] = packed.copy()
        refs = RR.ransac_ref_jobs([packed[off[j]:off[j + 1]] for j in range(len(off) - 1)], samples, hoff, threshold, refine_rounds)
        seen['inner'] = [r['transform'] for r in refs]
        return {'transform': np.stack([r['transform'] for r in refs]), 'inlier_count': np.array([r['count'] for r in refs], dtype=np.int32),
                'best_hyp': np.array([r['best'] for r in refs], dtype=np.int32), 'status': np.array([r['status'] for r in refs], dtype=np.int32),
                'inlier_mask': np.concatenate([r['mask'] for r in refs]), 'hyp_count': np.concatenate([r['hyp_count'] for r in refs])}

    monkeypatch.setattr(RG, '_ransac_numpy', fake)
    monkeypatch.setattr(RG, '_need_device', lambda what: None)
    T, info = RG.find_rigid_transform(corr, threshold=0.03, iters=16, seed=0)
    assert np.array_equal(seen['packed'].min(0), np.zeros(6)) and np.array_equal(seen['packed'] + corr.min(0), corr)
    assert np.allclose(seen['inner'][0][:3, :3], rz, atol=1e-13) and np.allclose(seen['inner'][0][:3, 3], [2.0, 0.0, 0.0], atol=1e-12)
    assert np.allclose(T[:3, :3], rz, atol=1e-13) and np.allclose(T[:3, 3], t, atol=1e-12) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert info['inlier_count'] == 4 and info['inlier_mask'].all() and info['status'] == 0 and info['best_hyp'] == 0
    assert np.array_equal(info['shift'], corr.min(0))
    # two jobs, the second without a model (two rows): None, and the first unchanged
    (T2, _), (none, info2) = RG.find_rigid_transform_pairs([corr, corr[:2]], threshold=0.03, iters=16, seed=0)
    assert np.array_equal(T2, T) and none is None and info2['status'] == 1 and info2['inlier_count'] == 0
    assert RG.find_rigid_transform_pairs([]) == []
