"""CPU tier of csrc/ransac_geo.hip and its Python layer: the C ABI refuses bad calls before it touches a buffer (host memory here, never
dereferenced), the kernels neither spill nor use scratch, the yardstick's own rules, the preconditions of the whole-path cases that
tests/test_ransac_geo_gpu.py compares exactly, and the keyword errors of the public entry."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ransac_geo_ref as GR  # noqa: E402
import ransac_ref as RR  # noqa: E402
from sgaligner_amd.utils.registration import hypothesis_models_batch, ransac_geometric_batch, score_transforms_batch  # noqa: E402,F401  (the feature under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from sgaligner_amd import _lib
    return _lib.lib()


def _host(a):
    a = np.asarray(a, dtype=np.int32)
    return a, a.ctypes.data


def test_workspace_bytes_are_16_per_job_and_slice():
    l = _lib()
    f = l.sga_score_transforms_workspace_bytes
    assert f(1, 0) == 16 and f(1, 1024) == 16 and f(1, 1025) == 32 and f(3, 2100) == 3 * 3 * 16
    assert f(0, 5) == 0 and f(-1, 5) == 0 and f(2, -1) == 0


def _score(l, h_off=(0, 2, 4), h_pr=((0, 1),), n_pairs=None, max_q=2, r2=1.0, ws=True, live=True, null=None, total=4):
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    off, off_p = _host(h_off)
    pr, pr_p = _host(h_pr)
    n = len(pr) if n_pairs is None else n_pairs
    args = dict(pts=p, offsets=p, pairs=p, cell=p, origin=p, dims=p, status=p, order=p, sk=p, tr=p, live=p if live else None, count=p, sum=p)
    if null:
        args[null] = None
    rc = l.sga_score_transforms_grid(args['pts'], args['offsets'], len(off) - 1, total, args['pairs'], n, max_q, off_p, pr_p, args['cell'],
                                     args['origin'], args['dims'], args['status'], args['order'], args['sk'], args['tr'], args['live'], r2,
                                     args['count'], args['sum'], p if ws else None, 64 * 8 if ws else 0, None)
    msg = l.sga_last_error() if rc else b''
    assert rc == 0 or msg.startswith(b'sga_score_transforms_grid:'), msg
    return rc, msg


def test_score_entry_refuses_bad_calls_before_any_launch():
    l = _lib()
    assert b'negative count' in _score(l, n_pairs=-1)[1]
    assert b'r2 must be' in _score(l, r2=-1.0)[1] and b'r2 must be' in _score(l, r2=float('nan'))[1]
    assert b'max_queries 9 exceeds' in _score(l, max_q=9)[1]
    assert b'offsets' in _score(l, h_off=(0, 3, 2))[1]
    assert b'pair 0 names cloud' in _score(l, h_pr=((0, 2),))[1]
    assert b'larger than max_queries' in _score(l, max_q=1)[1]
    rc, msg = _score(l, ws=False)
    assert rc == 3 and b'workspace of 16 bytes needed' in msg
    for name in ('offsets', 'pairs', 'tr', 'count', 'sum', 'pts', 'cell', 'order'):
        assert b'null' in _score(l, null=name)[1], name
    # a job list whose workgroup count overflows int (2^21 slices of the longest query cloud x 1024 jobs), and the smallest one that is
    # refused (2^24 workgroups = 2^32 threads), by their message.  Only the counts reach the check: no host copy is given, nothing is
    # dereferenced.
    p = np.zeros(8).ctypes.data
    for n_pairs, max_q in ((1024, 2 ** 31 - 1), (2 ** 24, 1024), (2 ** 23, 1025)):
        rc = l.sga_score_transforms_grid(p, p, 2, 2 ** 31 - 1, p, n_pairs, max_q, None, None, p, p, p, p, p, p, p, None, 1.0, p, p, p, 8, None)
        assert rc == 1 and b'exceed the grid limit; split the job list' in l.sga_last_error(), (n_pairs, max_q)
    rc = l.sga_score_transforms_grid(p, p, 2, 2 ** 31 - 1, p, 2 ** 24 - 1, 1024, None, None, p, p, p, p, p, p, p, None, 1.0, p, p, p, 8, None)
    assert rc == 3 and b'workspace' in l.sga_last_error()                # one workgroup fewer passes that check and stops at the next
    # nothing to do: no pointer is looked at
    assert l.sga_score_transforms_grid(None, None, 0, 0, None, 0, 0, None, None, None, None, None, None, None, None, None, None, 1.0, None, None,
                                       None, 0, None) == 0


def test_models_entry_refuses_bad_calls_before_any_launch():
    l = _lib()
    p = np.zeros(64).ctypes.data
    off, off_p = _host((0, 16))
    hoff, hoff_p = _host((0, 8))

    def call(n_jobs=1, total_rows=16, total_hyp=8, max_hyp=8, op=off_p, hp=hoff_p, models=p, corr=p):
        rc = l.sga_ransac_models(corr, p, n_jobs, total_rows, p, p, total_hyp, max_hyp, op, hp, models, p, p, None)
        msg = l.sga_last_error() if rc else b''
        assert rc == 0 or msg.startswith(b'sga_ransac_models:'), msg
        return msg

    assert b'negative count' in call(n_jobs=-1)
    assert b'max_hyp 9 exceeds' in call(max_hyp=9)
    assert b'offsets must run from 0 to total_rows' in call(total_rows=17)
    assert b'job 0 has more hypotheses than max_hyp 4' in call(max_hyp=4)
    assert b'null pointer' in call(models=None) and b'null corr' in call(corr=None)
    assert b'misaligned' in call(models=p + 4)
    assert l.sga_ransac_models(None, None, 0, 0, None, None, 0, 0, None, None, None, None, None, None) == 0
    assert l.sga_ransac_models(None, p, 1, 0, None, p, 0, 0, None, None, None, None, None, None) == 0          # no hypotheses: nothing to write


def test_kernels_use_no_scratch_and_do_not_spill():
    from sgaligner_amd import _build
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    assert _build.FILE_FLAGS['ransac_geo.hip'] == ['-ffp-contract=off']
    _, res = kernel_resources.analyse(os.path.join(_build.CSRC, 'ransac_geo.hip'))
    seen = set()
    for k, v in res.items():
        for name in ('geo_models_kernel', 'geo_score_kernel', 'geo_fold_kernel'):
            if name in k:
                seen.add(name)
                assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
                assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
    assert len(seen) == 3, seen


def test_the_shared_device_code_is_defined_once_in_a_header():
    """The solver, the wave helpers, the rank sort and the lookups of rigid_solver.h / wave_search.h / pair_jobs.h: a definition (a line
    that opens with a function qualifier; calls are indented) of any name that ends in theirs exists once, in that header."""
    import glob
    import re
    from sgaligner_amd import _build
    text = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(_build.CSRC, '*.hip')) + glob.glob(os.path.join(_build.CSRC, '*.h'))}
    shared = {'rigid_solver.h': ['rigid_from_moments'],
              'wave_search.h': ['wave_sync', 'd2j_less', 'point_d2', 'nn_offer', 'wave_best', 'lower_bound', 'move_point', 'rank_sort'],
              'pair_jobs.h': ['sga_hyp_job', 'sga_cloud', 'sga_cloud_of_point', 'sga_cloud_pair', 'sga_pair_job']}
    for header, names in shared.items():
        for name in names:
            found = [f for f, s in sorted(text.items()) for _ in re.finditer(rf'^__(?:host|device)__ [^\n;]*\b\w*{name}\(', s, re.M)]
            assert found == [header], (name, found)
    assert [f for f, s in sorted(text.items()) if 'offd <=' in s] == ['rigid_solver.h']       # the solver's convergence test, whatever its name


def test_the_yardsticks_own_rules():
    assert GR.select_ref([5, 9, 9, -1, 9], [0.1, 0.3, 0.2, np.inf, 0.2]) == 2          # count, then sum d2, then the lowest index
    assert GR.select_ref([2, 2, -1], [0.0, 0.0, np.inf]) == -1 and GR.select_ref([-1, -1], [np.inf, np.inf]) == -1 and GR.select_ref([], []) == -1
    assert GR.select_ref([3], [0.5]) == 0
    v = GR.validated_ref([1, 0, 1, 1, 1], [0.1, 0.0, 0.3, 0.25, 0.2], 0.25, 2)
    assert v.tolist() == [0, 3] and GR.validated_ref([1, 1], [0.1, 0.1], 0.25, 1000).tolist() == [0, 1]
    # the residual is taken from the model's own bits, in the search's operation order
    corr, T, _ = RR.make_case('clean', 8, 3)
    m = GR.model12(T)
    r = GR.resid2_ref(np.stack([m, np.full(12, np.nan)]), corr, [[0, 1, 2], [0, 1, 2]])
    d = (corr[:3, :3] @ T[:3, :3].T + T[:3, 3]) - corr[:3, 3:]
    assert np.isinf(r[1]) and abs(r[0] - (d * d).sum(1).max()) <= 1e-12 * max(r[0], 1e-30)
    s = GR.edge_length_ref(corr, [[0, 1, 2]])
    assert s.dtype == np.int32 and s.shape == (1, 3)


@functools.lru_cache(maxsize=None)
def _census(seed):
    case = GR.whole_case(seed)
    return case, GR.whole_case_census(case)


@pytest.mark.parametrize('seed', GR.SEEDS)
def test_the_whole_path_cases_meet_their_preconditions(seed):
    """A condition on the cases, not a measurement: at most 2 % of a case's hypotheses are ill or near (ransac_ref.EXCLUDED_CAP); enough
    hypotheses pass both checkers that max_validation = 1, 7 and 32 cut the list and 1000 does not; the best count is far above 3; and
    the planted partners are what the selection should find."""
    case, cen = _census(seed)
    out = (cen['ill'] | cen['near']) & cen['valid']
    n_pass = int(cen['passing'].sum())
    got = cen['count'][cen['passing']]
    print(f'seed {seed}: {int(cen["valid"].sum())} of {GR.N_HYP} pass the edge-length checker, {n_pass} both checkers; ill {int(cen["ill"].sum())}, '
          f'near {int(cen["near"].sum())}; geometric counts median {int(np.median(got))} best {int(got.max())}; '
          f'{int(case["partner"].sum())} of {GR.N_SRC} correspondences are true partners')
    assert out.sum() <= RR.EXCLUDED_CAP * GR.N_HYP
    assert not cen['near'].any()
    assert 32 < n_pass < 1000
    assert got.max() >= 280 and np.median(got) < got.max()
    assert int(case['partner'].sum()) >= GR.N_SRC - int(GR.REDIRECTED * GR.N_SRC)          # a redirected row may land on its partner again
    best = GR.select_ref(cen['count'], cen['sum_d2'])
    assert best >= 0 and case['partner'][case['samples'][best]].all()


def test_keyword_errors():
    from sgaligner_amd.utils import registration as RG
    import torch
    src, feats = np.zeros((4, 3)), np.zeros((4, 2), dtype=np.float32)
    with pytest.raises(ValueError, match='score must be one of'):
        RG.registration_with_ransac_from_feats(src, src, feats, feats, score='fitness')
    with pytest.raises(ValueError, match='score must be one of'):
        RG.registration_with_ransac_from_feats_pairs([(src, src, feats, feats)], score=None)
    assert RG.RANSAC_SCORES == ('correspondence', 'geometric')
    if not torch.cuda.is_available():
        for score in RG.RANSAC_SCORES:
            with pytest.raises(RuntimeError, match='needs a HIP device'):
                RG.registration_with_ransac_from_feats(src, src, feats, feats, score=score, return_info=True)
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            RG.hypothesis_models_batch(torch.zeros((4, 6), dtype=torch.float64), [0, 4], torch.zeros((1, 3), dtype=torch.int32), [0, 1])
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            RG.score_transforms_batch(torch.zeros((4, 3), dtype=torch.float64), [0, 2, 4], [(0, 1)], torch.zeros((1, 12), dtype=torch.float64), 0.1)
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            RG.ransac_geometric_batch(torch.zeros((4, 3), dtype=torch.float64), [0, 2, 4], [(0, 1)], torch.zeros((4, 6), dtype=torch.float64),
                                      [0, 4], torch.zeros((1, 3), dtype=torch.int32), [0, 1], 0.05, 10)
    with pytest.raises(ValueError, match='max_distance must be > 0'):
        RG.score_transforms_batch(None, [0], [], None, 0.0)
    with pytest.raises(ValueError, match='max_validation must be >= 1'):
        RG.ransac_geometric_batch(None, [0], [], None, [0], None, [0], 0.05, 0)
