"""CPU tier of the feature-space nearest-neighbour search (csrc/featnn.hip) and the registration from features built on it
(utils/registration.py, registration_evaluator.py): the C ABI is complete and refuses bad arguments without a device, each under its own
name; nothing falls back to the host; the kernels do not spill; the yardstick's mutual filter and edge-length rule hold on hand-made
cases; the sample triples come from the existing draw_samples."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import featnn_ref as FR  # noqa: E402


def _call(l, C=4, off=(0, 4), pairs=((0, 0),), tiles=((0, 0, 0),), n_sets=1, total_rows=4, chunk=1024, feats_shift=0, ws=True, n_qt=1):
    """sga_featnn_search on HOST memory that is never dereferenced: the call must stop before any launch.  -> the error text."""
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    h_off, h_pr, h_tiles = (np.ascontiguousarray(a, dtype=np.int32) for a in (off, pairs, tiles))
    rc = l.sga_featnn_search(p + feats_shift, C, p, n_sets, total_rows, p, len(h_pr), p, p, len(h_tiles), n_qt, 4, 4, 4, chunk, h_off.ctypes.data,
                             h_pr.ctypes.data, h_tiles.ctypes.data, p, p, p if ws else None, 64 * 8 if ws else 0, None)
    assert rc != 0
    msg = l.sga_last_error()
    assert msg.startswith(b'sga_featnn_search:'), msg
    return msg


def test_abi_has_the_entry_points_and_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    for name in ('sga_featnn_search', 'sga_featnn_workspace_bytes'):
        assert name + '(' in hdr and name in _lib.SIGNATURES
    l = _lib.lib()
    assert l.sga_featnn_workspace_bytes(1001, 500, 4000, 4000) == 4008                     # one pass: the norms only, rounded up to 8
    assert l.sga_featnn_workspace_bytes(1001, 500, 4000, 1000) == 4008 + 8 * 4 * 500       # + (score, idx) x 4 chunks x queries
    assert l.sga_featnn_workspace_bytes(1001, 500, 0, 1000) == 4008                        # every support empty: still the norms
    assert l.sga_featnn_workspace_bytes(1001, 0, 4000, 1000) == 0
    assert b'multiple of 4 (got 0)' in _call(l, C=0)
    assert b'multiple of 4 (got 6)' in _call(l, C=6)
    assert b'offsets decrease at set 1' in _call(l, off=(0, 3, 2, 4), n_sets=3)
    assert b'offsets must run from 0 to total_rows' in _call(l, off=(0, 5))
    assert b'pair 0 names set (0, 1) of 1' in _call(l, pairs=((0, 1),))
    assert b'misaligned' in _call(l, feats_shift=8)
    assert b'chunk must be >= 1' in _call(l, chunk=0)
    assert b'tile 0 = (job 1, query tile 0, chunk 0) is out of range' in _call(l, tiles=((1, 0, 0),))
    assert b'tile 0 = (job 0, query tile 1, chunk 0) is out of range' in _call(l, tiles=((0, 1, 0),))
    assert b'only they, have chunk 0' in _call(l, tiles=((0, 0, 0), (0, 0, 0)))
    assert b'workspace of 80 bytes needed, 0 given' in _call(l, chunk=2, tiles=((0, 0, 0), (0, 0, 1)), ws=False)
    assert b'negative count' in _call(l, n_sets=-1)


def test_no_silent_fallback():
    from sgaligner_amd.registration_evaluator import FeatureMatcher, RegistrationEvaluator
    from sgaligner_amd.utils import registration as RG
    f = torch.zeros((4, 8), dtype=torch.float32)
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        RG.feature_nn_batch(f, [0, 4], [(0, 0)])
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        RG.match_features_pairs([(f, f)])
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        RG.edge_length_filter(torch.zeros((4, 6), dtype=torch.float64), [0, 4], torch.zeros((2, 3), dtype=torch.int32), [0, 2])
    with pytest.raises(RuntimeError, match=r'must be torch.float32'):
        RG.feature_nn_batch(f.double(), [0, 4], [(0, 0)])
    with pytest.raises(ValueError, match='ransac_n == 3'):
        RG.registration_with_ransac_from_feats(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 8)), np.zeros((4, 8)), ransac_n=4)
    with pytest.raises(TypeError, match='match_many'):
        RegistrationEvaluator(lambda s, r, g: None).run_normal_registration({'src_points': np.zeros((4, 3)), 'ref_points': np.zeros((4, 3))})
    with pytest.raises(TypeError, match='descriptor must be callable'):
        FeatureMatcher(None)
    if torch.cuda.is_available():
        return                                             # the rest is about machines without a device
    a, b = np.zeros((5, 3)), np.ones((4, 3))
    fm = FeatureMatcher(lambda p: p.astype(np.float32))
    for fn in (lambda: RG.match_features_pairs([(np.zeros((5, 8)), np.ones((4, 8)))]),
               lambda: RG.registration_with_ransac_from_feats(a, b, np.zeros((5, 8)), np.ones((4, 8))),
               lambda: RG.registration_with_ransac_from_feats_pairs([(a, b, np.zeros((5, 8)), np.ones((4, 8)))]),
               lambda: fm(a, b, np.eye(4)), lambda: fm.match_many([(a, b)])):
        with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
            fn()


def test_featnn_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    assert '-ffp-contract=off' in _build.FILE_FLAGS['featnn.hip']
    _, res = kr.analyse(os.path.join(_build.CSRC, 'featnn.hip'))
    for tag in ('18featnn_norm_kernel', '13featnn_kernel', '20featnn_finish_kernel'):
        ks = [k for k in res if tag in k]
        assert ks, (tag, sorted(res))
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
            assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
    main, = [v for k, v in res.items() if '13featnn_kernel' in k]
    assert main['agpr'] + main['vgpr'] <= 256 and main['lds'] <= 80 * 1024                 # two workgroups of four waves fit a CU (160 KiB of LDS)


def test_tile_list_names_every_tile_once_and_the_query_tiles_first():
    from sgaligner_amd.utils import registration as RG
    tiles, n_qt = RG._featnn_tiles([300, 0, 129, 5], [257, 10, 0, 100], 100)
    assert n_qt == 3 + 0 + 2 + 1
    want = {(0, q, c) for q in range(3) for c in range(3)} | {(2, 0, 0), (2, 1, 0), (3, 0, 0)}     # ns = 100 = chunk: one pass
    assert len(tiles) == len(want) and {tuple(t) for t in tiles.tolist()} == want
    assert (tiles[:n_qt, 2] == 0).all() and (tiles[n_qt:, 2] > 0).all() and tiles.dtype == np.int32
    assert RG._featnn_tiles([], [], 7)[0].shape == (0, 3)


def test_yardstick_mutual_filter_and_edge_length_rule_on_hand_made_cases():
    # source rows 0..3, reference rows 0..2: 0 <-> 1 mutual, 1 -> 1 not returned, 2 <-> 0 mutual, 3 has no neighbour at all
    assert FR.mutual_filter([1, 1, 0, -1], [2, 0, 3]).tolist() == [[0, 1], [2, 0]]
    src = np.array([[0.0, 0.0], [1.0, 0.0], [5.0, 5.0]], dtype=np.float32)
    ref = np.array([[5.0, 4.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0]], dtype=np.float32)
    idx, d2 = FR.nn_ref(src, ref)
    assert idx.tolist() == [1, 1, 0] and d2.tolist() == [0.0, 1.0, 1.0]                # row 1 twice: ties to the lowest index
    assert FR.match_ref(src, ref, mutual=False).tolist() == [[0, 1], [1, 1], [2, 0]]
    assert FR.match_ref(src, ref, mutual=True).tolist() == [[0, 1], [2, 0]]             # ref 1 -> src 0, ref 3 -> src 1 (not mutual)
    assert FR.nn_ref(src, ref[:0])[0].tolist() == [-1, -1, -1] and np.isinf(FR.nn_ref(src, ref[:0])[1]).all()
    # edge lengths: a 3-4-5 triangle against itself moved (passes), against itself scaled by 0.5 (similarity 0.5: the boundary passes, >=),
    # by 0.25 and by 4 (fail, either way round), and with ONE edge of three off (fails)
    tri = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    bent = tri.copy()
    bent[2] = [0.0, 9.0, 0.0]                                                            # edges 3, sqrt(90), 9 against 3, 5, 4
    corr = np.concatenate([np.concatenate([tri, m], axis=1) for m in (tri + 7.0, tri * 0.5, tri * 0.25, tri * 4.0, bent)])
    samples = np.arange(15).reshape(5, 3)
    assert FR.edge_length_ok(corr, samples, 0.5).tolist() == [True, True, False, False, False]
    assert FR.edge_length_ok(corr, samples).tolist() == [True, False, False, False, False]
    assert FR.edge_length_ok(corr, samples[:, ::-1]).tolist() == [True, False, False, False, False]
    # the bound of the module docstring on a hand case: C = 2, a = (1, -2), b = (3, 4): 2 g (3 + 8) + g 25 with g = 4u / (1 - 4u)
    g = 4 * FR.U / (1 - 4 * FR.U)
    assert FR.error_bound([[1.0, -2.0]], [[3.0, 4.0]])[0, 0] == 2 * g * 11.0 + g * 25.0
    assert FR.seq_d2([1.0, -2.0], [3.0, 4.0]) == 40.0 and FR.d2_matrix([[1.0, -2.0]], [[3.0, 4.0]])[0, 0] == 40.0


def test_samples_come_from_draw_samples_unchanged():
    """registration_with_ransac_from_feats draws its triples with the existing draw_samples: same generator, same triples per job, so a
    seed means what it means for find_rigid_transform_pairs."""
    from sgaligner_amd.utils import registration as RG
    src = inspect.getsource(RG.registration_with_ransac_from_feats_pairs)
    assert 'draw_samples(sizes, num_iterations, seed)' in src
    s, off = RG.draw_samples([300, 2, 40], 64, 5)
    assert off.tolist() == [0, 64, 64, 128] and s.dtype == np.int32
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 300, 64), rng.integers(0, 299, 64)
    assert np.array_equal(s[:64, 0], a) and np.array_equal(s[:64, 1], b + (b >= a))
    assert (s[:64] < 300).all() and (s[64:] < 40).all() and all(len(set(t)) == 3 for t in s.tolist())


def test_planted_case_is_what_it_says():
    case = FR.planted_registration(3)
    assert len({tuple(r) for r in case['ref_feats'].tolist()}) == 400                   # distinct codes
    assert np.array_equal(case['ref_feats'][case['perm']], case['src_feats'])           # shared by true partners
    moved = case['src'] @ case['transform'][:3, :3].T + case['transform'][:3, 3]
    assert np.array_equal(case['ref'][case['perm']], moved)
    want = np.stack([np.arange(300), case['perm']], axis=1)
    assert np.array_equal(FR.match_ref(case['src_feats'], case['ref_feats'], True), want)
    assert np.array_equal(FR.match_ref(case['src_feats'], case['ref_feats'], False), want)
    r = case['transform'][:3, :3]
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-14) and np.linalg.det(r) > 0.999
