"""CPU tier of the cross-cloud grid search and of ICP (csrc/icp.hip, utils.point_cloud.nearest_neighbor_batch(search='grid'),
utils.registration.icp_pairs): the yardstick's own properties (tests/icp_ref.py), the C ABI refusing bad arguments without a device under
each entry's own name, no fallback to the host, kernels that do not spill, and the preconditions of the GPU tier's exact comparisons."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import fpfh_ref as PR  # noqa: E402
import icp_ref as IR  # noqa: E402
import nn_ref as NR  # noqa: E402

NAME = 'sga_nn_search_grid'


def test_yardstick_by_hand():
    """Support (0,0,0), (1,0,0), (1,0,0), (0,2,0).  The query (0.5, 0, 0) is 0.25 from rows 0, 1 and 2: the lowest index wins.  Moved by
    the quarter turn about z it lands on (0, 0.5, 0): row 0 at 0.25, exactly AT r2 = 0.25, which counts; 0.81 does not."""
    s = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    q = np.array([[0.5, 0.0, 0.0], [0.9, 0.0, 0.0], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]])
    d2, idx = IR.nn_grid_ref(q, s)
    assert d2.tolist() == [0.25, (0.9 - 1.0) * (0.9 - 1.0), np.inf, np.inf] and idx.tolist() == [0, 1, -1, -1]
    turn = np.array([0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    assert IR.move(q[:1], turn).tolist() == [[0.0, 0.5, 0.0]]
    d2, idx = IR.nn_grid_ref(q[:2], s, turn)
    assert d2.tolist() == [0.25, 0.9 * 0.9] and idx.tolist() == [0, 0]
    d2, idx = IR.nn_grid_ref(q[:2], s, turn, r2=0.25)                    # d2 <= r2: a point exactly AT the radius counts
    assert d2.tolist() == [0.25, np.inf] and idx.tolist() == [0, -1]
    assert IR.nn_grid_ref(q, np.zeros((0, 3)))[1].tolist() == [-1] * 4
    assert IR.nn_grid_ref(np.zeros((0, 3)), s)[0].shape == (0,)


def test_yardstick_properties():
    q, s = PR.surface(300, 3)[0], PR.lattice(200, 4)
    assert np.array_equal(IR.move(q, IR.IDENTITY12), q)                 # 1 * x + 0 * y + 0 * z + 0 is exact
    d2, idx = IR.nn_moved_ref(q, s)
    dist, ix = NR.nn_ref(q, s)                                           # the brute-force yardstick of sga_nn_search
    assert np.array_equal(np.sqrt(d2), dist) and np.array_equal(idx, ix)
    m = IR.rigid12([1.0, 2.0, -1.0], 25.0, [0.03, -0.02, 0.05])
    R = m[:9].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
    assert np.abs(IR.move(q, m) - (q @ R.T + m[9:])).max() < 1e-15
    d2m, idxm = IR.nn_moved_ref(q, s, m)
    dm, im = NR.nn_ref(IR.move(q, m), s)
    assert np.array_equal(np.sqrt(d2m), dm) and np.array_equal(idxm, im)
    for r in (0.05, 0.1, 0.25):
        dr, ir = IR.nn_grid_ref(q, s, m, r * r)
        inside = d2m <= r * r
        assert 0 < inside.sum() < len(q)                                 # the radius cuts through the case
        assert np.array_equal(ir[inside], idxm[inside]) and (ir[~inside] == -1).all() and np.isinf(dr[~inside]).all()
    # the lattice's cell midpoints: eight exactly equal minima where all eight corners are present, and the lowest index among them
    g = (np.arange(-4, 4, dtype=np.float64) + 0.5) / 8.0
    mid = np.stack([a.reshape(-1) for a in np.meshgrid(g, g, g, indexing='ij')], axis=1)
    s3 = PR.lattice(300, 7)
    d2, idx = IR.nn_moved_ref(mid, s3)
    _, _, cnt = NR.nn_ref(mid, s3, return_counts=True)
    assert cnt.max() >= 3 and (d2[cnt > 1] > 0).all()
    for i in np.flatnonzero(cnt > 1)[:20]:
        e = s3 - mid[i]
        assert idx[i] == np.flatnonzero((e * e).sum(1) == d2[i]).min()


def _refused(l, pairs=((0, 1),), off=(0, 2, 4), r2=float('inf'), total_q=2, max_q=2, n_pairs=None):
    """The entry on HOST memory that is never dereferenced: the call must stop before any launch.  -> (code, error text)."""
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    h_off = np.ascontiguousarray(off, dtype=np.int32)
    h_pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    rc = l.sga_nn_search_grid(p, p, len(h_off) - 1, 4, p, len(h_pr) if n_pairs is None else n_pairs, p, total_q, max_q, h_off.ctypes.data,
                              h_pr.ctypes.data, p, p, p, p, p, p, None, r2, 1, p, p, None)
    assert rc != 0
    msg = l.sga_last_error()
    assert msg.startswith(NAME.encode() + b':'), msg
    return rc, msg


def test_entry_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    assert NAME + '(' in hdr and NAME in _lib.SIGNATURES
    l = _lib.lib()
    assert b'pair 0 names cloud (0, 2) of 2' in _refused(l, pairs=((0, 2),))[1]
    assert b'pair 1 names cloud (-1, 0) of 2' in _refused(l, pairs=((0, 1), (-1, 0)), total_q=4)[1]
    assert b'offsets decrease at cloud 1' in _refused(l, off=(0, 3, 2, 4))[1]
    assert b'offsets must run from 0 to total_points' in _refused(l, off=(0, 2, 5))[1]
    assert b'pair 0 is larger than max_queries 1' in _refused(l, max_q=1)[1]
    assert b'max_queries 3 exceeds total_queries 2' in _refused(l, max_q=3)[1]
    assert b'negative count' in _refused(l, n_pairs=-1)[1]
    for bad in (-1.0, float('nan')):
        assert b'r2 must be >= 0' in _refused(l, r2=bad)[1]
    buf = np.zeros(8, dtype=np.float64).ctypes.data
    assert l.sga_nn_search_grid(buf, buf, 2, 4, buf, 1, buf, 2, 2, None, None, None, buf, buf, buf, buf, buf, None, 1.0, 1, buf, buf, None) != 0
    assert b'null grid array' in l.sga_last_error()
    assert l.sga_nn_search_grid(buf, buf, 2, 4, buf, 1, buf, 2, 2, None, None, buf, buf, buf, buf, buf, buf, buf + 4, 1.0, 1, buf, buf, None) != 0
    assert b'misaligned pointer' in l.sga_last_error()
    # nothing to do is not an error, and nothing is launched for it
    assert l.sga_nn_search_grid(None, None, 0, 0, None, 0, None, 0, 0, None, None, None, None, None, None, None, None, None, 1.0, 1, None, None, None) == 0


def test_no_cpu_fallback_and_argument_checks():
    from sgaligner_amd.utils import point_cloud as PC
    pts = torch.zeros((8, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match='search must be one of'):
        PC.nearest_neighbor_batch(pts, [0, 4, 8], [(0, 1)], search='tree')
    for kw in ({'radius': 0.1}, {'cell': 0.1}, {'transforms': torch.zeros((1, 12), dtype=torch.float64)}):
        with pytest.raises(ValueError, match="belong to search='grid'"):
            PC.nearest_neighbor_batch(pts, [0, 4, 8], [(0, 1)], **kw)
    with pytest.raises(RuntimeError, match=r'`transforms` must be torch.float64'):
        PC.nearest_neighbor_batch(pts, [0, 4, 8], [(0, 1)], search='grid', transforms=torch.zeros((1, 12)))
    with pytest.raises(RuntimeError, match=r'`points` must be torch.float64'):
        PC.nearest_neighbor_batch(pts.float(), [0, 4, 8], [(0, 1)], search='grid')
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU'):
        PC.nearest_neighbor_batch(pts, [0, 4, 8], [(0, 1)], search='grid', radius=0.1)
    import inspect
    sig = inspect.signature(PC.nearest_neighbor_batch).parameters
    assert sig['search'].default == 'brute' and sig['radius'].default is None and sig['transforms'].default is None and sig['cell'].default is None


def test_icp_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    assert _build.FILE_FLAGS.get('icp.hip') == ['-ffp-contract=off']
    _, res = kr.analyse(os.path.join(_build.CSRC, 'icp.hip'))
    for tag in ('icp_nn_grid_kernel', 'icp_accum_kernel', 'icp_step_kernel'):
        ks = [k for k in res if tag in k]
        assert len(ks) == (2 if tag == 'icp_accum_kernel' else 1), (tag, ks)
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0 and not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
    nn = [v for k, v in res.items() if 'icp_nn_grid_kernel' in k][0]
    assert nn['lds'] == 4 * 2 * 64 * 4 and nn['occ'] >= 5


# ---- sga_icp ------------------------------------------------------------------------------------------------------------------------------
def _icp_refused(l, pairs=((0, 1),), off=(0, 2, 4), method=0, normals=True, max_iters=3, ws_bytes=None, r2=0.01):
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    h_off = np.ascontiguousarray(off, dtype=np.int32)
    h_pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    need = l.sga_icp_workspace_bytes(len(h_pr), 2)
    rc = l.sga_icp(p, p, len(h_off) - 1, 4, p, len(h_pr), p, 2, 2, h_off.ctypes.data, h_pr.ctypes.data, p, p, p, p, p, p, r2, method,
                   p if normals else None, p, max_iters, 1e-6, 1e-6, p, p, p, p, p, p, p, p, p, need if ws_bytes is None else ws_bytes, None)
    assert rc != 0
    msg = l.sga_last_error()
    assert msg.startswith(b'sga_icp:'), msg
    return rc, msg


def test_icp_entry_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    for name in ('sga_icp', 'sga_icp_workspace_bytes'):
        assert name + '(' in hdr and name in _lib.SIGNATURES
    l = _lib.lib()
    assert b'pair 0 names cloud (0, 2) of 2' in _icp_refused(l, pairs=((0, 2),))[1]
    assert b'max_iters must be in [0, 100000] (got -1)' in _icp_refused(l, max_iters=-1)[1]
    assert b'method 1 (point-to-plane) needs the support normals' in _icp_refused(l, method=1, normals=False)[1]
    assert b'method must be 0' in _icp_refused(l, method=2)[1]
    assert b'r2 must be >= 0' in _icp_refused(l, r2=float('nan'))[1]
    assert b'offsets decrease at cloud 1' in _icp_refused(l, off=(0, 3, 2, 4))[1]
    need = l.sga_icp_workspace_bytes(1, 2)
    assert need == 32 + 32 * 8 and l.sga_icp_workspace_bytes(3, 1025) == 3 * (32 + 2 * 32 * 8) and l.sga_icp_workspace_bytes(0, 5) == 0
    rc, msg = _icp_refused(l, ws_bytes=need - 8)
    assert rc == 3 and b'workspace of %d bytes needed, %d given' % (need, need - 8) in msg


def test_icp_python_layer_has_no_cpu_fallback():
    from sgaligner_amd.utils import registration as RG
    pair = (np.zeros((5, 3)), np.zeros((6, 3)))
    if not torch.cuda.is_available():
        for call in (lambda: RG.icp_pairs([pair]), lambda: RG.icp(*pair), lambda: RG.evaluate_registration_pairs([pair], [np.eye(4)], 0.05)):
            with pytest.raises(RuntimeError, match='needs a HIP device'):
                call()
    pts, T = torch.zeros((11, 3), dtype=torch.float64), torch.zeros((1, 12), dtype=torch.float64)
    with pytest.raises(ValueError, match='method must be one of'):
        RG.icp_batch(pts, [0, 5, 11], [(0, 1)], T, 0.05, method='line')
    with pytest.raises(ValueError, match='max_iters must be >= 0'):
        RG.icp_batch(pts, [0, 5, 11], [(0, 1)], T, 0.05, max_iters=-1)
    with pytest.raises(ValueError, match="'plane' needs the reference clouds' normals"):
        RG.icp_batch(pts, [0, 5, 11], [(0, 1)], T, 0.05, method='plane')
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU'):
        RG.icp_batch(pts, [0, 5, 11], [(0, 1)], T, 0.05)
    assert np.array_equal(RG._matrix44(RG._model12(np.arange(16.0).reshape(4, 4)[None]))[0, :3], np.arange(16.0).reshape(4, 4)[:3])


def test_yardstick_solvers_by_hand():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((50, 3))
    m = IR.rigid12([0.3, -1.0, 0.5], 12.0, [0.2, -0.1, 0.4])
    b = IR.move(a, m)
    assert np.abs(IR.kabsch12(a, b) - m).max() < 1e-14                   # exact pairs: Kabsch returns the transform
    # point-to-plane on a curved patch with its true normals: one step from a small offset lands near the truth
    x, y = rng.uniform(-1, 1, 400), rng.uniform(-1, 1, 400)
    s = np.stack([x, y, 0.3 * x * x - 0.2 * y * y + 0.1 * x * y], axis=1)
    n = np.stack([-(0.6 * x + 0.1 * y), -(-0.4 * y + 0.1 * x), np.ones(400)], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    off = IR.rigid12([1.0, 1.0, 0.2], 0.05, [0.0, 0.0, 0.001])
    u = IR.plane12(IR.move(s, off), s, n, s.min(0))
    back = IR.move(IR.move(s, off), u)
    assert np.abs(((back - s) * n).sum(1)).max() < 1e-6 < np.abs(((IR.move(s, off) - s) * n).sum(1)).max()
    flat = np.stack([x, y, np.zeros(400)], axis=1)                       # a plane with equal normals: the normal matrix is singular
    assert IR.plane12(flat + [0.0, 0.0, 0.01], flat, np.tile([[0.0, 0.0, 1.0]], (400, 1)), flat.min(0)) is None
    assert np.array_equal(IR.compose12(IR.IDENTITY12, m), m)


def test_yardstick_icp_recovers_a_planted_transform():
    """planted_pair from a 3 degree / 0.02 perturbation: ICP ends nearer the truth than it started, with both methods."""
    src, ref, T, _, perm = PR.planted_pair(600, 11)
    truth = np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])
    c = ref.mean(0)
    P = IR.rigid12([0.2, -0.1, 1.0], 3.0, [0.02, 0.0, 0.0])
    P = np.concatenate([P[:9], c - P[:9].reshape(3, 3) @ c + P[9:]])
    start = IR.compose12(P, truth)
    normals = (PR.surface(600, 11, bump=True)[1] @ T[:3, :3].T)[perm]
    for method in (0, 1):
        r = IR.icp_ref(src, ref, start, 0.05, method, normals, 30)
        (rre0, rte0), (rre1, rte1) = IR.rre_rte(truth, start), IR.rre_rte(truth, r['transform'])
        print(f'method {method}: RRE {rre0:.3f} -> {rre1:.3f} deg, RTE {rte0:.4f} -> {rte1:.4f}, fitness {r["fitness"]:.3f}, {r["iters"]} iterations')
        assert r['status'] == 0 and rre1 < 0.5 * rre0 and rte1 < 0.5 * rte0 and r['fitness'] > 0.95
    r0 = IR.icp_ref(src, ref, start, 0.05, 0, None, 0)                   # max_iters = 0: evaluate_registration
    assert r0['iters'] == 0 and len(r0['trace']) == 1 and np.array_equal(r0['transform'], start)
    assert IR.icp_ref(src[:2], ref, start, 0.05, 0, None, 5)['status'] == 1 and IR.icp_ref(src[:5], ref, start, 0.05, 1, normals, 5)['status'] == 1


@pytest.mark.parametrize('sizes', IR.WHOLE_RUNS)
@pytest.mark.parametrize('method', [0, 1])
def test_preconditions_of_the_exact_gpu_comparison(method, sizes):
    """The GPU tier compares trace fitness, iteration counts and correspondence sets of whole runs EXACTLY against this yardstick, whose
    transforms differ from the kernel's by rounding.  That is sound while no query sits within 2 tau of a decision: its nearest and second
    nearest reference points that close in distance, or its nearest that close to max_distance -- in any iteration; and while the stop
    test is not that close to its thresholds."""
    c = IR.surface_case(*sizes)
    r = IR.icp_ref(c['src'], c['ref'], c['start'], IR.MAX_DISTANCE, method, c['normals'], 30, tau=IR.TAU)
    (rre0, rte0), (rre1, rte1) = IR.rre_rte(c['truth'], c['start']), IR.rre_rte(c['truth'], r['transform'])
    print(f'{sizes} method {method}: fitness {r["fitness"]:.4f} rmse {r["rmse"]:.5f} iterations {r["iters"]} RRE {rre0:.2f} -> {rre1:.3f} deg RTE {rte0:.4f} -> {rte1:.4f}')
    assert r['status'] == 0 and len(r['near']) == r['iters'] + 1 and sum(r['near']) == 0
    assert rre1 < rre0 and rte1 < rte0
    d = np.abs(np.diff(r['trace'], axis=0))
    assert (np.abs(d - 1e-6) > 1e-9).all()                               # no evaluation decides the stop test by a hair
