"""CPU tier of the exact nearest-neighbour search (csrc/nnsearch.hip, utils/point_cloud.py, utils/registration.py): the numpy yardstick
is pinned on cKDTree (which IS the reference's get_nearest_neighbor body), the C ABI is complete and refuses bad arguments without a
device, nothing falls back to the host, the kernels do not spill, and the closed-form registration helpers give hand-computed values."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import nn_ref as NR  # noqa: E402


@pytest.mark.parametrize('family', NR.FAMILIES)
def test_numpy_yardstick_is_bit_equal_to_ckdtree(family):
    from scipy.spatial import cKDTree
    q, s = NR.make_pair(family, 3000, 20000, seed=11)
    dist, idx, cnt = NR.nn_ref(q, s, return_counts=True)
    kd, ki = cKDTree(s).query(q, k=1)
    assert dist.dtype == kd.dtype == np.float64
    assert np.array_equal(dist.view(np.int64), kd.view(np.int64)), int((dist != kd).sum())
    uniq = cnt == 1
    assert np.array_equal(idx[uniq], ki[uniq])
    if family == 'scan':
        assert (dist == 0).sum() >= 500
    if family == 'lattice':
        assert (~uniq).mean() > 0.5                      # the family exists for its ties
        assert np.array_equal(idx, [int(np.flatnonzero((s == s[k]).all(1))[0]) for k in idx])      # argmin = the lowest of the duplicates


def test_abi_has_the_entry_points_and_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    for name in ('sga_nn_search', 'sga_nn_workspace_bytes'):
        assert name + '(' in hdr and name in _lib.SIGNATURES
    l = _lib.lib()
    assert l.sga_nn_workspace_bytes(1000, 5000, 5000) == 0                       # one pass: no workspace
    assert l.sga_nn_workspace_bytes(1000, 5000, 1000) == 12 * 5 * 1000
    nul = (None, None, 1, 4, None, 1, None, 4, 4, 4, 1024, None, None, 0, None, None, None, 0, None)
    assert l.sga_nn_search(*nul) != 0 and b'null pointer' in l.sga_last_error()
    off = np.array([0, 4], dtype=np.int32)
    pr = np.array([[0, 1]], dtype=np.int32)                                       # cloud 1 does not exist
    buf = np.zeros(16, dtype=np.float64)                                          # host memory: never dereferenced, the call must stop before
    p = buf.ctypes.data
    rc = l.sga_nn_search(p, p, 1, 4, p, 1, p, 4, 4, 4, 1024, off.ctypes.data, pr.ctypes.data, 0, p, p, None, 0, None)
    assert rc != 0 and b'pair 0 names cloud (0, 1) of 1' in l.sga_last_error()
    rc = l.sga_nn_search(p, p, 1, 4, p, 1, p, 4, 4, 4, 0, None, None, 0, p, p, None, 0, None)
    assert rc != 0 and b'chunk' in l.sga_last_error()
    rc = l.sga_nn_search(p, p, -1, 4, p, 1, p, 4, 4, 4, 8, None, None, 0, p, p, None, 0, None)
    assert rc != 0 and b'negative count' in l.sga_last_error()
    rc = l.sga_nn_search(p + 4, p, 1, 4, p, 1, p, 4, 4, 4, 8, None, None, 0, p, p, None, 0, None)
    assert rc != 0 and b'misaligned' in l.sga_last_error()
    rc = l.sga_nn_search(p, p, 1, 4, p, 1, p, 4, 4, 4, 2, None, None, 0, p, p, None, 0, None)      # split form without its workspace
    assert rc != 0 and b'workspace' in l.sga_last_error()


def test_no_silent_fallback():
    from sgaligner_amd.utils import point_cloud as PC, registration as RG
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        PC.nearest_neighbor_batch(torch.zeros((4, 3), dtype=torch.float64), [0, 4], [(0, 0)])
    if torch.cuda.is_available():
        return                                             # the rest is about machines without a device
    a, b = np.zeros((5, 3)), np.ones((4, 3))
    for fn in (lambda: PC.get_nearest_neighbor(a, b), lambda: PC.compute_pcl_overlap(a, b),
               lambda: PC.compute_pcl_overlap_pairs([a, b], [(0, 1)]), lambda: RG.nn_correspondence(a, b),
               lambda: RG.compute_mosaicking_error(a, b),
               lambda: RG.compute_modified_chamfer_distance(a, a, b, np.eye(4), np.eye(4))):
        with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
            fn()


def test_nn_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    assert '-ffp-contract=off' in _build.FILE_FLAGS['nnsearch.hip']
    _, res = kr.analyse(os.path.join(_build.CSRC, 'nnsearch.hip'))
    for tag in ('9nn_kernel', '15nn_merge_kernel'):
        ks = [k for k in res if tag in k]
        assert ks, (tag, sorted(res))
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
            assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)


def test_closed_form_registration_helpers():
    from sgaligner_amd.utils import registration as RG
    from sgaligner_amd.utils.point_cloud import apply_transform
    eye = np.eye(4)
    assert RG.compute_registration_error(eye, eye) == (0.0, 0.0)
    rz = np.eye(4)
    rz[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]           # 90 degrees about z
    assert abs(RG.compute_relative_rotation_error(eye[:3, :3], rz[:3, :3]) - 90.0) < 1e-12
    tr = np.eye(4)
    tr[:3, 3] = [3.0, 4.0, 12.0]
    rre, rte = RG.compute_registration_error(eye, tr)
    assert rre == 0.0 and rte == 13.0
    assert RG.compute_registration_error(eye, tr.T, inverse_trans=True)[1] == 13.0
    pts = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]])
    moved, nrm = apply_transform(pts, rz, normals=pts)
    assert np.array_equal(moved, [[0.0, 1.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, 3.0]]) and np.array_equal(nrm, moved)
    assert np.array_equal(apply_transform(pts, tr), pts + [3.0, 4.0, 12.0])
    # rigid metrics on the host: ref = src moved by `tr` exactly -> no residual; ref = src -> every residual is |t| = 13
    assert RG.compute_registration_rmse(pts + [3.0, 4.0, 12.0], pts, tr) == 0.0
    assert RG.compute_registration_rmse(pts, pts, tr) == 13.0
    assert RG.compute_inlier_ratio(pts + [3.0, 4.0, 12.0], pts, tr) == 1.0 and RG.compute_inlier_ratio(pts, pts, tr) == 0.0
    assert RG.nn_correspondence(np.zeros((0, 3)), pts) == ([], [])
