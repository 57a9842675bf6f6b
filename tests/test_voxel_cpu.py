"""CPU tier of the voxel grid (csrc/voxel.hip, utils/voxel.py): the yardstick's own properties (tests/voxel_ref.py), the C ABI refusing
bad arguments without a device under each entry's own name, no fallback to the host, kernels that do not spill, and the planted
end-to-end case of the GPU tier -- voxel down-sampling in front of the FPFH chain -- run through the yardsticks alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import featnn_ref as FR  # noqa: E402
import fpfh_ref as PR  # noqa: E402
import ransac_ref as RR  # noqa: E402
import voxel_ref as VR  # noqa: E402

ENTRIES = ('sga_cloud_bounds', 'sga_voxel_keys', 'sga_voxel_cells', 'sga_voxel_downsample', 'sga_knn_lists_grid')


def _clouds():
    nan_cloud = PR.lattice(40, 2)
    nan_cloud[17] = [np.nan, 0.0, 0.0]
    nan_cloud[30] = [0.0, np.inf, 0.0]
    return [PR.lattice(700, 3), PR.surface(600, 5)[0], PR.surface(600, 5)[0] + 1000.0, np.zeros((0, 3)), np.array([[0.3, -0.2, 0.1]]),
            np.tile([[0.25, -0.5, 1.0]], (40, 1)), nan_cloud, PR.lattice(100, 8) * 3.0 - 5.0]


def test_by_hand():
    """Four points, h = 1: min (0, 0, 0) -> origin -0.5; cells (0,0,0), (0,0,0), (1,0,0), (0,2,0); voxels numbered in ascending
    (kx, ky, kz): {0, 1}, {3}, {2}; the means by hand."""
    p = np.array([[0.0, 0.0, 0.0], [0.25, 0.25, 0.25], [1.0, 0.0, 0.0], [0.0, 2.0, 0.25]])
    v = VR.voxels_ref([p], 1.0)
    assert v['origin'].tolist() == [[-0.5, -0.5, -0.5]] and v['dims'].tolist() == [[2, 3, 1]] and v['status'].tolist() == [0]
    assert v['keys'].tolist() == [0, 0, 1 << 32, 2 << 16]
    assert v['order'].tolist() == [0, 1, 3, 2] and v['voxel_of_point'].tolist() == [0, 0, 2, 1]
    assert v['voxel_offsets'].tolist() == [0, 3] and v['voxel_first'].tolist() == [0, 2, 3] and v['counts'].tolist() == [2, 1, 1]
    assert v['out_points'].tolist() == [[0.125, 0.125, 0.125], [0.0, 2.0, 0.25], [1.0, 0.0, 0.0]]
    assert np.array_equal(VR.downsample_ref(p, 1.0), v['out_points'])
    assert VR.voxels_ref([p], 1e-9)['status'].tolist() == [2]                        # 2e9 cells along y: too fine for 16 bits


@pytest.mark.parametrize('h', [0.25, 0.07, 10.0, 1e-4])
def test_yardstick_properties(h):
    clouds = _clouds()
    normals = np.random.default_rng(1).standard_normal((sum(len(c) for c in clouds), 3))
    v = VR.voxels_ref(clouds, h, normals)
    off, voff = v['offsets'], v['voxel_offsets']
    assert (v['status'] == 0).all()
    pts = np.concatenate(clouds)
    dropped = ~np.isfinite(pts).all(1)
    assert int(dropped.sum()) == 2 and (v['voxel_of_point'][dropped] == -1).all() and (v['voxel_of_point'][~dropped] >= 0).all()
    assert int(v['counts'].sum()) == len(pts) - 2                                    # the counts sum to n minus the dropped points
    for c in range(len(clouds)):
        n_vox = voff[c + 1] - voff[c]
        kept = ~dropped[off[c]:off[c + 1]]
        assert n_vox == len(np.unique(v['keys'][off[c]:off[c + 1]][kept]))
        heads = v['sorted_keys'][v['voxel_first'][voff[c]:voff[c + 1]]]
        assert (np.diff(heads) > 0).all()                                            # ids ascend in (kx, ky, kz): the key is that triple
        k = np.stack([(heads >> 32) & 0xFFFF, (heads >> 16) & 0xFFFF, heads & 0xFFFF], axis=1).astype(np.float64)
        lo, hi = v['origin'][c] + k * h, v['origin'][c] + (k + 1) * h
        mean = v['out_points'][voff[c]:voff[c + 1]]
        slack = 4 * np.finfo(np.float64).eps * (np.abs(v['origin'][c]) + (k + 1) * h)   # every mean lies inside its voxel's box, to rounding
        assert (mean >= lo - slack).all() and (mean <= hi + slack).all()
        assert (v['dims'][c] == (k.max(0) + 1 if n_vox else 0)).all()
    if h == 10.0:                                                                    # one voxel per cloud that has a kept point
        assert np.diff(voff).tolist() == [1, 1, 1, 0, 1, 1, 1, 1] and v['counts'][0] == 700
        assert np.abs(v['out_points'][0] - clouds[0].mean(0)).max() < 1e-13
    if h == 1e-4:                                                                    # every distinct point its own voxel
        assert voff[2] - voff[1] == 600 and voff[6] - voff[5] == 1 and v['counts'][voff[5]] == 40
    # the normals are averaged like the points and not re-normalised
    g = voff[1]
    members = np.flatnonzero(v['voxel_of_point'][off[1]:off[2]] == 0) + off[1]
    acc = np.zeros(3)
    for i in members:
        acc = acc + normals[i]
    assert np.array_equal(v['out_normals'][g], acc / len(members))


def _refused(l, name, off=(0, 4), cell=(0.5,), max_nn=8, ws_bytes=None):
    """Entry `name` on HOST memory that is never dereferenced: the call must stop before any launch.  -> (code, error text)."""
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    h_off = np.ascontiguousarray(off, dtype=np.int32)
    h_cell = np.ascontiguousarray(cell, dtype=np.float64)
    n_clouds, total, ho = len(h_off) - 1, 4, h_off.ctypes.data
    if name == 'sga_cloud_bounds':
        rc = l.sga_cloud_bounds(p, p, n_clouds, total, ho, p, 15.0, p, None)
    elif name == 'sga_voxel_keys':
        rc = l.sga_voxel_keys(p, p, n_clouds, total, ho, p, h_cell.ctypes.data, p, p, p, p, None)
    elif name == 'sga_voxel_cells':
        need = l.sga_voxel_workspace_bytes(n_clouds, total)
        rc = l.sga_voxel_cells(p, n_clouds, total, ho, p, p, p, p, p, p, p, p, need if ws_bytes is None else ws_bytes, None)
    elif name == 'sga_voxel_downsample':
        rc = l.sga_voxel_downsample(p, None, p, n_clouds, total, ho, p, p, p, p, p, p, None, p, None)
    else:
        rc = l.sga_knn_lists_grid(p, p, n_clouds, total, ho, p, p, p, p, p, p, float('inf'), max_nn, p, p, p, None)
    assert rc != 0, name
    msg = l.sga_last_error()
    assert msg.startswith(name.encode() + b':'), msg
    return rc, msg


def test_entries_refuse_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    l = _lib.lib()
    assert 'sga_voxel_workspace_bytes(' in hdr and 'sga_voxel_workspace_bytes' in _lib.SIGNATURES
    for name in ENTRIES:
        assert name + '(' in hdr and name in _lib.SIGNATURES
        assert b'offsets decrease at cloud 1' in _refused(l, name, off=(0, 3, 2, 4), cell=(0.5, 0.5, 0.5))[1]
        assert b'offsets must run from 0 to total_points' in _refused(l, name, off=(0, 5))[1]
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert b'cell must be > 0 and finite (cloud 1' in _refused(l, 'sga_voxel_keys', off=(0, 2, 4), cell=(0.5, bad))[1]
    need = l.sga_voxel_workspace_bytes(1, 4)
    assert need >= 4 * (2 + 2 + 5) and need % 8 == 0
    rc, msg = _refused(l, 'sga_voxel_cells', ws_bytes=need - 8)
    assert rc == 3 and b'workspace of %d bytes needed, %d given' % (need, need - 8) in msg
    assert b'max_nn must be in [1, 128] (got 0)' in _refused(l, 'sga_knn_lists_grid', max_nn=0)[1]
    assert b'max_nn must be in [1, 128] (got 129)' in _refused(l, 'sga_knn_lists_grid', max_nn=129)[1]
    buf = np.zeros(8, dtype=np.float64).ctypes.data
    assert l.sga_knn_lists_grid(buf, buf, 1, 4, None, buf, buf, buf, buf, buf, buf, -1.0, 8, buf, buf, buf, None) != 0
    assert b'r2 must be >= 0' in l.sga_last_error()
    assert l.sga_voxel_downsample(buf, buf, buf, 1, 4, None, buf, buf, buf, buf, buf, buf, None, buf, None) != 0
    assert b'normals and out_normals go together' in l.sga_last_error()


def test_no_cpu_fallback_and_argument_checks():
    from sgaligner_amd.registration_evaluator import FeatureMatcher, RegistrationEvaluator
    from sgaligner_amd.utils import features as F
    from sgaligner_amd.utils import voxel as V
    pts = torch.zeros((8, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        V.voxel_downsample_batch(pts, [0, 8], 0.1)
    with pytest.raises(RuntimeError, match=r'`points` must be torch.float64'):
        V.voxel_downsample_batch(pts.float(), [0, 8], 0.1)
    with pytest.raises(RuntimeError, match=r'`normals` must be torch.float64'):
        V.voxel_downsample_batch(pts, [0, 8], 0.1, normals=pts.float())
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        F.neighbour_lists(pts, [0, 8], search='grid')
    with pytest.raises(ValueError, match='search must be one of'):
        F.FPFHDescriptor(search='tree')
    with pytest.raises(ValueError, match='voxel_size must be > 0'):
        RegistrationEvaluator(FeatureMatcher(lambda p: p), voxel_size=0.0)
    assert RegistrationEvaluator(FeatureMatcher(lambda p: p)).voxel_size is None
    assert F.FPFHDescriptor().search == 'brute'                                      # the default route stays brute force
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a HIP device'):
            V.voxel_downsample(np.zeros((5, 3)), 0.1)
        with pytest.raises(RuntimeError, match='needs a HIP device'):
            V.voxel_downsample_many([np.zeros((5, 3))], 0.1)


def test_voxel_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    assert _build.FILE_FLAGS.get('voxel.hip') == ['-ffp-contract=off']
    _, res = kr.analyse(os.path.join(_build.CSRC, 'voxel.hip'))
    for tag in ('vx_bounds_kernel', 'vx_keys_kernel', 'vx_verify_kernel', 'vx_heads_kernel', 'vx_scan_totals_kernel', 'vx_scan_kernel',
                'vx_finish_kernel', 'vx_means_kernel', 'vg_knn_kernel'):
        ks = [k for k in res if tag in k]
        assert ks, (tag, 'kernel not found')
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0 and not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
    knn = [v for k, v in res.items() if 'vg_knn_kernel' in k][0]
    assert knn['lds'] == 4 * 192 * 12 + 4 * 2 * 64 * 4 and knn['occ'] >= 5


def test_planted_registration_with_voxels_through_the_yardsticks():
    """The end-to-end case of the GPU tier on the host: planted_pair(6000, 11), both clouds through the yardstick's down-sampling at
    0.04, fpfh_ref descriptors -> featnn_ref's mutual matches -> ransac_ref (threshold 0.03, 5000 triples, seed 0).  Measured on the
    host: 956 / 929 voxels, 460 mutual matches, 270 inliers, RRE 0.376 deg, RTE 0.0006.  The limits are those of the existing
    end-to-end case: the inlier threshold over a half-metre lever."""
    from sgaligner_amd.utils import registration as RG
    src, ref, T, vp, _ = PR.planted_pair(6000, 11)
    src, ref = VR.downsample_ref(src, 0.04), VR.downsample_ref(ref, 0.04)
    fs, fr = (PR.descriptor_ref(c, 0.15, 30, 0.2, 100, vp) for c in (src, ref))
    cij = FR.match_ref(fs, fr, mutual=True)
    corr = np.concatenate([src[cij[:, 0]], ref[cij[:, 1]]], axis=1)
    shift = corr.min(axis=0)
    samples, hoff = RR.draw_samples([len(corr)], 5000, 0)
    res = RR.ransac_ref(corr - shift, samples, 0.03)
    assert res['status'] == 0
    est = RR.compose_shift(res['transform'], shift)
    rre, rte = RG.compute_registration_error(T, est)
    print(f'planted case with voxels on the host: {len(src)} / {len(ref)} voxels, {len(cij)} mutual matches, {res["count"]} inliers, '
          f'RRE {rre:.4f} deg, RTE {rte:.5f}')
    assert len(cij) >= 100
    assert rte < 0.03 and rre < 3.5
