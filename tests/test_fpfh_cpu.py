"""CPU tier of the FPFH chain (csrc/fpfh.hip, utils/features.py): the yardstick (tests/fpfh_ref.py) against cases worked by hand, the C
ABI refusing bad arguments without a device under each entry's own name, no fallback to the host, kernels that do not spill, and the
planted end-to-end case of the GPU tier run through the yardsticks alone."""
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

ENTRIES = ('sga_knn_lists', 'sga_normals', 'sga_spfh_counts', 'sga_fpfh')


def test_three_points_by_hand():
    """p0 = origin, p1 = (1, 0, 0), p2 = (0, 2, 0), all in one list.  Lists by (d2, j); the plane z = 0 gives the normal (0, 0, 1); with
    those normals every pair has a1 = a2 = 0, f = (0, 0, 0): bins 5 / 16 / 27 twice each; s = 100 there, and every point's weighted
    neighbours are rescaled to 100: 200 in three columns."""
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    count, idx, d2 = PR.lists_ref(p, None, 3)
    assert count.tolist() == [3, 3, 3]
    assert idx.tolist() == [[0, 1, 2], [1, 0, 2], [2, 0, 1]]
    assert d2.tolist() == [[0.0, 1.0, 4.0], [0.0, 1.0, 5.0], [0.0, 4.0, 5.0]]
    c2, i2, q2 = PR.lists_ref(p, 1.0, 2)                               # the radius is inclusive, the cut keeps the lower index
    assert c2.tolist() == [2, 2, 1] and i2.tolist() == [[0, 1], [1, 0], [2, -1]] and q2[2].tolist() == [0.0, np.inf]
    nr = PR.normals_ref(p, (count, idx, d2), viewpoint=(0.0, 0.0, 5.0))
    assert nr['status'].tolist() == [0, 0, 0] and np.allclose(nr['normals'], [[0, 0, 1]] * 3, atol=1e-15)
    assert np.allclose(PR.normals_ref(p, (count, idx, d2), viewpoint=(0.0, 0.0, -5.0))['normals'], [[0, 0, -1]] * 3, atol=1e-15)
    assert PR.normals_ref(p, (c2, i2, q2))['status'].tolist() == [1, 1, 1]
    counts, _, pairs = PR.spfh_ref(p, np.tile([0.0, 0.0, 1.0], (3, 1)), (count, idx, d2))
    want = np.zeros((3, 33), dtype=np.int32)
    want[:, [5, 16, 27]] = 2
    assert pairs == 6 and (counts == want).all()
    out = PR.fpfh_ref(counts, (count, idx, d2))
    assert np.allclose(out, want * 100.0, rtol=1e-14, atol=0)
    # point 0 by hand, in the contract's order: (100 / 1 + 100 / 4) * (100 / 125) + 100
    assert out[0, 5] == (100.0 / 1.0 + 100.0 / 4.0) * (100.0 / 125.0) + 100.0


def test_plane_lattice_and_line():
    for axis in (0, 2):
        p = PR.plane_lattice(axis)
        vp = np.zeros(3)
        vp[axis] = 5.0
        nr = PR.normals_ref(p, PR.lists_ref(p, None, 30), viewpoint=vp)
        want = np.zeros(3)
        want[axis] = 1.0
        assert not nr['ill'].any() and not nr['sign_near'].any() and (nr['status'] == 0).all()
        assert np.abs(nr['normals'] - want).max() <= 1e-15
        free = PR.normals_ref(p, PR.lists_ref(p, None, 30))['normals']                  # no viewpoint: the largest component positive
        assert np.abs(free - want).max() <= 1e-15
    # points on a line, normals along it: dp x n1 = 0, every pair lands in bins 5 / 16 / 27
    line = np.stack([np.arange(7.0) * 0.125, np.zeros(7), np.zeros(7)], axis=1)
    lists = PR.lists_ref(line, None, 5)
    counts, _, _ = PR.spfh_ref(line, np.tile([1.0, 0.0, 0.0], (7, 1)), lists)
    want = np.zeros((7, 33), dtype=np.int32)
    want[:, [5, 16, 27]] = 4
    assert (counts == want).all()


def test_every_group_sums_to_m_minus_1():
    for n, seed in ((65, 3), (257, 4)):
        p, nr = PR.surface(n, seed)
        lists = PR.lists_ref(p, 0.2, 50)
        counts, undecided, pairs = PR.spfh_ref(p, nr, lists)
        assert pairs == int(np.maximum(lists[0] - 1, 0).sum())
        for g in range(3):
            assert (counts[:, 11 * g:11 * g + 11].sum(1) == np.maximum(lists[0] - 1, 0)).all()
        assert undecided.mean() <= 0.01
    lat = PR.lattice(200, 5)
    lists = PR.lists_ref(lat, 0.25, 30)
    counts, _, _ = PR.spfh_ref(lat, np.tile([0.0, 0.0, 1.0], (200, 1)), lists)
    assert (counts.reshape(200, 3, 11).sum(2) == np.maximum(lists[0] - 1, 0)[:, None]).all()
    out = PR.fpfh_ref(counts, lists)
    assert np.isfinite(out).all() and (out >= 0).all()


def _refused(l, name, max_nn=8, ld=36, off=(0, 4)):
    """Entry `name` on HOST memory that is never dereferenced: the call must stop before any launch.  -> the error text."""
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    h_off = np.ascontiguousarray(off, dtype=np.int32)
    n_clouds, total, ho = len(h_off) - 1, 4, h_off.ctypes.data
    if name == 'sga_knn_lists':
        rc = l.sga_knn_lists(p, p, n_clouds, total, ho, float('inf'), max_nn, p, p, p, None)
    elif name == 'sga_normals':
        rc = l.sga_normals(p, p, n_clouds, total, ho, p, p, max_nn, None, p, p, None)
    elif name == 'sga_spfh_counts':
        rc = l.sga_spfh_counts(p, p, p, n_clouds, total, ho, p, p, p, max_nn, p, None)
    else:
        rc = l.sga_fpfh(p, p, n_clouds, total, ho, p, p, p, max_nn, p, p, ld, None)
    assert rc != 0, name
    msg = l.sga_last_error()
    assert msg.startswith(name.encode() + b':'), msg
    return msg


def test_entries_refuse_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    l = _lib.lib()
    for name in ENTRIES:
        assert name + '(' in hdr and name in _lib.SIGNATURES
        assert b'max_nn must be in [1, 128] (got 0)' in _refused(l, name, max_nn=0)
        assert b'max_nn must be in [1, 128] (got 129)' in _refused(l, name, max_nn=129)
        assert b'offsets decrease at cloud 1' in _refused(l, name, off=(0, 3, 2, 4))
        assert b'offsets must run from 0 to total_points' in _refused(l, name, off=(0, 5))
    assert b'ld must be >= 33 and a multiple of 4 (got 35)' in _refused(l, 'sga_fpfh', ld=35)
    assert b'ld must be >= 33 and a multiple of 4 (got 32)' in _refused(l, 'sga_fpfh', ld=32)
    buf = np.zeros(8, dtype=np.float64).ctypes.data
    assert l.sga_knn_lists(buf, buf, 1, 4, None, -1.0, 8, buf, buf, buf, None) != 0 and b'r2 must be >= 0' in l.sga_last_error()
    assert l.sga_knn_lists(buf, buf, 1, 4, None, float('nan'), 8, buf, buf, buf, None) != 0 and b'r2 must be >= 0' in l.sga_last_error()


def test_no_cpu_fallback_and_the_dtype_is_reported_first():
    from sgaligner_amd.utils import features as F
    pts = torch.zeros((8, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        F.fpfh_batch(pts, [0, 8])
    with pytest.raises(RuntimeError, match=r'`points` must be torch.float64'):
        F.fpfh_batch(pts.float(), [0, 8])
    with pytest.raises(RuntimeError, match=r'`normals` must be torch.float64'):
        F.fpfh_batch(pts, [0, 8], normals=pts.float())
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        F.neighbour_lists(pts, [0, 8])
    lists = (torch.zeros(8, dtype=torch.int32), torch.zeros((8, 4), dtype=torch.int32), torch.zeros((8, 4), dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        F.fpfh_from_counts(torch.zeros((8, 33), dtype=torch.int32), lists)
    with pytest.raises(RuntimeError, match=r'`lists.idx` must be torch.int32'):
        F.estimate_normals_batch(pts, [0, 8], lists=(lists[0], lists[1].long(), lists[2]))
    with pytest.raises(ValueError, match=r'max_nn must be in \[1, 128\]'):
        F.FPFHDescriptor(max_nn_feature=129)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a HIP device'):
            F.FPFHDescriptor()(np.zeros((5, 3)))
        with pytest.raises(RuntimeError, match='needs a HIP device'):
            F.estimate_normals(np.zeros((5, 3)))


def test_feature_matcher_uses_the_descriptors_batched_form():
    """match_many asks a descriptor that has `many` once, for all clouds in pair order; one without it is called per cloud as before."""
    from sgaligner_amd.registration_evaluator import FeatureMatcher
    seen = []

    class D:
        def __call__(self, p):
            raise AssertionError('the per-cloud form must not be used')

        def many(self, clouds):
            seen.append([len(c) for c in clouds])
            return [np.zeros((len(c), 4), dtype=np.float32) for c in clouds]

    pairs = [(np.zeros((3, 3)), np.zeros((5, 3))), (np.zeros((2, 3)), np.zeros((7, 3)))]
    with pytest.raises(RuntimeError, match='HIP device'):                       # the matching itself needs the device; the descriptor ran first
        FeatureMatcher(D()).match_many(pairs)
    assert seen == [[3, 5, 2, 7]]


def test_fpfh_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    assert _build.FILE_FLAGS.get('fpfh.hip') == ['-ffp-contract=off']
    _, res = kr.analyse(os.path.join(_build.CSRC, 'fpfh.hip'))
    for tag in ('knn_kernel', 'normals_kernel', 'spfh_kernel', 'fpfh_kernel'):
        ks = [k for k in res if tag in k]
        assert ks, (tag, 'kernel not found')
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0 and not v.get('loop_scratch'), (k, v)
    knn = [v for k, v in res.items() if 'knn_kernel' in k][0]
    assert knn['lds'] == 3 * 512 * 8 + 4 * 192 * 12


def test_planted_registration_through_the_yardsticks():
    """The end-to-end case of the GPU tier on the host: fpfh_ref descriptors -> featnn_ref's mutual matches -> ransac_ref with the
    evaluator's shift, threshold 0.03 and 5000 triples.  RTE < 0.03 and RRE < 3.5 degrees: the inlier threshold over a half-metre lever."""
    from sgaligner_amd.utils import registration as RG
    src, ref, T, vp, _ = PR.planted_pair()
    fs, fr = (PR.descriptor_ref(c, 0.15, 30, 0.2, 100, vp) for c in (src, ref))
    cij = FR.match_ref(fs, fr, mutual=True)
    assert len(cij) >= 100
    corr = np.concatenate([src[cij[:, 0]], ref[cij[:, 1]]], axis=1)
    shift = corr.min(axis=0)
    samples, hoff = RR.draw_samples([len(corr)], 5000, 0)
    res = RR.ransac_ref(corr - shift, samples, 0.03)
    assert res['status'] == 0
    est = RR.compose_shift(res['transform'], shift)
    rre, rte = RG.compute_registration_error(T, est)
    print(f'planted case on the host: {len(cij)} mutual matches, {res["count"]} inliers, RRE {rre:.4f} deg, RTE {rte:.5f}')
    assert rte < 0.03 and rre < 3.5
