"""GPU tier of the FPFH chain (csrc/fpfh.hip through utils/features.py) against the numpy yardstick tests/fpfh_ref.py.  Neighbour lists
and the FPFH weighting are compared bit for bit (pinned arithmetic); the census is compared exactly on every point the yardstick calls
decided; the normals within 1e-9 where the yardstick calls them well-conditioned.  Open3D is not available: the contract of
include/sgaligner_hip.h is what is tested, not Open3D's output."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fpfh_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

LATTICE_SIZES = (1, 2, 63, 64, 65, 257, 700)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(lists):
    return tuple(t.cpu().numpy() for t in lists)


def _pack(clouds):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return np.concatenate(clouds), off


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_lists_equal(got, want, max_nn):
    count, idx, d2 = got
    assert count.dtype == np.int32 and idx.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(count, want[0])
    assert np.array_equal(idx, want[1])
    assert _same_bits(d2, want[2])
    past = np.arange(max_nn)[None, :] >= count[:, None]
    assert (idx[past] == -1).all() and np.isposinf(d2[past]).all()
    assert (idx[~past] >= 0).all() and np.isfinite(d2[~past]).all()


@functools.lru_cache(maxsize=None)
def _lattice_clouds():
    return tuple(PR.lattice(n, 100 + n) for n in LATTICE_SIZES)


@functools.lru_cache(maxsize=None)
def _lattice_ref(radius, max_nn):
    return PR.lists_ref_packed(_lattice_clouds(), radius, max_nn)


@functools.lru_cache(maxsize=None)
def _surface(n):
    return PR.surface(n, 40 + n)


@functools.lru_cache(maxsize=None)
def _surface_lists(n, radius, max_nn):
    return PR.lists_ref(_surface(n)[0], radius, max_nn)


# ---- 1-3: neighbour lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [None, 0.25, 0.5])
@pytest.mark.parametrize('max_nn', [1, 30, 64, 128])
def test_lists_lattice_exact(max_nn, radius):
    from sgaligner_amd.utils import features as F
    pts, off = _pack(_lattice_clouds())
    got = _host(F.neighbour_lists(_dev(pts), off, radius, max_nn))
    _assert_lists_equal(got, _lattice_ref(radius, max_nn), max_nn)
    if radius is None:                                         # the family exists for this: the cut falls inside a run of equal d2
        assert int(PR.straddlers(_lattice_ref(None, max_nn + 1), max_nn).sum()) > 100


@pytest.mark.parametrize('max_nn,radius', [(1, None), (30, None), (30, 0.15), (50, 0.2), (100, 0.2), (128, None)])
def test_lists_continuous_exact(max_nn, radius):
    from sgaligner_amd.utils import features as F
    p = _surface(600)[0]
    got = _host(F.neighbour_lists(_dev(p), [0, 600], radius, max_nn))
    _assert_lists_equal(got, _surface_lists(600, radius, max_nn), max_nn)


def test_lists_edge_cases():
    from sgaligner_amd.utils import features as F
    a, b = PR.lattice(70, 1), _surface(65)[0]
    nan_cloud = PR.lattice(40, 2)
    nan_cloud[17] = [np.nan, 0.0, 0.0]
    small = PR.lattice(5, 3)
    clouds = [a, np.zeros((0, 3)), b, nan_cloud, small]
    pts, off = _pack(clouds)
    for radius, max_nn in ((None, 30), (0.3, 16)):
        got = _host(F.neighbour_lists(_dev(pts), off, radius, max_nn))
        _assert_lists_equal(got, PR.lists_ref_packed(clouds, radius, max_nn), max_nn)
        count, idx, _ = got
        lo = off[3]
        assert count[lo + 17] == 0                                                  # the NaN point: an empty list of its own ...
        assert not (idx[lo:off[4]] == 17).any()                                     # ... and it appears in no one's
        if radius is None:
            assert (count[off[4]:] == 5).all()                                      # a cloud smaller than max_nn: everything, no more
        for c, cloud in enumerate(clouds):                                          # a packed call equals per-cloud calls, bit for bit
            if len(cloud) == 0:
                continue
            alone = _host(F.neighbour_lists(_dev(cloud), [0, len(cloud)], radius, max_nn))
            assert all(_same_bits(x, y[off[c]:off[c + 1]]) for x, y in zip(alone, got))
    with pytest.raises(ValueError, match='max_nn must be in'):
        F.neighbour_lists(_dev(a), [0, 70], None, 129)


# ---- 4: normals ----------------------------------------------------------------------------------------------------------------------------
def test_normals_plane_lattices_bitwise():
    from sgaligner_amd.utils import features as F
    px, pz = PR.plane_lattice(0), PR.plane_lattice(2)
    pts, off = _pack([pz, px])
    nr, st = F.estimate_normals_batch(_dev(pts), off, None, 30, viewpoints=np.array([[0.0, 0.0, 5.0], [5.0, 0.0, 0.0]]))
    nr, st = nr.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all()
    assert _same_bits(nr[:81], np.tile([0.0, 0.0, 1.0], (81, 1))) and _same_bits(nr[81:], np.tile([1.0, 0.0, 0.0], (81, 1)))
    # viewpoints on the other side turn them; without a viewpoint the component of largest magnitude is made positive
    nr2, _ = F.estimate_normals_batch(_dev(pts), off, None, 30, viewpoints=np.array([[0.0, 0.0, -5.0], [-5.0, 0.0, 0.0]]))
    assert np.array_equal(nr2.cpu().numpy(), -nr)
    nr3, _ = F.estimate_normals_batch(_dev(pts), off, None, 30)
    assert np.array_equal(nr3.cpu().numpy(), nr)
    lat = PR.lattice(257, 9)
    free = F.estimate_normals(lat, radius=0.3, max_nn=30)
    ref = PR.normals_ref(lat, PR.lists_ref(lat, 0.3, 30))
    ok = (ref['status'] == 0) & ~ref['ill']
    big = np.abs(free).argmax(1)
    assert (free[np.arange(257), big][ok] > 0).all()
    assert np.abs(np.linalg.norm(free, axis=1) - 1.0).max() < 1e-12


@pytest.mark.parametrize('n', [257, 600])
def test_normals_surface(n):
    from sgaligner_amd.utils import features as F
    p = _surface(n)[0]
    vp = np.array([0.5, 0.5, 5.0])
    ref = PR.normals_ref(p, _surface_lists(n, 0.15, 30), vp)
    nr, st = F.estimate_normals_batch(_dev(p), [0, n], 0.15, 30, viewpoints=vp[None])
    nr, st = nr.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, ref['status'])
    use = (ref['status'] == 0) & ~ref['ill'] & ~ref['sign_near']
    excluded = int(((ref['status'] == 0) & ~use).sum())
    cross = np.linalg.norm(np.cross(nr[use], ref['normals'][use]), axis=1)
    dots = (nr[use] * ref['normals'][use]).sum(1)
    print(f'normals n={n}: excluded {excluded}, max |n x n_ref| {cross.max():.3e}, min n.n_ref {dots.min():.6f}')
    assert excluded <= 0.02 * n
    assert cross.max() <= 1e-9 and (dots > 0).all()
    # given lists are used as they are; a single-cloud call through the numpy form gives the same bits
    lists = F.neighbour_lists(_dev(p), [0, n], 0.15, 30)
    again, _ = F.estimate_normals_batch(_dev(p), [0, n], viewpoints=vp[None], lists=lists)
    assert _same_bits(again.cpu().numpy(), nr) and _same_bits(F.estimate_normals(p, 0.15, 30, vp), nr)


def test_normals_too_few_neighbours():
    from sgaligner_amd.utils import features as F
    p = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [5.0, 5.0, 5.0], [1.0, 0.0, 0.0], [1.0, 0.01, 0.0], [1.0, 0.0, 0.01], [1.01, 0.01, 0.0]])
    nr, st = F.estimate_normals_batch(_dev(p), [0, 7], 0.1, 30, viewpoints=np.array([[0.0, 0.0, -9.0]]))
    nr, st = nr.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [1, 1, 1, 0, 0, 0, 0]
    assert _same_bits(nr[:3], np.tile([0.0, 0.0, 1.0], (3, 1)))                     # not oriented: the viewpoint is below
    assert np.abs(np.linalg.norm(nr[3:], axis=1) - 1.0).max() < 1e-12


# ---- 5-6: SPFH census ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257, 600])
def test_spfh_census_exact(n):
    from sgaligner_amd.utils import features as F
    p, given = _surface(n)
    lists = _surface_lists(n, 0.2, 50)
    want, undecided, pairs = PR.spfh_ref(p, given, lists)
    d_lists = F.neighbour_lists(_dev(p), [0, n], 0.2, 50)
    got = F.spfh_counts(_dev(p), _dev(given), [0, n], d_lists).cpu().numpy()
    print(f'census n={n}: {pairs} pairs, {int(undecided.sum())} undecided points')
    assert got.dtype == np.int32 and got.shape == (n, 33)
    assert undecided.mean() <= 0.01
    assert np.array_equal(got[~undecided], want[~undecided])
    assert (got.reshape(n, 3, 11).sum(2) == np.maximum(lists[0] - 1, 0)[:, None]).all()        # on ALL points


def test_spfh_degenerate_exact():
    from sgaligner_amd.utils import features as F
    line = np.stack([np.arange(70.0) * 0.125, np.zeros(70), np.zeros(70)], axis=1)
    dup = np.tile([[0.25, -0.5, 1.0]], (9, 1))
    one = np.array([[3.0, 3.0, 3.0]])
    pts, off = _pack([line, dup, one])
    normals = np.concatenate([np.tile([1.0, 0.0, 0.0], (70, 1)), np.tile([0.0, 1.0, 0.0], (9, 1)), [[0.0, 0.0, 1.0]]])
    lists = F.neighbour_lists(_dev(pts), off, None, 8)
    got = F.spfh_counts(_dev(pts), _dev(normals), off, lists).cpu().numpy()
    want = np.zeros((80, 33), dtype=np.int32)
    want[:79, [5, 16, 27]] = 7                                                      # m = 8 everywhere but the single point: zeros
    assert np.array_equal(got, want)
    assert np.array_equal(PR.spfh_ref(line, normals[:70], PR.lists_ref(line, None, 8))[0], want[:70])      # and so says the yardstick


# ---- 7: FPFH weighting ---------------------------------------------------------------------------------------------------------------------
def test_fpfh_weighting_bit_equal():
    from sgaligner_amd.utils import features as F
    clouds = [PR.lattice(300, 21), _surface(100)[0], np.array([[0.0, 0.0, 0.0]]), PR.lattice(64, 22) * 4.0]
    pts, off = _pack(clouds)
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 40, (len(pts), 33)).astype(np.int32)
    for radius, max_nn in ((0.13, 20), (0.3, 100), (None, 7)):
        ref_lists = PR.lists_ref_packed(clouds, radius, max_nn)
        assert (ref_lists[2][:, 1:][np.arange(1, max_nn)[None, :] < ref_lists[0][:, None]] == 0).any()     # d2 == 0 entries past entry 0
        assert (ref_lists[0] <= 1).any()                                                                     # points with m <= 1
        want = PR.fpfh_ref_packed(counts, ref_lists, off)
        lists = F.neighbour_lists(_dev(pts), off, radius, max_nn)
        out32, out64 = F.fpfh_from_counts(_dev(counts), lists, want_f64=True)
        out32, out64 = out32.cpu().numpy(), out64.cpu().numpy()
        assert out64.shape == (len(pts), 33) and out32.shape == (len(pts), 36) and out32.dtype == np.float32
        assert _same_bits(out64, want)
        assert _same_bits(out32[:, :33], want.astype(np.float32))
        assert (out32[:, 33:] == 0).all()
        only32 = F.fpfh_from_counts(_dev(counts), lists)
        assert _same_bits(only32.cpu().numpy(), out32)


# ---- 8: composition ------------------------------------------------------------------------------------------------------------------------
def test_composition_bitwise():
    from sgaligner_amd.utils import features as F
    clouds = [_surface(257)[0], PR.lattice(65, 31), _surface(65)[0] + 2.0, np.zeros((0, 3)), _surface(600)[0][:40]]
    pts, off = _pack(clouds)
    vp = np.array([0.5, 0.5, 5.0])
    vps = np.tile(vp, (len(clouds), 1))
    d_pts = _dev(pts)
    whole = F.fpfh_batch(d_pts, off, None, 0.15, 30, 0.2, 100, vps).cpu().numpy()
    ln = F.neighbour_lists(d_pts, off, 0.15, 30)
    nr, _ = F.estimate_normals_batch(d_pts, off, viewpoints=vps, lists=ln)
    lf = F.neighbour_lists(d_pts, off, 0.2, 100)
    apart = F.fpfh_from_counts(F.spfh_counts(d_pts, nr, off, lf), lf, offsets=off).cpu().numpy()
    assert whole.shape == (len(pts), 36) and _same_bits(whole, apart)
    assert _same_bits(F.fpfh_batch(d_pts, off, nr, None, 30, 0.2, 100).cpu().numpy(), whole)            # given normals
    desc = F.FPFHDescriptor(radius_normal=0.15, radius_feature=0.2, viewpoint=vp)
    many = desc.many(clouds)
    assert [m.shape for m in many] == [(len(c), 33) for c in clouds] and all(m.dtype == np.float32 for m in many)
    for c, cloud in enumerate(clouds):
        assert _same_bits(many[c], whole[off[c]:off[c + 1], :33])
        assert _same_bits(desc(cloud), many[c])


# ---- 9: end to end -------------------------------------------------------------------------------------------------------------------------
def test_registration_from_fpfh_end_to_end():
    from sgaligner_amd.registration_evaluator import FeatureMatcher, RegistrationEvaluator
    from sgaligner_amd.utils import registration as RG
    from sgaligner_amd.utils.features import FPFHDescriptor
    src, ref, T, vp, perm = PR.planted_pair()
    ids = np.where(src[:, 0] < 0.5, 1, 2)                               # two objects: the halves of the surface
    moved = src @ T[:3, :3].T + T[:3, 3]
    ev = RegistrationEvaluator(FeatureMatcher(FPFHDescriptor(radius_normal=0.15, radius_feature=0.2, viewpoint=vp)), ransac_threshold=0.03)
    d = {'src_points': src, 'ref_points': ref, 'gt_transform': T, 'raw_points': ref, 'node_corrs': [(1, 11), (2, 12)],
         'src_plydata': {'objectId': ids}, 'ref_plydata': {'objectId': ids[perm] + 10},
         'gt_src_corr_points': src[::4], 'gt_ref_corr_points': moved[::4]}
    est, score = ev.run_normal_registration(d, evaluate_registration=False)
    rre, rte = RG.compute_registration_error(T, est)
    print(f'end to end: RRE {rre:.4f} deg, RTE {rte:.5f}, mean score {score:.4f}')
    assert rte < 0.03 and rre < 3.5
    normal, aligner = ev.run_registration(d)
    for res in (normal, aligner):
        assert set(res) == set(RegistrationEvaluator.RESULT_KEYS) and len(res) == 6
        assert res['RTE'] < 0.03 and res['RRE'] < 3.5
