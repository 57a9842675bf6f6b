"""GPU tier of the exact nearest-neighbour search.  Every comparison is exact: indices are integers and the distances are correctly
rounded fp64 values of a fixed arithmetic order (tests/nn_ref.py, pinned on cKDTree by tests/test_nn_cpu.py) -- there is no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nn_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu

JOBS = ((1, 1), (1, 1000), (63, 65), (257, 1023), (1024, 1025), (5000, 20000), (20000, 5000))
SIZES = (1, 1000, 63, 65, 257, 1023, 1024, 1025, 5000, 20000)           # the clouds the jobs share
PAIRS = ((0, 0), (0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (9, 8))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _clouds(family, seed=3):
    rng = np.random.default_rng(seed)
    clouds = [NR.make_cloud(family, n, rng) for n in SIZES]
    if family == 'scan':                                     # bitwise copies across the clouds of every job: distance exactly 0
        for a, b in PAIRS:
            if a != b:
                k = min(500, SIZES[a] // 2 + 1, SIZES[b])
                clouds[a][rng.choice(SIZES[a], k, replace=False)] = clouds[b][rng.choice(SIZES[b], k, replace=False)]
    return clouds


def _run(clouds, pairs, **kw):
    from sgaligner_amd.utils import point_cloud as PC
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    dist, idx, oo = PC.nearest_neighbor_batch(pts, off, pairs, **kw)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy(), oo


@pytest.mark.parametrize('family', NR.FAMILIES)
def test_batched_jobs_equal_the_yardstick_exactly(family):
    clouds = _clouds(family)
    assert tuple((len(clouds[a]), len(clouds[b])) for a, b in PAIRS) == JOBS
    dist, idx, oo = _run(clouds, PAIRS)
    assert dist.dtype == np.float64 and idx.dtype == np.int32 and oo[-1] == sum(j[0] for j in JOBS) == len(dist)
    for p, (a, b) in enumerate(PAIRS):
        rd, ri = NR.nn_ref(clouds[a], clouds[b])
        gd, gi = dist[oo[p]:oo[p + 1]], idx[oo[p]:oo[p + 1]]
        print(family, JOBS[p], 'dist mismatches', int((_bits(gd) != _bits(rd)).sum()), 'idx mismatches', int((gi != ri).sum()))
        assert np.array_equal(_bits(gd), _bits(rd)), (family, JOBS[p])
        assert np.array_equal(gi, ri), (family, JOBS[p])
    d2, _, _ = _run(clouds, PAIRS, squared=True)
    assert np.array_equal(_bits(np.sqrt(d2)), _bits(dist))


def _tie_case():
    """A 5000-point lattice support in which rows 990..1010 (across the 1000-point chunk boundary) and a few far-apart rows are bitwise
    copies of one point that is the exact nearest neighbour of a block of queries."""
    rng = np.random.default_rng(21)
    s = NR.make_cloud('lattice', 5000, rng)
    special = np.array([7.125, -3.5, 9.0625])                # off the lattice: nothing else is as close to the queries below
    dup = list(range(990, 1011)) + [1999, 2000, 3000, 4999]
    s[dup] = special
    q = NR.make_cloud('lattice', 3000, rng)
    q[:300] = special + rng.integers(-1, 2, size=(300, 3)) * 0.0625
    return q, s, dup


@pytest.mark.parametrize('chunk', (None, 1000, 1 << 20))
def test_ties_go_to_the_lowest_index_in_one_pass_and_split(chunk):
    from sgaligner_amd import _lib
    q, s, dup = _tie_case()
    if chunk == 1000:
        assert _lib.lib().sga_nn_workspace_bytes(len(q), len(s), chunk) == 12 * 5 * len(q)       # really the split form, 5 chunks
    if chunk == 1 << 20:
        assert _lib.lib().sga_nn_workspace_bytes(len(q), len(s), chunk) == 0                      # really one pass
    dist, idx, _ = _run([q, s], [(0, 1)], chunk=chunk)
    rd, ri = NR.nn_ref(q, s)
    assert np.array_equal(_bits(dist), _bits(rd)) and np.array_equal(idx, ri)
    assert (idx[:300] == min(dup)).all()                     # 25 bitwise-equal minima on both sides of a chunk boundary -> the first
    first = {}
    for k, row in enumerate(map(tuple, s)):
        first.setdefault(row, k)
    assert all(first[tuple(s[k])] == k for k in idx)         # never a later copy of a duplicated row


def test_module_attribute_forces_the_split_form():
    from sgaligner_amd.utils import point_cloud as PC
    q, s, dup = _tie_case()
    keep = PC.NN_CHUNK
    try:
        PC.NN_CHUNK = 777
        dist, idx, _ = _run([q, s], [(0, 1)])
    finally:
        PC.NN_CHUNK = keep
    rd, ri = NR.nn_ref(q, s)
    assert np.array_equal(_bits(dist), _bits(rd)) and np.array_equal(idx, ri)


@pytest.mark.parametrize('family', ('gaussian', 'scan'))
def test_large_job_is_bit_equal_to_ckdtree(family):
    from scipy.spatial import cKDTree
    from sgaligner_amd import _lib
    from sgaligner_amd.utils import point_cloud as PC
    n = 200_000
    q, s = NR.make_pair(family, n, n, seed=5)
    chunk = PC._nn_chunk([n], [n])
    assert _lib.lib().sga_nn_workspace_bytes(n, n, chunk) > 0          # takes the split form by default
    dist, idx = PC.get_nearest_neighbor(q, s, return_index=True)
    kd, _ = cKDTree(s).query(q, k=1)
    print(family, 'dist mismatches vs cKDTree', int((_bits(dist) != _bits(kd)).sum()))
    assert np.array_equal(_bits(dist), _bits(kd))
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < n
    d = q - s[idx]
    assert np.array_equal(_bits(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])), _bits(dist))


def test_two_runs_are_bit_identical():
    n = 200_000
    q, s = NR.make_pair('scan', n, n, seed=6)
    a = _run([q, s], [(0, 1)])
    b = _run([q, s], [(0, 1)])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


def test_compute_pcl_overlap():
    from scipy.spatial import cKDTree
    from sgaligner_amd.utils import point_cloud as PC
    rng = np.random.default_rng(8)
    thr = 1e-7
    source = NR.make_cloud('scan', 30000, rng).astype(np.float32)
    shared = rng.choice(30000, 12000, replace=False)
    target = np.concatenate([source[rng.permutation(shared)], NR.make_cloud('scan', 9000, rng).astype(np.float32)])
    ratio, common = PC.compute_pcl_overlap(source, target, thr)
    want = np.flatnonzero(cKDTree(target.astype(np.float64)).query(source.astype(np.float64))[0] <= thr)
    assert ratio == 0.4 and common.dtype == np.int64
    assert np.array_equal(common, want) and np.array_equal(common, np.sort(shared))
    ratio_t, common_t = PC.compute_pcl_overlap(target, source, thr)
    want_t = np.flatnonzero(cKDTree(source.astype(np.float64)).query(target.astype(np.float64))[0] <= thr)
    assert ratio_t == round(12000 / 21000, 4) and np.array_equal(common_t, want_t) and np.array_equal(common_t, np.arange(12000))
    r0, c0 = PC.compute_pcl_overlap(source, source + np.float32(100.0), thr)
    assert r0 == 0.0 and c0.shape == (0,) and c0.dtype == np.int64
    r1, c1 = PC.compute_pcl_overlap(source, source.copy(), thr)
    assert r1 == 1.0 and np.array_equal(c1, np.arange(30000))
    # the batched form over the C(5, 2) pairs of five overlapping subsets == the per-pair calls
    subs = [source[np.sort(rng.choice(30000, m, replace=False))] for m in (9000, 11000, 7000, 12000, 10000)]
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    batched = PC.compute_pcl_overlap_pairs(subs, pairs, thr)
    assert len(batched) == 10
    for (i, j), (r, c) in zip(pairs, batched):
        rs, cs = PC.compute_pcl_overlap(subs[i], subs[j], thr)
        assert r == rs and 0.0 < r < 1.0 and np.array_equal(c, cs) and c.dtype == np.int64


def test_registration_metrics_equal_their_restatement():
    from scipy.spatial import cKDTree
    from sgaligner_amd.utils import registration as RG
    rng = np.random.default_rng(9)
    nn = lambda qq, ss: cKDTree(ss).query(qq, k=1)
    ang = 0.3
    est = np.eye(4)
    est[:3, :3] = [[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]]
    est[:3, 3] = [0.2, -0.1, 0.05]
    gt = np.eye(4)
    src, ref, raw = NR.make_cloud('scan', 4000, rng), NR.make_cloud('scan', 5000, rng), NR.make_cloud('scan', 20000, rng)
    move = lambda p, t: np.matmul(p, t[:3, :3].T) + t[:3, 3]
    want = nn(move(src, est), raw)[0].mean() + nn(ref, move(raw, np.matmul(est, np.linalg.inv(gt))))[0].mean()
    got = RG.compute_modified_chamfer_distance(src, ref, raw, est, gt)
    assert isinstance(float(got), float) and float(got) == float(want)
    # mosaicking: prediction = ground truth with noise and a missing part (continuous data: no ties, so the indices are the tree's too)
    v_gt = NR.make_cloud('gaussian', 6000, rng)
    v_pred = v_gt[:4500] + rng.standard_normal((4500, 3)) * 0.03
    ind, dis = RG.nn_correspondence(v_pred, v_gt)
    kd, ki = nn(v_gt, v_pred)
    assert isinstance(ind, list) and isinstance(dis, list) and len(ind) == len(dis) == 6000
    assert [float(x) for x in dis] == [float(x) for x in kd] and ind == [int(x) for x in ki]
    res = RG.compute_mosaicking_error(v_pred, v_gt, threshold=0.05)
    d1, d2 = nn(v_gt, v_pred)[0], nn(v_pred, v_gt)[0]
    prec, rec = np.mean((d2 < 0.05).astype('float')), np.mean((d1 < 0.05).astype('float'))
    exp = {'prec': prec, 'recall': rec, 'acc': np.mean(d1), 'comp': np.mean(d2), 'fscore': 2 * prec * rec / (prec + rec)}
    assert set(res) == set(exp) and 0.0 < prec < 1.0 and 0.0 < rec < 1.0
    for k in exp:
        assert float(res[k]) == float(exp[k]), k
    a, b = NR.make_cloud('gaussian', 1000, rng), NR.make_cloud('gaussian', 1000, rng) * 0.05
    assert float(RG.compute_inlier_ratio(move(a, est) + b, a, est)) == float(np.mean(np.sqrt(((move(a, est) + b - move(a, est)) ** 2).sum(1)) < 0.1))
    assert float(RG.compute_registration_rmse(move(a, est) + b, a, est)) == float(np.sqrt(((move(a, est) + b - move(a, est)) ** 2).sum() / 1000))


def test_bad_input():
    from sgaligner_amd import ops
    from sgaligner_amd.utils import point_cloud as PC, registration as RG
    pts = torch.zeros((8, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
        PC.nearest_neighbor_batch(pts, [0, 8], [(0, 0)])
    with pytest.raises(RuntimeError, match='float32'):
        PC.nearest_neighbor_batch(pts.float().cuda(), [0, 8], [(0, 0)])
    with pytest.raises(ValueError):
        PC.nearest_neighbor_batch(pts.cuda(), [0, 8], [(0, 1)])
    with pytest.raises(ValueError):
        PC.get_nearest_neighbor(np.zeros((4, 3)), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        PC.compute_pcl_overlap(np.zeros((4, 3)), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        RG.compute_modified_chamfer_distance(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((0, 3)), np.eye(4), np.eye(4))
    assert ops.VALIDATE
    bad = pts.clone()
    bad[3, 1] = float('nan')
    with pytest.raises(RuntimeError, match='NaN'):
        PC.nearest_neighbor_batch(bad.cuda(), [0, 8], [(0, 0)])
    d, i = PC.get_nearest_neighbor(np.zeros((0, 3)), np.ones((5, 3)), return_index=True)
    assert d.shape == (0,) and i.shape == (0,) and d.dtype == np.float64
    # an empty query cloud and an empty support among real jobs: nothing written for the first, (+inf, -1) for the second
    clouds = [np.zeros((0, 3)), np.arange(15.0).reshape(5, 3), np.ones((3, 3))]
    dist, idx, oo = _run(clouds, [(0, 1), (2, 0), (2, 1)])
    assert list(oo) == [0, 0, 3, 6]
    assert np.isposinf(dist[:3]).all() and (idx[:3] == -1).all()
    rd, ri = NR.nn_ref(clouds[2], clouds[1])
    assert np.array_equal(_bits(dist[3:]), _bits(rd)) and np.array_equal(idx[3:], ri)
