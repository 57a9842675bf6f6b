"""GPU tier of csrc/icp.hip.  The cross-cloud grid search: sga_nn_search_grid = sga_nn_search on the numpy-moved points, masked by r2, =
tests/icp_ref.py -- everything compared as bit patterns, over every cell size, radius and transform form.  ICP (sga_icp through
utils.registration): one round and whole runs against the yardstick (SVD Kabsch / numpy.linalg.solve), statuses, a batch against its
jobs alone, evaluate_registration_pairs, and RegistrationEvaluator(refine=...)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fpfh_ref as PR  # noqa: E402
import icp_ref as IR  # noqa: E402
import voxel_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 16
SENT_D, SENT_I = -77.5, -77
RADII = (None, 0.1, 0.25)
FORMS = ('none', 'identity', 'rigid')
# r / 4, r, 4 r (r = 0.1), the whole cloud in one cell, and a cell far too fine for the key: status 2, every query walks the whole support
CELLS = (0.025, 0.1, 0.4, 100.0, 1e-9)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _case():
    """Clouds and jobs of the exact cases.  -> (clouds, pairs, out_offsets [n_pairs], total_queries)."""
    lat = PR.lattice(300, 5)                                             # 0: duplicates and equal distances are dense
    g = (np.arange(-4, 4, dtype=np.float64) + 0.5) / 8.0
    mid = np.stack([a.reshape(-1) for a in np.meshgrid(g, g, g, indexing='ij')], axis=1)      # 1: up to 8 exactly equal minima per query
    copies = np.tile([[0.25, -0.5, 0.125]], (200, 1))                    # 2: more than 64 candidates in one cell
    near = np.array([[0.25, -0.5, 0.125], [0.26, -0.5, 0.125], [0.3, -0.45, 0.2], [0.5, 0.5, 0.5]])                 # 3
    far = np.array([[1000.0, 0.1, 0.0], [-1000.0, 0.0, 0.1], [0.1, 1000.0, 0.0], [0.0, -1000.0, 0.1], [0.1, 0.0, 1000.0],
                    [0.0, 0.1, -1000.0], [1000.0, -1000.0, 1000.0]])     # 4: 1000 away from the box on each of the six sides, and off a corner
    bad_q = PR.surface(40, 2)[0] - 0.4                                   # 5: a query row with a NaN, one with an inf
    bad_q[7] = [np.nan, 0.1, 0.0]
    bad_q[19] = [0.1, -np.inf, 0.0]
    bad_s = PR.lattice(60, 9)                                            # 6: support rows with a NaN and an inf
    bad_s[0] = [0.0, np.nan, 0.0]
    bad_s[33] = [np.inf, 0.0, 0.0]
    empty = np.zeros((0, 3))                                             # 7
    one_a, one_b = np.array([[0.3, -0.2, 0.1]]), np.array([[0.35, -0.2, 0.1]])                                      # 8, 9
    surf = PR.surface(150, 4)[0] - 0.5                                   # 10: general position, partly outside the lattice's box
    clouds = [lat, mid, copies, near, far, bad_q, bad_s, empty, one_a, one_b, surf]
    # descending cloud order first, several jobs on support 0, query = support, empty query, empty support, one-point clouds
    pairs = [(10, 6), (10, 0), (8, 9), (9, 8), (8, 0), (1, 8), (7, 0), (1, 7), (7, 7), (5, 6), (5, 0), (4, 0), (4, 2), (4, 6), (3, 2), (1, 2),
             (1, 0), (1, 6), (0, 0), (6, 6), (2, 2), (0, 10)]
    nq = np.array([len(clouds[q]) for q, _ in pairs])
    order = np.random.default_rng(3).permutation(len(pairs))             # permuted out_offsets: job order[k] owns the k-th output segment
    oo = np.zeros(len(pairs), dtype=np.int64)
    oo[order] = np.concatenate([[0], np.cumsum(nq[order])])[:-1]
    return clouds, pairs, oo, int(nq.sum())


def _transforms(form, n_pairs):
    if form == 'none':
        return None
    if form == 'identity':
        return np.tile(IR.IDENTITY12, (n_pairs, 1))
    return np.stack([IR.rigid12([1.0, 2.0 - 0.1 * p, -1.0], 5.0 + 3.0 * p, [0.03, -0.02 + 0.004 * p, 0.05]) for p in range(n_pairs)])


@functools.lru_cache(maxsize=None)
def _reference(form):
    """The unmasked yardstick of every job, laid out by out_offsets: (d2 [total], idx [total]) -- computed once, masked per radius."""
    clouds, pairs, oo, total = _case()
    tr = _transforms(form, len(pairs))
    d2, idx = np.full(total, np.nan), np.zeros(total, dtype=np.int64)
    for p, (q, s) in enumerate(pairs):
        a, b = IR.nn_moved_ref(clouds[q], clouds[s], None if tr is None else tr[p])
        d2[oo[p]:oo[p] + len(a)], idx[oo[p]:oo[p] + len(a)] = a, b
    d2.setflags(write=False)
    idx.setflags(write=False)
    return d2, idx


def _brute(form):
    """sga_nn_search on the numpy-moved points: job p's moved queries and its support as clouds 2p, 2p + 1 of a fresh packed call."""
    from sgaligner_amd import ops
    from sgaligner_amd.utils import point_cloud as PC
    clouds, pairs, oo, total = _case()
    tr = _transforms(form, len(pairs))
    cl = []
    for p, (q, s) in enumerate(pairs):
        cl += [IR.move(clouds[q], None if tr is None else tr[p]), clouds[s]]
    off = np.concatenate([[0], np.cumsum([len(c) for c in cl])])
    was, ops.VALIDATE = ops.VALIDATE, False                             # the NaN and inf rows are the case
    try:
        d, i, bo = PC.nearest_neighbor_batch(_dev(np.concatenate(cl)), off, [(2 * p, 2 * p + 1) for p in range(len(pairs))], squared=True)
    finally:
        ops.VALIDATE = was
    d, i = d.cpu().numpy(), i.cpu().numpy()
    d2, idx = np.full(total, np.nan), np.zeros(total, dtype=np.int64)
    for p in range(len(pairs)):
        n = bo[p + 1] - bo[p]
        d2[oo[p]:oo[p] + n], idx[oo[p]:oo[p] + n] = d[bo[p]:bo[p + 1]], i[bo[p]:bo[p + 1]]
    return d2, idx


def _grid_search(pts, off, pairs, oo, total, G, tr, r2, squared=1):
    """The C entry with guard rows round both outputs -> (out_dist, out_idx) host arrays of the total_queries rows."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    from sgaligner_amd.packed import upload
    h_off, h_pr, h_oo = np.asarray(off, dtype=np.int32), np.asarray(pairs, dtype=np.int32).reshape(-1, 2), np.asarray(oo, dtype=np.int32)
    d_off, d_pr, d_oo = upload([h_off, h_pr, h_oo], pts.device)
    out_d = torch.full((total + 2 * GUARD,), SENT_D, device=pts.device, dtype=torch.float64)
    out_i = torch.full((total + 2 * GUARD,), SENT_I, device=pts.device, dtype=torch.int32)
    max_q = max([int(h_off[q + 1] - h_off[q]) for q, _ in pairs], default=0)
    rc = _lib.lib().sga_nn_search_grid(_p(pts), _p(d_off), len(h_off) - 1, int(pts.shape[0]), _p(d_pr), len(h_pr), _p(d_oo), total, max_q,
                                       h_off.ctypes.data, h_pr.ctypes.data, _p(G.cell), _p(G.origin), _p(G.dims), _p(G.status), _p(G.order),
                                       _p(G.sorted_keys), _p(tr) if tr is not None else None, r2, squared, _p(out_d[GUARD:]), _p(out_i[GUARD:]),
                                       _stream())
    _lib.check(rc, 'sga_nn_search_grid')
    out_d, out_i = out_d.cpu().numpy(), out_i.cpu().numpy()
    for g in (out_d[:GUARD], out_d[GUARD + total:]):
        assert (g == SENT_D).all()                                       # the guard rows are untouched
    for g in (out_i[:GUARD], out_i[GUARD + total:]):
        assert (g == SENT_I).all()
    return out_d[GUARD:GUARD + total], out_i[GUARD:GUARD + total]


@pytest.mark.parametrize('form', FORMS)
def test_grid_equals_brute_equals_yardstick_bitwise(form):
    from sgaligner_amd.utils import voxel as V
    clouds, pairs, oo, total = _case()
    ref_d2, ref_idx = _reference(form)
    brute_d2, brute_idx = _brute(form)
    assert (ref_idx >= 0).sum() > 1500 and (ref_idx < 0).sum() > 500      # both outcomes are well represented
    assert _same_bits(brute_d2, ref_d2) and np.array_equal(brute_idx, ref_idx)       # device brute force = numpy, unmasked
    pts = _dev(np.concatenate(clouds))
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    tr = _transforms(form, len(pairs))
    d_tr = None if tr is None else _dev(tr)
    for cell in CELLS:
        G = V.build_grid(pts, off, cell)
        status = VR.voxels_ref(list(clouds), cell)['status']
        assert np.array_equal(G.status.cpu().numpy(), status) and (status == 2).sum() == {0.025: 1, 1e-9: 7}.get(cell, 0)
        for r in RADII:
            r2 = np.inf if r is None else r * r
            want_d2, want_idx = IR.mask_r2(ref_d2, ref_idx, r2)
            got_d2, got_idx = _grid_search(pts, off, pairs, oo, total, G, d_tr, r2)
            assert got_idx.dtype == np.int32 and np.array_equal(got_idx, want_idx), (form, cell, r, np.flatnonzero(got_idx != want_idx)[:8])
            assert _same_bits(got_d2, want_d2), (form, cell, r)
            assert np.isposinf(got_d2[got_idx < 0]).all()
    # squared = 0: the correctly rounded square root of the same d2
    got_d, got_idx = _grid_search(pts, off, pairs, oo, total, G, d_tr, 0.0625, squared=0)
    want_d2, want_idx = IR.mask_r2(ref_d2, ref_idx, 0.0625)
    assert _same_bits(got_d, np.sqrt(want_d2)) and np.array_equal(got_idx, want_idx)


def test_lowest_index_among_equal_minima():
    """The lattice's cell midpoints against the lattice, no transform: where several corners are present they are exactly equally far, and
    the search must name the lowest index among them -- checked against the equalities themselves, not against another search."""
    clouds, pairs, oo, total = _case()
    ref_d2, ref_idx = _reference('none')
    p = pairs.index((1, 0))
    lat, mid = clouds[0], clouds[1]
    d2, idx = ref_d2[oo[p]:oo[p] + len(mid)], ref_idx[oo[p]:oo[p] + len(mid)]
    ties = 0
    for i in range(len(mid)):
        e = lat - mid[i]
        same = np.flatnonzero((e * e).sum(1) == d2[i])
        ties += len(same) > 1
        assert idx[i] == same.min()
    assert ties > 100


@pytest.mark.parametrize('radius', [None, 0.02])
def test_surfaces_device_grid_against_device_brute(radius):
    """Surfaces of 2 000 x 2 300 points through the Python layer: both directions, moved by a transform, default and given cells."""
    from sgaligner_amd.utils import point_cloud as PC
    a, b = PR.surface(2000, 11, bump=True)[0], PR.surface(2300, 12, bump=True)[0]
    tr = np.stack([IR.rigid12([0.2, -0.1, 1.0], 3.0, [0.02, -0.01, 0.015]), IR.rigid12([0.0, 0.0, 1.0], -4.0, [0.0, 0.01, 0.0])])
    pairs = [(0, 1), (1, 0)]
    pts, off = _dev(np.concatenate([a, b])), [0, 2000, 4300]
    moved = [IR.move(a, tr[0]), b, IR.move(b, tr[1]), a]
    bd, bi, bo = PC.nearest_neighbor_batch(_dev(np.concatenate(moved)), np.concatenate([[0], np.cumsum([len(c) for c in moved])]), [(0, 1), (2, 3)],
                                           squared=True)
    bd, bi = bd.cpu().numpy(), bi.cpu().numpy()
    if radius is not None:
        keep = bd <= radius * radius
        assert 100 < keep.sum() < len(keep) - 100                        # the radius cuts through the case
        bd, bi = IR.mask_r2(bd, bi, radius * radius)
    for cell in (None, 0.013, [0.2, 0.031]):
        gd, gi, go = PC.nearest_neighbor_batch(pts, off, pairs, squared=True, search='grid', radius=radius, transforms=_dev(tr), cell=cell)
        assert np.array_equal(go, bo) and gd.dtype == torch.float64 and gi.dtype == torch.int32
        assert np.array_equal(gi.cpu().numpy(), bi) and _same_bits(gd.cpu().numpy(), bd)


# ---- sga_icp --------------------------------------------------------------------------------------------------------------------------------
def _icp(pairs, starts, method, max_iters, normals=None, max_distance=IR.MAX_DISTANCE, **kw):
    from sgaligner_amd.utils import registration as RG
    return RG.icp_pairs(pairs, [IR.matrix44(s) for s in starts], max_distance, ('point', 'plane')[method],
                        None if method == 0 else normals, max_iters, **kw)


def _moved_gap(a12, b12, pts):
    """The largest distance between where two models move the points."""
    return float(np.linalg.norm(IR.move(pts, a12) - IR.move(pts, b12), axis=1).max()) if len(pts) else 0.0


def _model(res):
    T = res['transformation']
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


@functools.lru_cache(maxsize=None)
def _whole_ref(sizes, method):
    c = IR.surface_case(*sizes)
    return c, IR.icp_ref(c['src'], c['ref'], c['start'], IR.MAX_DISTANCE, method, c['normals'], 30)


@pytest.mark.parametrize('shift', [0.0, 1000.0])
@pytest.mark.parametrize('method', [0, 1])
def test_one_round_from_a_given_transform(method, shift):
    """Evaluation 0 is taken from the given transform's very bits: its correspondence set, count and fitness are exact, sum d2 and rmse
    within the fp64 summation bound.  The update moves the query points to within tau = 1e-7 max_distance of where the yardstick's update
    (Kabsch / linalg.solve on the same correspondence set) moves them -- the rule of the RANSAC refit tests, for the same reason: two
    solvers of one least-squares problem agree to rounding times conditioning, not to the bit."""
    c = IR.surface_case(600, 700, 3.0, shift)
    ev = _icp([(c['src'], c['ref'])], [c['start']], method, 0, [c['normals']])[0]
    want = IR.icp_ref(c['src'], c['ref'], c['start'], IR.MAX_DISTANCE, method, c['normals'], 0)
    has = want['idx'] >= 0
    assert ev['iterations'] == 0 and ev['status'] == 0 and np.array_equal(_model(ev), c['start'])
    assert np.array_equal(ev['correspondence_set'], np.stack([np.flatnonzero(has), want['idx'][has]], axis=1))
    assert ev['fitness'] == want['fitness'] and 0.5 < ev['fitness'] < 1.0
    sd2, cnt = want['sums'][0]
    # n terms in any order: |error| <= n 2^-53 sum |term| each; the quotient, the root and squaring it back add a few roundings
    got_sd2 = ev['inlier_rmse'] ** 2 * cnt
    assert abs(got_sd2 - sd2) <= (2 * cnt + 8) * 2.0 ** -53 * sd2
    assert abs(ev['inlier_rmse'] - want['rmse']) <= (cnt + 4) * 2.0 ** -53 * want['rmse']
    one = _icp([(c['src'], c['ref'])], [c['start']], method, 1, [c['normals']])[0]
    assert one['iterations'] == 1 and one['status'] == 0 and len(one['trace']) == 2
    assert one['trace'][0, 0] == want['fitness'] and one['trace'][0, 1] == ev['inlier_rmse']
    U = IR.update12(method, IR.move(c['src'], c['start']), c['ref'], want['idx'], c['normals'], IR.box_min(c['ref']))
    gap = _moved_gap(_model(one), IR.compose12(U, c['start']), c['src'])
    print(f'one round, method {method}, shift {shift}: update differs from the yardstick by {gap:.3e} on the moved points (tau {IR.TAU:.1e})')
    assert gap <= IR.TAU
    rre0, rre1 = IR.rre_rte(c['truth'], c['start'])[0], IR.rre_rte(c['truth'], _model(one))[0]
    assert rre1 < rre0                                                   # and it is a step towards the truth


def test_status_1_and_status_2():
    two = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    ref = PR.surface(50, 3)[0]
    r = _icp([(two, two + 0.001)], [IR.IDENTITY12], 0, 1)[0]
    assert r['status'] == 1 and r['iterations'] == 0 and r['fitness'] == 1.0 and np.array_equal(r['transformation'], np.eye(4))
    assert len(r['trace']) == 1 and len(r['correspondence_set']) == 2
    nr = np.tile([[0.0, 0.0, 1.0]], (50, 1))
    r = _icp([(ref[:5], ref)], [IR.IDENTITY12], 1, 1, [nr])[0]            # five pairs are too few for six unknowns
    assert r['status'] == 1 and r['fitness'] == 1.0 and r['inlier_rmse'] == 0.0
    plane = PR.plane_lattice(2)                                          # all normals equal: rotation about z and sliding are free
    r = _icp([(plane + [0.0, 0.0, 0.01], plane)], [IR.IDENTITY12], 1, 1, [np.tile([[0.0, 0.0, 1.0]], (81, 1))])[0]
    assert r['status'] == 2 and r['iterations'] == 0 and r['fitness'] == 1.0 and np.array_equal(r['transformation'], np.eye(4))
    assert IR.icp_ref(plane + [0.0, 0.0, 0.01], plane, IR.IDENTITY12, 0.05, 1, np.tile([[0.0, 0.0, 1.0]], (81, 1)), 1)['status'] == 2
    r = _icp([(plane + [0.0, 0.0, 0.01], plane)], [IR.IDENTITY12], 0, 1)[0]          # point-to-point has no such trouble
    assert r['status'] == 0 and r['iterations'] == 1 and r['inlier_rmse'] < 1e-12
    r = _icp([(np.zeros((0, 3)), plane), (plane, np.zeros((0, 3)))], [IR.IDENTITY12] * 2, 0, 2)       # empty clouds
    assert [x['status'] for x in r] == [1, 1] and [x['fitness'] for x in r] == [0.0, 0.0] and all(len(x['correspondence_set']) == 0 for x in r)


@pytest.mark.parametrize('sizes', IR.WHOLE_RUNS)
@pytest.mark.parametrize('method', [0, 1])
def test_whole_runs_against_the_yardstick(method, sizes):
    """30 iterations.  Under the precondition test_icp_cpu.py checks for these very cases -- no query within 2 tau of a decision in any
    iteration -- the fitness trace, the iteration count and the final correspondence set equal the yardstick's EXACTLY, and the final
    transforms agree within tau on the moved points."""
    c, want = _whole_ref(sizes, method)
    got = _icp([(c['src'], c['ref'])], [c['start']], method, 30, [c['normals']])[0]
    gap = _moved_gap(_model(got), want['transform'], c['src'])
    (rre0, rte0), (rre1, rte1) = IR.rre_rte(c['truth'], c['start']), IR.rre_rte(c['truth'], _model(got))
    print(f'{sizes} method {method}: fitness {got["fitness"]:.4f} rmse {got["inlier_rmse"]:.5f} iterations {got["iterations"]} '
          f'RRE {rre0:.2f} -> {rre1:.3f} deg RTE {rte0:.4f} -> {rte1:.4f}; final transform {gap:.3e} from the yardstick on the moved points')
    assert got['status'] == 0 and got['iterations'] == want['iters']
    assert np.array_equal(got['trace'][:, 0], want['trace'][:, 0])
    assert np.abs(got['trace'][:, 1] - want['trace'][:, 1]).max() < 1e-9
    has = want['idx'] >= 0
    assert np.array_equal(got['correspondence_set'], np.stack([np.flatnonzero(has), want['idx'][has]], axis=1))
    assert gap <= IR.TAU
    assert rre1 < rre0 and rte1 < rte0


def _bits(res):
    return [(r['transformation'].tobytes(), r['fitness'], r['inlier_rmse'], r['correspondence_set'].tobytes(), r['iterations'], r['status'],
             r['trace'].tobytes()) for r in res]


def test_batch_equals_single_jobs_bitwise():
    c = IR.surface_case(600, 700, 3.0)
    copy = PR.surface(300, 8)[0]
    two = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    pairs = [(copy, copy.copy()), (c['src'], c['ref']), (two, two + 0.001)]
    starts = [IR.IDENTITY12, c['start'], IR.IDENTITY12]
    for method in (0, 1):
        normals = [PR.surface(300, 8)[1], c['normals'], np.tile([[0.0, 0.0, 1.0]], (2, 1))]
        batch = _icp(pairs, starts, method, 30, normals)
        assert [r['status'] for r in batch] == [0, 0, 1]
        assert batch[0]['iterations'] == 1 and batch[0]['fitness'] == 1.0 and batch[0]['inlier_rmse'] < 1e-12       # aligned: done at k = 1
        assert _bits(batch) == _bits(_icp(pairs, starts, method, 30, normals))                                         # two calls, same bits
        for p in range(3):
            assert _bits([batch[p]]) == _bits(_icp([pairs[p]], [starts[p]], method, 30, [normals[p]])), (method, p)
        # a grid of another cell size changes nothing either
        assert _bits(batch) == _bits(_icp(pairs, starts, method, 30, normals, cell=0.013))


def test_evaluate_registration_pairs_is_icp_with_no_iterations():
    from sgaligner_amd.utils import registration as RG
    c = IR.surface_case(600, 700, 3.0)
    pairs = [(c['src'], c['ref']), (c['ref'], c['src'])]
    T = [IR.matrix44(c['start']), np.linalg.inv(IR.matrix44(c['truth']))]
    ev = RG.evaluate_registration_pairs(pairs, T, 0.05)
    assert _bits(ev) == _bits(RG.icp_pairs(pairs, T, 0.05, max_iters=0))
    for e, t, (s, r) in zip(ev, T, pairs):
        d2, idx = IR.nn_grid_ref(s, r, np.concatenate([t[:3, :3].reshape(9), t[:3, 3]]), 0.0025)
        assert np.array_equal(e['transformation'], t) and e['iterations'] == 0 and e['fitness'] == (idx >= 0).mean()
        assert np.array_equal(e['correspondence_set'][:, 1], idx[idx >= 0])
    one = RG.icp(c['src'], c['ref'], IR.matrix44(c['start']), max_iters=0)
    assert _bits([one]) == _bits(ev[:1])
    # 'plane' without given normals: estimated on the device from the reference clouds, and still a step towards the truth
    est = RG.icp(c['src'], c['ref'], IR.matrix44(c['start']), method='plane', max_iters=30)
    assert est['status'] == 0 and IR.rre_rte(c['truth'], _model(est))[0] < IR.rre_rte(c['truth'], c['start'])[0]


def test_evaluator_refines_the_ransac_transform():
    """planted_pair(6000, 11) through voxels of 0.04 and the grid route (the end-to-end case of the voxel tier).  refine=None is the
    evaluator as it was, bit for bit (RRE 0.17 deg, RTE 0.0017); refine='point' runs ICP from that transform on the clouds the matcher saw,
    and on the whole down-sampled clouds in the aligner runs: RRE / RTE are no larger than without it."""
    from sgaligner_amd.registration_evaluator import FeatureMatcher, RegistrationEvaluator
    from sgaligner_amd.utils import registration as RG
    from sgaligner_amd.utils.features import FPFHDescriptor
    src, ref, T, vp, perm = PR.planted_pair(6000, 11)
    ids = np.where(src[:, 0] < 0.5, 1, 2)
    d = {'src_points': src, 'ref_points': ref, 'gt_transform': T, 'node_corrs': [(1, 11), (2, 12)], 'src_plydata': {'objectId': ids},
         'ref_plydata': {'objectId': ids[perm] + 10}}
    make = lambda **kw: RegistrationEvaluator(FeatureMatcher(FPFHDescriptor(0.15, 30, 0.2, 100, vp, search='grid')), ransac_threshold=0.03,
                                              voxel_size=0.04, **kw)
    plain, _ = make().run_normal_registration(d, evaluate_registration=False)
    same, _ = make(refine=None).run_normal_registration(d, evaluate_registration=False)
    fine, _ = make(refine='point').run_normal_registration(d, evaluate_registration=False)
    assert _same_bits(np.asarray(plain), np.asarray(same))
    (rre0, rte0), (rre1, rte1) = RG.compute_registration_error(T, plain), RG.compute_registration_error(T, fine)
    print(f'evaluator, normal: RRE {rre0:.4f} -> {rre1:.4f} deg, RTE {rte0:.5f} -> {rte1:.5f} with refine=point')
    assert round(rre0, 2) == 0.17 and round(rte0, 4) == 0.0017
    assert rre1 <= rre0 and rte1 <= rte0
    a0, a1 = make().run_aligner_registration(d, False), make(refine='point', refine_distance=0.03).run_aligner_registration(d, False)
    (b0, b0b), (b1, b1b) = make().run_aligner_registration_batch([d, d], False), make(refine='point').run_aligner_registration_batch([d, d], False)
    assert _same_bits(a0, b0) and _same_bits(b0, b0b) and _same_bits(a1, b1) and _same_bits(b1, b1b)      # the batch refines as the single run does
    (rre0, rte0), (rre1, rte1) = RG.compute_registration_error(T, a0), RG.compute_registration_error(T, a1)
    print(f'evaluator, aligner: RRE {rre0:.4f} -> {rre1:.4f} deg, RTE {rte0:.5f} -> {rte1:.5f} with refine=point')
    assert rre1 <= rre0 and rte1 <= rte0
    with pytest.raises(ValueError, match='refine must be None'):
        make(refine='icp')
