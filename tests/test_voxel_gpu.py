"""GPU tier of the voxel grid (csrc/voxel.hip through utils/voxel.py, utils/features.py and registration_evaluator.py).  The grid and
the voxel means are compared bit for bit with the numpy yardstick tests/voxel_ref.py; the grid neighbour lists bit for bit with the brute
lists of sga_knn_lists AND with the yardstick fpfh_ref.lists_ref, for every cell size; the FPFH chain on the grid route bit for bit with
the chain on the brute route.  Open3D is not available: the contract of include/sgaligner_hip.h is what is tested."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fpfh_ref as PR  # noqa: E402
import voxel_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu

LATTICE_SIZES = (1, 2, 63, 64, 65, 257, 700)
CELLS = (0.07, 0.125, 0.25, 0.3, 10.0, None)
GUARD = 16
SENTINEL = -77


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


@functools.lru_cache(maxsize=None)
def _grid_clouds():
    nan_cloud = PR.lattice(40, 2)
    nan_cloud[17] = [np.nan, 0.0, 0.0]
    nan_cloud[30] = [0.0, np.inf, 0.0]
    surf, surf_normals = PR.surface(600, 5)
    clouds = (PR.lattice(700, 3), surf, surf + 1000.0, np.zeros((0, 3)), np.array([[0.3, -0.2, 0.1]]), np.tile([[0.25, -0.5, 1.0]], (40, 1)),
              nan_cloud, PR.lattice(100, 8) * 3.0 - 5.0)
    normals = np.random.default_rng(1).standard_normal((sum(len(c) for c in clouds), 3))
    normals[700:1300] = surf_normals                                   # the given normals of `surface`
    normals[1300:1900] = surf_normals
    return clouds, normals


@functools.lru_cache(maxsize=None)
def _grid_ref(h):
    clouds, normals = _grid_clouds()
    return VR.voxels_ref(clouds, h, normals)


# ---- 1: grid and means ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [0.25, 0.07, 10.0, 1e-4])
def test_grid_and_means_bit_equal(h):
    from sgaligner_amd.utils import voxel as V
    clouds, normals = _grid_clouds()
    pts, off = _pack(clouds)
    want = _grid_ref(h)
    G = V.build_grid(_dev(pts), off, h)
    assert (G.status.cpu().numpy() == 0).all()
    assert _same_bits(G.origin.cpu().numpy(), want['origin'])
    assert _same_bits(G.dims.cpu().numpy(), want['dims'])
    assert _same_bits(G.keys.cpu().numpy(), want['keys'])
    assert _same_bits(G.order.cpu().numpy(), want['order'])
    assert _same_bits(G.sorted_keys.cpu().numpy(), want['sorted_keys'])
    assert _same_bits(G.voxel_of_point.cpu().numpy(), want['voxel_of_point'])
    assert _same_bits(G.voxel_offsets.cpu().numpy(), want['voxel_offsets'])
    n_vox = int(want['voxel_offsets'][-1])
    first = G.voxel_first.cpu().numpy()
    assert _same_bits(first[:n_vox], want['voxel_first']) and first[n_vox] == len(pts)
    if h == 0.25:                                                                   # the bounds alone, and the default cell they feed
        from sgaligner_amd import _lib
        from sgaligner_amd.ops import _p, _stream
        box = torch.full((len(clouds), 6), 7.0, device='cuda', dtype=torch.float64)
        d_off = _dev(off.astype(np.int32))
        _lib.check(_lib.lib().sga_cloud_bounds(_p(_dev(pts)), _p(d_off), len(clouds), len(pts), off.astype(np.int32).ctypes.data, _p(box), 0.0, None, _stream()),
                   'sga_cloud_bounds')
        kept = [c[np.isfinite(c).all(1)] for c in clouds]
        lo = np.array([k.min(0) if len(k) else np.full(3, np.inf) for k in kept])
        hi = np.array([k.max(0) if len(k) else np.full(3, -np.inf) for k in kept])
        assert np.array_equal(box.cpu().numpy(), np.concatenate([lo, hi], axis=1))
        cell = V.default_cell(_dev(pts), off, None, 30).cpu().numpy()
        assert cell.shape == (len(clouds),) and (cell > 0).all() and np.isfinite(cell).all()
        assert cell[3] == 1.0 and cell[4] == 1.0 and cell[5] == 1.0                    # no extent: empty, one point, 40 copies of one
        ext = np.sort(hi[1] - lo[1])                                                   # the surface: half a list per cell of the sheet
        assert abs(cell[1] - np.sqrt(ext[2] * ext[1] * 15.0 / 600)) <= 1e-12
        assert (V.default_cell(_dev(pts), off, 0.2, 30).cpu().numpy() == 0.2).all()
    out, voff, out_nr, counts, vop = V.voxel_downsample_batch(_dev(pts), off, h, _dev(normals))
    assert voff.dtype == np.int64 and np.array_equal(voff, want['voxel_offsets'])
    assert _same_bits(counts.cpu().numpy(), want['counts'])
    assert _same_bits(out.cpu().numpy(), want['out_points'])
    assert _same_bits(out_nr.cpu().numpy(), want['out_normals'])
    assert _same_bits(vop.cpu().numpy(), want['voxel_of_point'])
    if h == 10.0:
        assert counts.cpu().numpy()[0] == 700                                       # one lane's 700-term sequential sum
    if h == 1e-4:
        assert voff[2] - voff[1] == 600                                             # every distinct point its own voxel
    no_normals = V.voxel_downsample_batch(_dev(pts), off, h)
    assert no_normals[2] is None and _same_bits(no_normals[0].cpu().numpy(), want['out_points'])
    for c, cloud in enumerate(clouds):                                              # a packed call equals per-cloud calls, bit for bit
        alone = V.voxel_downsample_batch(_dev(cloud), [0, len(cloud)], h, _dev(normals[off[c]:off[c + 1]]))
        a, b = int(voff[c]), int(voff[c + 1])
        assert alone[1].tolist() == [0, b - a]
        assert _same_bits(alone[0].cpu().numpy(), want['out_points'][a:b]) and _same_bits(alone[2].cpu().numpy(), want['out_normals'][a:b])
        assert _same_bits(alone[3].cpu().numpy(), want['counts'][a:b]) and _same_bits(alone[4].cpu().numpy(), want['voxel_of_point'][off[c]:off[c + 1]])
        p1, n1 = (cloud, normals[off[c]:off[c + 1]])
        host = V.voxel_downsample(p1, h, n1)                                        # the reference's signature, numpy in and out
        assert _same_bits(host[0], want['out_points'][a:b]) and _same_bits(host[1], want['out_normals'][a:b])
        assert _same_bits(V.voxel_downsample(p1, h), want['out_points'][a:b])
    per_cloud = V.voxel_downsample_batch(_dev(pts), off, np.full(len(clouds), h))   # one edge per cloud
    assert _same_bits(per_cloud[0].cpu().numpy(), want['out_points'])


# ---- 2: statuses ---------------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, cols=None):
    shape = (n + 2 * GUARD,) if cols is None else (n + 2 * GUARD, cols)
    return torch.full(shape, SENTINEL, device='cuda', dtype=dtype)


def _cells_with_guards(pts, off, keys, order, status):
    """sga_voxel_cells and sga_voxel_downsample through the C ABI on buffers with sentinel-filled guard rows either side -> the interiors
    as numpy arrays; asserts that no guard row was written."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    L = _lib.lib()
    total, n = len(pts), len(off) - 1
    d_pts, d_off, d_keys, d_order = _dev(pts), _dev(off.astype(np.int32)), _dev(keys), _dev(order.astype(np.int32))
    h_off = off.astype(np.int32)
    bufs = dict(sorted_keys=_guarded(total, torch.int64), voxel_of_point=_guarded(total, torch.int32), voxel_offsets=_guarded(n + 1, torch.int32),
                voxel_first=_guarded(total + 1, torch.int32), status=_guarded(n, torch.int32), out_pts=_guarded(total, torch.float64, 3),
                out_count=_guarded(total, torch.int32))
    inner = {k: v[GUARD:len(v) - GUARD] for k, v in bufs.items()}
    inner['status'].copy_(_dev(status.astype(np.int32)))
    ws = torch.empty((L.sga_voxel_workspace_bytes(n, total) // 8,), device='cuda', dtype=torch.float64)
    rc = L.sga_voxel_cells(_p(d_off), n, total, h_off.ctypes.data, _p(d_keys), _p(d_order), _p(inner['sorted_keys']), _p(inner['voxel_of_point']),
                           _p(inner['voxel_offsets']), _p(inner['voxel_first']), _p(inner['status']), _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, 'sga_voxel_cells')
    rc = L.sga_voxel_downsample(_p(d_pts), None, _p(d_off), n, total, h_off.ctypes.data, _p(d_order), _p(inner['sorted_keys']),
                                _p(inner['voxel_offsets']), _p(inner['voxel_first']), _p(inner['status']), _p(inner['out_pts']), None,
                                _p(inner['out_count']), _stream())
    _lib.check(rc, 'sga_voxel_downsample')
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v = v.cpu().numpy()
        assert (v[:GUARD] == SENTINEL).all() and (v[len(v) - GUARD:] == SENTINEL).all(), f'{k}: a guard row was written'
    return {k: v.cpu().numpy() for k, v in inner.items()}


def test_statuses_and_a_bad_order():
    from sgaligner_amd.utils import voxel as V
    unit = PR.surface(200, 9)[0]
    with pytest.raises(ValueError, match=r'cloud 0: the grid is too fine'):
        V.voxel_downsample_batch(_dev(unit), [0, 200], 1e-9)
    with pytest.raises(ValueError, match=r'cloud 1: the grid is too fine'):
        V.voxel_downsample_batch(_dev(np.concatenate([unit, unit])), [0, 200, 400], [0.1, 1e-9])
    with pytest.raises(ValueError, match='must be > 0 and finite'):
        V.voxel_downsample_batch(_dev(unit), [0, 200], 0.0)
    G = V.build_grid(_dev(np.concatenate([unit, unit])), [0, 200, 400], [0.1, 1e-9])     # the fine cloud has no cells, the other is whole
    assert G.status.cpu().numpy().tolist() == [0, 2] and G.dims.cpu().numpy()[1].tolist() == [0, 0, 0]
    alone = VR.voxels_ref([unit], 0.1)
    assert G.voxel_offsets.cpu().numpy().tolist() == [0, alone['voxel_offsets'][1], alone['voxel_offsets'][1]]
    vop = G.voxel_of_point.cpu().numpy()
    assert np.array_equal(vop[:200], alone['voxel_of_point']) and (vop[200:] == -1).all()

    clouds = [PR.lattice(300, 4), PR.surface(150, 6)[0], PR.lattice(65, 7), PR.surface(90, 8)[0], PR.lattice(257, 9)]
    pts, off = _pack(clouds)
    h = 0.125
    want = VR.voxels_ref(clouds, h)
    status0 = np.zeros(len(clouds), dtype=np.int32)
    good = _cells_with_guards(pts, off, want['keys'], want['order'], status0)
    n_vox = int(want['voxel_offsets'][-1])
    assert good['status'].tolist() == [0] * 5 and _same_bits(good['voxel_of_point'], want['voxel_of_point'])
    assert _same_bits(good['out_pts'][:n_vox], want['out_points']) and _same_bits(good['out_count'][:n_vox], want['counts'])
    assert (good['out_count'][n_vox:] == SENTINEL).all()                                # nothing past the voxels of the call

    def spoil(c, how):
        order = want['order'].copy()
        a, b = off[c], off[c + 1]
        if how == 'reversed':
            order[a:b] = order[a:b][::-1]
        elif how == 'duplicated':
            order[a + 5] = order[a + 4]
        elif how == 'other cloud':
            order[a + 3] = off[c + 1]                                                   # a valid row, but of the next cloud
        elif how == 'far outside':
            order[a] = 2 ** 31 - 1
            order[b - 1] = -5
        elif how == 'unstable':                                                         # two members of one voxel swapped: sorted, not stable
            t = a + int(np.flatnonzero(want['sorted_keys'][a:b - 1] == want['sorted_keys'][a + 1:b])[0])
            order[t], order[t + 1] = order[t + 1], order[t]
        return order

    for c, how in ((1, 'reversed'), (2, 'duplicated'), (0, 'other cloud'), (3, 'far outside'), (2, 'unstable')):
        got = _cells_with_guards(pts, off, want['keys'], spoil(c, how), status0)
        assert got['status'].tolist() == [3 if x == c else 0 for x in range(5)], how
        others = np.ones(len(pts), dtype=bool)
        others[off[c]:off[c + 1]] = False
        assert np.array_equal(got['voxel_of_point'][others], want['voxel_of_point'][others]), how
        assert (got['voxel_of_point'][~others] == -1).all(), how
        nv = np.diff(want['voxel_offsets'])
        nv[c] = 0                                                                       # the failed cloud produces nothing
        assert np.array_equal(np.diff(got['voxel_offsets']), nv), how
        for x in range(5):
            if x == c:
                continue
            a, b = got['voxel_offsets'][x], got['voxel_offsets'][x + 1]
            wa, wb = want['voxel_offsets'][x], want['voxel_offsets'][x + 1]
            assert _same_bits(got['out_pts'][a:b], want['out_points'][wa:wb]) and _same_bits(got['out_count'][a:b], want['counts'][wa:wb]), how
            assert np.array_equal(got['voxel_first'][a:b], want['voxel_first'][wa:wb]), how
        assert (got['out_count'][got['voxel_offsets'][-1]:] == SENTINEL).all(), how
    keep2 = _cells_with_guards(pts, off, want['keys'], want['order'], np.array([0, 2, 0, 0, 0]))      # status 2 comes in and stays
    assert keep2['status'].tolist() == [0, 2, 0, 0, 0]


# ---- 3: grid lists -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _list_clouds():
    return tuple(PR.lattice(n, 100 + n) for n in LATTICE_SIZES) + (PR.surface(600, 5)[0],)


@functools.lru_cache(maxsize=None)
def _list_ref(radius, max_nn):
    return PR.lists_ref_packed(_list_clouds(), radius, max_nn)


@pytest.mark.parametrize('radius', [None, 0.1, 0.25])
@pytest.mark.parametrize('max_nn', [1, 30, 128])
def test_grid_lists_equal_brute_and_yardstick(max_nn, radius):
    from sgaligner_amd.utils import features as F
    pts, off = _pack(_list_clouds())
    d_pts = _dev(pts)
    want = _list_ref(radius, max_nn)
    brute = _host(F.neighbour_lists(d_pts, off, radius, max_nn))
    _assert_lists_equal(brute, want, max_nn)
    for cell in CELLS:
        got = _host(F.neighbour_lists(d_pts, off, radius, max_nn, search='grid', cell=cell))
        _assert_lists_equal(got, want, max_nn)
        assert all(_same_bits(x, y) for x, y in zip(got, brute)), cell


@pytest.mark.parametrize('max_nn,radius', [(30, None), (100, 0.2), (128, None)])
def test_grid_lists_surface_2000(max_nn, radius):
    from sgaligner_amd.utils import features as F
    p = PR.surface(2000, 6)[0]
    want = PR.lists_ref(p, radius, max_nn)
    for cell in (0.07, 0.3):
        got = _host(F.neighbour_lists(_dev(p), [0, 2000], radius, max_nn, search='grid', cell=cell))
        _assert_lists_equal(got, want, max_nn)


def test_grid_lists_isolated_points_and_dropped_points():
    """The fallback: a query whose rings stay empty walks its whole cloud; so does a dropped query.  An infinite coordinate gives d2 = +inf,
    which a k-NN list without a radius admits when nothing nearer is left: the grid route must say the same."""
    from sgaligner_amd.utils import features as F
    surf = PR.surface(600, 5)[0]
    outlier = np.concatenate([surf, [[50.0, 50.0, 50.0]]])
    two = np.concatenate([surf[:300], surf[300:] + 100.0])
    for cloud in (outlier, two):
        got = _host(F.neighbour_lists(_dev(cloud), [0, len(cloud)], None, 30, search='grid', cell=0.07))
        _assert_lists_equal(got, PR.lists_ref(cloud, None, 30), 30)
    odd = PR.lattice(40, 2)
    odd[17] = [np.nan, 0.0, 0.0]
    odd[30] = [0.0, np.inf, 0.0]
    clouds = [PR.lattice(70, 1), np.zeros((0, 3)), odd, PR.lattice(5, 3), outlier]
    pts, off = _pack(clouds)
    for radius, max_nn in ((None, 30), (None, 64), (0.3, 16)):
        want = PR.lists_ref_packed(clouds, radius, max_nn)
        brute = _host(F.neighbour_lists(_dev(pts), off, radius, max_nn))
        for cell in (0.07, 0.3, None, [0.07, 0.1, 1e-9, 0.3, 1e-9]):                    # 1e-9: no grid for that cloud (status 2), still exact
            got = _host(F.neighbour_lists(_dev(pts), off, radius, max_nn, search='grid', cell=cell))
            assert all(_same_bits(x, y) for x, y in zip(got, want)), (radius, max_nn, cell)
            assert all(_same_bits(x, y) for x, y in zip(got, brute)), (radius, max_nn, cell)


@pytest.mark.parametrize('max_nn,radius', [(30, None), (100, 0.05)])
def test_grid_lists_20000_points_device_against_device(max_nn, radius):
    from sgaligner_amd.utils import features as F
    d_pts = _dev(PR.surface(20000, 7)[0])
    brute = F.neighbour_lists(d_pts, [0, 20000], radius, max_nn)
    grid = F.neighbour_lists(d_pts, [0, 20000], radius, max_nn, search='grid')
    for x, y in zip(grid, brute):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)


# ---- 4: the FPFH chain on the grid route ---------------------------------------------------------------------------------------------------
def test_fpfh_on_the_grid_route_bitwise():
    from sgaligner_amd.utils import features as F
    surface = lambda n: PR.surface(n, 40 + n)[0]
    clouds = [surface(257), PR.lattice(65, 31), surface(65) + 2.0, np.zeros((0, 3)), surface(600)[:40]]
    pts, off = _pack(clouds)
    vp = np.array([0.5, 0.5, 5.0])
    vps = np.tile(vp, (len(clouds), 1))
    d_pts = _dev(pts)
    brute = F.fpfh_batch(d_pts, off, None, 0.15, 30, 0.2, 100, vps).cpu().numpy()
    for cell in (None, 0.07):
        assert _same_bits(F.fpfh_batch(d_pts, off, None, 0.15, 30, 0.2, 100, vps, search='grid', cell=cell).cpu().numpy(), brute)
    nb, _ = F.estimate_normals_batch(d_pts, off, 0.15, 30, vps)
    ng, _ = F.estimate_normals_batch(d_pts, off, 0.15, 30, vps, search='grid')
    assert _same_bits(ng.cpu().numpy(), nb.cpu().numpy())
    assert _same_bits(F.estimate_normals(clouds[0], 0.15, 30, vp, search='grid'), F.estimate_normals(clouds[0], 0.15, 30, vp))
    many = F.FPFHDescriptor(0.15, 30, 0.2, 100, vp, search='grid').many(clouds)
    for c in range(len(clouds)):
        assert _same_bits(many[c], brute[off[c]:off[c + 1], :33])


# ---- 5: end to end -------------------------------------------------------------------------------------------------------------------------
def test_registration_with_voxels_and_grid_lists_end_to_end():
    """planted_pair(6000, 11) through voxel down-sampling at 0.04 and the grid route.  On the host chain (test_voxel_cpu.py): 956 / 929
    voxels, 460 mutual matches, 270 inliers, RRE 0.376 deg, RTE 0.0006; the device normals (Jacobi) differ from the yardstick's (eigh) in
    the last bits and SPFH has its knife edge, so those figures are the expectation, not a bit pattern."""
    from sgaligner_amd.registration_evaluator import FeatureMatcher, RegistrationEvaluator
    from sgaligner_amd.utils import registration as RG
    from sgaligner_amd.utils.features import FPFHDescriptor
    from sgaligner_amd.utils.voxel import voxel_downsample
    src, ref, T, vp, perm = PR.planted_pair(6000, 11)
    ids = np.where(src[:, 0] < 0.5, 1, 2)                               # two objects: the halves of the surface
    moved = src @ T[:3, :3].T + T[:3, 3]
    ev = RegistrationEvaluator(FeatureMatcher(FPFHDescriptor(0.15, 30, 0.2, 100, vp, search='grid')), ransac_threshold=0.03, voxel_size=0.04)
    d = {'src_points': src, 'ref_points': ref, 'gt_transform': T, 'raw_points': ref, 'node_corrs': [(1, 11), (2, 12)],
         'src_plydata': {'objectId': ids}, 'ref_plydata': {'objectId': ids[perm] + 10},
         'gt_src_corr_points': src[::4], 'gt_ref_corr_points': moved[::4]}
    n_src, n_ref = len(voxel_downsample(src, 0.04)), len(voxel_downsample(ref, 0.04))
    assert (n_src, n_ref) == (len(VR.downsample_ref(src, 0.04)), len(VR.downsample_ref(ref, 0.04)))
    est, score = ev.run_normal_registration(d, evaluate_registration=False)
    rre, rte = RG.compute_registration_error(T, est)
    print(f'end to end with voxels: {n_src} / {n_ref} voxels, RRE {rre:.4f} deg, RTE {rte:.5f}, mean score {score:.4f}')
    assert rte < 0.03 and rre < 3.5
    normal, aligner = ev.run_registration(d)
    for name, res in (('normal', normal), ('aligner', aligner)):
        assert set(res) == set(RegistrationEvaluator.RESULT_KEYS) and len(res) == 6
        print(f'end to end with voxels, {name}: RRE {res["RRE"]:.4f} deg, RTE {res["RTE"]:.5f}')
        assert res['RTE'] < 0.03 and res['RRE'] < 3.5
    # voxel_size=None is the evaluator as it was: the existing planted case gives the same transform with and without the argument
    src, ref, T, vp, perm = PR.planted_pair()
    d = {'src_points': src, 'ref_points': ref, 'gt_transform': T}
    desc = FPFHDescriptor(radius_normal=0.15, radius_feature=0.2, viewpoint=vp)
    before, _ = RegistrationEvaluator(FeatureMatcher(desc), ransac_threshold=0.03).run_normal_registration(d, evaluate_registration=False)
    after, _ = RegistrationEvaluator(FeatureMatcher(desc), ransac_threshold=0.03, voxel_size=None).run_normal_registration(d, evaluate_registration=False)
    assert _same_bits(np.asarray(before), np.asarray(after))
    rre, rte = RG.compute_registration_error(T, before)
    assert rte < 0.03 and rre < 3.5
