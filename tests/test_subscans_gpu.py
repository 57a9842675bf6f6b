"""GPU tier of subscan generation (csrc/visibility.hip).  Every comparison is exact: the masks are bits of a fixed fp64 operation order
(tests/subscan_ref.py, compared with the reference's own NumPy route by tests/test_subscans_cpu.py), the walk and the object counts are
integers -- there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import subscan_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 1000, 4097, 20000)
FS = (1, 2, 7, 33)
_SCANS = {}


def _scan(n, f):
    if (n, f) not in _SCANS:
        _SCANS[(n, f)] = SR.make_scan(n, f, seed=1000 * f + n % 997)
    return _SCANS[(n, f)]


def _layout(sizes, dev='cuda'):
    from sgaligner_amd.utils import point_cloud as PC
    pt_off = np.concatenate([[0], np.cumsum([n for n, _ in sizes])])
    fr_off = np.concatenate([[0], np.cumsum([f for _, f in sizes])])
    return PC.ScanLayout(pt_off, fr_off, int(pt_off[-1]), int(fr_off[-1]), device=dev)


def _rows(words, lay, s):
    """Scan s's [F, W] uint64 words out of the packed array."""
    f, w = int(lay.fr_off[s + 1] - lay.fr_off[s]), int(lay.words[s])
    return words[int(lay.vis_off[s]):int(lay.vis_off[s]) + f * w].reshape(f, w)


def _visibility(pts, w2c, intr):
    """Lists per scan -> (packed uint64 words, layout): one call of the packed form."""
    from sgaligner_amd.utils import point_cloud as PC
    lay = _layout([(len(p), len(m)) for p, m in zip(pts, w2c)])
    cat = lambda parts, shape, dt: torch.from_numpy(np.concatenate(parts).reshape(shape).astype(dt)).cuda()
    vis, vis_off = PC.visible_masks_batch(cat(pts, (-1, 3), np.float32), lay.pt_off, cat(w2c, (-1, 12), np.float64), lay.fr_off,
                                          torch.from_numpy(np.stack(intr)).cuda())
    torch.cuda.synchronize()
    assert vis.dtype == torch.int64 and vis.numel() == lay.total_words and np.array_equal(vis_off, lay.vis_off)
    return vis.cpu().numpy().view(np.uint64), lay


def _check_scan(words, lay, s, scan, tag):
    w2c, intr, masks = SR.projected(scan)
    got, want = _rows(words, lay, s), SR.pack_bits(masks)
    print(tag, 'visible share', round(float(masks.mean()), 4) if masks.size else 0.0, 'word mismatches', int((got != want).sum()))
    assert got.shape == want.shape and np.array_equal(got, want), tag
    n = masks.shape[1]
    if n % 64:
        assert not (got[:, -1] >> np.uint64(n % 64)).any(), tag                       # padding bits of the last word are 0


@pytest.mark.parametrize('f', FS)
@pytest.mark.parametrize('n', NS)
def test_masks_equal_the_yardstick_word_for_word(n, f):
    scan = _scan(n, f)
    w2c, intr, _ = SR.projected(scan)
    words, lay = _visibility([scan['pts']], [w2c], [intr])
    _check_scan(words, lay, 0, scan, (n, f))


def test_masks_of_a_mixed_batch_in_one_call():
    scans = [_scan(n, f) for n in NS for f in FS]
    proj = [SR.projected(s) for s in scans]
    words, lay = _visibility([s['pts'] for s in scans], [p[0] for p in proj], [p[1] for p in proj])
    assert lay.n_scans == len(NS) * len(FS)
    for i, s in enumerate(scans):
        _check_scan(words, lay, i, s, ('batch', i))


def test_masks_of_a_mid_size_scan():
    scan = SR.make_scan(50_000, 40, seed=77)
    w2c, intr, masks = SR.projected(scan)
    assert masks.any(1).sum() >= 30 and 0.03 < masks.mean() < 0.5
    words, lay = _visibility([scan['pts']], [w2c], [intr])
    _check_scan(words, lay, 0, scan, (50_000, 40))


def test_exact_edges_nan_and_the_swapped_bounds():
    """Identity pose, fx = fy = 512, cx = cy = 256, u_max = height = 768, v_max = width = 1024, points at depth 1: u = 512 x + 256 and
    v = 512 y + 256 are exact, so a point ON a frustum edge is on it in the arithmetic too."""
    f32 = np.float32
    up, down = (lambda a: np.nextafter(f32(a), f32(np.inf))), (lambda a: np.nextafter(f32(a), f32(-np.inf)))
    cases = [((0.0, 0.0, 1.0), True),                         # the image centre
             ((-0.5, 0.0, 1.0), True), ((down(-0.5), 0.0, 1.0), False),              # u = 0 | one step beyond
             ((1.0, 0.0, 1.0), True), ((up(1.0), 0.0, 1.0), False),                  # u = u_max = 768
             ((0.0, -0.5, 1.0), True), ((0.0, down(-0.5), 1.0), False),              # v = 0
             ((0.0, 1.5, 1.0), True), ((0.0, up(1.5), 1.0), False),                  # v = v_max = 1024
             ((-0.5, -0.5, 1.0), True), ((1.0, 1.5, 1.0), True),                     # two corners
             ((0.0, 0.0, 0.0), False), ((0.0, 0.0, -1e-30), False), ((0.0, 0.0, -1.0), False),      # Z = 0, slightly negative, behind
             ((np.nan, 0.0, 1.0), False), ((0.0, np.nan, 1.0), False), ((0.0, 0.0, np.nan), False),
             ((np.inf, 0.0, 1.0), False), ((0.0, 0.0, np.inf), False),               # infinite coordinates: inf * 0 in the other rows is NaN
             ((1.2578125, 0.0, 1.0), False),                  # u = 900 in (u_max, v_max]: invisible
             ((0.0, 1.2578125, 1.0), True)]                   # v = 900 in the same range: visible -- the reference's swapped bounds
    cases = cases + cases[:50]                                # 42 points ...
    cases = (cases * 4)[:130]                                 # ... repeated over three words, the last one partial
    pts = np.array([c[0] for c in cases], dtype=np.float32)
    want = np.array([c[1] for c in cases])
    ident = np.eye(4)[:3].reshape(12)
    bad = ident.copy()
    bad[7] = np.nan                                           # a NaN in the pose: the frame sees nothing
    shifted = ident.copy()
    shifted[11] = -1.0                                        # camera one unit further along +z: every depth-1 point lands on Z = 0
    w2c = np.stack([ident, bad, shifted, ident])
    info = SR.make_intrinsics(512.0, 512.0, 256.0, 256.0, width=1024.0, height=768.0)
    intr = SR.intr_row(info)
    assert intr.tolist() == [512.0, 512.0, 256.0, 256.0, 768.0, 1024.0]
    ref = SR.visible_ref(pts, w2c, intr)
    assert np.array_equal(ref[0], want) and np.array_equal(ref[3], want) and not ref[1].any()          # the yardstick itself gets the edges right
    assert not ref[2][np.array([c[0][2] == 1.0 for c in cases])].any()
    words, lay = _visibility([pts], [w2c], [intr])
    got = _rows(words, lay, 0)
    assert np.array_equal(got, SR.pack_bits(ref))
    from sgaligner_amd.utils import point_cloud as PC
    assert np.array_equal(PC.unpack_mask_words(got, len(pts))[0], want)
    # the same through the reference signature, which derives u_max / v_max from the intrinsics dict
    assert np.array_equal(PC.get_visible_pts_from_cam_pose(pts, np.eye(4), info), want)


def _walk(case_masks, budgets, in_place):
    """Yardstick masks (bool [F, N] per scan) packed and uploaded -> (per-scan walk results, vis words after, cum words, layout)."""
    from sgaligner_amd.preprocessing import subscans as SS
    lay = _layout([(m.shape[1], m.shape[0]) for m in case_masks])
    packed = np.concatenate([SR.pack_bits(m).reshape(-1) for m in case_masks] + [np.zeros(0, dtype=np.uint64)])
    vis = torch.from_numpy(packed.view(np.int64)).cuda()
    cum, out = SS.subscan_walk_batch(vis, lay, torch.tensor(budgets, dtype=torch.int32).cuda(), in_place=in_place)
    torch.cuda.synchronize()
    assert (cum.data_ptr() == vis.data_ptr()) == in_place
    return SS.split_walk_output(out.cpu().numpy(), lay), vis.cpu().numpy().view(np.uint64), cum.cpu().numpy().view(np.uint64), lay, packed


@pytest.mark.parametrize('in_place', (True, False))
def test_walk_equals_the_yardstick(in_place):
    cases = SR.walk_cases()
    big = cases[2]['masks']
    n_big = big.shape[1]
    masks = [c['masks'] for c in cases] + [cases[0]['masks'][:1],            # F = 1
                                           cases[1]['masks'],                # max_pts = 0: every frame closes, the blind one included
                                           big,                              # a budget never reached: no subscan
                                           np.zeros((3, 0), dtype=bool),     # an empty scan inside the batch
                                           np.zeros((0, 100), dtype=bool),   # a frameless scan inside the batch
                                           big[:7]]                          # one frame's own count as the budget
    budgets = [c['max_pts'] for c in cases] + [1, 0, n_big + 1, 5, 5, int(big[0].sum())]
    res, vis_after, cum, lay, packed = _walk(masks, budgets, in_place)
    if not in_place:
        assert np.array_equal(vis_after, packed)                             # the input matrix is left alone
    for s, (m, b) in enumerate(zip(masks, budgets)):
        seg_end, seg_count, frame_count = res[s]
        if m.shape[0] == 0 or m.shape[1] == 0:
            assert len(seg_end) == 0 and len(seg_count) == 0
            continue
        ref = SR.walk_ref(m, b)
        print('scan', s, m.shape, 'budget', b, 'subscans', ref['n_seg'], 'device', len(seg_end))
        assert len(seg_end) == ref['n_seg']
        assert np.array_equal(seg_end, ref['seg_end']) and np.array_equal(seg_count, ref['seg_count'])
        assert np.array_equal(frame_count, ref['frame_count'])
        assert np.array_equal(_rows(cum, lay, s), SR.pack_bits(ref['cum']))
        assert np.array_equal(_rows(cum, lay, s)[seg_end], SR.pack_bits(ref['seg_masks']))
    assert len(res[3][0]) == int(masks[3].sum() >= 1)                        # F = 1
    assert np.array_equal(res[4][0], np.arange(masks[4].shape[0])) and 0 in res[4][1]
    assert len(res[5][0]) == 0
    assert res[8][0][0] == 0 and res[8][1][0] == budgets[8]                  # met exactly by the first frame
    assert (res[1][1] == budgets[1]).any()                                   # the exact budget of the walk cases


@pytest.mark.parametrize('which', ('one', 'some', 'lds_bound', 'above_lds_bound'))
def test_object_counts_equal_bincount(which):
    from sgaligner_amd.preprocessing import subscans as SS
    bound = SS.object_count_lds_slots()
    n_slots = {'one': 1, 'some': 37, 'lds_bound': bound, 'above_lds_bound': bound + 1}[which]
    cases = SR.walk_cases()[1:]                                               # 4097 and 20000 points
    assert sum(c['masks'].shape[1] for c in cases) > n_slots
    rng = np.random.default_rng(n_slots)
    pool = (np.arange(n_slots) - n_slots // 2).astype(np.int16)               # negative ids included
    sizes = [c['masks'].shape[1] for c in cases]
    object_id = pool[rng.integers(0, n_slots, sum(sizes))]
    object_id[:n_slots] = pool                                                # every id occurs
    ids, slot = np.unique(object_id, return_inverse=True)
    assert len(ids) == n_slots and (ids[0] < 0 or n_slots == 1) and object_id.dtype == np.int16
    masks = [SR.walk_ref(c['masks'], c['max_pts'])['cum'] for c in cases]
    lay = _layout([(m.shape[1], m.shape[0]) for m in masks])
    bits = torch.from_numpy(np.concatenate([SR.pack_bits(m).reshape(-1) for m in masks]).view(np.int64)).cuda()
    rows = [(0, 0), (1, 39), (0, 32), (1, 5), (0, 5), (1, 17), (1, 17)]       # first and last rows, the blind frame, a repeated row
    counts = SS.object_counts_batch(bits, lay, rows, torch.from_numpy(slot.astype(np.int32)).cuda(), n_slots)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    assert counts.shape == (len(rows), n_slots) and counts.dtype == np.int32
    for r, (s, f) in enumerate(rows):
        want = np.bincount(slot[lay.pt_off[s]:lay.pt_off[s + 1]][masks[s][f]], minlength=n_slots)
        assert np.array_equal(counts[r], want), (which, r)
        assert counts[r].sum() == masks[s][f].sum()
    assert counts[1].sum() > 0 and counts[3].sum() >= 0


def _annotated_scan():
    scan = SR.make_scan(20000, 40, seed=31, blind=(4,))
    n = len(scan['pts'])
    rng = np.random.default_rng(5)
    ply = np.zeros(n, dtype=[('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('objectId', 'i4'),
                             ('globalId', 'i4'), ('NYU40', 'u1'), ('Eigen13', 'u1'), ('RIO27', 'u1')])
    ply['x'], ply['y'], ply['z'] = scan['pts'].T
    for k in ('red', 'green', 'blue', 'NYU40', 'Eigen13', 'RIO27'):
        ply[k] = rng.integers(0, 256, n)
    ply['objectId'] = scan['object_id']
    ply['globalId'] = scan['object_id'].astype(np.int32) * 7
    ids = np.unique(scan['object_id']).tolist()
    objects = [{'id': str(i), 'label': 'object %d' % i, 'attributes': {'n': [i]}} for i in ids + [99]]      # 99 has no vertex at all
    rels = [[a, b, (a + b) % 5, 'rel %d' % ((a + b) % 5)] for a in ids for b in ids if a != b and (a * 3 + b) % 4 == 0] + [[1, 99, 2, 'rel 2']]
    return scan, ply, objects, rels


def _subscans_restated(scan, ply, objects, rels, max_pts, min_obj_points, scan_id):
    """SubGenScan3R.__getitem__ + gen_scene_graph + scan3r.create_ply_data, restated on the yardstick masks."""
    _, _, frame_masks = SR.projected(scan)
    scene_pts = np.stack((ply['x'], ply['y'], ply['z'])).transpose()
    curr = np.zeros(scene_pts.shape[0]).astype('bool')
    out = []
    for frame_cnt in range(len(frame_masks)):
        curr = np.logical_or(frame_masks[frame_cnt], curr)
        if scene_pts[curr].shape[0] >= max_pts:
            subscan_id = '{}_{}'.format(scan_id, len(out))
            idx = np.where(curr)[0]
            pcl = np.empty(len(idx), dtype=[('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('objectId', 'h'),
                                            ('globalId', 'h'), ('NYU40', 'u1'), ('Eigen13', 'u1'), ('RIO27', 'u1')])
            for name in pcl.dtype.names:
                pcl[name] = ply[name][idx].astype(pcl.dtype[name])
            visible_ids = ply['objectId'][idx]
            uniq = np.unique(visible_ids)
            sub_obj = [o for o in objects if int(o['id']) in uniq]
            sub_rel = []
            for (sub_id, ob_id, rel_id, rel_name) in rels:
                if len(np.where(visible_ids == int(sub_id))[0]) > min_obj_points and len(np.where(visible_ids == int(ob_id))[0]) > min_obj_points:
                    sub_rel.append([sub_id, ob_id, rel_id, rel_name])
            out.append({'pcl': pcl, 'subscan_id': subscan_id, 'relationships': {'relationships': sub_rel, 'scan': subscan_id},
                        'objects': {'scan': subscan_id, 'objects': sub_obj}})
            curr = np.zeros(scene_pts.shape[0]).astype('bool')
    return out


def test_generate_subscans_equals_the_restated_reference():
    from sgaligner_amd.preprocessing import subscans as SS
    scan, ply, objects, rels = _annotated_scan()
    max_pts = int(0.2 * len(ply))
    first = _subscans_restated(scan, ply, objects, rels, max_pts, 0, 'x')[0]
    per_obj = {int(i): int((first['pcl']['objectId'] == i).sum()) for i in np.unique(first['pcl']['objectId'])}
    ends_of_rels = sorted({int(r[0]) for r in rels} | {int(r[1]) for r in rels})
    at = min((c, i) for i, c in per_obj.items() if i in ends_of_rels and c > 0)      # the least visible object that has relationships
    min_obj_points = at[0]                                    # object at[1] has EXACTLY this many visible points in subscan 0: excluded (strict >)
    want = _subscans_restated(scan, ply, objects, rels, max_pts, min_obj_points, 'scene0')
    assert len(want) >= 2
    kept0 = want[0]['relationships']['relationships']
    assert 0 < len(kept0) < len(rels) and all(at[1] not in (int(r[0]), int(r[1])) for r in kept0)
    assert any(at[1] in (int(r[0]), int(r[1])) for r in _subscans_restated(scan, ply, objects, rels, max_pts, min_obj_points - 1, 's')[0]['relationships']['relationships'])
    assert all('99' != o['id'] for w in want for o in w['objects']['objects'])
    got = SS.generate_subscans(ply, scan['poses'], scan['intrinsics'], max_pts, objects, rels, min_obj_points, scan_id='scene0')
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g['subscan_id'] == w['subscan_id'] and set(g) == set(w)
        assert g['pcl'].dtype == w['pcl'].dtype and g['pcl'].shape == w['pcl'].shape
        for name in w['pcl'].dtype.names:
            assert np.array_equal(g['pcl'][name], w['pcl'][name]), name
        assert g['objects'] == w['objects'] and g['relationships'] == w['relationships']
    assert SS.generate_subscans(ply[:0], scan['poses'], scan['intrinsics'], 0, objects, rels, 1) == []


def test_reference_signature_equals_the_yardstick_for_one_frame():
    from sgaligner_amd.utils import point_cloud as PC
    scan = _scan(4097, 7)
    _, _, masks = SR.projected(scan)
    for f in (0, 6):
        got = PC.get_visible_pts_from_cam_pose(scan['pts'], scan['poses'][f], scan['intrinsics'])
        assert got.dtype == bool and got.shape == (4097,) and np.array_equal(got, masks[f]) and got.any()
    assert PC.get_visible_pts_from_cam_pose(np.zeros((0, 3), dtype=np.float32), scan['poses'][0], scan['intrinsics']).shape == (0,)


def test_generate_subscan_masks_over_a_batch_twice():
    from sgaligner_amd.preprocessing import subscans as SS
    cases = SR.walk_cases()
    empty = (np.zeros((0, 3), dtype=np.float32), cases[0]['scan']['poses'][:3], cases[0]['scan']['intrinsics'])
    scans = [(c['scan']['pts'], c['scan']['poses'], c['scan']['intrinsics']) for c in cases] + [empty]
    budgets = [c['max_pts'] for c in cases] + [0]
    a = SS.generate_subscan_masks(scans, budgets)
    b = SS.generate_subscan_masks(scans, budgets)
    assert len(a) == len(b) == 4
    for (e1, c1, m1), (e2, c2, m2) in zip(a, b):
        assert np.array_equal(e1, e2) and np.array_equal(c1, c2) and np.array_equal(m1, m2)       # two runs, identical outputs
    for c, (seg_end, seg_count, masks) in zip(cases, a):
        ref = SR.walk_ref(c['masks'], c['max_pts'])
        assert np.array_equal(seg_end, ref['seg_end']) and np.array_equal(seg_count, ref['seg_count'])
        assert masks.dtype == bool and np.array_equal(masks, ref['seg_masks']) and np.array_equal(masks.sum(1), seg_count)
    assert a[3][0].shape == (0,) and a[3][2].shape == (0, 0)
    assert SS.generate_subscan_masks([], []) == []
