"""CPU tier of subscan generation (csrc/visibility.hip, utils/point_cloud.py, preprocessing/subscans.py): the numpy yardstick of the
frustum test agrees with the reference's own NumPy route away from the frustum edges, the walk yardstick equals a line-by-line
restatement of the reference's loop, the test inputs have the properties the GPU tier relies on, the C ABI refuses bad arguments without
a device, nothing falls back to the host, and the kernels do not spill."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import subscan_ref as SR  # noqa: E402


def test_yardstick_equals_the_reference_chain_away_from_the_thresholds():
    total = left_out = 0
    for n, f, seed in ((100_000, 40, 1), (100_000, 40, 2)):
        scan = SR.make_scan(n, f, seed)
        w2c, intr, masks = SR.projected(scan)
        assert masks.mean() > 0.03                                   # the frames do see the room
        for k in range(f):
            chain = SR.chain_ref(scan['pts'], scan['poses'][k], scan['intrinsics'])
            near = SR.near_threshold(*SR.project_ref(scan['pts'], w2c[k], intr), intr)
            total += n
            left_out += int(near.sum())
            bad = (chain != masks[k]) & ~near
            assert not bad.any(), (seed, k, int(bad.sum()))
    print('entries', total, 'within 1e-9 of a threshold', left_out)
    assert total == 8_000_000 and left_out <= 1e-5 * total


def _walk_literal(scene_pts, frame_masks, max_pts_subscan):
    """preprocessing/scan3r/subgenscan3r.py:188-234 line by line, the per-frame mask taken from `frame_masks`, the subscan kept instead of saved."""
    curr_visible_mask = np.zeros(scene_pts.shape[0]).astype('bool')
    frame_cnt = 0
    subscan_idx = 0
    closed = []
    while frame_cnt < len(frame_masks):
        frame_visible_mask = frame_masks[frame_cnt]
        curr_visible_mask = np.logical_or(frame_visible_mask, curr_visible_mask)
        subscan_pts = scene_pts[curr_visible_mask]
        if subscan_pts.shape[0] >= max_pts_subscan:
            closed.append((frame_cnt, subscan_pts.shape[0], curr_visible_mask))
            subscan_idx += 1
            curr_visible_mask = np.zeros(scene_pts.shape[0]).astype('bool')
        frame_cnt += 1
    assert subscan_idx == len(closed)
    return closed


def test_walk_yardstick_equals_the_reference_loop_and_the_inputs_are_what_the_gpu_tests_need():
    cases = SR.walk_cases()
    exact = 0
    for c in cases:
        masks, budget = c['masks'], c['max_pts']
        ref = SR.walk_ref(masks, budget)
        lit = _walk_literal(c['scan']['pts'], masks, budget)
        assert ref['n_seg'] == len(lit) >= 2                                             # at least two subscans ...
        assert ref['seg_end'][-1] < len(masks) - 1 and ref['frame_count'][-1] < budget    # ... and a tail that is discarded
        assert (masks.sum(1) == 0).any()                                                 # a frame that sees nothing
        for k, (f, n, m) in enumerate(lit):
            assert ref['seg_end'][k] == f and ref['seg_count'][k] == n and np.array_equal(ref['seg_masks'][k], m)
        assert np.array_equal(ref['frame_count'], ref['cum'].sum(1))
        exact += int((ref['seg_count'] == budget).sum())
    assert exact >= 1                                                                    # a budget met exactly: the comparison is >=
    # the bit packing the device uses
    m = np.zeros((2, 130), dtype=bool)
    m[0, [0, 63, 64, 129]] = True
    w = SR.pack_bits(m)
    assert w.shape == (2, 3) and w.dtype == np.uint64
    assert w[0].tolist() == [1 | (1 << 63), 1, 2] and w[1].tolist() == [0, 0, 0]


def test_abi_has_the_entry_points_and_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    from sgaligner_amd.preprocessing import subscans as SS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    for name in ('sga_frame_visibility', 'sga_subscan_walk', 'sga_subscan_object_counts', 'sga_subscan_lds_slots'):
        assert name + '(' in hdr and name in _lib.SIGNATURES
    l = _lib.lib()
    assert SS.object_count_lds_slots() == l.sga_subscan_lds_slots() >= 64
    buf = np.zeros(64, dtype=np.float64)                     # host memory: never dereferenced, every call must stop before its launch
    p = buf.ctypes.data
    i32 = lambda *v: np.array(v, dtype=np.int32)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    good_pt, good_fr, good_vis = i32(0, 100, 130), i32(0, 2, 5), i64(0, 4, 7)          # scans of 100 x 2 and 30 x 3: 2 * 2 + 3 * 1 words
    vis = lambda pt, fr, vo, **kw: l.sga_frame_visibility(p, p, p, p, p, p, kw.get('n', 2), 130, 5, kw.get('words', 7), kw.get('mp', 100), 3,
                                                          pt.ctypes.data, fr.ctypes.data, vo.ctypes.data, kw.get('out', p), None)
    assert l.sga_frame_visibility(None, None, None, None, None, None, 2, 130, 5, 7, 100, 3, None, None, None, None, None) != 0
    assert b'null pointer' in l.sga_last_error()
    assert vis(i32(0, 100, 129), good_fr, good_vis) != 0 and b'pt_off must run from 0 to total_points' in l.sga_last_error()
    assert vis(i32(0, 131, 130), good_fr, good_vis) != 0 and b'pt_off decreases at scan 1' in l.sga_last_error()
    assert vis(good_pt, i32(1, 2, 5), good_vis) != 0 and b'fr_off must run' in l.sga_last_error()
    assert vis(good_pt, good_fr, i64(0, 3, 7)) != 0 and b'vis_off of scan 0' in l.sga_last_error()
    assert vis(good_pt, good_fr, good_vis, words=6) != 0 and b'vis_off ends at 7 of 6' in l.sga_last_error()
    assert vis(good_pt, good_fr, good_vis, mp=99) != 0 and b'larger than max_points' in l.sga_last_error()
    assert vis(good_pt, good_fr, good_vis, n=-1) != 0 and b'negative count' in l.sga_last_error()
    assert vis(good_pt, good_fr, good_vis, out=p + 4) != 0 and b'misaligned' in l.sga_last_error()
    walk = lambda pt, fr, vo: l.sga_subscan_walk(p, p, p, p, p, p, 2, 130, 5, 7, pt.ctypes.data, fr.ctypes.data, vo.ctypes.data, p, p, p, p, None)
    assert walk(good_pt, i32(0, 6, 5), good_vis) != 0 and b'fr_off decreases at scan 1' in l.sga_last_error()
    assert walk(good_pt, good_fr, i64(1, 5, 8)) != 0 and b'vis_off must start at 0' in l.sga_last_error()
    assert l.sga_subscan_walk(p, p, p, p, p, None, 2, 130, 5, 7, None, None, None, p, p, p, p, None) != 0 and b'null pointer' in l.sga_last_error()
    cnt = lambda rows, **kw: l.sga_subscan_object_counts(p, p, p, p, 2, 130, 5, 7, 100, p, len(rows) // 2, p, kw.get('slots', 3), good_pt.ctypes.data,
                                                         good_fr.ctypes.data, good_vis.ctypes.data, rows.ctypes.data, kw.get('counts', p), None)
    assert cnt(i32(0, 1, 2, 0)) != 0 and b'row 1 names scan 2 of 2' in l.sga_last_error()
    assert cnt(i32(0, 2)) != 0 and b'row 0 names frame 2 of 2' in l.sga_last_error()
    assert cnt(i32(0, 1), slots=-1) != 0 and b'negative count' in l.sga_last_error()
    assert cnt(i32(0, 1), counts=None) != 0 and b'null pointer' in l.sga_last_error()


def test_python_argument_errors_and_no_silent_fallback():
    from sgaligner_amd.preprocessing import subscans as SS
    from sgaligner_amd.utils import point_cloud as PC
    pts, w2c, intr = torch.zeros((8, 3)), torch.zeros((2, 12), dtype=torch.float64), torch.zeros((1, 6), dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r'HIP device tensor.*no CPU path'):
        PC.visible_masks_batch(pts, [0, 8], w2c, [0, 2], intr)
    with pytest.raises(RuntimeError, match=r'`points` must be torch.float32'):
        PC.visible_masks_batch(pts.double(), [0, 8], w2c, [0, 2], intr)
    with pytest.raises(RuntimeError, match=r'`w2c` must be torch.float64'):
        PC.visible_masks_batch(pts, [0, 8], w2c.float(), [0, 2], intr)
    with pytest.raises(ValueError, match='pt_off must be a monotone prefix array'):
        PC.ScanLayout([0, 9], [0, 2], 8, 2)
    with pytest.raises(ValueError, match='fr_off must be a monotone prefix array'):
        PC.ScanLayout([0, 5, 8], [0, 3, 2], 8, 2)
    with pytest.raises(ValueError, match='names 2 scans'):
        PC.ScanLayout([0, 5, 8], [0, 2], 8, 2)
    lay = PC.ScanLayout([0, 100, 130], [0, 2, 5], 130, 5)
    assert lay.words.tolist() == [2, 1] and lay.vis_off.tolist() == [0, 4, 7] and lay.max_points == 100 and lay.max_frames == 3
    with pytest.raises(RuntimeError, match=r'`vis` must be torch.int64'):
        SS.subscan_walk_batch(torch.zeros(7, dtype=torch.int32), lay, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r'HIP device tensor.*no CPU path'):
        SS.subscan_walk_batch(torch.zeros(7, dtype=torch.int64), lay, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r'HIP device tensor.*no CPU path'):
        SS.object_counts_batch(torch.zeros(7, dtype=torch.int64), lay, [(0, 0)], torch.zeros(130, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match='2 scans need 2 point budgets'):
        SS.generate_subscan_masks([(np.zeros((4, 3)), np.eye(4)[None], SR.make_intrinsics())] * 2, [1])
    # host helpers
    pose = np.eye(4)
    pose[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    pose[:3, 3] = [1.0, 2.0, 3.0]
    inv = PC.inverse_relative(pose)
    assert inv.dtype == np.float32 and np.array_equal(inv, np.linalg.inv(pose).astype(np.float32))
    assert np.array_equal(inv, SR.inverse_relative(pose)) and np.array_equal(PC.world_to_cam_rows(pose[None]), SR.w2c_rows(pose[None]))
    info = SR.make_intrinsics()
    row = PC.intrinsic_row(info)
    assert row[4] == info['height'] == 540.0 and row[5] == info['width'] == 960.0          # the reference's swapped bounds, on purpose
    assert np.array_equal(row, SR.intr_row(info))
    m = np.random.default_rng(0).random((3, 130)) < 0.5
    assert np.array_equal(PC.unpack_mask_words(SR.pack_bits(m), 130), m)

    class R:
        def randint(self, a, b):
            return a, b
    assert SS.draw_max_pts(1001, R()) == (200, 500)
    if torch.cuda.is_available():
        return                                             # the rest is about machines without a device
    s = SR.make_scan(100, 2, 0)
    for fn in (lambda: PC.get_visible_pts_from_cam_pose(s['pts'], s['poses'][0], s['intrinsics']),
               lambda: SS.generate_subscan_masks([(s['pts'], s['poses'], s['intrinsics'])], [10])):
        with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
            fn()


def test_visibility_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    assert '-ffp-contract=off' in _build.FILE_FLAGS['visibility.hip']
    _, res = kr.analyse(os.path.join(_build.CSRC, 'visibility.hip'))
    for tag in ('vis_kernel', 'walk_kernel', 'objcount_kernel'):
        ks = [k for k in res if tag in k]
        assert ks, (tag, sorted(res))
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
            assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
