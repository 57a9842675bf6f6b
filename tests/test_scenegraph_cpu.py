"""CPU: the scene-graph record yardstick (tests/scenegraph_ref.py) equals the reference's own output (tests/golden/scenegraph_cases.npz, written
by tools/make_scenegraph_golden.py from process_scan and the two bag-of-words passes) key for key and bit for bit; the C ABI has the new
entry points and refuses bad arguments before any launch; nothing falls back to the host; the new kernels do not spill."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import scenegraph_ref as SG  # noqa: E402


def test_yardstick_equals_the_reference_records_bit_for_bit():
    cases, records, vocab = SG.load_fixture()
    assert [c['scan_id'] for c in cases] == [c['scan_id'] for c in SG.fixture_cases()]
    mine, info = [], {}
    for c in cases:
        np.random.seed(c['seed'])
        mine.append(SG.record_ref(c['scan_id'], c['vertices'], c['objects'], c['relationships'], SG.REL2IDX, c['resolutions'],
                                  c['min_obj_points'], info))
    attr, my_vocab = SG.bow_attr_ref(mine, SG.WORD_2_IX)
    assert my_vocab == vocab and list(my_vocab) == list(vocab) and len(vocab) > len(SG.WORD_2_IX)
    for c, m, r in zip(cases, mine, records):
        if not isinstance(m, int):
            m['bow_vec_object_edge_feats'] = SG.bow_edge_ref(m, SG.REL2IDX)
            m['bow_vec_object_attr_feats'] = attr[c['scan_id']]
        SG.assert_records_equal(m, r, what=c['scan_id'])
    # the fixture holds what the tests are about
    assert [isinstance(r, int) for r in records] == [False, False, False, False, True, True, True]
    a, b, c = records[0], records[1], records[2]
    assert len(a['triples']) == a['edges_count'] + 2 and len(c['triples']) == c['edges_count'] + 1       # edges and triples misaligned
    assert 8 not in a['object_id2idx'] and 9 not in a['object_id2idx'] and a['objects_count'] == 7       # below min_obj_points / no points
    assert a['pairs'].count([2, 4]) == 1 and a['pairs'].count([1, 2]) == 1 and [7, 7] in a['pairs']
    assert np.bincount(np.array(a['pairs'][:6]).flatten())[[1, 2]].tolist() == [3, 3] and a['root_obj_id'] == 1   # the tie goes to the lower id
    assert b['pairs'].count([2, 3]) == 2 and len(b['triples']) == b['edges_count']                       # string ids never de-duplicate
    assert info['fps'] > 0 and info['random'] > 0
    n512 = [int((cases[2]['vertices']['objectId'] == i).sum()) for i in c['objects_id']]
    assert min(n512) < 512 <= max(n512) and 512 in n512 and 511 in n512
    # the misaligned bag-of-words differs from the aligned one: the fixture can tell them apart
    first = {}
    for t in a['triples']:
        first.setdefault((t[0], t[1]), t[2])
    aligned = SG.bow_ref(a['edges'][:, 0], [first[tuple(q)] for q in a['pairs']], a['objects_count'], 41)
    assert not np.array_equal(aligned, a['bow_vec_object_edge_feats'])


def test_array_yardsticks_equal_the_literal_loops():
    rng = np.random.default_rng(0)
    slot = rng.integers(-1, 5, 300)
    counts, perm = SG.split_ref(slot, 4)
    assert counts.tolist() == [int((slot == k).sum()) for k in range(4)]
    assert perm.tolist() == [int(p) for k in range(4) for p in np.where(slot == k)[0]]
    for n, p in ((2, 1), (5, 7), (9, 30)):
        pairs = [[int(a), int(b)] for a, b in rng.integers(0, n, (p, 2))]
        rels = rng.integers(0, 6, p + 3).tolist()
        listed = [list(q) for q in pairs]
        triples = list(rels)
        for i in range(n):                                   # preprocess.py:176-182
            for j in range(n):
                if i == j or [i, j] in listed:
                    continue
                listed.append([i, j])
                triples.append(0)
        bow = np.zeros((n, 6), dtype=np.int64)
        for idx in range(len(listed)):                       # :303-306
            bow[listed[idx][0], triples[idx]] += 1
        edges, mine = SG.complete_ref(n, pairs, rels, 0, 6)
        assert edges.tolist() == listed and np.array_equal(mine, bow)


def test_abi_has_the_entry_points_and_refuses_bad_arguments_without_a_device():
    from sgaligner_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sgaligner_hip.h')).read()
    names = ('sga_object_counts', 'sga_object_partition', 'sga_object_partition_ws_bytes', 'sga_graph_complete', 'sga_graph_max_nodes',
             'sga_bow_counts', 'sga_scenegraph_lds_slots', 'sga_scenegraph_tile')
    for name in names:
        assert name + '(' in hdr and name in _lib.SIGNATURES, name
    l = _lib.lib()
    n_max = l.sga_graph_max_nodes()
    words = lambda n: n * ((n + 31) // 32) + n               # the bit matrix next to one counter per row, in 32-bit words
    assert words(n_max) * 4 <= 64 * 1024 < words(n_max + 1) * 4 + 256 and n_max >= 512
    assert l.sga_scenegraph_tile() >= 64 and l.sga_scenegraph_lds_slots() >= 300
    assert l.sga_object_partition_ws_bytes(3, 2 * l.sga_scenegraph_tile() + 1, 10) == 3 * 3 * 10 * 4
    buf = np.zeros(64, dtype=np.float64)                     # host memory: never dereferenced, every call must stop before its launch
    p = buf.ctypes.data
    i32 = lambda *v: np.array(v, dtype=np.int32)
    err = lambda: l.sga_last_error()
    pt, so = i32(0, 100, 130), i32(0, 3, 5)
    cnt = lambda a, b, **kw: l.sga_object_counts(p, p, p, 2, 130, 5, kw.get('mp', 100), a.ctypes.data, b.ctypes.data, kw.get('out', p), None)
    assert cnt(i32(0, 131, 130), so) != 0 and b'pt_off decreases at scan 1' in err()
    assert cnt(pt, i32(0, 6, 5)) != 0 and b'slot_off decreases at scan 1' in err()
    assert cnt(pt, i32(1, 3, 5)) != 0 and b'slot_off must run from 0' in err()
    assert cnt(pt, so, mp=99) != 0 and b'larger than max_points' in err()
    assert cnt(pt, so, out=None) != 0 and b'null pointer' in err()
    part = lambda a, b, dest, c, **kw: l.sga_object_partition(p, p, p, p, p, 2, 130, 5, 100, kw.get('ms', 3), kw.get('kept', 60), a.ctypes.data, b.ctypes.data,
                                                              dest.ctypes.data, c.ctypes.data, p, p, p, kw.get('ws', 1 << 20), None)
    counts = i32(10, 20, 70, 25, 5)
    assert part(i32(0, 131, 130), so, i32(0, 10, -1, 30, 55), counts) != 0 and b'pt_off decreases at scan 1' in err()
    assert part(pt, i32(0, 4, 3), i32(0, 10, -1, 30, 55), counts) != 0 and b'slot_off' in err()
    # wrong in both arrays: both ends are checked before either array's order, and the orders scan by scan
    assert part(i32(0, 131, 130), i32(0, 3, 4), i32(0, 10, -1, 30, 55), counts) != 0 and b'slot_off must run from 0 to total_slots' in err()
    assert part(i32(0, 131, 130), i32(1, 0, 5), i32(0, 10, -1, 30, 55), counts) != 0 and b'slot_off must run' in err()
    assert part(i32(0, 131, 130), i32(0, 6, 5), i32(0, 10, -1, 30, 55), counts) != 0 and b'pt_off decreases at scan 1' in err()
    assert part(i32(0, 100, 130), i32(0, 6, 5), i32(0, 10, -1, 30, 55), counts) != 0 and b'slot_off decreases at scan 1' in err()
    assert part(pt, so, i32(0, 5, -1, 30, 55), counts) != 0 and b'dest_off ranges overlap at output position 5' in err()
    assert part(pt, so, i32(0, 10, -1, 30, 56), counts) != 0 and b'slot 4 writes [56, 61) of 60 kept points' in err()
    assert part(pt, so, i32(0, 10, -1, 30, 55), counts, ms=2) != 0 and b'larger than max_points 100 / max_slots 2' in err()
    assert part(pt, so, i32(0, 10, -1, 30, 55), counts, ws=8) != 0 and b'workspace of 8 bytes' in err()
    assert l.sga_object_partition(p, p, p, p, p, 2, 130, 5, 100, 3, 60, pt.ctypes.data, so.ctypes.data, None, counts.ctypes.data, p, p, p, 1 << 20,
                                  None) != 0 and b'host copies' in err()
    too_many = l.sga_scenegraph_lds_slots() + 1
    assert l.sga_object_partition(p, p, p, p, p, 1, 130, too_many, 130, too_many, 60, p, p, p, p, p, p, p, 1 << 20, None) != 0 and b'slots in one scan' in err()

    def graph(node, pair, trip, edge, pairs=i32(0, 1, 1, 0, 2, 1), rels=i32(1, 2, 3, 4), none=0, V=6):
        return l.sga_graph_complete(p, p, p, p, len(node) - 1, p, p, none, V, node.ctypes.data, pair.ctypes.data, trip.ctypes.data, edge.ctypes.data,
                                    pairs.ctypes.data, rels.ctypes.data, p, p, p, None)
    node, pair, trip, edge = i32(0, 2, 5), i32(0, 2, 3), i32(0, 2, 4), i32(0, 4, 11)
    assert graph(i32(0, 2, 1), pair, trip, edge) != 0 and b'node_off decreases at 1' in err()
    assert graph(node, pair, i32(0, 1, 4), edge) != 0 and b'graph 0 lists 1 triples for 2 pairs' in err()
    assert graph(node, pair, trip, i32(0, 4, 10)) != 0 and b'graph 1 has room for 6 edges, 7 needed' in err()
    assert graph(node, pair, trip, edge, pairs=i32(0, 1, 2, 0, 2, 1)) != 0 and b'graph 0 lists node 2 of 2' in err()
    assert graph(node, pair, trip, edge, rels=i32(1, 2, 6, 4)) != 0 and b'relation 6 at triple 2' in err()
    assert graph(node, pair, trip, edge, none=6) != 0 and b'`none`' in err()
    big = i32(0, n_max + 1)
    assert graph(big, i32(0, 0), i32(0, 0), i32(0, (n_max + 1) * n_max), pairs=i32(), rels=i32()) != 0 and f'at most {n_max}'.encode() in err()
    bow = lambda r, c: l.sga_bow_counts(p, p, len(r), 3, 4, r.ctypes.data, c.ctypes.data, p, None)
    assert bow(i32(0, 1, 2), i32(0, 4, 1)) != 0 and b'cols[1] = 4 is outside [0, 4)' in err()
    assert bow(i32(0, 3, 2), i32(0, 1, 1)) != 0 and b'rows[1] = 3 is outside [0, 3)' in err()
    assert l.sga_bow_counts(p, p, 2, 3, 4, None, None, None, None) != 0 and b'null pointer' in err()


def test_python_argument_errors_and_no_silent_fallback():
    from sgaligner_amd.preprocessing import scene_graphs as G
    from sgaligner_amd.utils import point_cloud as PC
    n_max = G.graph_max_nodes()
    with pytest.raises(ValueError, match=f'at most {n_max}'):
        G.graph_complete_batch([3, n_max + 1], [np.zeros((0, 2)), np.zeros((0, 2))], [[], []], 0, 41)
    with pytest.raises(ValueError, match='1 triples for 2 pairs'):
        G.graph_complete_batch([3], [[[0, 1], [1, 2]]], [[0]], 0, 41)
    with pytest.raises(ValueError, match=r'objects in \[0, 3\)'):
        G.graph_complete_batch([3], [[[0, 3]]], [[0]], 0, 41)
    with pytest.raises(ValueError, match=r'cols must be in \[0, 4\)'):
        G.bow_counts([0, 1], [0, 4], 2, 4)
    with pytest.raises(ValueError, match='pt_off must be a monotone prefix array'):
        G.SlotLayout([0, 9, 8], [0, 1, 2])
    with pytest.raises(ValueError, match='names 2 scans'):
        G.SlotLayout([0, 5, 8], [0, 2])
    lay = G.SlotLayout([0, 100, 130], [0, 3, 5])
    assert (lay.max_points, lay.max_slots, lay.total_points, lay.total_slots) == (100, 3, 130, 5)
    pts, slot = torch.zeros((130, 3)), torch.zeros(130, dtype=torch.int32)
    with pytest.raises(ValueError, match='disjoint ranges'):
        G.object_partition_batch(pts, slot, lay, [0, 5, -1, 30, 55], [10, 20, 70, 25, 5])
    with pytest.raises(RuntimeError, match=r'`slot` must be torch.int32'):
        G.object_partition_batch(pts, slot.long(), lay, [0, 10, -1, 30, 55], [10, 20, 70, 25, 5])
    with pytest.raises(RuntimeError, match=r'HIP device tensor.*no CPU path'):
        G.object_partition_batch(pts, slot, lay, [0, 10, -1, 30, 55], [10, 20, 70, 25, 5])
    with pytest.raises(RuntimeError, match=r'HIP device tensor.*no CPU path'):
        G.object_counts_batch(slot, lay)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PC.convex_hull_barycenters_device(pts, [0, 130])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PC.hull_vertices_device(pts.double(), [0, 130])
    # the host side of the triples loop: raw ints de-duplicate, ids typed as strings never do
    t, pr, cat = G.filter_relationships([[1, 2, 0, 'left'], [1, 2, 0, 'right'], ['1', '2', 0, 'left'], [1, 3, 0, 'left'], [2, 1, 0, 'front']], [1, 2],
                                        SG.REL2IDX)
    assert pr == [[1, 2], [1, 2], [2, 1]] and [x[2] for x in t] == [2, 3, 2, 4] and cat == [2, 3, 2, 4]
    assert G.relation_columns(SG.REL2IDX) == {k: k for k in range(41)}
    if torch.cuda.is_available():
        return                                               # the rest is about machines without a device
    c = SG.fixture_cases()[0]
    scan = (c['scan_id'], c['vertices'], c['objects'], c['relationships'])
    for fn in (lambda: G.process_scans([scan], SG.REL2IDX, c['resolutions'], c['min_obj_points']), lambda: G.process_scan(*scan, SG.REL2IDX),
               lambda: G.bow_counts([0], [0], 1, 1), lambda: G.graph_complete_batch([2], [[[0, 1]]], [[0]], 0, 41)):
        with pytest.raises(RuntimeError, match=r'HIP device.*no CPU path'):
            fn()


def test_scenegraph_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    _, res = kr.analyse(os.path.join(_build.CSRC, 'scenegraph.hip'))
    for tag in ('object_counts_kernel', 'tile_hist_kernel', 'tile_scan_kernel', 'tile_place_kernel', 'graph_complete_kernel', 'bow_counts_kernel'):
        ks = [k for k in res if tag in k]
        assert ks, (tag, sorted(res))
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
            assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
