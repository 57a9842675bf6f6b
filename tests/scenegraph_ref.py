"""Yardstick of the scene-graph record tests: a plain-NumPy statement of what the reference's process_scan (preprocessing/scan3r/
preprocess.py:40-211) and its two bag-of-words passes (:280-361) compute, the synthetic subscans the tests share, and the reader of
tests/golden/scenegraph_cases.npz (written by tools/make_scenegraph_golden.py from the reference's own functions).

The split is vectorised (one stable sort instead of one np.where per object), the `none` supplement and the bag-of-words are array operations
(a boolean N x N matrix instead of the list search; np.add.at with the edge index applied to the TRIPLES list, as the reference does);
farthest-point sampling and the hull barycentre go through oracle/fps_oracle.py and oracle/hull_oracle.py, the yardsticks of the FPS and hull
tests.  The np.random draws are made where the reference makes them, so the same seed gives the same record."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PLY_DTYPE = [('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('objectId', 'h'), ('globalId', 'h'),
             ('NYU40', 'u1'), ('Eigen13', 'u1'), ('RIO27', 'u1')]

# 41 relation names, `none` first (what the reference reads from files/relationships.txt, one per line)
REL_NAMES = ['none', 'supported by', 'left', 'right', 'front', 'behind', 'close by', 'inside', 'bigger than', 'smaller than', 'higher than',
             'lower than', 'same symmetry as', 'same as', 'attached to', 'standing on', 'lying on', 'hanging on', 'connected to',
             'leaning against', 'part of', 'belonging to', 'build in', 'standing in', 'cover', 'lying in', 'hanging in', 'same color',
             'same material', 'same texture', 'same shape', 'same state', 'same object type', 'messy', 'cleaner', 'brighter', 'darker',
             'more open', 'more closed', 'fuller', 'more comfortable']
REL2IDX = {name: k for k, name in enumerate(REL_NAMES)}
WORD_2_IX = {'brown': 0, 'wooden': 1, 'square': 2, 'tall': 3}          # the attribute vocabulary the second pass starts from


# ---- the three device steps as array operations ------------------------------------------------------------------------------------------
def split_ref(slot, n_slots):
    """slot [N] ints (outside [0, n_slots): no object) -> (counts [n_slots], perm: the points of slot 0, then slot 1, ..., each ascending)."""
    slot = np.asarray(slot, dtype=np.int64)
    ok = (slot >= 0) & (slot < n_slots)
    counts = np.bincount(slot[ok], minlength=n_slots)
    idx = np.flatnonzero(ok)
    return counts, idx[np.argsort(slot[ok], kind='stable')]


def complete_ref(n_nodes, pairs, rels, none_id, vocab):
    """pairs [P, 2] listed (graph-local), rels [Tr >= P] the listed triples' relation ids -> (edges [E, 2] int64, bow [N, V] int64): the listed
    pairs, then every unlisted ordered pair i != j row-major; bow[edges[idx][0], triples_rel[idx]] += 1, triples = listed then `none`."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rels = np.asarray(rels, dtype=np.int64).reshape(-1)
    have = np.eye(n_nodes, dtype=bool)
    have[pairs[:, 0], pairs[:, 1]] = True
    extra = np.argwhere(~have)
    edges = np.concatenate([pairs, extra]).astype(np.int64)
    rel = np.concatenate([rels, np.full(len(extra), none_id, dtype=np.int64)])[:len(edges)]
    bow = np.zeros((n_nodes, vocab), dtype=np.int64)
    np.add.at(bow, (edges[:, 0], rel), 1)
    return edges, bow


def bow_ref(rows, cols, n_rows, vocab):
    out = np.zeros((n_rows, vocab), dtype=np.int64)
    np.add.at(out, (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)), 1)
    return out


# ---- the record ----------------------------------------------------------------------------------------------------------------------------
def record_ref(scan_id, vertices, objects_json, relationships_json, rel2idx, pc_resolutions, min_obj_points, info=None):
    """The record of one scan (or -1), np.random consumed as the reference consumes it.  `info`, when a dict, counts the FPS branches."""
    from oracle import fps_oracle, hull_oracle
    if len(relationships_json) == 0:
        return -1
    points = np.stack([vertices['x'], vertices['y'], vertices['z']]).transpose((1, 0))
    ids, slot = np.unique(np.asarray(vertices['objectId']), return_inverse=True)
    counts, perm = split_ref(slot.reshape(-1), len(ids))
    start = np.concatenate([[0], np.cumsum(counts)])
    slot_of = {int(v): k for k, v in enumerate(ids)}
    objects_ids, global_ids, attributes, bary = [], [], [], []
    obj_points = {r: [] for r in pc_resolutions}
    for obj in objects_json:
        k = slot_of.get(int(obj['id']))
        n = int(counts[k]) if k is not None else 0
        if n < min_obj_points:
            continue
        pcl = points[perm[start[k]:start[k + 1]]]
        bary.append(hull_oracle.hull_barycenter(pcl)[0])
        for r in obj_points:
            if len(pcl) < r:
                pcl = pcl[np.random.choice(len(pcl), r)]
                if info is not None:
                    info['random'] = info.get('random', 0) + 1
            else:
                pcl = pcl[fps_oracle.farthest_point_sample_idx(pcl, r, np.random.randint(0, len(pcl)))]
                if info is not None:
                    info['fps'] = info.get('fps', 0) + 1
            obj_points[r].append(pcl)
        objects_ids.append(int(obj['id']))
        global_ids.append(int(obj['global_id']))
        attributes.append([item for sub in obj['attributes'].values() for item in sub])
    if len(objects_ids) < 2:
        return -1
    id2idx = {v: k for k, v in enumerate(objects_ids)}
    triples, pairs, edges_cat = [], [], []
    for t in relationships_json:
        sub, obj = int(t[0]), int(t[1])
        if sub in id2idx and obj in id2idx:
            triples.append([sub, obj, int(rel2idx[t[3]])])
            edges_cat.append(rel2idx[t[3]])
            if t[:2] not in pairs:                               # the RAW entries: ids typed as strings never equal the stored ints
                pairs.append([sub, obj])
    if len(pairs) == 0:
        return -1
    root_obj_id = np.argmax(np.bincount(np.array(pairs).flatten()))
    bary = np.array(bary)
    rel_trans = bary[id2idx[root_obj_id]][None] - bary
    local = np.array([[id2idx[a], id2idx[b]] for a, b in pairs])
    edges, _ = complete_ref(len(objects_ids), local, [t[2] for t in triples], rel2idx['none'], len(rel2idx))
    extra = np.asarray(objects_ids)[edges[len(pairs):]].tolist()
    return {'scan_id': scan_id, 'objects_id': np.array(objects_ids), 'global_objects_id': np.array(global_ids), 'objects_cat': np.array(global_ids),
            'triples': triples + [[a, b, rel2idx['none']] for a, b in extra], 'pairs': pairs + extra, 'edges': edges,
            'obj_points': {r: np.array(v) for r, v in obj_points.items()}, 'objects_count': len(objects_ids), 'edges_count': len(edges),
            'object_id2idx': id2idx, 'object_attributes': attributes, 'edges_cat': edges_cat + [rel2idx['none']] * len(extra),
            'rel_trans': rel_trans, 'root_obj_id': root_obj_id}


def bow_edge_ref(record, rel2idx):
    """calculate_bow_node_edge_feats for one record: float64 [N, V]."""
    name_of = {idx: name for name, idx in rel2idx.items()}
    word = {name: k for k, name in enumerate(rel2idx.keys())}
    edges = record['edges']
    cols = [word[name_of[record['triples'][k][2]]] for k in range(len(edges))]          # the edge index applied to the triples list
    return bow_ref(edges[:, 0], cols, record['objects_count'], len(word)).astype(np.float64)


def bow_attr_ref(records, word_2_ix):
    """calculate_bow_node_attr_feats for a list of records (ints skipped): ({scan_id: float64 [N, V]}, the extended vocabulary)."""
    vocab = dict(word_2_ix)
    recs = sorted((r for r in records if not isinstance(r, int)), key=lambda r: r['scan_id'])
    for r in recs:
        for attrs in r['object_attributes']:
            for a in attrs:
                if a not in vocab:
                    vocab[a] = len(vocab)
    out = {}
    for r in recs:
        rows = [j for j, attrs in enumerate(r['object_attributes']) for _ in attrs]
        cols = [vocab[a] for attrs in r['object_attributes'] for a in attrs]
        out[r['scan_id']] = bow_ref(rows, cols, r['objects_count'], len(vocab)).astype(np.float64)
    return out, vocab


# ---- synthetic subscans --------------------------------------------------------------------------------------------------------------------
ATTR_WORDS = ['brown', 'wooden', 'square', 'tall', 'white', 'soft', 'round', 'shiny', 'low', 'narrow', 'metal', 'dark']


def make_scan(seed, sizes, background=200, first_id=1):
    """A subscan of len(sizes) objects (ids first_id, first_id + 1, ...) of the given point counts plus `background` points of id 0, in random
    point order: blobs and boxes in a 6 x 4.5 x 2.6 m room, float32.  Returns (vertices: PLY_DTYPE array, objects json list)."""
    rng = np.random.default_rng(seed)
    pts, oid = [rng.random((background, 3)) * [6.0, 4.5, 2.6]], [np.zeros(background, dtype=np.int64)]
    objects = []
    for k, n in enumerate(sizes):
        centre = rng.random(3) * [5.0, 3.5, 1.6] + 0.5
        extent = rng.uniform(0.15, 0.6, 3)
        p = rng.standard_normal((n, 3)) * extent * 0.4 if k % 2 == 0 else (rng.random((n, 3)) - 0.5) * extent
        pts.append(p + centre)
        oid.append(np.full(n, first_id + k, dtype=np.int64))
        words = [ATTR_WORDS[int(w)] for w in rng.choice(len(ATTR_WORDS), size=int(rng.integers(0, 4)), replace=False)]
        objects.append({'id': str(first_id + k), 'global_id': str(int(rng.integers(1, 500))), 'label': f'object{k}',
                        'attributes': {'color': words[:1], 'other': words[1:]} if words else {}})
    pts, oid = np.concatenate(pts), np.concatenate(oid)
    order = rng.permutation(len(pts))
    v = np.zeros(len(pts), dtype=PLY_DTYPE)
    v['x'], v['y'], v['z'] = pts[order, 0], pts[order, 1], pts[order, 2]
    v['objectId'] = oid[order]
    return v, objects


def _rel(sub, obj, name, as_str=False):
    return [str(sub), str(obj), REL2IDX[name], name] if as_str else [sub, obj, REL2IDX[name], name]


def fixture_cases():
    """The inputs of tests/golden/scenegraph_cases.npz: dicts {scan_id, vertices, objects, relationships, resolutions, min_obj_points, seed}."""
    cases = []
    # a: an object below min_obj_points (8), an id listed without points (9), a pair listed twice with different relations ((1, 2): from there
    # on edges and triples are misaligned), a pair listed twice identically, relationships naming the dropped object and the pointless id, and
    # a tie for the root object (1 and 2 both occur three times among the listed pairs: the lower id wins)
    v, objs = make_scan(11, [700, 500, 400, 300, 250, 200, 60, 30])
    objs.append({'id': '9', 'global_id': '77', 'label': 'ghost', 'attributes': {'color': ['white']}})
    rels = [_rel(1, 2, 'left'), _rel(3, 1, 'close by'), _rel(1, 2, 'bigger than'), _rel(2, 4, 'standing on'), _rel(2, 4, 'standing on'),
            _rel(8, 1, 'left'), _rel(1, 9, 'right'), _rel(5, 2, 'behind'), _rel(1, 6, 'same color'), _rel(7, 7, 'same as')]
    cases.append(dict(scan_id='scan_a', vertices=v, objects=objs, relationships=rels, resolutions=[64, 32], min_obj_points=50, seed=3))
    # b: ids typed as strings -- the identical listing of (2, 3) is NOT de-duplicated; objects_json not in id order
    v, objs = make_scan(12, [400, 350, 300, 120, 90])
    objs = [objs[3], objs[0], objs[4], objs[2], objs[1]]
    rels = [_rel(2, 3, 'left', True), _rel(2, 3, 'left', True), _rel(4, 1, 'lower than', True), _rel(3, 2, 'right', True), _rel(5, 4, 'close by', True)]
    cases.append(dict(scan_id='scan_b', vertices=v, objects=objs, relationships=rels, resolutions=[64, 32], min_obj_points=50, seed=4))
    # c: resolution 512 with objects on both sides of 512 points (the N < resolution draw and FPS in one scan)
    v, objs = make_scan(13, [900, 600, 512, 511, 300, 100], background=100)
    rels = [_rel(1, 2, 'left'), _rel(3, 4, 'same shape'), _rel(6, 5, 'smaller than'), _rel(4, 3, 'same shape'), _rel(1, 2, 'higher than')]
    cases.append(dict(scan_id='scan_c', vertices=v, objects=objs, relationships=rels, resolutions=[512], min_obj_points=50, seed=5))
    # d: a second resolution ABOVE the first: every object draws 64 of its 32 samples with replacement
    v, objs = make_scan(14, [300, 200, 150, 20], background=50)
    rels = [_rel(2, 1, 'front'), _rel(3, 1, 'front'), _rel(4, 1, 'front')]
    cases.append(dict(scan_id='scan_d', vertices=v, objects=objs, relationships=rels, resolutions=[32, 64], min_obj_points=50, seed=6))
    # the three -1 outcomes: no relationships (nothing drawn); fewer than two kept objects (its one object still consumes draws); no pair
    # between kept objects
    v, objs = make_scan(15, [200, 150], background=50)
    cases.append(dict(scan_id='scan_e', vertices=v, objects=objs, relationships=[], resolutions=[64, 32], min_obj_points=50, seed=7))
    v, objs = make_scan(16, [220, 40, 30], background=50)
    cases.append(dict(scan_id='scan_f', vertices=v, objects=objs, relationships=[_rel(1, 2, 'left')], resolutions=[64, 32], min_obj_points=50, seed=8))
    v, objs = make_scan(17, [220, 180, 40], background=50)
    cases.append(dict(scan_id='scan_g', vertices=v, objects=objs, relationships=[_rel(1, 3, 'left'), _rel(3, 2, 'right')], resolutions=[64, 32],
                      min_obj_points=50, seed=9))
    return cases


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------
ARRAY_KEYS = ('objects_id', 'global_objects_id', 'objects_cat', 'edges', 'rel_trans', 'root_obj_id', 'bow_vec_object_edge_feats',
              'bow_vec_object_attr_feats')
JSON_KEYS = ('triples', 'pairs', 'object_attributes', 'edges_cat')
INT_KEYS = ('objects_count', 'edges_count')


def _plain(o):
    """numpy scalars -> Python ones, for json (a list the reference built may hold either)."""
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    return o.item() if isinstance(o, np.generic) else o


def pack_case(prefix, case, record):
    """One case as flat arrays for np.savez (inputs, and the record the reference returned for them)."""
    out = {prefix + 'scan_id': np.array(case['scan_id']), prefix + 'objects_json': np.array(json.dumps(case['objects'])),
           prefix + 'relationships_json': np.array(json.dumps(case['relationships'])), prefix + 'resolutions': np.array(case['resolutions'], dtype=np.int64),
           prefix + 'min_obj_points': np.int64(case['min_obj_points']), prefix + 'seed': np.int64(case['seed']),
           prefix + 'is_record': np.int64(not isinstance(record, int))}
    for f in ('x', 'y', 'z', 'objectId'):
        out[prefix + 'in_' + f] = np.ascontiguousarray(case['vertices'][f])
    if isinstance(record, int):
        return out
    for k in ARRAY_KEYS:
        out[prefix + k] = np.asarray(record[k])
    for k in JSON_KEYS:
        out[prefix + k] = np.array(json.dumps(_plain(record[k])))
    for k in INT_KEYS:
        out[prefix + k] = np.int64(record[k])
    out[prefix + 'object_id2idx'] = np.array([[int(a), int(b)] for a, b in record['object_id2idx'].items()], dtype=np.int64).reshape(-1, 2)
    for r, v in record['obj_points'].items():
        out[prefix + f'obj_points_{r}'] = np.asarray(v)
    return out


def load_fixture():
    """-> (cases, records, attribute vocabulary after the second pass): cases as fixture_cases() returns them, records[k] the reference's
    record for cases[k] (with both bag-of-words matrices) or -1."""
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'scenegraph_cases.npz'), allow_pickle=False))
    cases, records = [], []
    for c in range(int(g['n_cases'])):
        p = f'c{c}_'
        n = len(g[p + 'in_x'])
        v = np.zeros(n, dtype=PLY_DTYPE)
        for f in ('x', 'y', 'z', 'objectId'):
            v[f] = g[p + 'in_' + f]
        cases.append(dict(scan_id=str(g[p + 'scan_id']), vertices=v, objects=json.loads(str(g[p + 'objects_json'])),
                          relationships=json.loads(str(g[p + 'relationships_json'])), resolutions=[int(r) for r in g[p + 'resolutions']],
                          min_obj_points=int(g[p + 'min_obj_points']), seed=int(g[p + 'seed'])))
        if not int(g[p + 'is_record']):
            records.append(-1)
            continue
        rec = {'scan_id': cases[-1]['scan_id']}
        for k in ARRAY_KEYS:
            rec[k] = g[p + k]
        rec['root_obj_id'] = rec['root_obj_id'][()]
        for k in JSON_KEYS:
            rec[k] = json.loads(str(g[p + k]))
        for k in INT_KEYS:
            rec[k] = int(g[p + k])
        rec['object_id2idx'] = {int(a): int(b) for a, b in g[p + 'object_id2idx']}
        rec['obj_points'] = {r: g[p + f'obj_points_{r}'] for r in cases[-1]['resolutions']}
        records.append(rec)
    return cases, records, json.loads(str(g['attr_vocabulary']))


def assert_records_equal(got, want, skip=(), what=''):
    """Key for key, dtype for dtype, bit for bit (`skip`: keys the caller compares itself)."""
    if isinstance(want, int):
        assert isinstance(got, int) and got == want, (what, got)
        return
    assert not isinstance(got, int), (what, 'got -1')
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        if k in skip:
            continue
        g = got[k]
        if k == 'obj_points':
            assert list(g) == list(w), (what, k)
            for r in w:
                assert g[r].dtype == w[r].dtype == np.float32 and g[r].shape == w[r].shape and np.array_equal(g[r], w[r]), (what, k, r)
        elif isinstance(w, np.ndarray) or isinstance(w, np.generic):
            g = np.asarray(g)
            assert g.dtype == np.asarray(w).dtype and g.shape == np.asarray(w).shape and np.array_equal(g, w), (what, k, g, w)
        else:
            assert _plain(g) == w if k in JSON_KEYS else g == w, (what, k, g, w)
