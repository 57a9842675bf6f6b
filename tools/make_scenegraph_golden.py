"""Writes tests/golden/scenegraph_cases.npz: the reference's own process_scan, calculate_bow_node_edge_feats and calculate_bow_node_attr_feats
(preprocessing/scan3r/preprocess.py) run on the synthetic subscans of tests/scenegraph_ref.fixture_cases().

    python tools/make_scenegraph_golden.py <checkout of the reference> [--example]

The reference's module imports packages this run never calls (cv2, open3d, trimesh, yacs) and its configs package; they are stubbed as empty
modules.  utils.define.SCAN3R_ORIG_DIR is pointed at a temporary directory that holds files/relationships.txt (the 41 names of
scenegraph_ref.REL_NAMES) and files/obj_attr.pkl (scenegraph_ref.WORD_2_IX); every case's data.npy is written there too.  np.random is seeded
with the case's seed before each process_scan call.  Only arrays and json-encoded lists are stored (allow_pickle=False); the output is
deterministic, so a second run regenerates the committed file bit for bit.  No test imports this tool.

--example: instead of writing anything, run the reference and (on a machine with a device) sgaligner_amd's process_scan on the reference's
example scan with a synthetic relationship list that holds one same-pair duplicate, and compare the two records."""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import scenegraph_ref as SG  # noqa: E402


def load_reference(ref_dir, work_dir):
    """Import the reference's preprocess module against `work_dir` as its dataset root."""
    for name in ('cv2', 'open3d', 'open3d.ml', 'open3d.ml.torch', 'trimesh', 'yacs', 'yacs.config'):
        sys.modules.setdefault(name, types.ModuleType(name))
    cfg_mod = types.ModuleType('configs')
    cfg_mod.config, cfg_mod.update_config = None, None
    sys.modules['configs'] = cfg_mod
    os.makedirs(os.path.join(work_dir, 'files'), exist_ok=True)
    with open(os.path.join(work_dir, 'files', 'relationships.txt'), 'w') as fh:
        fh.write('\n'.join(SG.REL_NAMES) + '\n')
    with open(os.path.join(work_dir, 'files', 'obj_attr.pkl'), 'wb') as fh:
        pickle.dump(dict(SG.WORD_2_IX), fh)
    sys.path.insert(0, ref_dir)
    from utils import define
    define.SCAN3R_ORIG_DIR = work_dir
    define.OBJ_ATTR_FILENAME = os.path.join(work_dir, 'files/obj_attr.pkl')
    from preprocessing.scan3r import preprocess
    assert dict(preprocess.REL2IDX) == SG.REL2IDX
    return preprocess


def run_reference(preprocess, work_dir, cases):
    """-> (records with both bag-of-words matrices, or -1; the attribute vocabulary after the second pass)."""
    args = types.SimpleNamespace(remove_node=False, remove_edge=False, change_node_semantic=False, change_edge_semantic=False)
    out_dir = os.path.join(work_dir, 'files', 'orig')
    os.makedirs(os.path.join(out_dir, 'data'), exist_ok=True)
    kept = []
    for case in cases:
        os.makedirs(os.path.join(work_dir, 'scans', case['scan_id']), exist_ok=True)
        np.save(os.path.join(work_dir, 'scans', case['scan_id'], 'data.npy'), case['vertices'])
        cfg = types.SimpleNamespace(preprocess=types.SimpleNamespace(pc_resolutions=list(case['resolutions']), min_obj_points=case['min_obj_points']))
        np.random.seed(case['seed'])
        rec = preprocess.process_scan(work_dir, {'scan': case['scan_id'], 'relationships': case['relationships']},
                                      {'scan': case['scan_id'], 'objects': case['objects']}, args, cfg, preprocess.REL2IDX)
        kept.append(not isinstance(rec, int))
        if kept[-1]:
            with open(os.path.join(out_dir, 'data', case['scan_id'] + '.pkl'), 'wb') as fh:
                pickle.dump(rec, fh, protocol=pickle.HIGHEST_PROTOCOL)
    # the vocabulary as the second pass extends it (it does not write it back): the same walk, in the same order
    vocab = dict(SG.WORD_2_IX)
    preprocess.calculate_bow_node_attr_feats(out_dir)
    preprocess.calculate_bow_node_edge_feats(out_dir, preprocess.REL2IDX)
    records = []
    for case, ok in zip(cases, kept):
        if not ok:
            records.append(-1)
            continue
        with open(os.path.join(out_dir, 'data', case['scan_id'] + '.pkl'), 'rb') as fh:
            records.append(pickle.load(fh))
    for rec in sorted((r for r in records if not isinstance(r, int)), key=lambda r: r['scan_id']):
        for attrs in rec['object_attributes']:
            for a in attrs:
                vocab.setdefault(a, len(vocab))
    for rec in records:
        assert isinstance(rec, int) or rec['bow_vec_object_attr_feats'].shape[1] == len(vocab)
    return records, vocab


def example_case(ref_dir):
    """The reference's example scan with every object of at least 50 points listed and a ring of relationships, one pair twice."""
    v = np.load(os.path.join(ref_dir, 'example_data', 'scene_1', 'data.npy'))
    ids, counts = np.unique(v['objectId'], return_counts=True)
    ids = [int(i) for i, c in zip(ids, counts) if c >= 50]
    objects = [{'id': str(i), 'global_id': str(i % 160 + 1), 'label': f'o{i}', 'attributes': {}} for i in ids]
    rels = [SG._rel(a, b, SG.REL_NAMES[1 + k % 6]) for k, (a, b) in enumerate(zip(ids, ids[1:] + ids[:1]))]
    rels.insert(3, SG._rel(ids[0], ids[1], 'bigger than'))
    return dict(scan_id='scene_1', vertices=v, objects=objects, relationships=rels, resolutions=[512, 128], min_obj_points=50, seed=1)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            member = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            member.compress_type = zipfile.ZIP_DEFLATED
            member.external_attr = 0o644 << 16
            zf.writestr(member, buf.getvalue())


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith('--')]
    ref_dir = argv[0] if argv else os.environ.get('SGA_REFERENCE')
    if not ref_dir:
        sys.exit(__doc__)
    import json
    with tempfile.TemporaryDirectory() as work_dir:
        preprocess = load_reference(os.path.abspath(ref_dir), work_dir)
        if '--example' in sys.argv:
            case = example_case(ref_dir)
            (rec,), _ = run_reference(preprocess, work_dir, [case])
            rec.pop('bow_vec_object_attr_feats')                                 # no attributes in this case
            print(f"reference: {len(case['vertices'])} points, {rec['objects_count']} objects, {rec['edges_count']} edges, {len(rec['triples'])} triples")
            np.random.seed(case['seed'])
            yard = SG.record_ref(case['scan_id'], case['vertices'], case['objects'], case['relationships'], SG.REL2IDX, case['resolutions'], 50)
            yard['bow_vec_object_edge_feats'] = SG.bow_edge_ref(yard, SG.REL2IDX)
            SG.assert_records_equal(yard, rec, what='yardstick')
            print('yardstick == reference, bit for bit')
            import torch
            if torch.cuda.is_available():
                from sgaligner_amd.preprocessing import scene_graphs
                np.random.seed(case['seed'])
                mine = scene_graphs.process_scan(case['scan_id'], case['vertices'], case['objects'], case['relationships'], SG.REL2IDX,
                                                 case['resolutions'], 50)
                SG.assert_records_equal(mine, rec, skip=('rel_trans',), what='device')
                print('device == reference; rel_trans differs by', np.abs(mine['rel_trans'] - rec['rel_trans']).max())
            return
        cases = SG.fixture_cases()
        records, vocab = run_reference(preprocess, work_dir, cases)
    out = {'n_cases': np.int64(len(cases)), 'rel_names': np.array(json.dumps(SG.REL_NAMES)), 'word_2_ix': np.array(json.dumps(SG.WORD_2_IX)),
           'attr_vocabulary': np.array(json.dumps(vocab))}
    for k, (case, rec) in enumerate(zip(cases, records)):
        out.update(SG.pack_case(f'c{k}_', case, rec))
        print(case['scan_id'], -1 if isinstance(rec, int) else (rec['objects_count'], rec['edges_count'], len(rec['triples'])))
    path = os.path.join(ROOT, 'tests', 'golden', 'scenegraph_cases.npz')
    write_npz(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
