"""Scene-graph records (csrc/scenegraph.hip, preprocessing/scene_graphs.py) beside the host statement of the reference's process_scan.
  python tools/bench_scenegraphs.py [--quick] [--out FILE]     # one JSON object to stdout and to profiles/scenegraphs_bench.json (or FILE)
Cases: one synthetic subscan of about 100 000 points x 40 objects (tests/scenegraph_ref.make_scan) and a batch of 64 such subscans.  Per
case: `kernel_ms` = each entry point alone on resident data (HIP events, after warm-up, median of the repeats): sga_object_counts,
sga_object_partition (its three launches), sga_graph_complete; `call_ms` = process_scans, NumPy in -> records out, with the packing, every
upload, launch and download, the hulls and the farthest-point samples (host clock); `host_ms` = tests/scenegraph_ref.record_ref, the NumPy
statement of the reference (Qhull and the NumPy FPS included), one thread, same process -- measured on ONE scan and, for the batch,
multiplied by the number of scans (marked as such).  No ratio is promised anywhere: the file records what was observed."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import scenegraph_ref as SG
from sgaligner_amd.preprocessing import scene_graphs as G

RESOLUTIONS = (512, 128)


def event_ms(fn, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def make_case(seed, n_points=100000, n_objects=40):
    rng = np.random.default_rng(seed)
    sizes = rng.multinomial(n_points - 2000, rng.dirichlet(np.full(n_objects, 2.0))).tolist()
    v, objs = SG.make_scan(seed, sizes, background=2000)
    ids = [int(o['id']) for o in objs]
    rels = [SG._rel(a, b, SG.REL_NAMES[1 + int(k) % 6]) for k, (a, b) in enumerate(zip(ids, ids[1:] + ids[:1]))]
    rels.insert(3, SG._rel(ids[0], ids[1], 'bigger than'))                             # one pair listed with two relations
    return (f'scan_{seed}', v, objs, rels)


def kernels(scans, reps):
    pts = [np.stack([s[1]['x'], s[1]['y'], s[1]['z']]).transpose((1, 0)) for s in scans]
    uniq = [np.unique(s[1]['objectId'], return_inverse=True) for s in scans]
    L = G.SlotLayout(np.concatenate([[0], np.cumsum([len(p) for p in pts])]), np.concatenate([[0], np.cumsum([len(u[0]) for u in uniq])]), device='cuda')
    d_pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(pts), dtype=np.float32)).cuda()
    d_slot = torch.from_numpy(np.concatenate([u[1].reshape(-1) for u in uniq]).astype(np.int32)).cuda()
    counts = G.object_counts_batch(d_slot, L).cpu().numpy().astype(np.int64)
    dest = np.concatenate([[0], np.cumsum(counts)])[:-1]
    n = [len(u[0]) for u in uniq]
    pairs = [np.stack([np.arange(k), (np.arange(k) + 1) % k], axis=1) for k in n]
    rels = [np.arange(k + 1) % 41 for k in n]
    out = {}
    for name, fn in (('object_counts', lambda: G.object_counts_batch(d_slot, L)),
                     ('object_partition', lambda: G.object_partition_batch(d_pts, d_slot, L, dest, counts)),
                     ('graph_complete', lambda: G.graph_complete_batch(n, pairs, rels, 0, 41))):
        fn()
        torch.cuda.synchronize()
        med, lo, hi = event_ms(fn, reps)
        out[name] = {'median_ms': med, 'min_ms': lo, 'max_ms': hi,
                     'note': 'wrapper call between two events: includes its small uploads' + (' and the download of the edges' if name == 'graph_complete' else '')}
    return out


def run_case(name, scans, reps, host_scans=1):
    res = {'scans': len(scans), 'points': int(sum(len(s[1]) for s in scans)), 'objects': int(sum(len(s[2]) for s in scans)),
           'resolutions': list(RESOLUTIONS), 'kernel_ms': kernels(scans, reps)}
    times = []
    for _ in range(reps + 1):                                                          # the first call warms up
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = G.process_scans(scans, SG.REL2IDX, RESOLUTIONS, 50)
        times.append((time.perf_counter() - t0) * 1e3)
    res['call_ms'] = {'median_ms': float(np.median(times[1:])), 'min_ms': float(min(times[1:])), 'max_ms': float(max(times[1:])), 'first_ms': times[0]}
    res['records'] = int(sum(not isinstance(r, int) for r in recs))
    res['edges'] = int(sum(r['edges_count'] for r in recs if not isinstance(r, int)))
    t0 = time.perf_counter()
    for s in scans[:host_scans]:
        np.random.seed(0)
        SG.record_ref(*s, SG.REL2IDX, RESOLUTIONS, 50)
    one = (time.perf_counter() - t0) * 1e3 / host_scans
    res['host_ms'] = {'per_scan_ms': one, 'total_ms': one * len(scans), 'extrapolated': len(scans) > host_scans}
    return res


def main():
    quick = '--quick' in sys.argv
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'scenegraphs_bench.json')
    if not torch.cuda.is_available():
        sys.exit('bench_scenegraphs needs a HIP device')
    reps = 3 if quick else 7
    n_batch = 8 if quick else 64
    result = {'device': torch.cuda.get_device_name(0), 'graph_max_nodes': G.graph_max_nodes(), 'partition_tile': G.partition_tile(), 'cases': {}}
    result['cases']['one_subscan'] = run_case('one_subscan', [make_case(100)], reps)
    result['cases'][f'batch_{n_batch}'] = run_case(f'batch_{n_batch}', [make_case(100 + k) for k in range(n_batch)], max(reps // 2, 2))
    text = json.dumps(result, indent=1)
    print(text)
    with open(out_path, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
