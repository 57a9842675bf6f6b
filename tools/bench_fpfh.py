"""FPFH descriptors on the device (csrc/fpfh.hip through utils/features.py) next to the host route on the same box: scipy's
cKDTree.query(k=max_nn, distance_upper_bound=radius) for the neighbour lists plus the vectorised numpy of tests/fpfh_ref.py for normals,
census and weighting.
  python tools/bench_fpfh.py [--quick] [--out PATH]     # one JSON object to stdout and to PATH (default profiles/fpfh_bench.json)
Two shapes: two clouds of 10 000 points (RegistrationEvaluator.run_normal_registration), and 200 objects of 50..2000 points in one call (the
node pairs of one scan pair through FeatureMatcher.match_many).  Normals from the 30 nearest neighbours (the reference's default),
features from at most 100 neighbours within a radius.
Device figures: `stages_ms` and `chain_ms` are device-event times on resident tensors (each stage alone; fpfh_batch as a whole), after a
warm-up, median (min, max) of `reps` runs.  `descriptor_many_ms` is host wall time of FPFHDescriptor.many -- numpy in, numpy out: upload,
the launch set, one download -- ending with the data on the host, which is what the host route's wall time is compared with
(`host_over_device`).  The host route runs `host_reps` times, objects grouped into batches of about 20 000 points so that its [n, k, 3]
temporaries stay in memory.  Its answer is not compared here: the tests pin the kernels against the same yardstick.  Reported, not gated."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import fpfh_ref as PR
from sgaligner_amd import _lib
from sgaligner_amd.utils import features as F

MAX_NN_NORMAL, MAX_NN_FEATURE = 30, 100


def spread(ms):
    return {'median': round(float(np.median(ms)), 3), 'min': round(float(min(ms)), 3), 'max': round(float(max(ms)), 3)}


def event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def kdtree_lists(p, radius, max_nn):
    """The host route's neighbour lists for one cloud -> (count, idx, d2) in the layout of fpfh_ref.lists_ref."""
    from scipy.spatial import cKDTree
    k = min(max_nn, len(p))
    dist, idx = cKDTree(p).query(p, k=k, distance_upper_bound=np.inf if radius is None else radius)
    dist, idx = dist.reshape(len(p), k), idx.reshape(len(p), k)
    found = np.isfinite(dist)
    count = found.sum(1).astype(np.int32)
    out_i = np.full((len(p), max_nn), -1, dtype=np.int32)
    out_d = np.full((len(p), max_nn), np.inf)
    out_i[:, :k] = np.where(found, idx, -1)
    out_d[:, :k] = np.where(found, dist * dist, np.inf)
    return count, out_i, out_d


def host_route(clouds, radius_feature, viewpoint, batch_points=20000):
    """cKDTree per cloud, then normals / census / weighting vectorised over batches of clouds (indices made batch-global)."""
    out, batch, size = [], [], 0
    for c in list(clouds) + [None]:
        if c is not None and (not batch or size + len(c) <= batch_points):
            batch.append(c)
            size += len(c)
            continue
        base = np.concatenate([[0], np.cumsum([len(b) for b in batch])])
        pts = np.concatenate(batch)

        def packed(radius, max_nn):
            parts = [kdtree_lists(b, radius, max_nn) for b in batch]
            idx = np.concatenate([np.where(q[1] >= 0, q[1] + o, -1) for q, o in zip(parts, base)])
            return np.concatenate([q[0] for q in parts]), idx, np.concatenate([q[2] for q in parts])

        nr = PR.normals_ref(pts, packed(None, MAX_NN_NORMAL), viewpoint)['normals']
        lf = packed(radius_feature, MAX_NN_FEATURE)
        out.append(PR.fpfh_ref(PR.spfh_ref(pts, nr, lf)[0], lf).astype(np.float32))
        batch, size = ([c], len(c)) if c is not None else ([], 0)
    return out


def case(name, clouds, radius_feature, reps, host_reps):
    vp = np.array([0.5, 0.5, 5.0])
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    vps = torch.from_numpy(np.tile(vp, (len(clouds), 1))).cuda()
    ln = F.neighbour_lists(pts, off, None, MAX_NN_NORMAL)
    nr, _ = F.estimate_normals_batch(pts, off, viewpoints=vps, lists=ln)
    lf = F.neighbour_lists(pts, off, radius_feature, MAX_NN_FEATURE)
    cn = F.spfh_counts(pts, nr, off, lf)
    stages = {
        'knn_lists_normal': lambda: F.neighbour_lists(pts, off, None, MAX_NN_NORMAL),
        'normals': lambda: F.estimate_normals_batch(pts, off, viewpoints=vps, lists=ln),
        'knn_lists_feature': lambda: F.neighbour_lists(pts, off, radius_feature, MAX_NN_FEATURE),
        'spfh_counts': lambda: F.spfh_counts(pts, nr, off, lf),
        'fpfh': lambda: F.fpfh_from_counts(cn, lf, offsets=off),
    }
    out = {'case': name, 'clouds': len(clouds), 'points': [int(min(map(len, clouds))), int(max(map(len, clouds)))], 'total_points': int(off[-1]),
           'max_nn_normal': MAX_NN_NORMAL, 'radius_feature': radius_feature, 'max_nn_feature': MAX_NN_FEATURE,
           'mean_feature_list': round(float(lf[0].float().mean()), 1), 'reps': reps, 'host_reps': host_reps,
           'stages_ms': {k: spread(event_ms(fn, reps)) for k, fn in stages.items()},
           'chain_ms': spread(event_ms(lambda: F.fpfh_batch(pts, off, None, None, MAX_NN_NORMAL, radius_feature, MAX_NN_FEATURE, vps), reps))}
    desc = F.FPFHDescriptor(None, MAX_NN_NORMAL, radius_feature, MAX_NN_FEATURE, viewpoint=vp)
    desc.many(clouds)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        desc.many(clouds)
        wall.append((time.perf_counter() - t0) * 1e3)
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        host_route(clouds, radius_feature, vp)
        host.append((time.perf_counter() - t0) * 1e3)
    out['descriptor_many_ms'], out['host_route_ms'] = spread(wall), spread(host)
    out['host_over_device'] = round(out['host_route_ms']['median'] / out['descriptor_many_ms']['median'], 1)
    return out


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_fpfh needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'fpfh_bench.json')
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()),
           'timing': 'stages_ms / chain_ms: device events on resident tensors; descriptor_many_ms / host_route_ms: host wall time, numpy in, '
                     'numpy out; warm-up first, median (min, max) of the runs',
           'host_route': 'scipy.spatial.cKDTree.query(k=max_nn, distance_upper_bound=radius) + the vectorised numpy of tests/fpfh_ref.py, '
                         'same box', 'cases': []}
    n = 2000 if quick else 10000
    reps, host_reps = (5, 1) if quick else (9, 3)
    two = [PR.surface(n, 1)[0], PR.surface(n, 2)[0]]
    out['cases'].append(case(f'two clouds of {n} points', two, 0.1 if not quick else 0.2, reps, host_reps))
    print(json.dumps(out['cases'][-1]), file=sys.stderr, flush=True)
    sizes = rng.integers(50, 2001, 40 if quick else 200)
    objects = [PR.surface(int(s), 100 + i)[0] for i, s in enumerate(sizes)]
    out['cases'].append(case(f'{len(objects)} objects of 50..2000 points', objects, 0.25, reps, 1))
    print(json.dumps(out['cases'][-1]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
