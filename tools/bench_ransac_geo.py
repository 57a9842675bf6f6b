"""The geometric score of many hypotheses on the device (csrc/ransac_geo.hip through utils/registration.py).
  python tools/bench_ransac_geo.py [--quick] [--out PATH]     # one JSON object to stdout and to PATH (default profiles/ransac_geo_bench.json)
Scoring: V transforms per cloud pair -- the truth followed by a random rotation of up to 3 degrees and a shift of up to 0.03, what
validated hypotheses look like -- at r = 0.05, on a grid that is already there (one build serves every hypothesis).  `fused`:
sga_score_transforms_grid.  `unfused`: the route made of the entry points there were before it -- sga_nn_search_grid with one job per
transform, which writes 12 B per query, then torch reductions over [jobs, nq] (count of idx >= 0, sum of the d2 of those).  The two routes
alternate within every repetition and their counts are asserted equal (sum d2 to 1e-12 relative: the orders of summation differ).
`unfused_bytes`: the per-query outputs the unfused route allocates (the reductions' temporaries come on top).  Shapes: one pair of
10 000 x 10 000 points with 1000 transforms; 45 pairs of 2000 with 1000 each; 200 pairs of 300 (objects) with 1000 each.
End to end: registration_with_ransac_from_feats_pairs on planted pairs of 300 / 400 points at the defaults (50 000 triples, 1000
validations), score='geometric' against score='correspondence', host wall time around the call with a synchronise.
Device events on resident tensors, warm-up first, median (min, max) of `reps` runs.  Reported, not gated."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import featnn_ref as FR
import fpfh_ref as PR
import icp_ref as IR
from sgaligner_amd import _lib
from sgaligner_amd.ops import _p, _stream
from sgaligner_amd.packed import PairJobs, upload, workspace
from sgaligner_amd.utils import point_cloud as PC
from sgaligner_amd.utils import registration as RG
from sgaligner_amd.utils import voxel as V
from sgaligner_amd.utils.features import _Clouds

RADIUS = 0.05


def spread(ms):
    return {'median': round(float(np.median(ms)), 3), 'min': round(float(min(ms)), 3), 'max': round(float(max(ms)), 3)}


def event_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating_ms(fns, reps, warmup=2):
    """{name: fn} -> {name: [ms]}: the routes take turns within every repetition, so drift hits them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(event_once(fn))
    return out


def hypotheses(truth, centre, n, seed):
    """n models: `truth` followed by a rotation of up to 3 degrees about a random axis through `centre` and a shift of up to 0.03."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        P = IR.rigid12(rng.standard_normal(3), rng.uniform(0.0, 3.0), rng.uniform(-0.03, 0.03, 3))
        Rp = P[:9].reshape(3, 3)
        out.append(IR.compose12(np.concatenate([P[:9], centre - Rp @ centre + P[9:]]), truth))
    return np.stack(out)


def scoring_case(name, n_pairs, n_points, n_val, reps):
    T = PR.planted_pair(8, 11)[2]
    truth = np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])
    clouds = []
    for p in range(n_pairs):
        src = PR.surface(n_points, 11 + 2 * p, bump=True)[0]
        ref = PR.surface(n_points, 12 + 2 * p, bump=True)[0] @ T[:3, :3].T + T[:3, 3]
        clouds += [src, ref]
    tr = [hypotheses(truth, clouds[1].mean(0), n_val, 0)] * n_pairs         # every pair samples the same surface: one list serves all
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    pairs = np.repeat(np.array([(2 * p, 2 * p + 1) for p in range(n_pairs)]), n_val, axis=0)
    pts, d_tr = torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(np.concatenate(tr)).cuda()
    J = PairJobs(off, pts.shape[0], pairs, 'bench', 'cloud')
    C = _Clouds(pts, J.off)
    G = V.build_grid(C, None, PC.nn_grid_cell(C, RADIUS))
    d_off, d_pr, d_oo = upload(J.host_parts(), pts.device)
    L, n, r2 = _lib.lib(), J.n_pairs, RADIUS * RADIUS
    dist = torch.empty((J.total_q,), device='cuda', dtype=torch.float64)
    idx = torch.empty((J.total_q,), device='cuda', dtype=torch.int32)
    count = torch.empty((n,), device='cuda', dtype=torch.int32)
    sum_d2 = torch.empty((n,), device='cuda', dtype=torch.float64)
    ws_bytes = int(L.sga_score_transforms_workspace_bytes(n, J.max_q))
    ws = workspace(ws_bytes, pts.device)
    res = {}

    # the search launches a workgroup of 256 threads per four queries: the unfused job list goes in as many calls as keep a launch below
    # 2^32 threads (45 x 1000 jobs of 2000 queries are 5.8e9)
    per_call = max(1, (2 ** 32 - 1) // 256 // -(-J.max_q // 4))
    calls = [(a, min(n, a + per_call), np.ascontiguousarray(J.h_pr[a:a + per_call])) for a in range(0, n, per_call)]

    def unfused():
        for a, b, h_pr in calls:
            rc = L.sga_nn_search_grid(_p(pts), _p(d_off), J.n_sets, int(pts.shape[0]), _p(d_pr[2 * a:2 * b]), b - a, _p(d_oo[a:b]), J.total_q, J.max_q,
                                      J.h_off.ctypes.data, h_pr.ctypes.data, _p(G.cell), _p(G.origin), _p(G.dims), _p(G.status), _p(G.order),
                                      _p(G.sorted_keys), _p(d_tr[a:b]), r2, 1, _p(dist), _p(idx), _stream())
            _lib.check(rc, 'sga_nn_search_grid')
        has = idx.view(n, n_points) >= 0                                 # every job of a case has n_points queries
        res['unfused'] = (has.sum(1).to(torch.int32), torch.where(has, dist.view(n, n_points), torch.zeros_like(dist[:1])).sum(1))

    def fused():
        rc = L.sga_score_transforms_grid(_p(pts), _p(d_off), J.n_sets, int(pts.shape[0]), _p(d_pr), n, J.max_q, J.h_off.ctypes.data,
                                         J.h_pr.ctypes.data, _p(G.cell), _p(G.origin), _p(G.dims), _p(G.status), _p(G.order), _p(G.sorted_keys),
                                         _p(d_tr), None, r2, _p(count), _p(sum_d2), _p(ws), ws_bytes, _stream())
        _lib.check(rc, 'sga_score_transforms_grid')
        res['fused'] = (count, sum_d2)

    ms = alternating_ms({'unfused': unfused, 'fused': fused}, reps)
    (uc, us), (fc, fs) = res['unfused'], res['fused']
    assert torch.equal(uc, fc), name
    assert bool(((us - fs).abs() <= 1e-12 * us.abs()).all()), name
    fit = fc.double().mean().item() / n_points
    print(f'[bench_ransac_geo] {name}: done', file=sys.stderr, flush=True)
    return {'case': name, 'pairs': n_pairs, 'points': n_points, 'transforms_per_pair': n_val, 'jobs': n, 'queries': J.total_q,
            'mean_fitness': round(fit, 4), 'unfused_ms': spread(ms['unfused']), 'fused_ms': spread(ms['fused']),
            'speedup': round(float(np.median(ms['unfused']) / np.median(ms['fused'])), 3), 'unfused_bytes': 12 * J.total_q, 'unfused_calls': len(calls),
            'fused_workspace_bytes': ws_bytes}


def end_to_end(n_pairs, iters, val, reps):
    clouds = []
    for s in range(n_pairs):
        c = FR.planted_registration(s, 300, 100)
        ref = c['ref'] + np.random.default_rng(1000 + s).uniform(-0.03, 0.03, c['ref'].shape)
        clouds.append((c['src'], ref, c['src_feats'], c['ref_feats']))
    out = {'pairs': n_pairs, 'num_iterations': iters, 'val_iterations': val}
    for score in RG.RANSAC_SCORES:
        ms = []
        for k in range(reps + 1):                                        # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RG.registration_with_ransac_from_feats_pairs(clouds, num_iterations=iters, val_iterations=val, score=score)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        out[score + '_wall_ms'] = spread(ms[1:])
    return out


def main(argv):
    quick = '--quick' in argv
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'ransac_geo_bench.json')
    reps, n_val = (3, 50) if quick else (9, 1000)
    out = {'device': torch.cuda.get_device_name(0), 'radius': RADIUS, 'reps': reps,
           'scoring': [scoring_case('one pair of 10 000', 1, 10000, n_val, reps), scoring_case('45 pairs of 2000', 45, 2000, n_val, reps),
                       scoring_case('200 object pairs of 300', 200, 300, n_val, reps)],
           'end_to_end': end_to_end(4 if quick else 16, 5000 if quick else 50000, n_val, 3 if quick else 9)}
    text = json.dumps(out, indent=1)
    print(text)
    with open(path, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
