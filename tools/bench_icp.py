"""The cross-cloud grid search and ICP on the device (csrc/icp.hip through utils/point_cloud.py and utils/registration.py).
  python tools/bench_icp.py [--quick] [--out PATH]     # one JSON object to stdout and to PATH (default profiles/icp_bench.json)
Search: the queries of one surface, moved by a transform 3 degrees off, against another surface of the same size -- 10 000, 50 000 and
200 000 points each -- at r = 0.05 and without a radius.  `brute`: sga_nn_search on the moved points (moved beforehand, not timed) and no
mask; `grid`: nearest_neighbor_batch(search='grid') as a user calls it, the grid build with its torch.sort included, at the default cell
(point_cloud.nn_grid_cell: about 16 points per occupied cell, never above the radius); `grid_search_only`: sga_nn_search_grid on a grid
that is already there (ICP's case: one build, many searches); `first_rule` / `first_rule_search_only`: the same at the cell rule first
tried -- the radius where one is given, else voxel.default_cell(max_nn=1), half a point per cell; `cells_search_only_ms`: the search alone
at 0.5 .. 64 points per occupied cell.  The routes alternate within every repetition and their outputs are asserted equal, bit for bit.
ICP: one pair of 10 000, 45 pairs of 10 000, one pair of 200 000, point-to-point and point-to-plane, max_distance 0.05.  `call_ms`: sga_icp
with 10 iterations that never stop early (negative thresholds); `round_ms` = (call(10) - call(0)) / 10, one search + accumulate + step;
the mean round of a run (the search gets faster as the clouds close in); `search_first_ms` / `search_last_ms`: sga_nn_search_grid alone at
the start and at the final transforms; `evaluation`: sga_icp(max_iters=0) on a grid that is already there (zero-fill, search, accumulate,
step); `accumulate_step_ms` = evaluation - search_first (a difference of medians).  Device events on resident tensors, warm-up first, median (min, max) of `reps` runs.  Reported, not gated."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import fpfh_ref as PR
import icp_ref as IR
from sgaligner_amd import _lib
from sgaligner_amd.ops import _p, _stream
from sgaligner_amd.packed import PairJobs, upload
from sgaligner_amd.utils import point_cloud as PC
from sgaligner_amd.utils import registration as RG
from sgaligner_amd.utils import voxel as V
from sgaligner_amd.utils.features import _Clouds


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


def pair_of(n, seed=0):
    """(source, reference, start [12]): two samplings of the bumped surface, the start 3 degrees and (0.02, -0.01, 0.015) off."""
    src, ref = PR.surface(n, 11 + 2 * seed, bump=True)[0], PR.surface(n, 12 + 2 * seed, bump=True)
    c = ref[0].mean(0)
    P = IR.rigid12([0.2, -0.1, 1.0], 3.0, [0.02, -0.01, 0.015])
    return src, ref[0], ref[1], np.concatenate([P[:9], c - P[:9].reshape(3, 3) @ c + P[9:]])


def grid_search_fn(pts, J, G, d_tr, r2, dist, idx):
    L = _lib.lib()
    d_off, d_pr, d_oo = upload(J.host_parts(), pts.device)

    def run():
        rc = L.sga_nn_search_grid(_p(pts), _p(d_off), J.n_sets, int(pts.shape[0]), _p(d_pr), J.n_pairs, _p(d_oo), J.total_q, J.max_q,
                                  J.h_off.ctypes.data, J.h_pr.ctypes.data, _p(G.cell), _p(G.origin), _p(G.dims), _p(G.status), _p(G.order),
                                  _p(G.sorted_keys), _p(d_tr), r2, 1, _p(dist), _p(idx), _stream())
        _lib.check(rc, 'sga_nn_search_grid')
    return run


def search_case(n, radius, reps):
    src, ref, _, start = pair_of(n)
    pts, off, pairs = torch.from_numpy(np.concatenate([src, ref])).cuda(), [0, n, 2 * n], [(0, 1)]
    d_tr = torch.from_numpy(start[None]).cuda()
    moved = torch.from_numpy(np.concatenate([IR.move(src, start), ref])).cuda()
    r2 = float('inf') if radius is None else radius * radius
    J = PairJobs(off, 2 * n, pairs, 'bench_icp', 'cloud')
    fine = V.default_cell(pts, off, radius, 1)
    sweep = (0.5, 2, 4, 8, 16, 32, 64)
    grids = {'grid_search_only': V.build_grid(pts, off, PC.nn_grid_cell(_Clouds(pts, J.off), radius)), 'first_rule_search_only': V.build_grid(pts, off, fine)}
    for per in sweep:
        grids[f'per_cell_{per}'] = V.build_grid(pts, off, V.default_cell(pts, off, None, int(2 * per)))
    outs = {k: (torch.empty((n,), device='cuda', dtype=torch.float64), torch.empty((n,), device='cuda', dtype=torch.int32)) for k in grids}
    res = {}

    def keep(name, fn):
        def run():
            res[name] = fn()
        return run
    fns = {'brute': keep('brute', lambda: PC.nearest_neighbor_batch(moved, off, pairs, squared=True)[:2]),
           'grid': keep('grid', lambda: PC.nearest_neighbor_batch(pts, off, pairs, squared=True, search='grid', radius=radius, transforms=d_tr)[:2]),
           'first_rule': keep('first_rule', lambda: PC.nearest_neighbor_batch(pts, off, pairs, squared=True, search='grid', radius=radius,
                                                                               transforms=d_tr, cell=fine)[:2])}
    for k, G in grids.items():
        fns[k] = grid_search_fn(pts, J, G, d_tr, r2, *outs[k])
    ms = {k: spread(v) for k, v in alternating_ms(fns, reps).items()}
    bd, bi = res['brute']
    keep_mask = bd <= r2
    bd, bi = torch.where(keep_mask, bd, torch.full_like(bd, float('inf'))), torch.where(keep_mask, bi, torch.full_like(bi, -1))
    for k in ('grid', 'first_rule'):
        assert torch.equal(res[k][0].view(torch.int64), bd.view(torch.int64)) and torch.equal(res[k][1], bi), (n, radius, k)
    for k, (d, i) in outs.items():
        assert torch.equal(d.view(torch.int64), bd.view(torch.int64)) and torch.equal(i, bi), (n, radius, k)
    return {'case': f'{n} x {n} points', 'radius': radius, 'within_radius': round(float(keep_mask.double().mean()), 4), 'reps': reps,
            'cell': round(float(grids['grid_search_only'].cell[1]), 5), 'first_rule_cell': round(float(fine[1]), 5),
            'ms': {k: v for k, v in ms.items() if not k.startswith('per_cell_')}, 'outputs_equal': True,
            'cells_search_only_ms': {str(per): ms[f'per_cell_{per}']['median'] for per in sweep},
            'brute_over_grid': round(ms['brute']['median'] / ms['grid']['median'], 2),
            'brute_over_grid_search_only': round(ms['brute']['median'] / ms['grid_search_only']['median'], 2),
            'brute_over_first_rule': round(ms['brute']['median'] / ms['first_rule']['median'], 2),
            'brute_over_first_rule_search_only': round(ms['brute']['median'] / ms['first_rule_search_only']['median'], 2)}


def icp_case(n_pairs, n, method, reps, iters=10):
    data = [pair_of(n, p) for p in range(n_pairs)]
    clouds = [c for s, r, _, _ in data for c in (s, r)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    pairs = [(2 * p, 2 * p + 1) for p in range(n_pairs)]
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    normals = torch.from_numpy(np.concatenate([x for s, _, nr, _ in data for x in (np.zeros_like(s), nr)])).cuda()
    T0 = torch.from_numpy(np.stack([d[3] for d in data])).cuda()
    J = PairJobs(off, int(pts.shape[0]), pairs, 'bench_icp', 'cloud')
    C = _Clouds(pts, J.off)
    G = V.build_grid(C, None, PC.nn_grid_cell(C, 0.05))
    dist, idx = torch.empty((J.total_q,), device='cuda', dtype=torch.float64), torch.empty((J.total_q,), device='cuda', dtype=torch.int32)
    last = {}

    def call(k):
        def run():
            last[k] = RG.icp_batch(pts, off, pairs, T0, 0.05, method, normals, k, -1.0, -1.0)
        return run
    call(iters)()
    T1 = last[iters]['transform'].clone()
    # one evaluation on a grid that is already there: zero-fill, search, accumulate, step
    L = _lib.lib()
    d_off, d_pr, d_oo = upload(J.host_parts(), pts.device)
    pivot = torch.from_numpy(np.stack([d[1].min(0) for d in data])).cuda()
    ws = torch.empty((L.sga_icp_workspace_bytes(n_pairs, J.max_q) // 8 + 1,), device='cuda', dtype=torch.float64)
    T = T0.clone()
    o = {k: torch.empty((n_pairs,), device='cuda', dtype=dt) for k, dt in (('f', torch.float64), ('r', torch.float64), ('i', torch.int32), ('s', torch.int32))}
    trace = torch.empty((n_pairs, 1, 2), device='cuda', dtype=torch.float64)

    def evaluation():
        rc = L.sga_icp(_p(pts), _p(d_off), J.n_sets, int(pts.shape[0]), _p(d_pr), n_pairs, _p(d_oo), J.total_q, J.max_q, J.h_off.ctypes.data,
                       J.h_pr.ctypes.data, _p(G.cell), _p(G.origin), _p(G.dims), _p(G.status), _p(G.order), _p(G.sorted_keys), 0.0025,
                       RG.ICP_METHODS[method], _p(normals), _p(pivot), 0, -1.0, -1.0, _p(T), _p(o['f']), _p(o['r']), _p(o['i']), _p(o['s']),
                       _p(trace), _p(idx), _p(dist), _p(ws), ws.numel() * 8, _stream())
        _lib.check(rc, 'sga_icp')
    fns = {'call_0': call(0), f'call_{iters}': call(iters), 'grid_build': lambda: V.build_grid(C, None, PC.nn_grid_cell(C, 0.05)),
           'evaluation': evaluation, 'search_first': grid_search_fn(pts, J, G, T0, 0.0025, dist, idx),
           'search_last': grid_search_fn(pts, J, G, T1, 0.0025, dist, idx)}
    ms = {k: spread(v) for k, v in alternating_ms(fns, reps).items()}
    assert int(last[iters]['iterations'].min()) == iters and int(last[iters]['status'].max()) == 0
    round_ms = (ms[f'call_{iters}']['median'] - ms['call_0']['median']) / iters
    return {'case': f'{n_pairs} pair(s) of {n} points', 'method': method, 'iters': iters, 'reps': reps, 'ms': ms, 'round_ms': round(round_ms, 3),
            'search_first_ms': ms['search_first']['median'], 'search_last_ms': ms['search_last']['median'],
            'accumulate_step_ms': round(ms['evaluation']['median'] - ms['search_first']['median'], 3),
            'fitness': [round(float(last[0]['fitness'].mean()), 4), round(float(last[iters]['fitness'].mean()), 4)],
            'rmse': [round(float(last[0]['inlier_rmse'].mean()), 5), round(float(last[iters]['inlier_rmse'].mean()), 5)]}


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_icp needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'icp_bench.json')
    reps = 3 if quick else 9
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()),
           'timing': 'device events on resident tensors, warm-up first, median (min, max) of `reps` runs, the routes of one case taking turns '
                     'within every repetition; round_ms and accumulate_step_ms are differences of medians, not timed on their own',
           'search': [], 'icp': []}

    def emit(kind, case):
        out[kind].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)

    for n in ((2000,) if quick else (10000, 50000, 200000)):
        for radius in (0.05, None):
            emit('search', search_case(n, radius, reps))
    for n_pairs, n in (((1, 2000), (3, 2000)) if quick else ((1, 10000), (45, 10000), (1, 200000))):
        for method in ('point', 'plane'):
            emit('icp', icp_case(n_pairs, n, method, reps))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
