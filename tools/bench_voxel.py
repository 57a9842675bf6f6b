"""The voxel grid on the device (csrc/voxel.hip through utils/voxel.py and utils/features.py): voxel down-sampling by stage, and the grid
route of the neighbour lists against the brute route.
  python tools/bench_voxel.py [--quick] [--out PATH]     # one JSON object to stdout and to PATH (default profiles/voxel_bench.json)
Down-sampling: two clouds of 200 000 points at a voxel size that leaves about 10 000 voxels each, and 200 objects of 50..2000 points.
`stages_ms` (keys, torch.sort, cells, means) and `call_ms` (voxel_downsample_batch: the stages plus the one small download that sizes the
outputs) are device-event times on resident tensors.  Beside the two-cloud case: `device_wall_ms`, host wall time of voxel_downsample_many
-- numpy in, numpy out -- and `host_route_ms`, the yardstick's definition vectorised with np.add.at, same box, ending with the data on the
host.  Lists: search='grid' against search='brute' at 2 x 10 000, 2 x 50 000 and 1 x 200 000 points for (30 nearest, no radius) and (at
most 100 within a radius), the two routes alternating in the same run; `cell` swept over four values around the default rule
(voxel.default_cell); `sort_share` is torch.sort's share of the grid route at the default cell.  Warm-up first, median (min, max) of
`reps` runs.  The answers are not compared here: the tests pin the kernels.  Reported, not gated."""
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
from sgaligner_amd.ops import _p, _stream
from sgaligner_amd.utils import features as F
from sgaligner_amd.utils import voxel as V


def spread(ms):
    return {'median': round(float(np.median(ms)), 3), 'min': round(float(min(ms)), 3), 'max': round(float(max(ms)), 3)}


def event_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [event_once(fn) for _ in range(reps)]


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


def host_downsample(p, h):
    """The contract's definition on the host, vectorised: keys, a stable argsort, np.add.at for the sums (not the pinned summation order)."""
    origin = p.min(0) - 0.5 * h
    k = np.floor((p - origin) / h).astype(np.int64)
    key = (k[:, 0] << 32) | (k[:, 1] << 16) | k[:, 2]
    uniq, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    acc = np.zeros((len(uniq), 3))
    np.add.at(acc, inv, p)
    return acc / counts[:, None]


def downsample_case(name, clouds, h, reps, host_reps):
    L = _lib.lib()
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    G = V.build_grid(pts, off, h)
    C = G.clouds
    n, total = C.n_scans, C.total_points
    cell_host = np.full(n, h)
    ws = torch.empty((L.sga_voxel_workspace_bytes(n, total) // 8,), device='cuda', dtype=torch.float64)
    out_pts = torch.empty((total, 3), device='cuda', dtype=torch.float64)
    out_count = torch.empty((total,), device='cuda', dtype=torch.int32)
    status = G.status.clone()

    def keys():
        _lib.check(L.sga_voxel_keys(_p(C.pts), *C.args(), _p(G.cell), cell_host.ctypes.data, _p(G.origin), _p(G.dims), _p(G.keys), _p(status),
                                    _stream()), 'sga_voxel_keys')

    def cells():
        _lib.check(L.sga_voxel_cells(*C.args(), _p(G.keys), _p(G.order), _p(G.sorted_keys), _p(G.voxel_of_point), _p(G.voxel_offsets),
                                     _p(G.voxel_first), _p(status), _p(ws), ws.numel() * 8, _stream()), 'sga_voxel_cells')

    def means():
        _lib.check(L.sga_voxel_downsample(_p(C.pts), None, *C.args(), _p(G.order), _p(G.sorted_keys), _p(G.voxel_offsets), _p(G.voxel_first),
                                          _p(status), _p(out_pts), None, _p(out_count), _stream()), 'sga_voxel_downsample')

    stages = {'keys': keys, 'torch_sort': lambda: torch.sort(G.keys, stable=True)[1].to(torch.int32), 'cells': cells, 'means': means}
    n_vox = np.diff(G.check())
    out = {'case': name, 'clouds': n, 'points': [int(min(map(len, clouds))), int(max(map(len, clouds)))], 'total_points': total, 'voxel_size': h,
           'voxels': [int(n_vox.min()), int(n_vox.max())], 'total_voxels': int(n_vox.sum()), 'reps': reps,
           'stages_ms': {k: spread(event_ms(fn, reps)) for k, fn in stages.items()},
           'call_ms': spread(event_ms(lambda: V.voxel_downsample_batch(pts, off, h), reps))}
    out['sort_share_of_stages'] = round(out['stages_ms']['torch_sort']['median'] / sum(v['median'] for v in out['stages_ms'].values()), 3)
    if host_reps:
        V.voxel_downsample_many(clouds, h)
        wall, host = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            V.voxel_downsample_many(clouds, h)
            wall.append((time.perf_counter() - t0) * 1e3)
        for _ in range(host_reps):
            t0 = time.perf_counter()
            for c in clouds:
                host_downsample(c, h)
            host.append((time.perf_counter() - t0) * 1e3)
        out['device_wall_ms'], out['host_route_ms'], out['host_reps'] = spread(wall), spread(host), host_reps
        out['host_over_device'] = round(out['host_route_ms']['median'] / out['device_wall_ms']['median'], 1)
    return out


def lists_case(name, clouds, max_nn, radius, reps, factors=(0.5, 0.75, 1.5, 2.0)):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    default = V.default_cell(pts, off, radius, max_nn)
    G = V.build_grid(pts, off, default)
    fns = {'brute': lambda: F.neighbour_lists(pts, off, radius, max_nn), 'grid': lambda: F.neighbour_lists(pts, off, radius, max_nn, search='grid'),
           'grid_sort_only': lambda: torch.sort(G.keys, stable=True)[1].to(torch.int32),
           'grid_build_only': lambda: V.build_grid(pts, off, default)}
    for f in factors:
        fns[f'grid_cell_x{f}'] = (lambda f=f: F.neighbour_lists(pts, off, radius, max_nn, search='grid', cell=default * f))
    ms = {k: spread(v) for k, v in alternating_ms(fns, reps).items()}
    return {'case': name, 'clouds': len(clouds), 'total_points': int(off[-1]), 'max_nn': max_nn, 'radius': radius, 'reps': reps,
            'default_cell': [round(float(x), 5) for x in default.cpu().numpy()], 'ms': ms,
            'brute_over_grid': round(ms['brute']['median'] / ms['grid']['median'], 2),
            'sort_share': round(ms['grid_sort_only']['median'] / ms['grid']['median'], 3),
            'build_share': round(ms['grid_build_only']['median'] / ms['grid']['median'], 3)}


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_voxel needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'voxel_bench.json')
    rng = np.random.default_rng(0)
    reps = 3 if quick else 9
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()),
           'timing': 'device events on resident tensors, warm-up first, median (min, max) of `reps` runs, the routes of one lists case taking '
                     'turns within every repetition; device_wall_ms / host_route_ms: host wall time, numpy in, numpy out',
           'host_route': 'keys, np.unique and np.add.at per cloud, same box', 'downsample': [], 'lists': []}

    def emit(kind, case):
        out[kind].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)

    n = 20000 if quick else 200000
    emit('downsample', downsample_case(f'two clouds of {n} points', [PR.surface(n, 1)[0], PR.surface(n, 2)[0]], 0.03 if quick else 0.0105, reps, 1 if quick else 3))
    sizes = rng.integers(50, 2001, 40 if quick else 200)
    objects = [PR.surface(int(s), 100 + i)[0] for i, s in enumerate(sizes)]
    emit('downsample', downsample_case(f'{len(objects)} objects of 50..2000 points', objects, 0.05, reps, 0))
    shapes = [(2, 2000)] if quick else [(2, 10000), (2, 50000), (1, 200000)]
    for n_clouds, n in shapes:
        clouds = [PR.surface(n, 10 + c)[0] for c in range(n_clouds)]
        # the radius holds about 150 points of the surface, as 0.1 does at 10 000: more than max_nn, so the cut is by rank
        for max_nn, radius in ((30, None), (100, round(0.1 * (10000 / n) ** 0.5, 4))):
            emit('lists', lists_case(f'{n_clouds} x {n} points', clouds, max_nn, radius, reps))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
