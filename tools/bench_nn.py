"""Exact nearest-neighbour search (csrc/nnsearch.hip) against the route it replaces, cKDTree build + query on one thread in the same process.
  python tools/bench_nn.py [--quick]        # one JSON object to stdout and to profiles/nn_bench.json
Per case: `kernel_ms` = sga_nn_search alone on resident data (HIP events, after warm-up, median of the repeats); `call_ms` = the whole
numpy -> numpy call (upload, launch, download; host clock, ends in a synchronise); `ckdtree_ms` = tree build + query; `speedup` = ckdtree / call.
`gop_per_s` counts 11 fp64 operations per (query, support) pair over kernel time and is compared with the part's published vector fp64
rate (78.6 TFLOP/s counting an FMA as two: 39.3 T instructions/s for this kernel, which may not fuse) -- a spec figure, not a measurement."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy.spatial import cKDTree

from sgaligner_amd import _lib
from sgaligner_amd.ops import _p, _stream
from sgaligner_amd.utils import point_cloud as pc

SPEC_FP64_INSTR_PER_S = 78.6e12 / 2
OPS_PER_PAIR = 11


def scan_cloud(n, rng):
    return (rng.standard_normal((n, 3)) * np.array([4.0, 3.0, 0.8])).astype(np.float32).astype(np.float64)


def kernel_ms(clouds, pairs, reps):
    """sga_nn_search alone: everything resident, buffers allocated once."""
    sizes = np.array([len(c) for c in clouds], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pr = np.ascontiguousarray(pairs, dtype=np.int32)
    nq, ns = sizes[pr[:, 0]], sizes[pr[:, 1]]
    oo = np.concatenate([[0], np.cumsum(nq)])
    total_q = int(oo[-1])
    chunk = pc._nn_chunk(nq, ns)
    dev = 'cuda'
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_off, d_pr, d_oo = (torch.from_numpy(a).to(dev) for a in (off, pr.reshape(-1), oo[:-1].astype(np.int32)))
    dist = torch.empty(total_q, device=dev, dtype=torch.float64)
    idx = torch.empty(total_q, device=dev, dtype=torch.int32)
    L = _lib.lib()
    wsb = int(L.sga_nn_workspace_bytes(total_q, int(ns.max()), chunk))
    ws = torch.empty(max((wsb + 7) // 8, 1), device=dev, dtype=torch.float64)

    def go():
        _lib.check(L.sga_nn_search(_p(pts), _p(d_off), len(sizes), int(pts.shape[0]), _p(d_pr), len(pr), _p(d_oo), total_q, int(nq.max()),
                                   int(ns.max()), chunk, off.ctypes.data, pr.ctypes.data, 0, _p(dist), _p(idx), _p(ws), wsb, _stream()), 'sga_nn_search')
    go()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), chunk, wsb, float((nq * ns).sum())


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def case(name, clouds, pairs, reps, kd_reps):
    k_ms, chunk, wsb, n_pairs_eval = kernel_ms(clouds, pairs, reps)
    if len(pairs) == 1:
        (a, b), = pairs
        call = host_ms(lambda: pc.get_nearest_neighbor(clouds[a], clouds[b], return_index=True), reps)
    else:
        call = host_ms(lambda: pc.compute_pcl_overlap_pairs(clouds, pairs), reps)
    kd = []
    for _ in range(kd_reps):
        t0 = time.perf_counter()
        for a, b in pairs:
            cKDTree(clouds[b]).query(clouds[a], k=1)
        kd.append((time.perf_counter() - t0) * 1e3)
    kd = float(np.median(kd))
    rate = n_pairs_eval * OPS_PER_PAIR / (k_ms * 1e-3)
    return {'case': name, 'jobs': len(pairs), 'points': [int(len(c)) for c in clouds][:2], 'chunk': chunk, 'workspace_bytes': wsb,
            'kernel_ms': round(k_ms, 3), 'call_ms': round(call, 3), 'ckdtree_ms': round(kd, 3), 'speedup_call_vs_ckdtree': round(kd / call, 2),
            'gop_per_s': round(rate / 1e9, 1), 'share_of_spec_fp64_vector_rate': round(rate / SPEC_FP64_INSTR_PER_S, 3)}


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_nn needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()), 'ops_per_pair': OPS_PER_PAIR,
           'compared_with': 'published vector fp64 rate 78.6 TFLOP/s (FMA = 2) -> 39.3e12 instructions/s; a spec figure, not measured here',
           'ckdtree': 'scipy.spatial.cKDTree(s).query(q, k=1): build + query, one thread, same process', 'cases': []}
    sizes = [20_000, 200_000] + ([] if quick else [1_000_000])
    for n in sizes:
        clouds = [scan_cloud(n, rng), scan_cloud(n, rng)]
        big = n >= 1_000_000
        out['cases'].append(case(f'{n} x {n}', clouds, [(0, 1)], 2 if big else 7, 1 if big else 3))
        print(json.dumps(out['cases'][-1]), file=sys.stderr, flush=True)
    clouds = [scan_cloud(50_000, rng) for _ in range(10)]
    pairs = [(i, j) for i in range(10) for j in range(i + 1, 10)]
    out['cases'].append(case('45 jobs of 50000 x 50000 (the C(10, 2) subscan pairs of a scan)', clouds, pairs, 5, 1))
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'nn_bench.json'), 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main(sys.argv[1:])
