"""Batched RANSAC rigid registration (csrc/ransac.hip) at the reference's configuration: 5000 three-point hypotheses against up to 20000
correspondences, threshold 0.03, two refinement rounds.
  python tools/bench_ransac.py [--quick]        # one JSON object to stdout and to profiles/ransac_bench.json
Per case: `pipeline_ms` = sga_ransac_rigid alone on resident data (every kernel; HIP events, after warm-up, median of the repeats);
`score_ms` = the same call stopped after the scoring stage (hypothesis fit + ransac_score_kernel + count fold; refine_rounds = -1);
`call_ms` = the whole numpy -> numpy find_rigid_transform[_pairs] call (shift, sample draw, upload, launches, download; host clock).
`gop_per_s` counts 15 fp64 instructions per (hypothesis, row) over score_ms -- so it charges the two small kernels around the scoring
kernel and their launch gaps to it -- and is compared with the 33.1e12 instructions/s nn_kernel sustains (profiles/nn_bench.json), a kernel
of the same broadcast-LDS, register-resident structure.  `yardstick_ms`: tests/ransac_ref.py (numpy, one thread) on the first case."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import ransac_ref as RR
from sgaligner_amd import _lib
from sgaligner_amd.ops import _p, _stream
from sgaligner_amd.utils import registration as rg

NN_KERNEL_INSTR_PER_S = 33.1e12
OPS_PER_TEST = 15
THRESHOLD = 0.03
ROUNDS = 2


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


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


def case(name, corrs, iters, reps):
    sizes = [len(c) for c in corrs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    samples, hoff = rg.draw_samples(sizes, iters, 0)
    d_corr = torch.from_numpy(np.concatenate(corrs)).cuda()
    d_samples = torch.from_numpy(samples).cuda()
    chunk = rg._ransac_chunk(sizes, np.diff(hoff))
    # sga_ransac_rigid alone: everything resident, buffers allocated once
    L = _lib.lib()
    n_jobs, total, total_h = len(corrs), int(off[-1]), len(samples)
    h_off, h_hoff = off.astype(np.int32), hoff.astype(np.int32)
    d_off, d_hoff = torch.from_numpy(h_off).cuda(), torch.from_numpy(h_hoff).cuda()
    T = torch.empty((n_jobs, 4, 4), device='cuda', dtype=torch.float64)
    cnt, best, status = (torch.empty(n_jobs, device='cuda', dtype=torch.int32) for _ in range(3))
    mask = torch.empty(total, device='cuda', dtype=torch.uint8)
    hyp_count = torch.empty(total_h, device='cuda', dtype=torch.int32)
    wsb = int(L.sga_ransac_workspace_bytes(n_jobs, total_h, max(sizes), chunk))
    ws = torch.empty((wsb + 7) // 8, device='cuda', dtype=torch.float64)

    def go(rounds):
        _lib.check(L.sga_ransac_rigid(_p(d_corr), _p(d_off), n_jobs, total, _p(d_samples), _p(d_hoff), total_h, max(sizes), iters, chunk,
                                      h_off.ctypes.data, h_hoff.ctypes.data, THRESHOLD, rounds, _p(T), _p(cnt), _p(best), _p(status), _p(mask),
                                      _p(hyp_count), _p(ws), wsb, _stream()), 'sga_ransac_rigid')
    full = event_ms(lambda: go(ROUNDS), reps)
    score = event_ms(lambda: go(-1), reps)
    if len(corrs) == 1:
        call = host_ms(lambda: rg.find_rigid_transform(corrs[0], THRESHOLD, iters, 0, ROUNDS), reps)
    else:
        call = host_ms(lambda: rg.find_rigid_transform_pairs(corrs, THRESHOLD, iters, 0, ROUNDS), reps)
    res = rg.find_rigid_transform_batch(d_corr, off, d_samples, hoff, THRESHOLD, ROUNDS)
    tests = float(sum(n * iters for n in sizes))
    rate = tests * OPS_PER_TEST / (score * 1e-3)
    return {'case': name, 'jobs': len(corrs), 'rows': sizes[0], 'hypotheses': iters, 'chunk': chunk,
            'workspace_bytes': wsb,
            'pipeline_ms': round(full, 4), 'score_ms': round(score, 4), 'call_ms': round(call, 3),
            'pipeline_ms_per_job': round(full / len(corrs), 4), 'score_ms_per_job': round(score / len(corrs), 4),
            'gop_per_s': round(rate / 1e9, 1), 'ratio_to_nn_kernel_rate': round(rate / NN_KERNEL_INSTR_PER_S, 3),
            'inliers_first_job': int(res['inlier_count'][0]), 'status_sum': int(res['status'].sum())}


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_ransac needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    torch.set_num_threads(1)
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()), 'ops_per_test': OPS_PER_TEST,
           'threshold': THRESHOLD, 'refine_rounds': ROUNDS,
           'compared_with': 'the 33.1e12 fp64 instructions/s nn_kernel sustains (profiles/nn_bench.json); reported, not gated',
           'cases': []}
    big = [RR.make_case('loose', 20000, 50 + j)[0] for j in range(1 if quick else 45)]
    plan = [('1 job of 20000 x 5000 (the reference configuration)', big[:1], 5000, 15)]
    if not quick:
        plan.append(('45 jobs of 20000 x 5000', big, 5000, 5))
    plan.append(('1 job of 2000 x 5000', [RR.make_case('loose', 2000, 99)[0]], 5000, 15))
    for name, corrs, iters, reps in plan:
        out['cases'].append(case(name, corrs, iters, reps))
        print(json.dumps(out['cases'][-1]), file=sys.stderr, flush=True)
    samples, _ = rg.draw_samples([20000], 500 if quick else 5000, 0)
    t0 = time.perf_counter()
    ref = RR.ransac_ref(big[0], samples, THRESHOLD, ROUNDS)
    out['yardstick'] = {'case': out['cases'][0]['case'], 'hypotheses': len(samples), 'yardstick_ms': round((time.perf_counter() - t0) * 1e3, 1),
                        'inliers': int(ref['count']), 'what': 'tests/ransac_ref.py: numpy fp64, one thread, one SVD and one residual pass per hypothesis'}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'ransac_bench.json'), 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main(sys.argv[1:])
