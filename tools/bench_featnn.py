"""Feature-space nearest-neighbour search (csrc/featnn.hip through utils/registration.feature_nn_batch) next to torch.cdist(...).argmin(1)
on the same device.
  python tools/bench_featnn.py [--quick] [--out PATH]     # one JSON object to stdout and to PATH (default profiles/featnn_bench.json)
Every figure is WHOLE-CALL wall time on resident device tensors: host clock from the call to the end of a device synchronise, so it holds
the wrapper's host work (tile list, one small upload, allocations) and every kernel of the launch set.  Both routes are warmed up, then
timed alternately in the same run, `reps` times each; the median is reported with the minimum and maximum beside it.  `tflops` counts
2 * nq * ns * C per job (C the caller's width, not the padded one) over that time; `share_of_fp32_matrix_peak` is that over 157.3 TFLOP/s,
the part's published fp32 matrix rate -- a spec figure, not measured here.  torch.cdist runs job by job (it has no ragged batch form) and
its answer is not compared here: the tests pin the kernel against an fp64 yardstick.  Reported, not gated."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from sgaligner_amd import _lib
from sgaligner_amd.utils import registration as RG

PEAK_FP32_MATRIX = 157.3e12


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return {'median': round(float(np.median(ms)), 3), 'min': round(float(min(ms)), 3), 'max': round(float(max(ms)), 3)}


def case(name, sizes, pairs, c, reps, rng):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    feats = torch.from_numpy(rng.standard_normal((int(off[-1]), c)).astype(np.float32)).cuda()
    sets = [feats[off[i]:off[i + 1]] for i in range(len(sizes))]

    def ours():
        RG.feature_nn_batch(feats, off, pairs)

    def cdist():
        for a, b in pairs:
            torch.cdist(sets[a], sets[b]).argmin(1)

    for fn in (ours, cdist, ours, cdist):                      # warm-up: code objects, allocator pools
        timed(fn)
    t_ours, t_cdist = [], []
    for _ in range(reps):                                      # alternating: both see the same clocks and neighbours
        t_ours.append(timed(ours))
        t_cdist.append(timed(cdist))
    nq, ns = np.asarray(sizes)[[a for a, _ in pairs]], np.asarray(sizes)[[b for _, b in pairs]]
    flop = 2.0 * float((nq.astype(np.float64) * ns).sum()) * c
    o, t = spread(t_ours), spread(t_cdist)
    rate = flop / (o['median'] * 1e-3)
    return {'case': name, 'C': c, 'jobs': len(pairs), 'rows': [int(min(sizes)), int(max(sizes))], 'chunk': RG._featnn_chunk(nq, ns), 'reps': reps,
            'feature_nn_batch_ms': o, 'torch_cdist_argmin_ms': t, 'tflops': round(rate / 1e12, 2),
            'share_of_fp32_matrix_peak': round(rate / PEAK_FP32_MATRIX, 3), 'torch_tflops': round(flop / (t['median'] * 1e-3) / 1e12, 2)}


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_featnn needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'featnn_bench.json')
    rng = np.random.default_rng(0)
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()),
           'timing': 'whole call on resident tensors, host clock ending in a device synchronise; median (min, max) of `reps` alternating runs',
           'compared_with': 'published fp32 matrix rate 157.3 TFLOP/s; a spec figure, not measured here', 'cases': []}
    n = 2000 if quick else 10000
    ragged = [int(v) for v in rng.integers(200, 4001, 64)]
    for c in (256, 33):
        out['cases'].append(case(f'{n} x {n}, both directions', [n, n], [(0, 1), (1, 0)], c, 5 if quick else 9, rng))
        print(json.dumps(out['cases'][-1]), file=sys.stderr, flush=True)
        out['cases'].append(case('32 ragged jobs of 200..4000 rows', ragged, [(2 * j, 2 * j + 1) for j in range(32)], c, 5 if quick else 9, rng))
        print(json.dumps(out['cases'][-1]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
