"""Offset attention next to self-attention: the forward and backward kernels of both in one process, alternating, at T = 160 (the
reference-default step: 4 pairs x ~40 objects) and T = 2048 objects of N = 512 points; then the 'pct' training step of tools/bench_pct_step.py
with attention 'sa' and 'oa'.  Writes profiles/pct_oa_bench.json.  Reported, not gated.
  python tools/bench_pct_oa.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sgaligner_amd import _lib  # noqa: E402
from sgaligner_amd.ops import _p, _stream  # noqa: E402
from sgaligner_amd.synthetic import make_batch, to_device  # noqa: E402
from sgaligner_amd.trainer import AlignerSteps  # noqa: E402

N = 512
ROUNDS, REPS = 7, 5


def kernels(T):
    """Median over ROUNDS of the mean of REPS launches, SA and OA taking turns inside every round."""
    L, st = _lib.lib(), _stream()
    gen = torch.Generator(device='cuda').manual_seed(T)
    R = T * N
    q = torch.randn(R, 32, device='cuda', generator=gen) * 0.5
    v, g, x = (torch.randn(R, 128, device='cuda', generator=gen) for _ in range(3))
    out, dq, dv = torch.empty(R, 128, device='cuda'), torch.empty(R, 32, device='cuda'), torch.empty(R, 128, device='cuda')
    diff = torch.empty(R, 128, device='cuda')
    stats, work = torch.empty(3 * R, device='cuda'), torch.empty(130 * R, device='cuda')
    calls = {
        'sa_fwd': lambda: L.sga_pct_attention(_p(q), 32, _p(v), 128, T, N, _p(stats), _p(out), 128, st),
        'oa_fwd': lambda: L.sga_pct_offset_attention(_p(q), 32, _p(v), 128, _p(x), 128, T, N, _p(stats), _p(out), 128, _p(diff), 128, st),
        'sa_bwd': lambda: L.sga_pct_attention_bwd(_p(q), 32, _p(v), 128, _p(g), 128, T, N, _p(stats), _p(work), _p(dq), 32, _p(dv), 128, st),
        'oa_bwd': lambda: L.sga_pct_offset_attention_bwd(_p(q), 32, _p(v), 128, _p(out), 128, _p(g), 128, -1.0, T, N, _p(stats), _p(work), _p(dq), 32,
                                                         _p(dv), 128, st),
    }
    # each backward reads the statistics (and OA its Xr) of its own forward: run that forward just before timing it
    before = {'sa_bwd': 'sa_fwd', 'oa_bwd': 'oa_fwd'}
    times = {k: [] for k in calls}
    for rnd in range(ROUNDS + 1):
        for name, fn in calls.items():
            if name in before:
                assert calls[before[name]]() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                assert fn() == 0
            e1.record()
            torch.cuda.synchronize()
            if rnd:                                   # round 0 warms up
                times[name].append(e0.elapsed_time(e1) / REPS)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = dict(T=T, N=N, **{k + '_ms': round(v, 4) for k, v in med.items()},
               **{k + '_spread': round((max(v) - min(v)) / sorted(v)[len(v) // 2], 3) for k, v in times.items()},
               oa_over_sa_fwd=round(med['oa_fwd'] / med['sa_fwd'], 3), oa_over_sa_bwd=round(med['oa_bwd'] / med['sa_bwd'], 3))
    print(json.dumps(row), flush=True)
    return row


def step(attention, n=30):
    dev = torch.device('cuda:0')
    steps = AlignerSteps(['pct', 'gat', 'rel', 'attr'], device=dev, seed=42, pct_attention=attention)
    dd = [to_device(make_batch(4, 40, 512, seed=7 + i, ragged=True), dev) for i in range(4)]
    for i in range(6):
        steps.forward_backward(dd[i % 4])
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(n):
            steps.forward_backward(dd[i % 4])
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / n * 1e3)
    row = dict(attention=attention, step_ms=round(sorted(runs)[1], 3), runs_ms=[round(r, 3) for r in runs],
               objects_per_step=sum(int(d['tot_obj_pts'].shape[0]) for d in dd) / 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'pct_oa_bench.json')
    doc = dict(what='SA and OA attention kernels (forward: statistics + apply; backward: all its launches) alternating in one process, median of '
                    f'{ROUNDS} rounds of {REPS} launches, ms; spread = (max - min) / median over the rounds; then the pct+gat+rel+attr training '
                    'step (forward + backward, 4 pairs x ~40 objects x 512 points), median of 3 runs of 30 steps',
               device=torch.cuda.get_device_name(0), kernels=[kernels(160), kernels(2048)], steps=[step('sa'), step('oa'), step('sa'), step('oa')])
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
