"""Time the dense GAT attention kernels: forward and backward at (heads, channels) = (2, 128) -- the reference model's shape, on the kernels
written for it -- and (2, 100), (8, 32), (1, 256) on the general ones, over BASELINE configs[1]'s graph mix (1024 complete graphs of 64
nodes: the fast path, features LDS-resident).  Every figure stands beside the 2 x 128 row's time from the same run.  Writes
profiles/gat_general_bench.json.  Needs the card:  python tools/bench_gat_general.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sgaligner_amd import ops  # noqa: E402

G, N = 1024, 64
SHAPES = ((2, 128), (2, 100), (8, 32), (1, 256))
WARMUP, ROUNDS, ITERS = 5, 7, 20


def timed(fn):
    """Median over ROUNDS of the mean time of ITERS back-to-back launches, in microseconds (HIP events on the current stream)."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1000.0 / ITERS)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gat_general_bench.json')
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    one = np.stack([ii[ii != jj], jj[ii != jj]], 1).astype(np.int64)
    gb = ops.GraphBatch(np.full(G, N), np.full(G, len(one)), torch.from_numpy(np.tile(one, (G, 1))).cuda())
    assert gb.complete is not None and bool(gb.complete.all())
    gen = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    rows, base = [], {}
    for heads, c in SHAPES:
        hc = heads * c
        h, a_s, a_d, b, d_o = rnd(G * N, hc), rnd(hc) / c ** 0.5, rnd(hc) / c ** 0.5, rnd(hc), rnd(G * N, hc)
        f = timed(lambda: ops._attn_fwd_hc(h, heads, c, a_s, a_d, b, gb))
        w = timed(lambda: ops._attn_bwd_hc(h, d_o, heads, c, a_s, a_d, gb))
        for d, t in (('fwd', f), ('bwd', w)):
            base.setdefault(d, t[0])                                     # SHAPES[0] is 2 x 128
            rows.append(dict(heads=heads, channels=c, direction=d, us=round(t[0], 2), min_us=round(t[1], 2), max_us=round(t[2], 2),
                             ratio_to_2x128=round(t[0] / base[d], 3),
                             us_per_feature_mb=round(t[0] / (G * N * hc * 4 / 2 ** 20), 3)))
            print(json.dumps(rows[-1]), flush=True)
    doc = dict(what=f'attention kernels alone, {G} complete graphs of {N} nodes (configs[1]); median of {ROUNDS} rounds of {ITERS} launches after '
                    f'{WARMUP} warm-up launches, HIP events; ratio_to_2x128 = against the 2 x 128 row of the same run',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
