"""Time the sparse GAT route (csrc/gat_sparse.hip) at 2 heads x 128 channels, forward and backward, with the structure build on its own:
  (a) BASELINE configs[1]'s graph mix, 1024 complete graphs of 64 nodes, beside the dense route at the same shape in the same
      process -- the ratio is reported, not gated: the default stays dense and is expected to win there;
  (b) 8 graphs of 1024 nodes with 16 n random pairs;   (c) one complete graph of 1000 nodes;
  (d) the 601-node double star 256 times (two segments of 601 entries among 1200 of 2: what one wave per destination costs under skew).
For (b)-(d) the dense route cannot run (more than 256 nodes per graph), so there is no earlier figure: each time stands beside the bytes
the kernels must move -- entries x channels x 4 per head and gather pass (one forward, two backward), plus the output rows -- and the
rate that implies.  Median of ROUNDS rounds of ITERS launches after WARMUP launches, HIP events.  Writes profiles/gat_sparse_bench.json.
Needs the card:  python tools/bench_gat_sparse.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gat_general_gate import _complete as complete  # noqa: E402
from gat_sparse_gate import double_star  # noqa: E402
from sgaligner_amd import ops  # noqa: E402

HEADS, C = 2, 128
WARMUP, ROUNDS, ITERS = 3, 7, 10


def timed(fn):
    """Median, min, max over ROUNDS of the mean time of ITERS back-to-back launches, in microseconds."""
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


def cases():
    rng = np.random.default_rng(0)
    yield 'a', '1024 complete graphs of 64 nodes (configs[1])', 1024, 64, [complete(64)] * 1024
    yield 'b', '8 graphs of 1024 nodes, 16 n random pairs each', 8, 1024, [rng.integers(0, 1024, size=(16 * 1024, 2)).astype(np.int64) for _ in range(8)]
    yield 'c', 'one complete graph of 1000 nodes', 1, 1000, [complete(1000)]
    yield 'd', 'the 601-node double star 256 times', 256, 601, [double_star(601)] * 256


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gat_sparse_bench.json')
    gen = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    hc = HEADS * C
    rows = []
    for tag, text, G, N, lists in cases():
        edges = torch.from_numpy(np.concatenate(lists)).cuda()
        gb = ops.GraphBatch(np.full(G, N), np.asarray([len(e) for e in lists]), edges)
        T = G * N
        h, a_s, a_d, b, d_o = rnd(T, hc), rnd(hc) / C ** 0.5, rnd(hc) / C ** 0.5, rnd(hc), rnd(T, hc)
        build = timed(lambda: ops.SparseGraph(gb))
        sp = gb.sparse()
        U = int(sp.row_ptr[-1])
        seg = torch.diff(sp.row_ptr).cpu().numpy()
        f = timed(lambda: ops._attn_fwd_sp(h, HEADS, C, a_s, a_d, b, gb))
        w = timed(lambda: ops._attn_bwd_sp(h, d_o, HEADS, C, a_s, a_d, gb))
        out_bytes = T * hc * 4
        model = dict(fwd=U * C * 4 * HEADS + out_bytes, bwd=2 * U * C * 4 * HEADS + out_bytes)
        r = dict(case=tag, what=text, graphs=G, nodes=T, listed_edges=int(edges.shape[0]), entries=U, segment_median=int(np.median(seg)),
                 segment_max=int(seg.max()), build_us=round(build[0], 1), build_min_us=round(build[1], 1), build_max_us=round(build[2], 1))
        for d, t in (('fwd', f), ('bwd', w)):
            r.update({f'{d}_us': round(t[0], 1), f'{d}_min_us': round(t[1], 1), f'{d}_max_us': round(t[2], 1), f'{d}_model_mb': round(model[d] / 1e6, 2),
                      f'{d}_model_tb_per_s': round(model[d] / (t[0] * 1e-6) / 1e12, 3)})
        if tag == 'a':
            assert gb.complete is not None and bool(gb.complete.all())
            df = timed(lambda: ops._attn_fwd_hc(h, HEADS, C, a_s, a_d, b, gb))
            dw = timed(lambda: ops._attn_bwd_hc(h, d_o, HEADS, C, a_s, a_d, gb))
            r.update(dense_fwd_us=round(df[0], 1), dense_bwd_us=round(dw[0], 1), sparse_over_dense_fwd=round(f[0] / df[0], 2),
                     sparse_over_dense_bwd=round(w[0] / dw[0], 2))
        else:
            r.update(dense='cannot run: more than 256 nodes per graph (SGA_ERR_ARG); no earlier figure exists for this shape')
        rows.append(r)
        print(json.dumps(r), flush=True)
    doc = dict(what=f'sparse GAT attention kernels alone at {HEADS} x {C}; median of {ROUNDS} rounds of {ITERS} launches after {WARMUP} warm-up launches, '
                    'HIP events; model bytes = entries x channels x 4 per head and gather pass (1 forward, 2 backward) + the output rows; the '
                    'per-entry index, multiplicity and coefficient traffic is not in the model.  Reference rates for whole-row gathers on this '
                    'card: rows shared out of L2 16.8-18.8 TB/s, out of the Infinity Cache 8.6 TB/s, random rows from HBM 5.5-5.8 TB/s',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
