"""Time MultiGCN on the sparse route (csrc/gcn_sparse.hip), forward + backward, with the structure build on its own:
  (a) the baseline's own regime: n_units [3, 200, 400] over 1024 complete graphs of 64 nodes, dense route against sparse route in the same
      process -- the ratio is reported, not gated: the default stays dense, and 'auto' stays dense up to 256 nodes whatever it says;
  (b) the sparse route alone where the dense one cannot run: one random graph of 2 000 nodes with 4 n listed pairs, one of 20 000 nodes, and a
      20 000-node star (j -> 0 and 0 -> j: one row and one column of 20 000 entries, walked by one wave each).
Also the four aggregation launches of a step on their own (forward with ReLU, forward, two transposed) beside the bytes they must move
(entries x channels x 4 per gather, plus the output rows).  Median of ROUNDS rounds of ITERS steps after WARMUP steps, HIP events around
each round.  Writes profiles/gcn_sparse_bench.json.
Needs the card:  python tools/bench_gcn_sparse.py [out.json]"""
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
from sgaligner_amd.aligner.networks.gat import MultiGCN  # noqa: E402

UNITS = [3, 200, 400]
WARMUP, ROUNDS, ITERS = 3, 7, 10


def timed(fn):
    """Median, min, max over ROUNDS of the mean time of ITERS back-to-back calls, in microseconds."""
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
    yield 'a', '1024 complete graphs of 64 nodes', 1024, 64, [complete(64)] * 1024
    yield 'b1', 'one random graph of 2 000 nodes, 4 n listed pairs', 1, 2000, [rng.integers(0, 2000, size=(8000, 2)).astype(np.int64)]
    yield 'b2', 'one random graph of 20 000 nodes, 4 n listed pairs', 1, 20000, [rng.integers(0, 20000, size=(80000, 2)).astype(np.int64)]
    yield 'b3', 'the 20 000-node double star', 1, 20000, [double_star(20000)]


def put(r, name, t):
    r.update({f'{name}_us': round(t[0], 1), f'{name}_min_us': round(t[1], 1), f'{name}_max_us': round(t[2], 1)})


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gcn_sparse_bench.json')
    gen = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen)
    rows = []
    for tag, text, G, N, lists in cases():
        edges = torch.from_numpy(np.concatenate(lists)).cuda()
        gb = ops.GraphBatch(np.full(G, N), np.asarray([len(e) for e in lists]), edges)
        T = G * N
        x, cot = rnd(T, UNITS[0]), rnd(T, UNITS[-1])
        nets = {}
        for route in ('sparse', 'dense'):
            torch.manual_seed(1)
            nets[route] = MultiGCN(UNITS, route=route).cuda()

        def step(route):
            net = nets[route]
            for p in net.parameters():
                p.grad = None
            net.forward_batched(x, gb).backward(cot)

        build = timed(lambda: ops.SparseGraph(gb).dinv())
        sp = gb.sparse()
        sp.dinv()
        U = int(sp.row_ptr[-1])
        seg = torch.diff(sp.row_ptr).cpu().numpy()
        r = dict(case=tag, what=text, n_units=UNITS, graphs=G, nodes=T, listed_edges=int(edges.shape[0]), entries=U, row_median=int(np.median(seg)),
                 row_max=int(seg.max()))
        put(r, 'build_with_dinv', build)
        put(r, 'sparse_step', timed(lambda: step('sparse')))
        h0, h1, b0, b1 = rnd(T, UNITS[1]), rnd(T, UNITS[2]), rnd(UNITS[1]), rnd(UNITS[2])

        def aggs(route):
            ops.gcn_aggregate(h0, gb, b0, relu=True, route=route)
            ops.gcn_aggregate(h1, gb, b1, route=route)
            ops.gcn_aggregate(h1, gb, transpose=True, route=route)
            ops.gcn_aggregate(h0, gb, transpose=True, route=route)

        t = timed(lambda: aggs('sparse'))
        put(r, 'sparse_4_aggregations', t)
        model = 2 * (U + T) * (UNITS[1] + UNITS[2]) * 4
        r.update(aggregations_model_mb=round(model / 1e6, 2), aggregations_model_tb_per_s=round(model / (t[0] * 1e-6) / 1e12, 3))
        if tag == 'a':
            d, da = timed(lambda: step('dense')), timed(lambda: aggs('dense'))
            put(r, 'dense_step', d)
            put(r, 'dense_4_aggregations', da)
            r.update(sparse_over_dense_step=round(r['sparse_step_us'] / d[0], 2), sparse_over_dense_aggregations=round(t[0] / da[0], 2))
        else:
            r.update(dense='cannot run: more than 256 nodes per graph (SGA_ERR_ARG); no earlier figure exists for this shape')
        rows.append(r)
        print(json.dumps(r), flush=True)
    doc = dict(what=f'MultiGCN {UNITS} forward + backward per route, the structure build (with dinv) and the four aggregation launches of a step on '
                    f'their own; median of {ROUNDS} rounds of {ITERS} calls after {WARMUP} warm-up calls, HIP events; model bytes = (entries + nodes) '
                    'x channels x 4 per aggregation (gathered rows + output rows); index, multiplicity and dinv traffic is not in the model',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
