"""GPU: the sparse GCN route (csrc/gcn_sparse.hip) -- the same bits as the dense route wherever that route can run, exact against fp64 where it
cannot (long rows and columns, a pair listed 1023 times), the fp32-faithful gate of tests/gcn_sparse_gate.py over the light graph mix for
stacks of one, two and three layers, the exact properties the route promises (repeatable bits, a graph alone = the graph in a batch, edge order
irrelevant, out-of-range endpoints dropped), the 300-fold pair the dense route cannot count, 'auto', and EVA on a 300-object scene."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import eva_gate as EG  # noqa: E402
import gat_general_gate as GG  # noqa: E402
import gat_sparse_gate as SG  # noqa: E402
import gcn_sparse_gate as CG  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTHS = (1, 3, 200, 256, 257, 400)        # one lane, a ragged slot, the EVA widths, a full slab, one channel into the second slab
PROBE_C = 257


def _mix():
    return SG.mix_graphs('light', torch.Generator().manual_seed(0))


def _small(graphs):
    """The graphs of the mix the dense route can take: at most 256 nodes, without the 300-fold pair."""
    return [g for i, g in enumerate(graphs) if g[0] <= 256 and i != SG.FOLD_AT]


def _aggregate(h, graphs, route, bias=None, **kw):
    from sgaligner_amd import ops
    out = ops.gcn_aggregate(h.float().cuda().contiguous(), GG.graph_batch(graphs), None if bias is None else bias.float().cuda(), route=route, **kw)
    torch.cuda.synchronize()
    return out


def _three(h, graphs, route, bias):
    """The three uses of the aggregation: forward with bias, forward with bias and ReLU, transpose."""
    return (_aggregate(h, graphs, route, bias), _aggregate(h, graphs, route, bias, relu=True), _aggregate(h, graphs, route, transpose=True))


# ------------------------------------------------------------------------------------------------ 1. the same bits as the dense route
@pytest.mark.parametrize('C', WIDTHS)
def test_aggregation_has_the_dense_routes_bits(C):
    graphs = _small(_mix())
    assert [g[0] for g in graphs] == [1, 2, 3, 64, 65, 0, 7, 40]
    gen = torch.Generator().manual_seed(100 + C)
    T = sum(g[0] for g in graphs)
    h, bias = torch.randn(T, C, generator=gen), torch.randn(C, generator=gen)
    for d, s, what in zip(_three(h, graphs, 'dense', bias), _three(h, graphs, 'sparse', bias), ('bias', 'bias + relu', 'transpose')):
        assert torch.equal(d, s), (C, what, (d - s).abs().max().item())
    assert (_aggregate(h, graphs, 'sparse', bias, relu=True) == 0).any() or C == 1


def _recorded_stack_run(units, graphs, layers, x, cot, route, monkeypatch):
    """gcn_sparse_gate.stack_run with every aggregation call of the step recorded in order: (transpose, input, output)."""
    from sgaligner_amd import gcn_ops
    calls, real = [], gcn_ops.gcn_aggregate

    def recording(h, gb, bias=None, transpose=False, **kw):
        out = real(h, gb, bias, transpose=transpose, **kw)
        calls.append((bool(transpose), h, out))
        return out
    monkeypatch.setattr(gcn_ops, 'gcn_aggregate', recording)
    try:
        return CG.stack_run(units, graphs, layers, x, cot, route=route), calls
    finally:
        monkeypatch.setattr(gcn_ops, 'gcn_aggregate', real)


@pytest.mark.parametrize('units', [(3, 200, 400), (3, 48, 100, 32)])
def test_stacks_have_the_dense_routes_bits(units, monkeypatch):
    """MultiGCN on the two routes: the output, every bias gradient and EVERY aggregation of the step, forward and transposed -- so both
    operands of every weight-gradient GEMM -- are torch.equal.
    The weight gradients themselves are torch.equal wherever ops.gemm_plan walks K in one piece.  Where it splits K (the library's
    weight-gradient routes add their S partial sums with fp32 atomics, in an order that two runs of the SAME route do not share: measured
    here, dense against sparse, one ulp on layer 0's dW), equal operands are all a route can promise, and dW is held to what a reordering
    of S partial sums can move an entry by: S u sum |terms|, u = 2^-24."""
    from sgaligner_amd import ops
    graphs = _small(_mix())
    gen = torch.Generator().manual_seed(7 + len(units))
    T = sum(g[0] for g in graphs)
    L = len(units) - 1
    layers = [(EG._glorot(gen, units[i + 1], units[i]), (torch.rand(units[i + 1], generator=gen) * 2 - 1) * 0.1) for i in range(L)]
    x, cot = torch.randn(T, units[0], generator=gen), torch.randn(T, units[-1], generator=gen)
    (dense, dcalls), (sparse, scalls) = (_recorded_stack_run(units, graphs, layers, x, cot, r, monkeypatch) for r in ('dense', 'sparse'))
    assert set(dense) == set(CG.outputs_of(units))
    assert [c[0] for c in dcalls] == [c[0] for c in scalls] == [False] * L + [True] * L
    for n, (d, s) in enumerate(zip(dcalls, scalls)):
        assert torch.equal(d[1], s[1]) and torch.equal(d[2], s[2]), ('aggregation call', n)
    assert torch.equal(dense['gcn_out'], sparse['gcn_out'])
    for i in range(L):
        assert torch.equal(dense[f'gcn_gb{i}'], sparse[f'gcn_gb{i}']), i
        dh, xin = scalls[2 * L - 1 - i][2], (x.cuda() if i == 0 else scalls[i - 1][2])        # the GEMM's operands: dW_i = dh_i^T x_i
        route, splits, _ = ops.gemm_plan(True, False, units[i + 1], units[i], T)
        a, b = dense[f'gcn_gw{i}'], sparse[f'gcn_gw{i}']
        print(f'layer {i}: dW on {route}, {splits} K splits, max |dense - sparse| = {(a - b).abs().max().item():.3e}')
        if splits == 1:
            assert torch.equal(a, b), i
        else:
            assert splits <= 8
            room = splits * 2.0 ** -24 * (dh.abs().double().t() @ xin.abs().double())
            assert ((a.double() - b.double()).abs() <= room).all(), (i, route, splits)


# ------------------------------------------------------------------------------------------------ 2. exact where the dense route cannot go
def _exact_graphs():
    """Every degree is a power of four, so every dinv is a power of two: a 1-node graph, a 1024-node in-star (j -> 0: the centre's row has 1024
    entries, deg 1024), a 1024-node out-star with every edge 0 -> j listed three times (the centre's column has 1024 entries of multiplicity 3,
    deg_j = 4), 5 nodes without edges, and 4 nodes with the pair (1 -> 2) listed 1023 times (deg 1024; a count 8 bits cannot hold)."""
    j = np.arange(1, 1024, dtype=np.int64)
    z = np.zeros_like(j)
    none = np.zeros((0, 2), dtype=np.int64)
    return [(1, none, False), (1024, np.stack([j, z], 1), False), (1024, np.repeat(np.stack([z, j], 1), 3, axis=0), False), (5, none, False),
            (4, np.repeat(np.asarray([[1, 2]], dtype=np.int64), 1023, axis=0), False)]


@pytest.mark.parametrize('C', (3, 200, 400))
def test_aggregation_exact_beyond_the_dense_route(C):
    """Integer inputs in [-8, 8], coefficients m / 2^k: every term and every partial sum is a multiple of the graph's smallest coefficient and
    stays far below 2^24 of them, so any correct evaluation equals the fp64 reference bit for bit -- forward, forward with ReLU, transpose."""
    graphs = _exact_graphs()
    adj = CG.BlockAdjacency(graphs)
    degs = sorted({int(round(1.0 / float(v))) for a in adj.blocks for v in torch.diagonal(a)})         # the self loop's entry is 1 / deg
    assert set(degs) <= {1, 4, 16, 1024} and 1024 in degs and 4 in degs, degs
    gen = torch.Generator().manual_seed(C)
    off = GG._offsets(graphs)
    h = torch.randint(-8, 9, (int(off[-1]), C), generator=gen).double()
    bias = torch.randint(-8, 9, (C,), generator=gen).double()
    for gi, a in enumerate(adj.blocks):                                  # per graph: every coefficient is a multiple of its smallest one
        step = float(a[a > 0].min())
        assert torch.equal(a / step, (a / step).round()) and 1.0 / step == round(1.0 / step)
        ha = h[off[gi]:off[gi + 1]].abs()
        bound = max(float((a @ ha).max()), float((a.t() @ ha).max())) + 8.0
        print(f'C = {C}, graph {gi}: the largest sum of magnitudes is {bound:.1f} = {bound / step:.0f} steps of {step}')
        assert bound / step < 2.0 ** 24 / 16
    want = (adj.mm(h) + bias, (adj.mm(h) + bias).clamp_min(0), adj.tmm(h))
    got = _three(h, graphs, 'sparse', bias)
    for w, g, what in zip(want, got, ('bias', 'bias + relu', 'transpose')):
        assert torch.equal(g.cpu().double(), w), (C, what, (g.cpu().double() - w).abs().max().item())
    with pytest.raises(RuntimeError, match='at most 256 per graph'):
        _aggregate(h, graphs, 'dense', bias)


# ------------------------------------------------------------------------------------------------ 3. the gate
@pytest.mark.parametrize('which', range(len(CG.CASES)))
def test_stack_cases_pass_the_gate(which):
    units = CG.CASES[which]
    meas = CG.measure(which)
    assert tuple(meas) == CG.outputs_of(units)
    CG.assert_gate(meas, f'sparse GCN {list(units)} light mix')


# ------------------------------------------------------------------------------------------------ 4. the properties the route promises
@functools.lru_cache(maxsize=1)
def _probe():
    graphs = _mix()
    gen = torch.Generator().manual_seed(12)
    T = sum(g[0] for g in graphs)
    h, bias = torch.randn(T, PROBE_C, generator=gen), torch.randn(PROBE_C, generator=gen)
    return graphs, h, bias, _three(h, graphs, 'sparse', bias)


def test_two_runs_give_the_same_bits():
    graphs, h, bias, base = _probe()
    for a, b in zip(base, _three(h, graphs, 'sparse', bias)):
        assert torch.equal(a, b)


def test_a_graph_alone_has_the_bits_it_has_in_the_batch():
    graphs, h, bias, base = _probe()
    off = GG._offsets(graphs)
    for gi, n in ((8, 257), (SG.STAR_AT, SG.STAR), (SG.FOLD_AT, 130)):
        assert graphs[gi][0] == n
        rows = slice(int(off[gi]), int(off[gi + 1]))
        for a, b in zip(_three(h[rows], [graphs[gi]], 'sparse', bias), base):
            assert torch.equal(a, b[rows]), n


def test_edge_order_changes_no_bit():
    graphs, h, bias, base = _probe()
    for a, b in zip(_three(h, SG.shuffled(graphs, 5), 'sparse', bias), base):
        assert torch.equal(a, b)


def test_out_of_range_endpoints_change_no_bit(monkeypatch):
    """50 edges with an endpoint outside their graph (negative, == N, huge) are dropped: the outputs are those of the run without them."""
    from sgaligner_amd import ops
    monkeypatch.setattr(ops, 'VALIDATE', False)                          # the host-side range check would (rightly) object to this batch
    graphs, h, bias, base = _probe()
    rng = np.random.default_rng(11)
    live = [i for i, g in enumerate(graphs) if g[0] > 0]
    extra = {}
    for t in range(50):
        gi = live[int(rng.integers(len(live)))]
        n = graphs[gi][0]
        bad = (-1, n, 2 ** 40, -2 ** 35, n + 7)[t % 5]
        inside = int(rng.integers(n))
        extra.setdefault(gi, []).append((bad, inside) if t % 2 else (inside, bad))
    other = []
    for gi, (n, e, c) in enumerate(graphs):
        if gi in extra:
            e = np.concatenate([e, np.asarray(extra[gi], dtype=np.int64)])
            e = e[rng.permutation(len(e))]
        other.append((n, e, c))
    assert sum(len(g[1]) for g in other) == sum(len(g[1]) for g in graphs) + 50
    for a, b in zip(_three(h, other, 'sparse', bias), base):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. the 300-fold pair
def test_the_300_fold_pair_is_counted_where_the_dense_route_saturates():
    from sgaligner_amd import ops
    c = CG.case(0)
    gi = SG.FOLD_AT
    n, e, _ = c['graphs'][gi]
    assert n == 130 and int(((e[:, 0] == SG.FOLD_PAIR[0]) & (e[:, 1] == SG.FOLD_PAIR[1])).sum()) >= SG.FOLD_COPIES > 255
    off = GG._offsets(c['graphs'])
    rows = slice(int(off[gi]), int(off[gi + 1]))
    x, g = c['x'][rows], c['g'][rows]
    ref = CG._reference([c['graphs'][gi]], c['layers'], x, g)
    yard = CG.gcn_chain(x, CG.BlockAdjacency([c['graphs'][gi]], torch.float32), c['layers'], g, torch.float32, masks=ref['masks'])[0]
    keys = CG.outputs_of(c['units'])
    ke = CG.gcn_errors(CG.stack_run(c['units'], [c['graphs'][gi]], c['layers'], x, g), ref, keys)
    ye = CG.gcn_errors(yard, ref, keys)
    CG.assert_gate({k: (ke[k], ye[k]) for k in keys}, 'sparse GCN [3, 200, 400], 130 nodes with a 300-fold pair')
    # the dense route on the same graph: its 8-bit count saturates and the status word says so (existing behaviour, shown for the difference)
    ops.DEFERRED_CHECKS.flush()
    ops.gcn_aggregate(torch.randn(130, 8).cuda(), GG.graph_batch([c['graphs'][gi]]), check_status=True)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='more than 255 times'):
        ops.DEFERRED_CHECKS.flush()
    ops.DEFERRED_CHECKS.flush()


# ------------------------------------------------------------------------------------------------ 6. 'auto'
def test_auto_switches_at_257_nodes(monkeypatch):
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    mix = _mix()
    small, large = _small(mix), _small(mix) + [mix[8]]
    assert max(g[0] for g in small) == 65 and large[-1][0] == 257
    for units in ([3, 200, 400], [3, 48, 100, 32]):
        outs, seen = {}, {}
        for graphs, tag in ((small, 'small'), (large, 'large')):
            x = torch.randn(sum(g[0] for g in graphs), 3, generator=torch.Generator().manual_seed(4)).cuda()
            for route in ('auto', 'dense'):
                torch.manual_seed(5)
                net = MultiGCN(units, route=route).cuda()
                events = {}
                monkeypatch.setattr(ops, 'KERNEL_EVENTS', events)
                try:
                    if (tag, route) == ('large', 'dense'):
                        with pytest.raises(RuntimeError, match='at most 256 per graph'):
                            net.forward_batched(x, GG.graph_batch(graphs))
                        continue
                    outs[tag, route] = net.forward_batched(x, GG.graph_batch(graphs))
                    torch.cuda.synchronize()
                finally:
                    monkeypatch.setattr(ops, 'KERNEL_EVENTS', None)
                seen[tag, route] = {k for k in events if k.startswith('gcn_')}
        assert seen['small', 'auto'] == seen['small', 'dense'] == {'gcn_aggregate'} and seen['large', 'auto'] == {'gcn_sp_aggregate'}, seen
        assert torch.equal(outs['small', 'auto'], outs['small', 'dense'])


# ------------------------------------------------------------------------------------------------ 7. EVA end to end
def test_eva_on_a_300_object_scene():
    """EVA(gcn_route='auto') on one pair of 300 and 40 objects against tests/eva_ref.py in fp64: the gcn and joint tables and the four GCN
    parameter gradients of one cotangent pass the gate; gcn_route='dense' refuses the same batch."""
    from sgaligner_amd.aligner.eva import EVA
    from sgaligner_amd.synthetic import to_device
    CG.assert_gate(CG.measure_eva(), "EVA gcn_route='auto', 300 + 40 objects")
    dd, sd, _, _, _ = CG.eva_case()
    dense = EVA(modules=list(EG.EVA_MODULES), rel_dim=41, attr_dim=164, gcn_route='dense').cuda()
    with pytest.raises(RuntimeError, match='at most 256 per graph'):
        dense(to_device(dd, 'cuda'))


def test_reference_signature_on_a_700_node_graph():
    """MultiGCN.forward(x, edges) -- one graph, edges [2, E] -- with route='auto' on the 700-node graph of the mix: the bits of forward_batched."""
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    n, e, _ = _mix()[9]
    assert n == 700
    torch.manual_seed(6)
    net = MultiGCN([3, 200, 400], route='auto').cuda()
    x = torch.randn(n, 3, generator=torch.Generator().manual_seed(8)).cuda()
    out = net(x, torch.from_numpy(np.ascontiguousarray(e.T)).cuda())
    want = net.forward_batched(x, GG.graph_batch([(n, e, False)]))
    torch.cuda.synchronize()
    assert out.shape == (700, 400) and torch.isfinite(out).all() and torch.equal(out, want)
    ref = CG.gcn_chain(x.cpu(), CG.BlockAdjacency([(n, e)]), [(l.lin.weight.detach().cpu(), l.bias.detach().cpu()) for l in net.layer_stack],
                       torch.zeros(n, 400), torch.float64)[0]['gcn_out']
    assert (out.detach().cpu().double() - ref).abs().max().item() < 1e-4
