"""The fp32-faithful gate of the SPARSE GAT route (csrc/gat_sparse.hip: graphs of any size, no atomics) and the inputs its tests, its profile
and its tools share (no tests in this module).  Reference, yardstick, metric, gate rule and guard are those of gat_general_gate, whose
helpers are imported: fp64 oracle.sga_oracle.gat_conv / multi_gat graph by graph; the same functions in float32 torch on the CPU; flat
envelope in u = 2^-24; eva_gate.gate_ok at r per output kind; every pre-activation on a counted edge clear of LeakyReLU's kink by
2^-16 (|a_s| + |a_d|) in fp64 at the frozen seed -- nothing is excluded from any comparison.

r = ceil(2 x the worst measured kernel / yardstick ratio, rms or max) over the cases of profiles/gat_sparse_accuracy_vs_fp32.json
(tools/gat_sparse_accuracy.py writes it on the card), outputs of one entry apart from those of many (R1 / R below);
tests/test_gat_sparse_cpu.py keeps both tables and the profile together.

Graph mixes: the smallest shapes that cross every boundary of the route -- the 64-entry chunk, the 256-node limit of the dense route, empty
and long segments.
  light   1, 2, 3 nodes (random pairs), 64 complete, 65 random, 0 nodes, 7 without edges, 40 with duplicates and explicit self loops, 257, 700,
          1025 random, a 601-node double star (j -> 0 and 0 -> j: node 0 has 601 entries in its row and its column, 9 chunks and a tail of 25),
          130 random plus the pair (5 -> 9) listed 300 times (more than 8 bits hold)
  dense   light plus 257 complete and 300 nodes with duplicates and explicit self loops (about 63 000 pairs)"""
import functools
import json
import math
import os

import numpy as np
import torch

import eva_gate as EG
import gat_general_gate as GG

PROFILE = os.path.join(GG.ROOT, 'profiles', 'gat_sparse_accuracy_vs_fp32.json')
KERNEL_CASES = (('light', 1, 1), ('light', 2, 65), ('light', 3, 100), ('light', 8, 32), ('light', 1, 256), ('light', 2, 128),
                ('dense', 2, 128), ('dense', 1, 64))                                            # (mix, heads, channels)
STACKS = (((3, 128, 128), (2, 2), False), ((17, 128, 100), (2, 2), True), ((3, 48, 100, 32), (3, 1, 8), False))     # (units, heads, masked)
OUTPUTS = GG.OUTPUTS
STAR, STAR_AT = 601, 11           # the double star and its place in the light mix
FOLD_PAIR, FOLD_COPIES, FOLD_AT = (5, 9), 300, 12

# r per output kind for outputs of MORE THAN ONE entry: ceil(2 x the worst ratio measured, rms or max) over the rows with n > 1 of
# profiles/gat_sparse_accuracy_vs_fp32.json.
R = {'out': 2, 'dw': 4, 'das': 4, 'dad': 7, 'db': 3, 'dx': 3}
# Outputs of ONE entry (d att_src / d att_dst of the 1 x 1 case: a scalar) are judged on their own: R1[kind] = max(R[kind], ceil(2 x the ratio
# of the rows with n = 1)).  Such a scalar is a sum over all 2895 nodes of terms that cancel (|ref| = 0.104 against sum |terms| = 2.8), so in
# units of |ref| both the kernel's error and the yardstick's are single draws of a wide distribution (per-node d a_d is as accurate
# as the yardstick's, the expected error of the scalar is about 300 u, the yardstick's own draw moves between 3 u and 50 u with the order of
# the edge lists) and their ratio says nothing about the outputs of many entries -- nor can a lucky ratio below 1 set a tighter bound than
# those measure, hence the max.
R1 = {'das': 4, 'dad': 85}

# the first seed (from 0) at which the guard holds, per case
SEEDS = {('kernel', 'light', 1, 1): 0, ('kernel', 'light', 2, 65): 0, ('kernel', 'light', 3, 100): 6, ('kernel', 'light', 8, 32): 1,
         ('kernel', 'light', 1, 256): 1, ('kernel', 'light', 2, 128): 0, ('kernel', 'dense', 2, 128): 0, ('kernel', 'dense', 1, 64): 4,
         ('stack', 0): 3, ('stack', 1): 1, ('stack', 2): 27}


def ratios_from_profile(path=PROFILE):
    """(R, R1) as the comments above derive them from the profile."""
    worst, single = {}, {}
    for c in json.load(open(path))['cases']:
        d = single if c['n'] <= 1 else worst
        d[c['output']] = max(d.get(c['output'], 0.0), c['ratio_rms'], c['ratio_max'])
    up = lambda v: int(math.ceil(2.0 * v - 1e-9))
    r = {k: up(v) for k, v in worst.items()}
    return r, {k: max(r[k], up(v)) for k, v in single.items()}


def r_of(output, n):
    k = GG.kind(output)
    return R1[k] if n <= 1 else R[k]


def assert_gate(meas, what=''):
    """gat_general_gate.assert_gate at this route's R / R1: every figure is printed before it is judged."""
    bad = []
    for k, (ke, ye) in meas.items():
        r = r_of(k, ke[2])
        print(f'{what} {k}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | n = {ke[2]} r = {r}')
        if not EG.gate_ok(ke, ye, r):
            bad.append((k, ke, ye, r))
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ graphs
def double_star(n):
    j = np.arange(1, n, dtype=np.int64)
    z = np.zeros_like(j)
    return np.concatenate([np.stack([j, z], 1), np.stack([z, j], 1)])


def mix_graphs(mix, gen, zero_node=True):
    """(nodes, edges [E, 2], complete) per graph, in the module text's order."""
    none = np.zeros((0, 2), dtype=np.int64)
    rnd = lambda n: (n, GG._random_pairs(n, gen), False)
    graphs = [rnd(1), rnd(2), rnd(3), (64, GG._complete(64), True), rnd(65), (0, none, False), (7, none, False),
              (40, GG.dup_graphs(40, [40])[0][1], False), rnd(257), rnd(700), rnd(1025), (STAR, double_star(STAR), False)]
    n, e, _ = rnd(130)
    graphs.append((n, np.concatenate([e, np.repeat(np.asarray([FOLD_PAIR], dtype=np.int64), FOLD_COPIES, axis=0)]), False))
    assert graphs[STAR_AT][0] == STAR and graphs[FOLD_AT][0] == 130
    if mix == 'dense':
        graphs += [(257, GG._complete(257), True), (300, GG.dup_graphs(300, [300])[0][1], False)]
    else:
        assert mix == 'light', mix
    return graphs if zero_node else [g for g in graphs if g[0] > 0]


def shuffled(graphs, seed=0):
    """The same graphs with every edge list in another order."""
    rng = np.random.default_rng(seed)
    return [(n, e[rng.permutation(len(e))], c) for n, e, c in graphs]


# ------------------------------------------------------------------------------------------------ one attention kernel
def _kernel_inputs(mix, heads, channels, seed):
    gen = torch.Generator().manual_seed(1000003 * heads + 1009 * channels + 7 * (mix == 'dense') + seed)
    graphs = mix_graphs(mix, gen)
    T, hc = int(GG._offsets(graphs)[-1]), heads * channels
    H = torch.randn(T, hc, generator=gen)
    att_s = torch.randn(hc, generator=gen) / math.sqrt(channels)
    att_d = torch.randn(hc, generator=gen) / math.sqrt(channels)
    bias = (torch.rand(hc, generator=gen) * 2 - 1) * 0.1
    cot = torch.randn(T, hc, generator=gen)
    return graphs, H, att_s, att_d, bias, cot


def find_kernel_seed(mix, heads, channels, limit=200):
    for seed in range(limit):
        if GG._kernel_guard(heads, channels, *_kernel_inputs(mix, heads, channels, seed)[:4]):
            return seed
    raise AssertionError(f'no seed below {limit} satisfies the guard for {mix} {heads} x {channels}')


@functools.lru_cache(maxsize=16)
def kernel_case(mix, heads, channels):
    """The inputs at the frozen seed (guard asserted) with the per-graph fp64 reference and float32 yardstick; computed once, never modified."""
    graphs, H, att_s, att_d, bias, cot = _kernel_inputs(mix, heads, channels, SEEDS[('kernel', mix, heads, channels)])
    assert GG._kernel_guard(heads, channels, graphs, H, att_s, att_d), 'a pre-activation on a LeakyReLU edge: the frozen seed no longer fits the generator'
    ref = GG._attn_chain(H, graphs, att_s, att_d, bias, cot, heads, channels, torch.float64)
    yard = GG._attn_chain(H, graphs, att_s, att_d, bias, cot, heads, channels, torch.float32)
    return dict(mix=mix, heads=heads, channels=channels, graphs=graphs, H=H, att_s=att_s, att_d=att_d, bias=bias, cot=cot, ref=ref, yard=yard)


def sparse_run(case, graphs=None, rows=None):
    """The sparse attention kernels, forward and backward, on the card: over the case's batch, or over `graphs` with the node rows `rows`."""
    from sgaligner_amd import ops
    heads, channels = case['heads'], case['channels']
    gb = GG.graph_batch(case['graphs'] if graphs is None else graphs)
    rows = slice(None) if rows is None else rows
    dev = lambda t: t.float().cuda().contiguous()
    H, a_s, a_d, b, cot = dev(case['H'][rows]), dev(case['att_s']), dev(case['att_d']), dev(case['bias']), dev(case['cot'][rows])
    out = ops._attn_fwd_sp(H, heads, channels, a_s, a_d, b, gb)
    dh, das, dad = ops._attn_bwd_sp(H, cot, heads, channels, a_s, a_d, gb)
    torch.cuda.synchronize()
    return dict(out=out, dw=dh, das=das, dad=dad)


def measure_kernel(mix, heads, channels):
    """{output: (kernel errors, yardstick errors)} over the whole batch."""
    case = kernel_case(mix, heads, channels)
    idx = range(len(case['graphs']))
    ref, yard = GG._collect(case['ref'], idx), GG._collect(case['yard'], idx)
    ke, ye = GG.errors(sparse_run(case), ref), GG.errors(yard, ref)
    return {k: (ke[k], ye[k]) for k in GG.KERNEL_OUTPUTS}


# ------------------------------------------------------------------------------------------------ stacks
def _stack_inputs(which, seed):
    units, heads, masked = STACKS[which]
    gen = torch.Generator().manual_seed(104729 * which + 31 * int(masked) + seed)
    graphs = mix_graphs('light', gen, zero_node=False)
    T = int(GG._offsets(graphs)[-1])
    layers = GG.stack_params(units, heads, gen)
    x = torch.randn(T, units[0], generator=gen)
    cot = torch.randn(T, units[-1] * heads[-1], generator=gen)
    masks = None
    if masked:                                                        # p = 0.5: entries 0 or 1 / (1 - p) = 2
        masks = [(torch.rand(T, l['lin_w'].shape[1], generator=gen) >= 0.5).float() * 2.0 for l in layers]
    return graphs, layers, x, cot, masks


def find_stack_seed(which, limit=200):
    for seed in range(limit):
        if GG._stack_guard(*_stack_inputs(which, seed)):
            return seed
    raise AssertionError(f'no seed below {limit} satisfies the guard for stack {which}')


@functools.lru_cache(maxsize=8)
def stack_case(which):
    units, heads, masked = STACKS[which]
    graphs, layers, x, cot, masks = _stack_inputs(which, SEEDS[('stack', which)])
    assert GG._stack_guard(graphs, layers, x, cot, masks), 'a pre-activation on a LeakyReLU edge: the frozen seed no longer fits the generator'
    ref = GG._stack_chain(x, graphs, layers, cot, torch.float64, masks)
    yard = GG._stack_chain(x, graphs, layers, cot, torch.float32, masks)
    return dict(units=units, heads=heads, graphs=graphs, layers=layers, x=x, cot=cot, masks=masks, ref=ref, yard=yard)


def stack_run(case, route='sparse'):
    """MultiGAT(route).forward_batched and its backward on the card, as gat_general_gate.stack_run."""
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    masked = case['masks'] is not None
    net = MultiGAT(n_units=list(case['units']), n_heads=list(case['heads']), dropout=0.5 if masked else 0.0, route=route).cuda()
    with torch.no_grad():
        for layer, lp in zip(net.layer_stack, case['layers']):
            layer.lin_src.weight.copy_(lp['lin_w'])
            layer.att_src.copy_(lp['att_src'])
            layer.att_dst.copy_(lp['att_dst'])
            layer.bias.copy_(lp['bias'])
    net.train(masked)
    x = case['x'].cuda().requires_grad_(masked)
    out = net.forward_batched(x, GG.graph_batch(case['graphs']), masks=[m.cuda() for m in case['masks']] if masked else None)
    out.backward(case['cot'].cuda())
    torch.cuda.synchronize()
    return GG.stack_grads(net, out.detach(), x if masked else None)


def measure_stack(which):
    case = stack_case(which)
    got = stack_run(case)
    keys = GG.stack_outputs(case)
    ref = {k: case['ref'][k] for k in keys}
    ke, ye = GG.errors(got, ref), GG.errors(case['yard'], ref)
    return {k: (ke[k], ye[k]) for k in keys}
