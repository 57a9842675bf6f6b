"""The fp32-faithful gate of the general GAT path (any heads, 1 <= channels <= 256, any depth, dropout), and the inputs its tests and its
profile share (no tests in this module).  Convention of gemm_gate / pointnet_gate / eva_gate:

Reference.  oracle.sga_oracle.gat_conv / multi_gat in fp64, graph by graph (an attention kernel alone: gat_conv with the identity as projection,
so that x is the projected H and x.grad is dH).  With dropout masks: the same layers applied to the masked inputs (F.elu between them).

Yardstick.  The same functions in plain float32 torch on the CPU -- never the library.

Metric.  gemm_gate.rel_errors in u = 2^-24 with a FLAT envelope: every entry of an output is judged against max |ref| of that output (not a
propagated envelope -- the softmax makes that one long; the flat one is scale-free per output and the same for kernel and yardstick).

Gate.  pointnet_gate.gate_ok at r per output kind -- layer output, dW (dH for a kernel alone), d att_src, d att_dst, d bias, dx (the input
gradient of a layer after the first / of a masked input) --, through eva_gate.gate_ok, which adds the one rule an output of a SINGLE entry
needs (heads * channels = 1: its yardstick is one draw, floored at FLOOR_U).  r = ceil(2 x the worst measured kernel / yardstick ratio, rms
or max) over the cases of profiles/gat_general_accuracy_vs_fp32.json (tools/gat_general_accuracy.py writes it on the card);
tests/test_gat_general_cpu.py keeps table and profile together.

Guard, a condition on the INPUTS.  LeakyReLU's derivative jumps at 0: in the fp64 reference every pre-activation a_s[j] + a_d[i] on a counted
edge (self loops included), in every layer and head, satisfies |pre| > DELTA (|a_s[j]| + |a_d[i]|), DELTA = 2^-16.  The generator advances
its seed from 0 until that holds; the seed it stops at is frozen in SEEDS and the condition is asserted when the case is built.  Nothing is
excluded from any comparison."""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import eva_gate as EG
import gemm_gate as G
from oracle import sga_oracle as O

ROOT = G.ROOT
PROFILE = os.path.join(ROOT, 'profiles', 'gat_general_accuracy_vs_fp32.json')
DELTA = 2.0 ** -16
KERNEL_CASES = ((1, 1), (1, 64), (2, 65), (3, 100), (1, 129), (8, 32), (2, 200), (1, 256), (4, 192))      # (heads, channels)
KERNEL_SIZES = (1, 2, 3, 64, 65, 128, 129, 256)
STACKS = (((17, 128, 100), (2, 2)), ((3, 48, 100, 32), (3, 1, 8)), ((3, 1), (1,)), ((5, 256), (8,)), ((3, 65, 129), (2, 1)))
STACK_SIZES = (1, 2, 7, 33, 64, 129, 200)          # 7: no edges; 33: duplicates and explicit self loops; 64: complete; others 4 n random pairs
# the shapes of tests/test_gat_gpu.py::test_multigat_fwd_bwd (the attention kernels at 2 x 128)
CANON_SHAPES = (((5, 7), True), ((64, 64, 33, 1, 2, 128), False), ((9, 17, 100, 3), True), ((129, 40), True), ((256, 3, 200), True),
                ((130, 255, 64), False))
KERNEL_OUTPUTS = ('out', 'dw', 'das', 'dad')       # 'dw' of a kernel alone: dH (the projection is the identity)
STACK_OUTPUTS = ('out', 'dw', 'das', 'dad', 'db')
OUTPUTS = ('out', 'dw', 'das', 'dad', 'db', 'dx')

# r per output kind: ceil(2 x the worst ratio measured, rms or max) over the cases of profiles/gat_general_accuracy_vs_fp32.json.
R = {'out': 4, 'dw': 5, 'das': 5, 'dad': 9, 'db': 5, 'dx': 2}

# the first seed (from 0) at which the guard holds, per case
SEEDS = {('kernel', 1, 1): 0, ('kernel', 1, 64): 0, ('kernel', 2, 65): 0, ('kernel', 3, 100): 2, ('kernel', 1, 129): 0, ('kernel', 8, 32): 0,
         ('kernel', 2, 200): 0, ('kernel', 1, 256): 0, ('kernel', 4, 192): 0,
         ('canon', 0): 0, ('canon', 1): 1, ('canon', 2): 0, ('canon', 3): 0, ('canon', 4): 7, ('canon', 5): 1,
         ('stack', 0, False): 0, ('stack', 1, False): 0, ('stack', 2, False): 0, ('stack', 3, False): 0, ('stack', 4, False): 0,
         ('stack', 0, True): 0}
# The masked case (dropout masks at p = 0.5) is STACKS[0] alone: a mask that zeroes a whole 3- or 5-wide input row makes every logit of
# that node exactly 0, which the guard's strict inequality excludes; 17 inputs are never all masked at these sizes.
MASKED_STACK = 0


def ratios_from_profile(path=PROFILE):
    """output kind -> ceil(2 x worst measured kernel / yardstick ratio), the derivation R states."""
    worst = {}
    for c in json.load(open(path))['cases']:
        worst[c['output']] = max(worst.get(c['output'], 0.0), c['ratio_rms'], c['ratio_max'])
    return {k: int(math.ceil(2.0 * v - 1e-9)) for k, v in worst.items()}


def kind(output):
    """'dw1' (layer 1's dW) -> 'dw'."""
    return output.rstrip('0123456789')


def assert_gate(meas, what=''):
    """meas: output -> (kernel errors, yardstick errors); every figure is printed before it is judged."""
    bad = []
    for k, (ke, ye) in meas.items():
        r = R[kind(k)]
        print(f'{what} {k}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
        if not EG.gate_ok(ke, ye, r):
            bad.append((k, ke, ye, r))
    assert not bad, (what, bad)


def errors(out, ref):
    """output -> gemm_gate.rel_errors against the flat envelope max |ref| of that output."""
    res = {}
    for k, r in ref.items():
        o = out[k].detach().cpu().reshape(r.shape)
        res[k] = G.rel_errors(o, r, torch.full_like(r, float(r.abs().max())))
    return res


# ------------------------------------------------------------------------------------------------ graphs
def lds_nodes(channels, bwd):
    from sgaligner_amd import _lib
    return int(_lib.lib().sga_gat_lds_nodes(int(channels), int(bwd)))


def _random_pairs(n, gen):
    """4 n uniformly random (source, target) pairs -- self loops and duplicates included --, none for a 1-node graph."""
    return torch.randint(0, n, (4 * n, 2), generator=gen).numpy().astype(np.int64) if n > 1 else np.zeros((0, 2), dtype=np.int64)


def _complete(n):
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    m = ii != jj
    return np.stack([ii[m], jj[m]], 1).astype(np.int64)


def dup_graphs(seed, sizes, extra_dups=True):
    """tests/test_gat_gpu.py's _graphs: all pairs, then (n > 2) 30 % dropped, n // 2 edges listed twice and n // 2 explicit self loops."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        e = _complete(n)
        if extra_dups and n > 2:
            e = e[rng.random(e.shape[0]) > 0.3]
            dup = e[rng.integers(0, e.shape[0], size=max(1, n // 2))]
            loops = np.stack([np.arange(n // 2)] * 2, 1)
            e = np.concatenate([e, dup, loops]).astype(np.int64)
        out.append((n, e))
    return out


def kernel_graphs(channels, gen):
    """The mix of one attention-kernel case: (nodes, edges [E, 2], complete) per graph.  Node counts KERNEL_SIZES (the 64-node one complete:
    the fast path), a zero-node graph in the middle, L and L + 1 for L = sga_gat_lds_nodes(channels, forward / backward) where at most 256, a
    40-node graph with duplicates and explicit self loops, a 7-node graph with no edges."""
    sizes = list(KERNEL_SIZES[:5]) + [0] + list(KERNEL_SIZES[5:])
    for bwd in (0, 1):
        L = lds_nodes(channels, bwd)
        sizes += [n for n in (L, L + 1) if n <= 256 and n not in sizes]
    graphs = [(n, _complete(n), True) if n == 64 else (n, _random_pairs(n, gen) if n else np.zeros((0, 2), dtype=np.int64), False) for n in sizes]
    graphs.append((40, dup_graphs(40, [40])[0][1], False))
    graphs.append((7, np.zeros((0, 2), dtype=np.int64), False))
    return graphs


def caps_of(channels):
    """The batches a kernel case is run as: all graphs (nmax = 256), and the graphs of at most L, L + 1 nodes for both L above -- so the launch
    sits on both sides of each LDS-residency boundary."""
    caps = [256]
    for bwd in (0, 1):
        L = lds_nodes(channels, bwd)
        caps += [n for n in (L, L + 1) if n <= 256 and n not in caps]
    return caps


def graph_batch(graphs, device='cuda'):
    from sgaligner_amd import ops
    edges = torch.from_numpy(np.concatenate([g[1] for g in graphs] + [np.zeros((0, 2), dtype=np.int64)])).to(device)
    return ops.GraphBatch(np.asarray([g[0] for g in graphs]), np.asarray([len(g[1]) for g in graphs]), edges)


def _offsets(graphs):
    return np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(int)


def _ei(e):
    return torch.from_numpy(np.ascontiguousarray(e.T))


def guard_holds(x, e, lin_w, att_s, att_d):
    """The module text's condition for one graph and layer, in fp64 (x [n, F] the layer's input)."""
    n = x.shape[0]
    if n == 0:
        return True
    h_, c_ = att_s.shape[1], att_s.shape[2]
    h = (x.double() @ lin_w.double().t()).view(n, h_, c_)
    a_s, a_d = (h * att_s.double()).sum(-1), (h * att_d.double()).sum(-1)
    src, dst = O._canon_edges(_ei(e), n)
    pre = a_s[src] + a_d[dst]
    return bool((pre.abs() > DELTA * (a_s[src].abs() + a_d[dst].abs())).all())


# ------------------------------------------------------------------------------------------------ one attention kernel
def _attn_chain(H, graphs, att_s, att_d, bias, cot, heads, channels, dtype):
    """gat_conv with the identity projection, graph by graph, in `dtype`: per graph (out, dH, d att_src, d att_dst)."""
    hc = heads * channels
    eye = torch.eye(hc, dtype=dtype)
    off = _offsets(graphs)
    res = []
    for gi, (n, e, _) in enumerate(graphs):
        if n == 0:
            res.append(None)
            continue
        h = H[off[gi]:off[gi + 1]].to(dtype).clone().requires_grad_(True)
        a_s = att_s.to(dtype).view(1, heads, channels).clone().requires_grad_(True)
        a_d = att_d.to(dtype).view(1, heads, channels).clone().requires_grad_(True)
        o = O.gat_conv(h, _ei(e), eye, a_s, a_d, bias.to(dtype))
        gh, gs, gd = torch.autograd.grad((o * cot[off[gi]:off[gi + 1]].to(dtype)).sum(), (h, a_s, a_d))
        res.append((o.detach(), gh, gs.reshape(-1), gd.reshape(-1)))
    return res


def _kernel_inputs(heads, channels, seed):
    gen = torch.Generator().manual_seed(1000003 * heads + 1009 * channels + seed)
    graphs = kernel_graphs(channels, gen)
    T, hc = int(_offsets(graphs)[-1]), heads * channels
    H = torch.randn(T, hc, generator=gen)
    att_s = torch.randn(hc, generator=gen) / math.sqrt(channels)
    att_d = torch.randn(hc, generator=gen) / math.sqrt(channels)
    bias = (torch.rand(hc, generator=gen) * 2 - 1) * 0.1
    cot = torch.randn(T, hc, generator=gen)
    return graphs, H, att_s, att_d, bias, cot


def _kernel_guard(heads, channels, graphs, H, att_s, att_d):
    off = _offsets(graphs)
    eye = torch.eye(heads * channels, dtype=torch.float64)
    return all(guard_holds(H[off[gi]:off[gi + 1]], e, eye, att_s.view(1, heads, channels), att_d.view(1, heads, channels))
               for gi, (n, e, _) in enumerate(graphs))


def find_kernel_seed(heads, channels):
    seed = 0
    while not _kernel_guard(heads, channels, *_kernel_inputs(heads, channels, seed)[:4]):
        seed += 1
    return seed


@functools.lru_cache(maxsize=16)
def kernel_case(heads, channels):
    """dict(graphs, H, att_s, att_d, bias, cot, ref, yard): the inputs at the frozen seed (guard asserted) with the per-graph fp64 reference
    and float32 yardstick.  Computed once; nothing in it is modified afterwards."""
    graphs, H, att_s, att_d, bias, cot = _kernel_inputs(heads, channels, SEEDS[('kernel', heads, channels)])
    assert _kernel_guard(heads, channels, graphs, H, att_s, att_d), 'a pre-activation on a LeakyReLU edge: the frozen seed no longer fits the generator'
    ref = _attn_chain(H, graphs, att_s, att_d, bias, cot, heads, channels, torch.float64)
    yard = _attn_chain(H, graphs, att_s, att_d, bias, cot, heads, channels, torch.float32)
    return dict(heads=heads, channels=channels, graphs=graphs, H=H, att_s=att_s, att_d=att_d, bias=bias, cot=cot, ref=ref, yard=yard)


def _collect(per_graph, idx):
    keep = [per_graph[i] for i in idx if per_graph[i] is not None]
    return dict(out=torch.cat([k[0] for k in keep]), dw=torch.cat([k[1] for k in keep]),
                das=torch.stack([k[2] for k in keep]).sum(0), dad=torch.stack([k[3] for k in keep]).sum(0))


def kernel_subset(case, cap):
    """(graph indices, rows, reference, yardstick) of the batch holding the graphs of at most `cap` nodes."""
    idx = [i for i, g in enumerate(case['graphs']) if g[0] <= cap]
    off = _offsets(case['graphs'])
    rows = torch.cat([torch.arange(off[i], off[i + 1]) for i in idx])
    return idx, rows, _collect(case['ref'], idx), _collect(case['yard'], idx)


def kernel_run(case, idx, rows):
    """The attention kernel, forward and backward, on the card."""
    from sgaligner_amd import ops
    heads, channels = case['heads'], case['channels']
    graphs = [case['graphs'][i] for i in idx]
    gb = graph_batch(graphs)
    if gb.complete is not None:                                      # the fast path is taken where the case means it to be (n > 2)
        got = gb.complete.cpu().tolist()
        assert all(f == int(g[2]) for f, g in zip(got, graphs) if g[0] > 2), (got, [g[2] for g in graphs])
    dev = lambda t: t.float().cuda().contiguous()
    H, a_s, a_d, b, cot = dev(case['H'][rows]), dev(case['att_s']), dev(case['att_d']), dev(case['bias']), dev(case['cot'][rows])
    out = ops._attn_fwd_hc(H, heads, channels, a_s, a_d, b, gb, check_status=True)
    dh, das, dad = ops._attn_bwd_hc(H, cot, heads, channels, a_s, a_d, gb)
    torch.cuda.synchronize()
    ops.DEFERRED_CHECKS.flush()
    return dict(out=out, dw=dh, das=das, dad=dad)


def measure_kernel(heads, channels):
    """cap -> {output: (kernel errors, yardstick errors)}."""
    case = kernel_case(heads, channels)
    res = {}
    for cap in caps_of(channels):
        idx, rows, ref, yard = kernel_subset(case, cap)
        ke, ye = errors(kernel_run(case, idx, rows), ref), errors(yard, ref)
        res[cap] = {k: (ke[k], ye[k]) for k in KERNEL_OUTPUTS}
    return res


# 2 x 128 (the kernels of that shape) on the shapes of test_multigat_fwd_bwd
@functools.lru_cache(maxsize=8)
def canon_case(which):
    sizes, dups = CANON_SHAPES[which]
    seed = SEEDS[('canon', which)]
    graphs, H, att_s, att_d, bias, cot = _canon_inputs(which, seed)
    assert _kernel_guard(2, 128, graphs, H, att_s, att_d), 'a pre-activation on a LeakyReLU edge: the frozen seed no longer fits the generator'
    ref = _attn_chain(H, graphs, att_s, att_d, bias, cot, 2, 128, torch.float64)
    yard = _attn_chain(H, graphs, att_s, att_d, bias, cot, 2, 128, torch.float32)
    return dict(heads=2, channels=128, graphs=graphs, H=H, att_s=att_s, att_d=att_d, bias=bias, cot=cot, ref=ref, yard=yard)


def _canon_inputs(which, seed):
    sizes, dups = CANON_SHAPES[which]
    gen = torch.Generator().manual_seed(7919 * which + seed)
    graphs = [(n, e, (not dups or n <= 2) and n > 0) for n, e in dup_graphs(sum(sizes), sizes, dups)]
    T = sum(sizes)
    H = torch.randn(T, 256, generator=gen)
    att_s = torch.randn(256, generator=gen) / math.sqrt(128)
    att_d = torch.randn(256, generator=gen) / math.sqrt(128)
    bias = (torch.rand(256, generator=gen) * 2 - 1) * 0.1
    cot = torch.randn(T, 256, generator=gen)
    return graphs, H, att_s, att_d, bias, cot


def find_canon_seed(which):
    seed = 0
    while not _kernel_guard(2, 128, *_canon_inputs(which, seed)[:4]):
        seed += 1
    return seed


def measure_canon(which):
    case = canon_case(which)
    idx, rows, ref, yard = kernel_subset(case, 256)
    ke, ye = errors(kernel_run(case, idx, rows), ref), errors(yard, ref)
    return {k: (ke[k], ye[k]) for k in KERNEL_OUTPUTS}


# ------------------------------------------------------------------------------------------------ stacks
def stack_graphs(gen, sizes=STACK_SIZES):
    out = []
    for n in sizes:
        if n == 64:
            out.append((n, _complete(n), True))
        elif n == 33:
            out.append((n, dup_graphs(33, [33])[0][1], False))
        elif n == 7:
            out.append((n, np.zeros((0, 2), dtype=np.int64), False))
        else:
            out.append((n, _random_pairs(n, gen), False))
    return out


def stack_params(units, heads, gen):
    """PyG's shapes, glorot weights and attention vectors; the biases uniform in +-0.1 (zero-initialised biases would hide them)."""
    layers = []
    for i in range(len(units) - 1):
        in_c = units[i] * heads[i - 1] if i else units[i]
        h, c = heads[i], units[i + 1]
        glorot = lambda shape, a, b: (torch.rand(shape, generator=gen) * 2 - 1) * math.sqrt(6.0 / (a + b))
        layers.append(dict(lin_w=glorot((h * c, in_c), in_c, h * c), att_src=glorot((1, h, c), h, c), att_dst=glorot((1, h, c), h, c),
                           bias=(torch.rand(h * c, generator=gen) * 2 - 1) * 0.1))
    return layers


def _stack_chain(x, graphs, layers, cot, dtype, masks=None):
    """O.multi_gat graph by graph in `dtype` (with masks: O.gat_conv on the masked input of every layer, F.elu between) and the gradients of
    every parameter and of x for the upstream gradient cot."""
    L = [{k: v.to(dtype).clone().requires_grad_(True) for k, v in l.items()} for l in layers]
    xl = x.to(dtype).clone().requires_grad_(True)
    off = _offsets(graphs)
    outs = []
    for gi, (n, e, _) in enumerate(graphs):
        xi = xl[off[gi]:off[gi + 1]]
        if masks is None:
            outs.append(O.multi_gat(xi, _ei(e), L))
            continue
        for i, lp in enumerate(L):
            xi = O.gat_conv(xi * masks[i][off[gi]:off[gi + 1]].to(dtype), _ei(e), lp['lin_w'], lp['att_src'], lp['att_dst'], lp['bias'])
            if i + 1 < len(L):
                xi = F.elu(xi)
        outs.append(xi)
    out = torch.cat(outs)
    (out * cot.to(dtype)).sum().backward()
    res = dict(out=out.detach(), dx=xl.grad)
    for i, lp in enumerate(L):
        res.update({f'dw{i}': lp['lin_w'].grad, f'das{i}': lp['att_src'].grad, f'dad{i}': lp['att_dst'].grad, f'db{i}': lp['bias'].grad})
    return res


def _stack_layer_inputs(x, graphs, layers, masks):
    """fp64 input of every layer, per graph (for the guard)."""
    off = _offsets(graphs)
    for gi, (n, e, _) in enumerate(graphs):
        xi = x[off[gi]:off[gi + 1]].double()
        for i, lp in enumerate(layers):
            if masks is not None:
                xi = xi * masks[i][off[gi]:off[gi + 1]].double()
            yield xi, e, lp
            if n:
                xi = O.gat_conv(xi, _ei(e), lp['lin_w'].double(), lp['att_src'].double(), lp['att_dst'].double(), lp['bias'].double())
                if i + 1 < len(layers):
                    xi = F.elu(xi)


def _stack_inputs(which, masked, seed):
    units, heads = STACKS[which]
    gen = torch.Generator().manual_seed(104729 * which + 31 * int(masked) + seed)
    graphs = stack_graphs(gen)
    T = int(_offsets(graphs)[-1])
    layers = stack_params(units, heads, gen)
    x = torch.randn(T, units[0], generator=gen)
    cot = torch.randn(T, units[-1] * heads[-1], generator=gen)
    masks = None
    if masked:                                                        # p = 0.5: entries 0 or 1 / (1 - p) = 2
        masks = [(torch.rand(T, l['lin_w'].shape[1], generator=gen) >= 0.5).float() * 2.0 for l in layers]
    return graphs, layers, x, cot, masks


def _stack_guard(graphs, layers, x, cot, masks):
    return all(guard_holds(xi, e, lp['lin_w'], lp['att_src'], lp['att_dst']) for xi, e, lp in _stack_layer_inputs(x, graphs, layers, masks))


def find_stack_seed(which, masked):
    seed = 0
    while not _stack_guard(*_stack_inputs(which, masked, seed)):
        seed += 1
    return seed


@functools.lru_cache(maxsize=16)
def stack_case(which, masked=False):
    """dict(units, heads, graphs, layers, x, cot, masks, ref, yard) at the frozen seed (guard asserted); computed once, never modified."""
    units, heads = STACKS[which]
    graphs, layers, x, cot, masks = _stack_inputs(which, masked, SEEDS[('stack', which, masked)])
    assert _stack_guard(graphs, layers, x, cot, masks), 'a pre-activation on a LeakyReLU edge: the frozen seed no longer fits the generator'
    ref = _stack_chain(x, graphs, layers, cot, torch.float64, masks)
    yard = _stack_chain(x, graphs, layers, cot, torch.float32, masks)
    return dict(units=units, heads=heads, graphs=graphs, layers=layers, x=x, cot=cot, masks=masks, ref=ref, yard=yard)


def stack_model(case, dropout=0.0):
    """MultiGAT on the card with the case's parameters."""
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    net = MultiGAT(n_units=list(case['units']), n_heads=list(case['heads']), dropout=dropout).cuda()
    with torch.no_grad():
        for layer, lp in zip(net.layer_stack, case['layers']):
            layer.lin_src.weight.copy_(lp['lin_w'])
            layer.att_src.copy_(lp['att_src'])
            layer.att_dst.copy_(lp['att_dst'])
            layer.bias.copy_(lp['bias'])
    return net


def stack_grads(net, out, x=None):
    res = dict(out=out)
    for i, l in enumerate(net.layer_stack):
        res.update({f'dw{i}': l.lin_src.weight.grad, f'das{i}': l.att_src.grad, f'dad{i}': l.att_dst.grad, f'db{i}': l.bias.grad})
    if x is not None:
        res['dx'] = x.grad
    return res


def stack_run(case):
    """MultiGAT.forward_batched and its backward on the card (with the case's masks, where it has them: p = 0.5, train mode, and x asks for
    its gradient so that the mask's part in dx shows).  Returns (outputs, net, out tensor with its graph)."""
    masked = case['masks'] is not None
    net = stack_model(case, dropout=0.5 if masked else 0.0)
    net.train(masked)
    x = case['x'].cuda().requires_grad_(masked)
    out = net.forward_batched(x, graph_batch(case['graphs']), masks=[m.cuda() for m in case['masks']] if masked else None)
    out.backward(case['cot'].cuda(), retain_graph=True)
    torch.cuda.synchronize()
    return stack_grads(net, out, x if masked else None), net, out


def stack_outputs(case):
    n = len(case['layers'])
    keys = ['out'] + [f'{k}{i}' for i in range(n) for k in ('dw', 'das', 'dad', 'db')]
    return keys + (['dx'] if case['masks'] is not None else [])


def measure_stack(which, masked=False):
    case = stack_case(which, masked)
    got = stack_run(case)[0]
    keys = stack_outputs(case)
    ref = {k: case['ref'][k] for k in keys}
    ke, ye = errors(got, ref), errors(case['yard'], ref)
    return {k: (ke[k], ye[k]) for k in keys}
