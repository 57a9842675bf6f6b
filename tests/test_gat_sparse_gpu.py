"""GPU: the sparse GAT route (csrc/gat_sparse.hip) -- the device-built structure against its NumPy restatement, every kernel and stack case
against the fp32-faithful gate of tests/gat_sparse_gate.py, the hand-derived case, the exact properties the route promises (repeatable
bits, a graph alone = the graph in a batch, edge order irrelevant, out-of-range endpoints dropped), the 300-fold pair the dense route
cannot count, the encoder on a 300-object scene, and 'auto' staying on the dense kernels for small graphs."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gat_csr_ref as CSR  # noqa: E402
import gat_general_gate as GG  # noqa: E402
import gat_sparse_gate as SG  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ('out', 'dw', 'das', 'dad')
PROBE = ('light', 3, 100)              # the case the exact properties are shown on: 3 heads, a ragged second channel slot


def _mix(mix):
    return SG.mix_graphs(mix, torch.Generator().manual_seed(0))


def _device_structure(graphs):
    sp = GG.graph_batch(graphs).sparse()
    torch.cuda.synchronize()
    U = int(sp.row_ptr[-1])
    assert U == int(sp.col_ptr[-1]) and U <= sp.cap == sum(g[0] + len(g[1]) for g in graphs)
    assert not any(int(t[U:].abs().max()) for t in (sp.src, sp.mult, sp.tgt, sp.perm) if U < sp.cap)        # the slots behind U are cleared
    got = {k: getattr(sp, k).cpu().numpy().astype(np.int64) for k in ('row_ptr', 'col_ptr')}
    got.update({k: getattr(sp, k)[:U].cpu().numpy().astype(np.int64) for k in ('src', 'mult', 'tgt', 'perm')})
    return U, got


@pytest.mark.parametrize('mix,shuffle', [('light', False), ('dense', False), ('light', True)])
def test_device_structure_equals_the_restatement(mix, shuffle):
    graphs = _mix(mix)
    want = CSR.csr(graphs)                                               # the shuffled lists must give the SAME arrays
    U, got = _device_structure(SG.shuffled(graphs, 3) if shuffle else graphs)
    assert U == want['U']
    for k in ('row_ptr', 'src', 'mult', 'col_ptr', 'tgt', 'perm'):
        assert np.array_equal(got[k], want[k]), k


def test_structure_of_empty_batches():
    none = np.zeros((0, 2), dtype=np.int64)
    for graphs in ([], [(0, none, False)], [(0, none, False), (2, none, False)], [(2, np.asarray([[1, 1], [0, 0]], dtype=np.int64), False)]):
        want = CSR.csr(graphs)
        U, got = _device_structure(graphs)
        assert U == want['U'] and np.array_equal(got['row_ptr'], want['row_ptr']) and np.array_equal(got['col_ptr'], want['col_ptr'])


@pytest.mark.parametrize('mix,heads,channels', SG.KERNEL_CASES)
def test_kernel_cases_pass_the_gate(mix, heads, channels):
    SG.assert_gate(SG.measure_kernel(mix, heads, channels), f'sparse kernel {mix} {heads}x{channels}')


@pytest.mark.parametrize('which', range(len(SG.STACKS)))
def test_stack_cases_pass_the_gate(which):
    units, heads, masked = SG.STACKS[which]
    meas = SG.measure_stack(which)
    assert ('dx' in meas) == masked and all(f'db{i}' in meas for i in range(len(heads)))
    SG.assert_gate(meas, f'sparse stack {list(units)}/{list(heads)}' + (' masks p=0.5' if masked else ''))


def test_sparse_route_vs_hand_derived_case():
    """tests/gat_handcase.py (not through the oracle) through the sparse kernels, alone and as the middle graph of a batch, to the tolerance
    of test_gat_gpu.py::test_gat_kernel_vs_hand_derived_case."""
    import gat_handcase as G
    from sgaligner_amd import ops
    h, a_s, a_d, b = G.inputs()
    for sizes, off in (([3], 0), ([2, 3, 4], 2)):
        T = sum(sizes)
        hh = np.zeros((T, G.H * G.C))
        hh[off:off + 3] = h
        ecnt = np.asarray([len(G.EDGES)] if len(sizes) == 1 else [0, len(G.EDGES), 0])
        gb = ops.GraphBatch(np.asarray(sizes), ecnt, torch.from_numpy(G.EDGES).cuda())
        f = lambda a: torch.from_numpy(a).float().cuda()
        out = ops._attn_fwd_sp(f(hh), G.H, G.C, f(a_s), f(a_d), f(b), gb)
        torch.cuda.synchronize()
        got = out.cpu().double().numpy()[off:off + 3]
        assert np.allclose(got, G.expected(), rtol=0, atol=2e-5), np.abs(got - G.expected()).max()


@functools.lru_cache(maxsize=2)
def _probe_run():
    case = SG.kernel_case(*PROBE)
    return case, SG.sparse_run(case)


def test_two_runs_give_the_same_bits():
    case, base = _probe_run()
    again = SG.sparse_run(case)
    for k in KEYS:
        assert torch.equal(base[k], again[k]), k


def test_a_graph_alone_has_the_bits_it_has_in_the_batch():
    case, base = _probe_run()
    off = GG._offsets(case['graphs'])
    for gi, n in ((8, 257), (SG.STAR_AT, SG.STAR), (SG.FOLD_AT, 130)):
        assert case['graphs'][gi][0] == n
        rows = slice(int(off[gi]), int(off[gi + 1]))
        alone = SG.sparse_run(case, graphs=[case['graphs'][gi]], rows=rows)
        assert torch.equal(alone['out'], base['out'][rows]) and torch.equal(alone['dw'], base['dw'][rows]), n


def test_edge_order_changes_no_bit():
    case, base = _probe_run()
    other = SG.sparse_run(case, graphs=SG.shuffled(case['graphs'], 5))
    for k in KEYS:
        assert torch.equal(base[k], other[k]), k


def test_out_of_range_endpoints_change_no_bit(monkeypatch):
    """50 edges with an endpoint outside the graph (negative, == N, huge) are dropped: the outputs are those of the run without them."""
    from sgaligner_amd import ops
    monkeypatch.setattr(ops, 'VALIDATE', False)                          # the host-side range check would (rightly) object to this batch
    case, base = _probe_run()
    rng = np.random.default_rng(11)
    live = [i for i, g in enumerate(case['graphs']) if g[0] > 0]
    extra = {}
    for t in range(50):
        gi = live[int(rng.integers(len(live)))]
        n = case['graphs'][gi][0]
        bad = (-1, n, 2 ** 40, -2 ** 35, n + 7)[t % 5]
        inside = int(rng.integers(n))
        extra.setdefault(gi, []).append((bad, inside) if t % 2 else (inside, bad))
    graphs = []
    for gi, (n, e, c) in enumerate(case['graphs']):
        if gi in extra:
            e = np.concatenate([e, np.asarray(extra[gi], dtype=np.int64)])
            e = e[rng.permutation(len(e))]
        graphs.append((n, e, c))
    assert sum(len(g[1]) for g in graphs) == sum(len(g[1]) for g in case['graphs']) + 50
    other = SG.sparse_run(case, graphs=graphs)
    for k in KEYS:
        assert torch.equal(base[k], other[k]), k


def test_the_300_fold_pair_is_counted_where_the_dense_route_saturates():
    from sgaligner_amd import ops
    case = SG.kernel_case('light', 2, 128)
    gi = SG.FOLD_AT
    n, e, _ = case['graphs'][gi]
    assert n == 130 and int(((e[:, 0] == SG.FOLD_PAIR[0]) & (e[:, 1] == SG.FOLD_PAIR[1])).sum()) >= SG.FOLD_COPIES > 255
    off = GG._offsets(case['graphs'])
    rows = slice(int(off[gi]), int(off[gi + 1]))
    ref, yard = GG._collect(case['ref'], [gi]), GG._collect(case['yard'], [gi])
    ke, ye = GG.errors(SG.sparse_run(case, graphs=[case['graphs'][gi]], rows=rows), ref), GG.errors(yard, ref)
    SG.assert_gate({k: (ke[k], ye[k]) for k in KEYS}, 'sparse kernel 2x128, 130 nodes with a 300-fold pair')
    # the dense route on the same graph: its 8-bit count saturates and the status word says so (existing behaviour, shown for the difference)
    dev = lambda t: t.float().cuda().contiguous()
    ops.DEFERRED_CHECKS.flush()
    ops._attn_fwd_hc(dev(case['H'][rows]), 2, 128, dev(case['att_s']), dev(case['att_d']), dev(case['bias']), GG.graph_batch([case['graphs'][gi]]),
                     check_status=True)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='more than 255 times'):
        ops.DEFERRED_CHECKS.flush()
    ops.DEFERRED_CHECKS.flush()


def test_encoder_on_a_300_object_scene():
    """MultiModalEncoder(gat_route='auto') on one pair of 300 and 40 objects against the oracle: the joint embedding and every parameter
    gradient of one cotangent, at the tolerances of test_gat_gpu.py::test_multigat_fwd_bwd; the dense route refuses the same batch."""
    from oracle import sga_oracle as O
    from sgaligner_amd.aligner.sg_aligner import MultiModalEncoder
    from sgaligner_amd.synthetic import make_batch, to_device
    mods = ['point', 'gat', 'rel']
    dd = make_batch(1, (300, 40), 32, seed=9)
    assert [int(v) for v in np.asarray(dd['graph_per_obj_count']).reshape(-1)] == [300, 40]
    torch.manual_seed(2)
    model = MultiModalEncoder(mods, rel_dim=41, attr_dim=164, gat_route='auto')
    params = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items() if 'num_batches' not in k and v.dtype.is_floating_point}
    joint_o = O.encoder_forward(params, dd, mods)['joint']
    cot = torch.randn(joint_o.shape, generator=torch.Generator().manual_seed(3))
    (joint_o * cot).sum().backward()
    model = model.cuda()
    ddd = to_device(dd, 'cuda')
    joint = model(ddd)['joint']
    (joint * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    err = (joint.detach().cpu() - joint_o.detach()).abs().max().item()
    print(f'joint embedding: max abs err {err:.3e}')
    assert err < 1e-4, err
    seen = 0
    for name, p in model.named_parameters():
        ref = params[name].grad if name in params else None
        if ref is None:
            continue
        assert p.grad is not None, name
        e, scale = (p.grad.cpu() - ref).abs().max().item(), max(1.0, ref.abs().max().item())
        print(f'{name}: max abs grad err {e:.3e} of {scale:.3e}')
        assert e < 1e-3 * scale, (name, e, scale)
        seen += name.startswith('structure_encoder.')
    assert seen == 8                                                    # lin, att_src, att_dst, bias of both GAT layers
    dense = MultiModalEncoder(mods, rel_dim=41, attr_dim=164, gat_route='dense').cuda()
    with pytest.raises(RuntimeError, match='at most 256'):
        dense(ddd)


def test_auto_stays_on_the_dense_kernels_for_small_graphs(monkeypatch):
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    graphs = [g for i, g in enumerate(_mix('light')) if g[0] <= 256 and i != SG.FOLD_AT]          # (the 300-fold pair is beyond the dense route)
    assert max(g[0] for g in graphs) == 65
    T = sum(g[0] for g in graphs)
    x = torch.randn(T, 3, generator=torch.Generator().manual_seed(4)).cuda()
    outs = {}
    for units, heads in (([3, 128, 128], [2, 2]), ([3, 48, 100], [3, 1])):           # the dense kernels of 2 x 128 and the general ones
        for route in ('auto', 'dense', 'sparse'):
            torch.manual_seed(5)
            net = MultiGAT(units, heads, route=route).cuda()
            events = {}
            monkeypatch.setattr(ops, 'KERNEL_EVENTS', events)
            outs[route] = net.forward_batched(x, GG.graph_batch(graphs))
            torch.cuda.synchronize()
            monkeypatch.setattr(ops, 'KERNEL_EVENTS', None)
            sparse_launched = any(k.startswith('gat_sp_') for k in events)
            dense_launched = any(k.startswith('gat_attn_') for k in events)
            assert (sparse_launched, dense_launched) == ((True, False) if route == 'sparse' else (False, True)), (route, sorted(events))
        assert torch.equal(outs['auto'], outs['dense'])
        assert (outs['sparse'] - outs['dense']).abs().max().item() < 1e-4
