"""GPU: the EVA baseline -- GCN aggregation (exact, gated, limits), NCA loss (gated at every width and row-block budget, bitwise repeatable,
closed form, the reference's recorded cases), fusion over tables of different widths, PointNetfeat(out_size=200), and the training step end
to end against tests/eva_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eva_gate as EG  # noqa: E402
import eva_ref as ER  # noqa: E402
import gcn_handcase as HC  # noqa: E402

pytestmark = pytest.mark.gpu


def _aggregate(h, graphs, bias=None, transpose=False, relu=False):
    from sgaligner_amd import ops
    return ops.gcn_aggregate(h.float().cuda().contiguous(), EG.graph_batch(graphs), None if bias is None else bias.float().cuda(),
                             transpose=transpose, relu=relu).cpu().double()


# ------------------------------------------------------------------------------------------------ GCN
def test_gcn_hand_case():
    graphs = [(HC.N, HC.EDGES)]
    assert torch.equal(_aggregate(torch.from_numpy(HC.H), graphs, torch.from_numpy(HC.BIAS)), torch.from_numpy(HC.OUT))
    assert torch.equal(_aggregate(torch.from_numpy(HC.G), graphs, transpose=True), torch.from_numpy(HC.DH))


def _exact_graphs():
    """Every deg in {1, 4, 16}: a 16-node star (the centre hears 15 leaves), a graph whose nodes 0 and 2 hear three edges one of which is
    duplicated (the hand case, with its explicit self loop and isolated nodes), a 1-node graph, a 0-edge graph, and a second star whose
    leaves are listed last-to-first with an explicit self loop on the centre."""
    star = np.array([[j, 0] for j in range(1, 16)], dtype=np.int64)
    star_b = np.array([[5, 5]] + [[j, 5] for j in range(15, -1, -1) if j != 5], dtype=np.int64)
    none = np.zeros((0, 2), dtype=np.int64)
    return [(16, star), (HC.N, HC.EDGES), (1, none), (5, none), (16, star_b)]


def test_gcn_aggregation_exact():
    """Integer-valued h, bias and upstream gradient with power-of-two coefficients: every partial sum is an integer multiple of 2^-4 below
    2^24 / 16, so any correct evaluation equals the fp64 reference bit for bit -- forward, forward with ReLU, and the transpose."""
    graphs = _exact_graphs()
    adj = ER.block_adjacency(graphs)
    deg = torch.cat([torch.from_numpy(np.bincount(e[e[:, 0] != e[:, 1], 1], minlength=n)) + 1 for n, e in graphs])
    assert set(deg.tolist()) == {1, 4, 16}
    gen = torch.Generator().manual_seed(5)
    T = adj.shape[0]
    for C in (3, 200, 400):                              # one lane slot, one workgroup with a ragged last slot, two workgroups
        h = torch.randint(-64, 65, (T, C), generator=gen).double()
        b = torch.randint(-8, 9, (C,), generator=gen).double()
        g = torch.randint(-64, 65, (T, C), generator=gen).double()
        assert (adj.abs() @ h.abs()).max().item() + 8 < 2.0 ** 20
        ref = adj @ h + b
        assert torch.equal(_aggregate(h, graphs, b), ref), C
        assert torch.equal(_aggregate(h, graphs, b, relu=True), ref.clamp_min(0)), C
        assert torch.equal(_aggregate(g, graphs, transpose=True), adj.t() @ g), C


@pytest.mark.parametrize('seed', [0, 1])
def test_gcn_gate(seed):
    """MultiGCN n_units=[3,200,400] over graphs of 1, 2, 64, 65, 128, 129, 256 and 7 nodes: forward and both layers' weight / bias gradients within
    r x the float32 yardstick (guarded hidden channels left out of dW0 / db0)."""
    EG.assert_gate(EG.measure_gcn(seed), f'gcn seed {seed}')


def test_gcn_reference_signature_and_limits():
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    x, graphs, ws, g, ref = EG.gcn_input(0)
    net = MultiGCN(n_units=[3, 200, 400]).cuda()
    n, e = graphs[3]                                      # the 65-node graph through forward(x, edges [2, E]), as eva.py:66 calls it
    o = sum(k for k, _ in graphs[:3])
    xg = x[o:o + n].cuda()
    one = net(xg, torch.from_numpy(e).t().to(torch.int32).cuda())
    gb = EG.graph_batch([(n, e)])
    assert torch.equal(one, net.forward_batched(xg, gb)) and one.shape == (n, 400)
    big = EG.graph_batch([(257, np.zeros((0, 2), dtype=np.int64))])
    with pytest.raises(RuntimeError, match='at most 256 per graph'):
        net.forward_batched(torch.zeros(257, 3, device='cuda'), big)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.multi_gcn_layers(gb, xg.cpu(), [l.params() for l in net.layer_stack])
    # more than 255 copies of one edge: the deferred status error of the GAT path
    ops.DEFERRED_CHECKS.flush()
    many = EG.graph_batch([(2, np.tile(np.array([[0, 1]], dtype=np.int64), (300, 1)))])
    net.forward_batched(torch.zeros(2, 3, device='cuda'), many)
    with pytest.raises(RuntimeError, match='more than 255 times'):
        ops.DEFERRED_CHECKS.flush()


# ------------------------------------------------------------------------------------------------ NCA
@pytest.mark.parametrize('small', [False, True])
@pytest.mark.parametrize('A,D', EG.NCA_SHAPES)
def test_nca_gate(A, D, small):
    """Loss and table gradient within r x the float32 yardstick, with the default budget (one row block) and with one forced small enough for at
    least three row blocks and a ragged last one (A >= 3; below that a block is a row)."""
    from sgaligner_amd import nca_ops, ops
    stash = EG.small_stash(A) if small else None
    if small and A >= 3:
        keep, ops.STASH_BYTES = ops.STASH_BYTES, stash
        try:
            assert len(nca_ops._row_blocks(A)) >= 3
        finally:
            ops.STASH_BYTES = keep
    EG.assert_gate(EG.measure_nca(A, D, stash), f'nca A={A} D={D} small={small}')


@pytest.mark.parametrize('small', [False, True])
def test_nca_bitwise_repeatable(small):
    """Two consecutive runs: the same bits in loss, dZ1 | dZ2 and the table gradient."""
    from sgaligner_amd import nca_ops, ops
    A, D = 257, 400
    emb, dd, _ = EG.nca_input(A, D)
    keep = ops.STASH_BYTES
    try:
        if small:
            ops.STASH_BYTES = EG.small_stash(A)
        runs = []
        for _ in range(2):
            x = emb.float().cuda()
            idx, a = nca_ops._anchor_index(dd, x.device, x.shape[0])
            loss, state = nca_ops._nca_forward(x, idx, a, 1.0, 1.0, 0.0, keep=True)
            dz = nca_ops._nca_backward(state, torch.ones(1, device='cuda', dtype=torch.float64))
            out = EG.nca_run(emb, dd, ops.STASH_BYTES)
            runs.append((loss.cpu(), dz.cpu(), out['nca_loss'].cpu(), out['nca_grad'].cpu()))
        assert len(state['cfg'][7]) == (5 if small else 1)
        for a0, a1 in zip(*runs):
            assert torch.equal(a0, a1)
        assert torch.equal(runs[0][0], runs[0][2]) and runs[0][1].abs().max() > 0
        # the reference's engine calls backward(retain_graph=True): a second backward over the same graph finds its saved blocks unchanged
        x = emb.float().cuda().requires_grad_(True)
        loss = ops.nca_loss(x, dd)
        loss.backward(retain_graph=True)
        g1 = x.grad.clone()
        loss.backward()
        assert torch.equal(x.grad, 2 * g1) and torch.equal(g1.cpu(), runs[0][3])
    finally:
        ops.STASH_BYTES = keep


def test_nca_closed_form_and_empty():
    """All rows equal: every score is 1, loss = 2 log(1 + (A - 1) e) - log 2.  A missed diagonal mask moves it by more than 1e-3 at A = 33."""
    from sgaligner_amd import ops
    A = 33
    emb = torch.ones(2 * A, 100).cuda() * 3.0
    dd = {'e1i': np.arange(A, dtype=np.int32), 'e2i': np.arange(A, 2 * A, dtype=np.int32)}
    want = 2 * np.log1p((A - 1) * np.e) - np.log(2.0)
    for stash in (None, EG.small_stash(A)):
        keep = ops.STASH_BYTES
        try:
            if stash is not None:
                ops.STASH_BYTES = stash
            got = float(ops.nca_loss(emb, dd))
        finally:
            ops.STASH_BYTES = keep
        print('closed form', stash, got, want)
        assert abs(got - want) <= 1e-5 * want
    assert abs((2 * np.log1p(A * np.e) - np.log(2.0)) - want) > 1e-3
    empty = ops.nca_loss(emb.requires_grad_(True), {'e1i': np.zeros(0, dtype=np.int32), 'e2i': np.zeros(0, dtype=np.int32)})
    assert torch.isnan(empty)
    with pytest.raises(RuntimeError, match='_sga_shard'):
        ops.nca_loss(emb, dict(dd, _sga_shard=(0, 1)))


def test_nca_reference_golden_cases():
    """The reference's recorded OverallNCALoss case (tools/make_eva_golden.py) through the GPU path: per-key losses, their sum, table gradients."""
    from sgaligner_amd.aligner.losses import OverallNCALoss
    g = load_golden('nca_cases')
    keys = [str(k) for k in g['ov__keys']]
    dd = {'e1i': g['ov__e1i'], 'e2i': g['ov__e2i']}
    tabs = {k: torch.from_numpy(g[f'ov__tab__{k}']).float().cuda().requires_grad_(True) for k in keys}
    losses = OverallNCALoss([k for k in keys if k != 'joint'], 'cuda')(tabs, dd)
    losses['loss'].backward()
    assert set(losses) == set(keys) | {'loss'}
    for k in keys + ['loss']:
        assert abs(float(losses[k].detach()) - float(g[f'ov__loss__{k}'])) <= 2e-6 * abs(float(g[f'ov__loss__{k}'])), k
    for k in keys:
        ref = torch.from_numpy(g[f'ov__grad__{k}'])
        assert (tabs[k].grad.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), k
    # NCALoss with other constants (alpha 2, beta 0.5, ep 0.25) on rows that are already normalised
    from sgaligner_amd import ops
    z = torch.cat([torch.from_numpy(g['a40_ab__z1']), torch.from_numpy(g['a40_ab__z2'])]).float().cuda().requires_grad_(True)
    a, b, ep = [float(v) for v in g['a40_ab__abe']]
    loss = ops.nca_loss(z, {'e1i': np.arange(40, dtype=np.int32), 'e2i': np.arange(40, 80, dtype=np.int32)}, alpha=a, beta=b, ep=ep)
    loss.backward()
    assert abs(float(loss.detach()) - float(g['a40_ab__loss'])) <= 2e-6 * abs(float(g['a40_ab__loss']))
    # the recorded gradients are with respect to the rows themselves; the table gradient is their tangent part
    zz = torch.cat([torch.from_numpy(g['a40_ab__z1']), torch.from_numpy(g['a40_ab__z2'])])
    gg = torch.cat([torch.from_numpy(g['a40_ab__g1']), torch.from_numpy(g['a40_ab__g2'])])
    ref = gg - zz * (zz * gg).sum(1, keepdim=True)
    assert (z.grad.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ fusion, PointNet
@pytest.mark.parametrize('T', [1, 5])
def test_fusion_differing_widths(T):
    from sgaligner_amd import ops
    gen = torch.Generator().manual_seed(T)
    embs = [torch.randn(T, d, generator=gen) for d in (400, 200, 100, 100)]
    w = torch.randn(4, 1, generator=gen)
    gj = torch.randn(T, 800, generator=gen)
    r64 = [e.double().requires_grad_(True) for e in embs]
    w64 = w.double().requires_grad_(True)
    ref = ER.fusion(w64, r64)
    ref.backward(gj.double())
    d32 = [e.cuda().requires_grad_(True) for e in embs]
    wd = w.cuda().requires_grad_(True)
    out = ops.fusion(wd, d32)
    out.backward(gj.cuda())
    assert out.shape == (T, 800)
    # the bounds of test_linear_fusion_gpu.py::test_fusion_golden
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-5
    assert (wd.grad.cpu().double() - w64.grad).abs().max().item() < 1e-4
    for a, b in zip(d32, r64):
        assert (a.grad.cpu().double() - b.grad).abs().max().item() < 1e-4


def test_fusion_equal_widths_keep_the_old_entry_point():
    """Equal widths: FusionFn (sga_fusion_fwd / bwd) as before, and the bits it gives; the new route on the same tables agrees with it."""
    from sgaligner_amd import ops
    gen = torch.Generator().manual_seed(9)
    embs = [torch.randn(37, 100, generator=gen).cuda().requires_grad_(True) for _ in range(3)]
    w = torch.randn(3, 1, generator=gen).cuda().requires_grad_(True)
    gj = torch.randn(37, 300, generator=gen).cuda()
    out = ops.fusion(w, embs)
    assert type(out.grad_fn).__name__.startswith('FusionFn')
    old = ops.FusionFn.apply(w, *embs)
    assert torch.equal(out, old)
    var = ops.FusionVarFn.apply(w, *embs)
    assert torch.equal(var, old)                          # the same arithmetic per table and row
    g_old = torch.autograd.grad(old, [w] + embs, gj)
    g_var = torch.autograd.grad(var, [w] + embs, gj)
    for a, b in zip(g_old[1:], g_var[1:]):
        assert torch.equal(a, b)
    assert torch.allclose(g_old[0], g_var[0], rtol=1e-5, atol=1e-7)     # (the weight gradient folds fp64 atomics: order-dependent in the last bit)
    mixed = ops.fusion(w, [embs[0], embs[1], torch.randn(37, 60, generator=gen).cuda()])
    assert type(mixed.grad_fn).__name__.startswith('FusionVarFn') and mixed.shape == (37, 260)


def test_pointnet_out_size_200_equals_the_padded_256_run():
    """PointNetfeat(out_size=200) against a 256-wide run whose conv3 carries the same 200 rows plus 56 zero rows: forward, parameter gradients
    and BatchNorm running statistics with torch.equal.  The backward sums winner rows with fp32 atomics in no fixed order, so the inputs are
    pointnet_gate's 'narrow' lattice (integer-valued, every partial sum exact in any order; zero rows only shrink its envelopes): equality
    bit for bit is then owed by any correct evaluation."""
    import pointnet_gate as PG
    from sgaligner_amd.aligner.networks.pointnet import PointNetfeat
    x, ws, ref = PG.lattice('narrow', 9, 33, 256)
    small, wide = PointNetfeat(input_transform=False, out_size=200).cuda(), PointNetfeat(input_transform=False, out_size=256).cuda()
    w3, b3 = ws[4].clone(), ws[5].clone()
    w3[200:] = 0
    b3[200:] = 0
    with torch.no_grad():
        for net, rows in ((small, 200), (wide, 256)):
            for conv, w, b in ((net.conv1, ws[0], ws[1]), (net.conv2, ws[2], ws[3]), (net.conv3, w3[:rows], b3[:rows])):
                conv.weight.copy_(w.reshape(conv.weight.shape))
                conv.bias.copy_(b)
    xd = x.permute(0, 2, 1).contiguous().cuda()                      # [T, 3, P], the reference's layout
    gy = ref['gy'].float().cuda().clone()
    gy[:, 200:] = 0
    small.train(); wide.train()
    ys, yw = small(xd), wide(xd)
    assert ys.shape == (9, 200) and torch.equal(ys, yw[:, :200]) and float(yw[:, 200:].detach().abs().max()) == 0.0
    assert torch.equal(ys.detach().cpu().double(), ref['y'][:, :200])        # and both are the lattice's exact answer
    ys.backward(gy[:, :200].contiguous())
    yw.backward(gy)
    for k in ('conv1', 'conv2'):
        assert torch.equal(getattr(small, k).weight.grad, getattr(wide, k).weight.grad), k
        assert torch.equal(getattr(small, k).bias.grad, getattr(wide, k).bias.grad), k
    assert torch.equal(small.conv3.weight.grad, wide.conv3.weight.grad[:200]) and torch.equal(small.conv3.bias.grad, wide.conv3.bias.grad[:200])
    assert float(wide.conv3.weight.grad[200:].abs().max()) == 0.0 and float(small.conv3.weight.grad.abs().max()) > 0
    for k in ('bn1', 'bn2'):
        assert torch.equal(getattr(small, k).running_mean, getattr(wide, k).running_mean) and torch.equal(getattr(small, k).running_var, getattr(wide, k).running_var)
    assert torch.equal(small.bn3.running_mean, wide.bn3.running_mean[:200]) and torch.equal(small.bn3.running_var, wide.bn3.running_var[:200])
    assert int(small.bn3.num_batches_tracked) == 1 and small.bn3.running_mean.shape == (200,)
    small.eval(); wide.eval()
    with torch.no_grad():
        assert torch.equal(small(xd), wide(xd)[:, :200])


# ------------------------------------------------------------------------------------------------ EVA end to end
def test_eva_train_step_against_the_reference():
    dd, sd, ref = EG.eva_case()
    steps, out, losses = EG.eva_run(dd, sd)
    assert list(out) == EG.EVA_MODULES + ['joint'] and set(losses) == set(out) | {'loss'}
    assert [tuple(out[k].shape)[1] for k in out] == [400, 200, 100, 100, 800]
    ke = EG.eva_errors(out, losses, ref, dd)
    ye = EG.eva_errors(ref['yard_tables'], ref['yard_losses'], ref, dd)
    EG.assert_gate({k: (ke[k], ye[k]) for k in ke}, 'eva')
    e_tot = sum(EG.loss_envelope(ref['tables'][k], dd) for k in out)                             # the total: the sum of the five envelopes
    kt = EG.G.rel_errors(losses['loss'].detach().cpu().reshape(1), ref['losses']['loss'].reshape(1), e_tot)
    yt = EG.G.rel_errors(ref['yard_losses']['loss'].reshape(1), ref['losses']['loss'].reshape(1), e_tot)
    EG.assert_gate({'loss_total': (kt, yt)}, 'eva')
    params = dict(steps.model.named_parameters())
    before = {k: p.detach().clone() for k, p in params.items()}
    for k, p in params.items():
        if k.startswith('object_encoder.bn'):             # the reference's BatchNorm outputs are discarded: no gradient
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        g64 = ref['grads'][k]
        assert p.grad is not None, k
        err = (p.grad.cpu().double() - g64).abs().max().item()
        print(f'eva grad {k}: max err {err:.3e} of max {g64.abs().max().item():.3e}')
        assert err <= 1e-3 * g64.abs().max().item(), k
    steps.optimizer_step()
    for k, p in params.items():
        if p.grad is not None and float(p.grad.abs().max()) > 0:
            assert not torch.equal(p.detach(), before[k]), k
    # test_step: the same tables (of the updated model) with grad disabled
    from sgaligner_amd.synthetic import to_device
    ddd = to_device(dd, 'cuda')
    steps.model.eval()
    t1 = steps.test_step(0, ddd)
    assert all(not v.requires_grad for v in t1.values())
    with torch.enable_grad():
        t2 = steps.model(ddd)
    assert all(torch.equal(t1[k], t2[k]) for k in t2)


def test_eva_single_module_has_no_joint():
    dd, sd, ref = EG.eva_case()
    steps, out, losses = EG.eva_run(dd, {k: v for k, v in sd.items() if k != 'fusion.weight'} | {'fusion.weight': torch.ones(1, 1)}, modules=['gcn'])
    assert list(out) == ['gcn'] and set(losses) == {'gcn', 'loss'}
    assert float(losses['loss'].detach()) == float(losses['gcn'].detach())
    e = EG.G.rel_errors(losses['gcn'].detach().cpu().reshape(1), ref['losses']['gcn'].reshape(1), EG.loss_envelope(ref['tables']['gcn'], dd))
    y = EG.G.rel_errors(ref['yard_losses']['gcn'].reshape(1), ref['losses']['gcn'].reshape(1), EG.loss_envelope(ref['tables']['gcn'], dd))
    assert EG.gate_ok(e, y, EG.R['nca_loss']), (e, y)
