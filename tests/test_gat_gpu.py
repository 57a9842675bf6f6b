"""GPU parity: batched GAT structure encoder (C-ABI) vs the oracle's PyG-2.2.0 restatement (GAT-UNPINNED)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _graphs(seed, sizes, extra_dups=True):
    rng = np.random.default_rng(seed)
    edges, ecnt = [], []
    for n in sizes:
        ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        m = ii != jj
        e = np.stack([ii[m], jj[m]], 1)
        if extra_dups and n > 2:
            keep = rng.random(e.shape[0]) > 0.3                       # not complete
            e = e[keep]
            dup = e[rng.integers(0, e.shape[0], size=max(1, n // 2))]  # duplicate edges
            loops = np.stack([np.arange(n // 2)] * 2, 1)               # explicit self loops in the input
            e = np.concatenate([e, dup, loops])
        edges.append(e)
        ecnt.append(e.shape[0])
    return np.concatenate(edges).astype(np.int64), np.asarray(ecnt)


@pytest.mark.parametrize('sizes,dups', [([5, 7], True), ([64, 64, 33, 1, 2, 128], False), ([9, 17, 100, 3], True),
                                        ([129, 40], True), ([256, 3, 200], True), ([130, 255, 64], False)])
def test_multigat_fwd_bwd(sizes, dups):
    from oracle import sga_oracle as O
    from sgaligner_amd import ops
    torch.manual_seed(len(sizes))
    edges, ecnt = _graphs(sum(sizes), sizes, dups)
    T = sum(sizes)
    x = torch.randn(T, 3, dtype=torch.float64)
    p = O.init_params(['point', 'gat'], dtype=torch.float64, seed=3)
    layers = O._gat_layers(p)
    for l in layers:
        l['bias'] = torch.randn_like(l['bias']) * 0.1
        for k in l:
            l[k] = l[k].clone().requires_grad_(True)
    cot = torch.randn(T, 256, dtype=torch.float64)
    outs, so, se = [], 0, 0
    et = torch.from_numpy(edges)
    for n, ne in zip(sizes, ecnt):
        outs.append(O.multi_gat(x[so:so + n], et[se:se + ne].t(), layers))
        so += n
        se += ne
    ref = torch.cat(outs)
    (ref * cot).sum().backward()

    gb = ops.GraphBatch(np.asarray(sizes), ecnt, et.cuda())
    dl = [[l[k].detach().float().cuda().requires_grad_(True) for k in ('lin_w', 'att_src', 'att_dst', 'bias')] for l in layers]
    out = ops.multi_gat_layers(gb, x.cuda(), dl)
    (out * cot.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert (out.detach().cpu().double() - ref.detach()).abs().max() < 1e-4
    for li in range(2):
        for t, k in zip(dl[li], ('lin_w', 'att_src', 'att_dst', 'bias')):
            gref = layers[li][k].grad
            err = (t.grad.cpu().double() - gref).abs().max().item()
            assert err < 1e-3 * max(1.0, gref.abs().max().item()), (li, k, err, gref.abs().max().item())


def test_gat_too_many_nodes_fails_loudly():
    from sgaligner_amd import ops
    edges, ecnt = _graphs(0, [257], False)
    gb = ops.GraphBatch(np.asarray([257]), ecnt, torch.from_numpy(edges).cuda())
    h = torch.randn(257, 256, device='cuda')
    with pytest.raises(RuntimeError, match='at most 256'):
        ops._attn_fwd_hc(h, 2, 128, torch.randn(256, device='cuda'), torch.randn(256, device='cuda'), torch.zeros(256, device='cuda'), gb)


def test_gat_kernel_vs_hand_derived_case():
    """The HIP attention kernel against the hand-derived GATConv case of tests/gat_handcase.py (not through the oracle): duplicate
    edge counted twice, the input's self loop replaced by exactly one, LeakyReLU(0.2) on both signs, both heads, bias."""
    import gat_handcase as G
    from sgaligner_amd import ops
    h, a_s, a_d, b = G.inputs()
    for sizes, off in (([3], 0), ([2, 3, 4], 2)):                  # alone, and as the middle graph of a batch
        T = sum(sizes)
        hh = np.zeros((T, G.H * G.C))
        hh[off:off + 3] = h
        ecnt = np.asarray([len(G.EDGES)] if len(sizes) == 1 else [0, len(G.EDGES), 0])
        gb = ops.GraphBatch(np.asarray(sizes), ecnt, torch.from_numpy(G.EDGES).cuda())
        f = lambda a: torch.from_numpy(a).float().cuda()
        out = ops._attn_fwd_hc(f(hh), 2, 128, f(a_s), f(a_d), f(b), gb, check_status=True)
        torch.cuda.synchronize()
        ops.DEFERRED_CHECKS.flush()
        got = out.cpu().double().numpy()[off:off + 3]
        assert np.allclose(got, G.expected(), rtol=0, atol=2e-5), np.abs(got - G.expected()).max()


def test_gat_multiplicity_overflow_fails_loudly():
    """More than 255 copies of one (source, target) edge saturate the kernels' 8-bit multiplicity matrix: the wrapper must raise
    (deferred by at most one step), never return numbers PyG would not produce.  255 copies are fine and match the oracle."""
    from oracle import sga_oracle as O
    from sgaligner_amd import ops
    torch.manual_seed(0)
    n = 5
    h = torch.randn(n, 256)
    a_s, a_d, b = torch.randn(256) * 0.1, torch.randn(256) * 0.1, torch.zeros(256)
    base = np.array([[1, 0], [2, 0], [3, 4]], dtype=np.int64)
    for copies, ok in ((255, True), (256, False), (700, False)):
        e = np.concatenate([base, np.repeat(np.array([[4, 2]], dtype=np.int64), copies, axis=0)])
        gb = ops.GraphBatch(np.asarray([n]), np.asarray([len(e)]), torch.from_numpy(e).cuda())
        out = ops._attn_fwd_hc(h.cuda(), 2, 128, a_s.cuda(), a_d.cuda(), b.cuda(), gb, check_status=True)
        torch.cuda.synchronize()
        if ok:
            ops.DEFERRED_CHECKS.flush()
            # x = identity, lin_w = h^T  ->  the oracle's projection reproduces h
            ref = O.gat_conv(torch.eye(n, dtype=torch.float64), torch.from_numpy(e.T.copy()), h.double().t().contiguous(),
                             a_s.double().view(1, 2, 128), a_d.double().view(1, 2, 128), b.double())
            assert (out.cpu().double() - ref).abs().max() < 1e-4
        else:
            with pytest.raises(RuntimeError, match='more than 255 times'):
                ops.DEFERRED_CHECKS.flush()
    ops.DEFERRED_CHECKS.flush()                                    # the status word was reset: nothing pending raises again


def test_complete_graph_fast_path_flags_and_equality():
    """Complete graphs (every ordered pair once, in ANY order: preprocess.py:158-182 writes the annotated relations first, the supplemented 'none'
    pairs after them) are recognised on the device per batch and never read their edge list; anything else -- a missing pair, a duplicate, an
    explicit self loop, an out-of-range id -- takes the edge-list path.  Output and every gradient equal the edge-list kernels' exactly."""
    from oracle import sga_oracle as O
    from sgaligner_amd import ops
    rng = np.random.default_rng(0)
    sizes = [40, 128, 1, 2, 57, 200, 33]
    edges, ecnt = [], []
    for gi, n in enumerate(sizes):
        ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        m = ii != jj
        e = np.stack([ii[m], jj[m]], 1)
        e = e[rng.permutation(e.shape[0])]                              # arbitrary order
        if gi == 4:
            e[3] = e[5]                                                  # one pair missing, another listed twice: same edge count
        if gi == 6:
            e = np.concatenate([e, [[2, 2]]])                            # an explicit self loop on top
        edges.append(e)
        ecnt.append(e.shape[0])
    edges, ecnt = np.concatenate(edges).astype(np.int64), np.asarray(ecnt)
    T = sum(sizes)
    et = torch.from_numpy(edges).cuda()
    gb = ops.GraphBatch(np.asarray(sizes), ecnt, et)
    assert gb.complete is not None and gb.complete.cpu().tolist() == [1, 1, 1, 1, 0, 1, 0]
    torch.manual_seed(1)
    x = torch.randn(T, 3, dtype=torch.float64).cuda()
    p = O.init_params(['point', 'gat'], dtype=torch.float64, seed=3)
    layers = O._gat_layers(p)
    cot = torch.randn(T, 256).cuda()

    def run(fast):
        keep = ops.GAT_COMPLETE_FAST_PATH
        ops.GAT_COMPLETE_FAST_PATH = fast
        try:
            g2 = ops.GraphBatch(np.asarray(sizes), ecnt, et)
            assert (g2.complete is None) == (not fast)
            dl = [[l[k].detach().float().cuda().requires_grad_(True) for k in ('lin_w', 'att_src', 'att_dst', 'bias')] for l in layers]
            out = ops.multi_gat_layers(g2, x, dl)
            (out * cot).sum().backward()
            torch.cuda.synchronize()
            return out.detach(), [t.grad for li in dl for t in li]
        finally:
            ops.GAT_COMPLETE_FAST_PATH = keep
    of, gf = run(True)
    og, gg = run(False)
    assert torch.equal(of, og)
    for a, b in zip(gf, gg):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item())


def test_vs_real_pyg():
    """Closes SURVEY 8(a) row G wherever torch-geometric imports (it is not installable in the build container: the oracle's GATConv is
    "parity unpinned" there): the REAL torch_geometric.nn.GATConv(in, out, heads) stack the reference builds -- GATConv(3, 128, 2), ELU,
    GATConv(256, 128, 2): src/aligner/networks/gat.py:36-37,40-48 -- against BOTH the oracle's restatement and the HIP kernels, on the
    hand-evaluated graph and three random graphs (incomplete, duplicate edges, explicit self loops), forward and every parameter gradient."""
    pytest.importorskip('torch_geometric')
    import torch.nn.functional as F
    from torch_geometric.nn import GATConv
    from oracle import sga_oracle as O
    from sgaligner_amd import ops
    import gat_handcase as hc
    torch.manual_seed(0)
    cases = [(3, hc.EDGES)]
    for seed, n in ((1, 9), (2, 33), (3, 128)):
        e, _ = _graphs(seed, [n], True)
        cases.append((n, e))
    for n, edges in cases:
        x = torch.randn(n, 3, dtype=torch.float64)
        convs = [GATConv(3, 128, heads=2).double(), GATConv(256, 128, heads=2).double()]
        with torch.no_grad():
            for c in convs:
                c.bias.copy_(0.1 * torch.randn(256, dtype=torch.float64))
        ei = torch.from_numpy(np.ascontiguousarray(edges.T))
        ref = convs[1](F.elu(convs[0](x, ei)), ei)                    # MultiGAT.forward: dropout(p = 0) is a no-op
        cot = torch.randn_like(ref)
        (ref * cot).sum().backward()
        lws = [c.lin_src.weight if hasattr(c, 'lin_src') else c.lin.weight for c in convs]
        ref_g = [(lw.grad, c.att_src.grad, c.att_dst.grad, c.bias.grad) for lw, c in zip(lws, convs)]
        layers = [dict(lin_w=lw.detach().clone().requires_grad_(True), att_src=c.att_src.detach().clone().requires_grad_(True),
                       att_dst=c.att_dst.detach().clone().requires_grad_(True), bias=c.bias.detach().clone().requires_grad_(True))
                  for lw, c in zip(lws, convs)]
        out_o = O.multi_gat(x, ei, layers)
        (out_o * cot).sum().backward()
        assert (out_o - ref).abs().max().item() < 1e-10, n
        for li in range(2):
            for k, pg in zip(('lin_w', 'att_src', 'att_dst', 'bias'), ref_g[li]):
                assert (layers[li][k].grad - pg).abs().max().item() < 1e-9 * max(1.0, pg.abs().max().item()), (n, li, k)
        gb = ops.GraphBatch(np.asarray([n]), np.asarray([edges.shape[0]]), torch.from_numpy(edges).cuda())
        dl = [[l[k].detach().float().cuda().requires_grad_(True) for k in ('lin_w', 'att_src', 'att_dst', 'bias')] for l in layers]
        out_g = ops.multi_gat_layers(gb, x.cuda(), dl)
        (out_g * cot.float().cuda()).sum().backward()
        torch.cuda.synchronize()
        assert (out_g.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-4, n
        for li in range(2):
            for t, pg in zip(dl[li], ref_g[li]):
                assert (t.grad.cpu().double() - pg).abs().max().item() < 1e-3 * max(1.0, pg.abs().max().item()), (n, li)
