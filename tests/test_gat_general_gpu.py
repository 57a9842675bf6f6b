"""GPU: the general GAT path -- any heads, 1 <= channels <= 256, any depth, dropout -- against the oracle's PyG-2.2.0 restatement under the
fp32-faithful gate of tests/gat_general_gate.py, the hand-derived case re-laid at 3 x 70, the kernels of 2 x 128 under the same
gate, and the encoder with a non-default stack."""
import numpy as np
import pytest
import torch

import gat_general_gate as GG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('heads,channels', GG.KERNEL_CASES)
def test_attention_kernel_one_layer(heads, channels):
    """Forward and backward of one attention launch on a given H against gat_conv with an identity projection: one batch mixing 1 .. 256
    nodes, a zero-node graph in the middle, a complete graph (fast path), duplicates and explicit self loops, a graph with no edges, and
    L, L + 1 nodes for both LDS-residency bounds L; then the same batch cut at each L and L + 1, so that the launch's nmax sits on both
    sides of the bound."""
    for cap, meas in GG.measure_kernel(heads, channels).items():
        GG.assert_gate(meas, f'kernel {heads}x{channels} nmax<={cap}')


def test_hand_derived_case_at_three_heads_of_seventy():
    """tests/gat_handcase.py's three-node case (not through the oracle) re-laid at H = 3, C = 70: the same three non-zero channels, and a
    third head all zero, whose attention is uniform and whose output is its bias."""
    import gat_handcase as HC
    from sgaligner_amd import ops
    H, C = 3, 70
    h0, as0, ad0, b0 = HC.inputs()
    exp0 = HC.expected()

    def relay(a):                                                   # [.., 2 * 128] -> [.., 3 * 70]
        out = np.zeros(a.shape[:-1] + (H * C,))
        for hd in range(2):
            out[..., hd * C:hd * C + C] = a[..., hd * HC.C:hd * HC.C + C]
        return out
    assert all(np.abs(a[..., C:HC.C]).max() == 0 and np.abs(a[..., HC.C + C:]).max() == 0 for a in (h0, as0, ad0, b0, exp0))
    h, a_s, a_d, b, want = relay(h0), relay(as0), relay(ad0), relay(b0), relay(exp0)
    b[2 * C:] = np.linspace(-1.0, 1.0, C)                           # the zero head: out = bias
    want[:, 2 * C:] = b[2 * C:]
    for sizes, off in (([3], 0), ([2, 3, 4], 2)):                   # alone, and as the middle graph of a batch
        T = sum(sizes)
        hh = np.zeros((T, H * C))
        hh[off:off + 3] = h
        ecnt = np.asarray([len(HC.EDGES)] if len(sizes) == 1 else [0, len(HC.EDGES), 0])
        gb = ops.GraphBatch(np.asarray(sizes), ecnt, torch.from_numpy(HC.EDGES).cuda())
        f = lambda a: torch.from_numpy(a).float().cuda()
        out = ops._attn_fwd_hc(f(hh), H, C, f(a_s), f(a_d), f(b), gb, check_status=True)
        torch.cuda.synchronize()
        ops.DEFERRED_CHECKS.flush()
        got = out.cpu().double().numpy()[off:off + 3]
        assert np.allclose(got, want, rtol=0, atol=2e-5), np.abs(got - want).max()


@pytest.mark.parametrize('which', range(len(GG.CANON_SHAPES)))
def test_kernel_at_two_heads_of_128(which):
    """2 x 128 on the shapes of test_multigat_fwd_bwd: that shape's kernels inside the gate of the fp64 reference."""
    GG.assert_gate(GG.measure_canon(which), f'2x128 shapes[{which}]')


def _existing_bounds(got, ref, keys):
    """The bounds of test_multigat_fwd_bwd: output < 1e-4, gradients < 1e-3 max(1, |g|max)."""
    for k in keys:
        err = (got[k].detach().cpu().double().reshape(ref[k].shape) - ref[k]).abs().max().item()
        bound = 1e-4 if k == 'out' else 1e-3 * max(1.0, ref[k].abs().max().item())
        assert err < bound, (k, err, bound)


@pytest.mark.parametrize('which', range(len(GG.STACKS)))
def test_stacks(which):
    case = GG.stack_case(which)
    got, net, out = GG.stack_run(case)
    keys = GG.stack_outputs(case)
    ref = {k: case['ref'][k] for k in keys}
    ke, ye = GG.errors(got, ref), GG.errors(case['yard'], ref)
    GG.assert_gate({k: (ke[k], ye[k]) for k in keys}, f'stack {case["units"]}/{case["heads"]}')
    _existing_bounds(got, ref, keys)
    # backward a second time on the retained graph: the same gradients (nothing saved was changed or freed)
    first = {k: v.clone() for k, v in got.items() if k != 'out'}
    for p in net.parameters():
        p.grad = None
    out.backward(case['cot'].cuda(), retain_graph=True)
    torch.cuda.synchronize()
    again = GG.stack_grads(net, out)
    for k, v in first.items():
        # equal up to the order of the kernels' floating-point atomics (d a_s across a workgroup's waves, d att_* across graphs, split-K dW)
        assert (again[k] - v).abs().max().item() <= 1e-5 * max(1.0, v.abs().max().item()), k


def test_dropout_given_masks():
    """p = 0.5 with the masks given: the stack equals the oracle's layers applied to the masked inputs, and the mask multiplies dx."""
    case = GG.stack_case(GG.MASKED_STACK, True)
    got = GG.stack_run(case)[0]
    keys = GG.stack_outputs(case)
    ref = {k: case['ref'][k] for k in keys}
    ke, ye = GG.errors(got, ref), GG.errors(case['yard'], ref)
    GG.assert_gate({k: (ke[k], ye[k]) for k in keys}, 'masked stack')
    dropped = case['masks'][0] == 0
    assert dropped.any() and (got['dx'].cpu()[dropped] == 0).all() and (got['dx'].cpu()[~dropped] != 0).any()


def test_dropout_drawn_masks():
    case = GG.stack_case(1)
    gb = GG.graph_batch(case['graphs'])
    x = case['x'].cuda()
    net0, netp = GG.stack_model(case, 0.0), GG.stack_model(case, 0.3)
    with torch.no_grad():
        base = net0.eval().forward_batched(x, gb)
        assert torch.equal(netp.eval().forward_batched(x, gb), base)             # eval: the identity, whatever p
        assert torch.equal(net0.train().forward_batched(x, gb), base)            # p = 0: the identity, whatever the mode
        netp.train()
        torch.manual_seed(5)
        a = netp.forward_batched(x, gb)
        torch.manual_seed(5)
        b = netp.forward_batched(x, gb)
        assert torch.equal(a, b) and not torch.equal(a, base)
        # eval and p = 0 draw nothing: the generator is where it was
        torch.manual_seed(5)
        state = torch.cuda.get_rng_state()
        netp.eval().forward_batched(x, gb)
        net0.train().forward_batched(x, gb)
        assert torch.equal(torch.cuda.get_rng_state(), state)


def test_encoder_with_a_non_default_stack():
    from oracle import sga_oracle as O
    from sgaligner_amd.aligner.sg_aligner import MultiModalEncoder
    from sgaligner_amd.synthetic import make_batch, to_device
    units, heads = [3, 64, 96, 64], [4, 2, 4]
    dd = make_batch(2, (6, 5), 16, ragged=True)
    torch.manual_seed(3)
    enc = MultiModalEncoder(['point', 'gat', 'rel'], rel_dim=41, attr_dim=164, hidden_units=units, heads=heads).cuda()
    with torch.no_grad():
        for l in enc.structure_encoder.layer_stack:
            l.bias.uniform_(-0.1, 0.1)
    out = enc(to_device(dd, 'cuda'))['gat']
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    out.backward(cot.float().cuda())
    torch.cuda.synchronize()
    # fp64: O.multi_gat graph by graph, then structure_embedding
    sd = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
    layers = [{k: v.clone().requires_grad_(True) for k, v in l.items()}
              for l in O._gat_layers({k: v for k, v in sd.items()}, len(units) - 1)]
    pose = dd['tot_rel_pose'].double()
    outs, so, se = [], 0, 0
    for b in range(int(dd['batch_size'])):
        for side in range(2):
            n, ne = int(dd['graph_per_obj_count'][b][side]), int(dd['graph_per_edge_count'][b][side])
            outs.append(O.multi_gat(pose[so:so + n], dd['edges'][se:se + ne].t(), layers))
            so, se = so + n, se + ne
    ref = torch.cat(outs) @ sd['structure_embedding.weight'].t() + sd['structure_embedding.bias']
    (ref * cot).sum().backward()
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-4
    for i, l in enumerate(enc.structure_encoder.layer_stack):
        for t, k in zip(l.params(), ('lin_w', 'att_src', 'att_dst', 'bias')):
            g = layers[i][k].grad
            err = (t.grad.cpu().double() - g).abs().max().item()
            assert err < 1e-3 * max(1.0, g.abs().max().item()), (i, k, err)
    # the reference hard-codes structure_embedding = Linear(256, emb_dim): a stack that ends 200 wide fails in forward, naming both widths
    bad = MultiModalEncoder(['point', 'gat', 'rel'], rel_dim=41, attr_dim=164, hidden_units=[3, 64, 100], heads=[4, 2]).cuda()
    with pytest.raises(RuntimeError, match='200 wide.*256'):
        bad(to_device(dd, 'cuda'))


def test_limits_fail_loudly_on_the_general_path():
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    with pytest.raises(NotImplementedError, match='256'):
        MultiGAT([3, 300, 128], [1, 2])
    n = 257
    e = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int64)
    gb = ops.GraphBatch(np.asarray([n]), np.asarray([len(e)]), torch.from_numpy(e).cuda())
    net = MultiGAT([3, 48, 100], [3, 1]).cuda()
    with pytest.raises(RuntimeError, match='at most 256'):
        net.forward_batched(torch.randn(n, 3, device='cuda'), gb)
