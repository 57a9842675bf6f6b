"""Offset attention on the card (tests/pct_oa_gate.py, tests/pct_oa_ref.py): the kernels bit for bit on the lattices at every tile and block
edge from N = 1 on, in the contiguous and in the training layout with NaN canaries round every buffer; within the measured multiple of plain
fp32's own error on four families of random inputs, the shadowed one with column sums below eps among them; the modules OA, SPCT and
NaivePCT(attention='oa') against the reference's recorded run and the fp64 restatement; and the 'sa' default bit for bit what it was."""
import numpy as np
import pytest
import torch

import pct_gate as PG
import pct_oa_gate as OG
import pct_oa_ref as REF
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _assert_equal(got, want, what):
    got = got.detach().cpu().double()
    want = want.double()
    if not torch.equal(got, want):
        bad = ((got != want) | torch.isnan(got)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: differs from the exact reference at {len(bad)} of {got.numel()} entries; first {i}: '
                             f'got {got[i].item()!r}, want {want[i].item()!r}')


# ------------------------------------------------------------------------------------------------ kernels, exact
@pytest.mark.parametrize('layout', OG.LAYOUTS)
@pytest.mark.parametrize('N', OG.N_EXACT)
def test_offset_attention_exact_group_lattice(N, layout):
    """Q[i] = 64 e_g(i), power-of-two groups spread over tiles and blocks: every column sum is 1 and 1 + eps = 1, so Xr and dV are group means
    of small integers and Diff = X - Xr, bit for bit; nothing is written outside the outputs.  N = 1: Xr = V, dV = G, dQ = 0."""
    T = 3
    q, v, g, x, exact = OG.lattice('groups', T, N)
    got = OG.run(q, v, g, T, N, layout, x=x)
    _assert_equal(got['xr'], exact['xr'], f'Xr N={N} {layout}')
    _assert_equal(got['dv'], exact['dv'], f'dV N={N} {layout}')
    _assert_equal(got['diff'], exact['diff'], f'Diff N={N} {layout}')
    if N == 1:
        _assert_equal(got['xr'], v, 'Xr = V at N = 1')
        _assert_equal(got['dv'], g, 'dV = G at N = 1')
        _assert_equal(got['dq'], torch.zeros(T, OG.DA), 'dQ = 0 at N = 1')
    assert torch.equal(OG.run(q, v, g, T, N, layout)['xr'], got['xr']), 'Xr depends on whether Diff is asked for'


@pytest.mark.parametrize('layout', OG.LAYOUTS)
@pytest.mark.parametrize('N', [1, 2, 4, 32, 64, 128])
def test_offset_attention_exact_uniform(N, layout):
    """Q = 0: every attention weight is 1 / N, every column sum 1; Xr and dV are the object's means, dQ is exactly 0."""
    q, v, g, x, exact = OG.lattice('uniform', 3, N)
    got = OG.run(q, v, g, 3, N, layout, x=x)
    _assert_equal(got['xr'], exact['xr'], f'Xr N={N} {layout}')
    _assert_equal(got['dv'], exact['dv'], f'dV N={N} {layout}')
    _assert_equal(got['diff'], exact['diff'], f'Diff N={N} {layout}')
    _assert_equal(got['dq'], torch.zeros(3 * N, OG.DA), f'dQ N={N} {layout}')


@pytest.mark.parametrize('layout', OG.LAYOUTS)
def test_offset_attention_no_objects_touches_nothing(layout):
    """T = 0 returns SGA_OK (run checks the codes) and every buffer keeps its NaN."""
    got = OG.run(torch.zeros(0, OG.DA), torch.zeros(0, OG.DV), torch.zeros(0, OG.DV), 0, 7, layout, x=torch.zeros(0, OG.DV))
    assert all(t.numel() == 0 for t in got.values())


# ------------------------------------------------------------------------------------------------ kernels, gate
@pytest.mark.parametrize('layout', OG.LAYOUTS)
@pytest.mark.parametrize('N', OG.N_GATE)
@pytest.mark.parametrize('family', OG.FAMILIES)
def test_offset_attention_gate(family, N, layout):
    """Xr, dV and dQ within r x the float32 yardstick's envelope-relative error: (a) moderate logits, (b) one-hot rows, (c) every row's maximum
    in the last tile, (d) shadowed columns whose sum is below eps."""
    OG.check(OG.measure(family, 2, N, layout), 'oa_' + family, f'offset attention {family} N={N} {layout}')


@pytest.mark.parametrize('layout', OG.LAYOUTS)
@pytest.mark.parametrize('N', OG.N_EXACT)
def test_offset_attention_gate_dq_on_the_lattice(N, layout):
    OG.check(OG.measure('lattice', 3, N, layout, ('dq',)), 'oa_lattice', f'offset attention lattice N={N} {layout}')


def test_segment_mean_fixed_order_and_backward():
    """sga_segment_mean: integers (exact in any order) bit for bit, its backward dG / N bit for bit at power-of-two N; random values within
    float32 of the fp64 mean."""
    from sgaligner_amd import pct_ops
    gen = torch.Generator().manual_seed(3)
    for T, N, C in ((3, 1, 65), (2, 5, 64), (3, 64, 200), (2, 45, 1024)):
        y0 = torch.randint(-9, 10, (T * N, C), generator=gen).float()
        y = y0.cuda().requires_grad_()
        m = pct_ops.segment_mean(y, T, N)
        cot = torch.randint(-4, 5, (T, C), generator=gen).float()
        (m * cot.cuda()).sum().backward()
        want = (y0.view(T, N, C).double().sum(1).float() / N)
        _assert_equal(m, want, f'mean T={T} N={N} C={C}')
        _assert_equal(y.grad, (cot / N)[:, None, :].expand(T, N, C).reshape(T * N, C), f'mean backward T={T} N={N} C={C}')
        r = torch.randn(T * N, C, generator=gen)
        err = (pct_ops.segment_mean(r.cuda(), T, N).cpu().double() - r.view(T, N, C).double().mean(1)).abs().max().item()
        assert err <= N * 2.0 ** -24 * r.abs().max().item(), err


@pytest.mark.parametrize('with_x', [False, True])
def test_autograd_nodes_split_and_fused_layouts_agree(with_x):
    """pct_ops.PCTOffsetAttentionFn (q and v apart) and PCTOffsetAttentionQVFn (one [T*N,160] tensor): the same kernels on two layouts give
    the same bits, forward and backward, with the result Xr (no x) or x - Xr; and both are the gate's reference to 1e-4."""
    from sgaligner_amd import pct_ops
    T, N = 2, 33
    q0, v0, g0, ref = OG.gate_input('a', T, N)
    x0 = PG._randn(PG._gen('oa-nodes', T, N), T * N, OG.DV)
    res = []
    for fused in (False, True):
        x = x0.cuda().requires_grad_() if with_x else None
        if fused:
            qv = torch.cat([q0, v0], 1).cuda().requires_grad_()
            y = pct_ops.pct_offset_attention_qv(qv, T, N, x=x)
        else:
            q, v = q0.cuda().requires_grad_(), v0.cuda().requires_grad_()
            y = pct_ops.pct_offset_attention(q, v, T, N, x=x)
        (y * g0.cuda()).sum().backward()
        dq, dv = (qv.grad[:, :32], qv.grad[:, 32:]) if fused else (q.grad, v.grad)
        res.append((y.detach(), dq, dv, x.grad if with_x else None))
    (ya, dqa, dva, dxa), (yb, dqb, dvb, dxb) = res
    assert torch.equal(ya, yb) and torch.equal(dqa, dqb) and torch.equal(dva, dvb)
    sign = -1.0 if with_x else 1.0                              # y = x - Xr: dL/dXr = -g
    want = (x0.double() - ref['xr']) if with_x else ref['xr']
    for got, exp, name in ((ya, want, 'y'), (dqa, sign * ref['dq'], 'dq'), (dva, sign * ref['dv'], 'dv')):
        err = (got.cpu().double() - exp).abs().max().item()
        assert err < 1e-4 * max(1.0, exp.abs().max().item()), (name, err)
    if with_x:
        assert torch.equal(dxa, g0.cuda()) and torch.equal(dxb, g0.cuda())


# ------------------------------------------------------------------------------------------------ modules
def _close(got, ref, tol, floor, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref).max()
    assert err < tol * max(np.abs(ref).max(), floor), (what, err, np.abs(ref).max())


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_oa_module_against_golden_and_restatement(mode):
    """OA(128), T = 2, N = 37: output 1e-3 of the maximum; every parameter gradient and the input gradient 1e-3 of max(own maximum, 1e-2 of
    the largest gradient); the updated running statistics.  Against the reference's recorded run and the restatement alike."""
    from sgaligner_amd.aligner.networks.pct import OA
    g = load_golden('pct_oa')
    sd32 = REF.golden_state_dict('oa')
    m = OA(128)
    m.load_state_dict(sd32, strict=True)
    m = m.cuda().train(mode == 'train')
    x, cot = REF.oa_inputs()
    xd = x.cuda().requires_grad_()
    y = m(xd)
    (y * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    sd, leaves = REF.leaves64(sd32)
    xi = x.double().transpose(1, 2).clone().requires_grad_()
    up = {}
    yr = REF.oa_layer(xi, sd, '', mode == 'train', up)
    (yr * cot.double().transpose(1, 2)).sum().backward()
    for ref_y, tag in ((g[f'oa_{mode}__y'], 'golden'), (yr.detach().transpose(1, 2).numpy(), 'restatement')):
        _close(y.detach().cpu().numpy(), ref_y, 1e-3, 1.0, f'y {tag}')
    if mode == 'eval':
        with torch.no_grad():                                   # inference: folded BatchNorm, Diff straight from the attention kernel
            _close(m(x.cuda()).cpu().numpy(), g['oa_eval__y'], 1e-3, 1.0, 'y golden (inference path)')
    named = dict(m.named_parameters())
    grads = {k: p.grad.cpu().numpy() for k, p in named.items()}
    grads['__dx'] = xd.grad.cpu().numpy()
    gmax = max(np.abs(v).max() for v in grads.values())
    for k, got in grads.items():
        ref_g = g[f'oa_{mode}__dx'] if k == '__dx' else g[f'oa_{mode}__g__{k}']
        ref_r = xi.grad.transpose(1, 2).numpy() if k == '__dx' else leaves[k].grad.numpy()
        _close(got, ref_g, 1e-3, 1e-2 * gmax, f'{k} golden')
        _close(got, ref_r, 1e-3, 1e-2 * gmax, f'{k} restatement')
    if mode == 'train':
        after = m.state_dict()
        for k in ('after_norm.running_mean', 'after_norm.running_var'):
            _close(after[k].cpu().numpy(), g['oa_train__after__' + k], 1e-4, 1.0, k)
            _close(after[k].cpu().numpy(), up[k].numpy(), 1e-4, 1.0, k)
        assert int(after['after_norm.num_batches_tracked']) == int(g['oa_train__after__after_norm.num_batches_tracked']) == 1


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_spct_against_golden_and_restatement(mode):
    """SPCT(), T = 2, N = 24: the three outputs and the parameter gradients of the recorded linear functional, same tolerances; x is a view
    [T, 1024, N] of the point-major activation."""
    from sgaligner_amd.aligner.networks.pct import SPCT
    g = load_golden('pct_oa')
    sd32 = REF.golden_state_dict('spct')
    m = SPCT()
    m.load_state_dict(sd32, strict=True)
    m = m.cuda().train(mode == 'train')
    x, cx, cmax, cmean = REF.spct_inputs()
    y, ymax, ymean = m(x.cuda())
    assert y.shape == (REF.SP_T, 1024, REF.SP_N) and y.stride(1) == 1, 'x must be a permuted view of the point-major activation'
    ((y * cx.cuda()).sum() + (ymax * cmax.cuda()).sum() + (ymean * cmean.cuda()).sum()).backward()
    torch.cuda.synchronize()
    sd, leaves = REF.leaves64(sd32)
    yr, rmax, rmean, up = REF.spct(x.double(), sd, mode == 'train')
    ((yr * cx.double()).sum() + (rmax * cmax.double()).sum() + (rmean * cmean.double()).sum()).backward()
    yc = y.detach().cpu().numpy()
    _close(yc[:, ::REF.SUB], g[f'spct_{mode}__x'], 1e-3, 1.0, 'x golden')
    _close(yc, yr.detach().numpy(), 1e-3, 1.0, 'x restatement')
    for got, name, ref_r in ((ymax, 'max', rmax), (ymean, 'mean', rmean)):
        _close(got.detach().cpu().numpy(), g[f'spct_{mode}__{name}'], 1e-3, 1.0, name + ' golden')
        _close(got.detach().cpu().numpy(), ref_r.detach().numpy(), 1e-3, 1.0, name + ' restatement')
    if mode == 'eval':
        with torch.no_grad():                                   # inference path
            for got, name in zip(m(x.cuda()), ('x', 'max', 'mean')):
                got = got.cpu().numpy()
                _close(got[:, ::REF.SUB] if name == 'x' else got, g[f'spct_eval__{name}'], 1e-3, 1.0, name + ' golden (inference path)')
    named = dict(m.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in named.values())
    for k, p in named.items():
        _close(REF.sub_rows(p.grad).cpu().numpy(), g[f'spct_{mode}__g__{k}'], 1e-3, 1e-2 * gmax, k + ' golden')
        _close(p.grad.cpu().numpy(), leaves[k].grad.numpy(), 1e-3, 1e-2 * gmax, k + ' restatement')
    if mode == 'train':
        after = m.state_dict()
        for k, v in up.items():
            if 'num_batches' in k:
                assert int(after[k]) == int(v) == int(g['spct_train__after__' + k])
            else:
                _close(after[k].cpu().numpy(), g['spct_train__after__' + k], 1e-4, 1.0, k)
                _close(after[k].cpu().numpy(), v.numpy(), 1e-4, 1.0, k)


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_naive_pct_with_offset_attention_against_restatement(mode):
    """NaivePCT(attention='oa'), Dropout p = 0, on SPCT's recorded input: output and every parameter gradient against the restatement (which
    tests/test_pct_oa_cpu.py pins on the golden through the trunk it shares with SPCT)."""
    from sgaligner_amd.aligner.networks.pct import NaivePCT
    sd32 = REF.golden_state_dict('naive')
    m = NaivePCT(attention='oa')
    m.load_state_dict(sd32, strict=True)
    m = m.cuda().train(mode == 'train')
    m.dp1.p = m.dp2.p = 0.0
    x = REF.spct_inputs()[0]
    cot = torch.randn(REF.SP_T, 256, generator=torch.Generator().manual_seed(9))
    y = m(x.cuda())
    (y * cot.cuda()).sum().backward()
    sd, leaves = REF.leaves64(sd32)
    yr, _ = REF.naive_pct_oa(x.double(), sd, mode == 'train')
    (yr * cot.double()).sum().backward()
    _close(y.detach().cpu().numpy(), yr.detach().numpy(), 1e-3, 1.0, 'y')
    named = dict(m.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in named.values())
    for k, p in named.items():
        _close(p.grad.cpu().numpy(), leaves[k].grad.numpy(), 1e-3, 1e-2 * gmax, k)
    if mode == 'eval':
        with torch.no_grad():
            _close(m(x.cuda()).cpu().numpy(), yr.detach().numpy(), 1e-3, 1.0, 'y (inference path)')


def test_oa_rejects_untied_weights_and_other_widths():
    from sgaligner_amd.aligner.networks.pct import OA
    m = OA(128).cuda().eval()
    m.q_conv.weight = torch.nn.Parameter(m.k_conv.weight.detach().clone() + 1.0)
    with pytest.raises(RuntimeError), torch.no_grad():
        m(torch.randn(1, 128, 5, device='cuda'))
    with pytest.raises(NotImplementedError), torch.no_grad():
        OA(256).cuda().eval()(torch.randn(1, 256, 5, device='cuda'))


def test_pct_oa_train_step_inside_the_aligner():
    """modules = ['pct', 'gat', 'rel', 'attr'] with pct_attention='oa': optimiser steps run and lower the loss on the same batch."""
    from sgaligner_amd.aligner.networks.pct import OA
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    steps = AlignerSteps(['pct', 'gat', 'rel', 'attr'], device='cuda', seed=1, pct_attention='oa')
    assert isinstance(steps.model.object_encoder.sa1, OA)
    dd = to_device(make_batch(4, 10, 64, seed=3), 'cuda')
    opt = torch.optim.Adam(steps.params, lr=1e-3)
    losses = []
    for _ in range(4):
        steps.model.train()
        opt.zero_grad(set_to_none=True)
        _, ld = steps.train_step(0, 0, dd)
        ld['loss'].backward()
        opt.step()
        losses.append(float(ld['loss'].detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    steps.model.eval()
    with torch.no_grad():
        assert torch.isfinite(steps.model(dd)['joint']).all()


def test_pct_oa_eval_chunked_and_alone_equal_the_batch():
    """Inference with attention='oa': chunked equals unchunked bit for bit, and an object of the batch equals the same object run alone."""
    from sgaligner_amd.aligner.networks.pct import NaivePCT, SPCT
    torch.manual_seed(4)
    m = NaivePCT(attention='oa').cuda().eval()
    x = torch.randn(23, 3, 70, device='cuda')
    with torch.no_grad():
        y_all = m(x)
        m.eval_chunk_rows = 5 * 70                                # 5 objects per chunk: 4 full chunks + 3
        y_chunk = m(x)
        y_one = m(x[7:8])
        s = SPCT().cuda().eval()
        a_all, a_one = s(x), s(x[7:8])
    assert y_all.shape == (23, 256) and torch.equal(y_all, y_chunk) and torch.equal(y_all[7:8], y_one)
    assert all(torch.equal(a[7:8], b) for a, b in zip(a_all, a_one))


@pytest.mark.parametrize('tag', ['small', 'p512', 'ragged'])
def test_sa_default_is_bit_for_bit_what_it_was(tag):
    """attention='sa' (the default): the inference output on the seeded inputs of test_pct_eval_forward_golden has the bits recorded from the
    build before offset attention existed (tests/golden/pct_sa_bits.npz, written on the card by that build)."""
    from sgaligner_amd.aligner.networks.pct import NaivePCT
    g, bits = load_golden('pct_eval'), load_golden('pct_sa_bits')
    m = NaivePCT()
    assert m.attention == 'sa'
    m.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith('sd__')}, strict=True)
    m = m.cuda().eval()
    with torch.no_grad():
        y = m(torch.from_numpy(g['x_' + tag]).cuda()).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), bits['y_' + tag].view(np.uint32))
