"""PCT encoder kernels on the card against the fp64 references of tests/pct_gate.py: bit for bit on the lattices (attention at every tile and
block edge from N = 1 on, in the contiguous and in the training layout with NaN canaries around every buffer; point max with ties in every
row walker; BatchNorm through both statistics paths), and within the measured multiple of plain fp32's own error on guarded random inputs
(three softmax regimes; BatchNorm columns at mean / std 0, 4 and 32; the widest stage as the fused node and as the chain of separate nodes)."""
import pytest
import torch

import pct_gate as PG

pytestmark = pytest.mark.gpu


def _assert_equal(got, want, what):
    got = got.detach().cpu().double()
    want = want.double()
    if not torch.equal(got, want):
        bad = ((got != want) | torch.isnan(got)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: differs from the exact reference at {len(bad)} of {got.numel()} entries; first {i}: '
                             f'got {got[i].item()!r}, want {want[i].item()!r}')


# ------------------------------------------------------------------------------------------------ attention, exact
@pytest.mark.parametrize('layout', PG.LAYOUTS)
@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('N', PG.ATTN_N_EXACT)
def test_attention_exact_group_lattice(N, T, layout):
    """Q[i] = 64 e_g(i), group sizes powers of two, members spread over tiles and blocks: Xs and dV are group means of small integers, bit for
    bit; nothing is written outside the outputs.  N = 1: Xs = V, dV = dXs and dQ = 0 exactly."""
    q, v, dxs, exact = PG.attention_lattice('groups', T, N)
    got = PG.run_attention(q, v, dxs, T, N, layout)
    _assert_equal(got['xs'], exact['xs'], f'Xs N={N} T={T} {layout}')
    _assert_equal(got['dv'], exact['dv'], f'dV N={N} T={T} {layout}')
    if N == 1:
        _assert_equal(got['xs'], v, 'Xs = V at N = 1')
        _assert_equal(got['dv'], dxs, 'dV = dXs at N = 1')
        _assert_equal(got['dq'], torch.zeros(T, PG.DA), 'dQ = 0 at N = 1')


@pytest.mark.parametrize('layout', PG.LAYOUTS)
@pytest.mark.parametrize('N', [1, 2, 4, 32, 64, 128])
def test_attention_exact_uniform(N, layout):
    """Q = 0: every attention weight is 1 / N, a power of two; Xs and dV are the object's means, dQ is exactly 0."""
    q, v, dxs, exact = PG.attention_lattice('uniform', 3, N)
    got = PG.run_attention(q, v, dxs, 3, N, layout)
    _assert_equal(got['xs'], exact['xs'], f'Xs N={N} {layout}')
    _assert_equal(got['dv'], exact['dv'], f'dV N={N} {layout}')
    _assert_equal(got['dq'], torch.zeros(3 * N, PG.DA), f'dQ N={N} {layout}')


@pytest.mark.parametrize('layout', PG.LAYOUTS)
def test_attention_no_objects_touches_nothing(layout):
    """T = 0 returns SGA_OK (run_attention checks the codes) and every buffer keeps its NaN."""
    e = torch.zeros(0, PG.DA)
    got = PG.run_attention(e, torch.zeros(0, PG.DV), torch.zeros(0, PG.DV), 0, 7, layout)
    assert all(t.numel() == 0 for t in got.values())


# ------------------------------------------------------------------------------------------------ attention, gate
@pytest.mark.parametrize('layout', PG.LAYOUTS)
@pytest.mark.parametrize('N', PG.ATTN_N_GATE)
@pytest.mark.parametrize('family', PG.ATTN_FAMILIES)
def test_attention_gate(family, N, layout):
    """Xs, dV and dQ within r x the float32 yardstick's envelope-relative error: (a) the logits of the existing tests, (b) near-one-hot rows,
    (c) every row's maximum in the last tile."""
    PG.check(PG.measure_attention(family, 2, N, layout), 'attn_' + family, f'attention {family} N={N} {layout}')


@pytest.mark.parametrize('layout', PG.LAYOUTS)
@pytest.mark.parametrize('N', PG.ATTN_N_EXACT)
def test_attention_gate_dq_on_the_lattice(N, layout):
    """dQ carries the irrational 1 / sqrt(32): judged by the gate on the lattice's inputs."""
    PG.check(PG.measure_attention('lattice', 3, N, layout, ('dq',)), 'attn_lattice', f'attention lattice N={N} {layout}')


# ------------------------------------------------------------------------------------------------ point max, exact
@pytest.mark.parametrize('C', PG.SEG_C)
@pytest.mark.parametrize('N', PG.SEG_N)
def test_segment_max_exact(N, C):
    """Integers with the first maximiser of column c in row c % N (every row walker, every fold slot) and repeated below it, an all-equal
    object, an all -inf column; row strides above C with NaN in the padding.  G, arg-max and dY equal the fp64 reference; the affine form with
    power-of-two scales of both signs, integer shifts and slope 0.25 likewise."""
    y, dg = PG.segmax_lattice(N, C)
    g_ref, am_ref = PG.segmax_reference(y)
    assert (am_ref[:, :C] == (torch.arange(C) % N)[None])[[0, 2], 1:].all()                   # the builder's placement (object 1 is all-equal)
    g, am, dy = PG.run_segmax(y, dg)
    _assert_equal(g, g_ref, f'G N={N} C={C}')
    _assert_equal(am, am_ref, f'arg-max N={N} C={C}')
    _assert_equal(dy, PG.segmax_bwd_reference(dg, am_ref, N), f'dY N={N} C={C}')
    gen = torch.Generator().manual_seed(N * 1000 + C)
    for sign in (1.0, -1.0, None):
        scale = torch.ldexp(torch.ones(C), torch.randint(-2, 3, (C,), generator=gen))
        scale = scale * (sign if sign is not None else (torch.randint(0, 2, (C,), generator=gen) * 2 - 1).float())
        shift = torch.randint(-6, 7, (C,), generator=gen).float()
        g_ref, am_ref = PG.segmax_reference(y, scale, shift, 0.25)
        g, am, dy = PG.run_segmax(y, dg, scale, shift, 0.25)
        _assert_equal(g, g_ref, f'affine G N={N} C={C} sign={sign}')
        _assert_equal(am, am_ref, f'affine arg-max N={N} C={C} sign={sign}')
        _assert_equal(dy, PG.segmax_bwd_reference(dg, am_ref, N), f'affine dY N={N} C={C} sign={sign}')


# ------------------------------------------------------------------------------------------------ BatchNorm, exact
@pytest.mark.parametrize('C', PG.BN_C_EXACT)
@pytest.mark.parametrize('R', PG.BN_R_EXACT)
def test_batchnorm_exact_lattice(R, C):
    """Integer x = a w^T: the fp64 sums of sga_bn_stats and of the GEMM epilogue are the same exact doubles at every R (across the R = 256
    boundary of the row blocks, C off the 64-channel blocks); at power-of-two R the lattice has rstd = 2^-j, and y (every activation, with and
    without residual, strided x / resid / out), running_mean and num_batches_tracked are exact on both paths."""
    x, p, exact_ok, (a, w) = PG.bn_lattice(R, C)
    want_sums = torch.cat([x.double().sum(0), (x.double() ** 2).sum(0)])
    xg, sums_g = PG.run_gemm_bnstats(a, w)
    _assert_equal(xg, x, f'x of the producing GEMM R={R} C={C}')
    for strided in (True, False):
        sums_s = PG.run_bn_stats(PG._hold(x, strided))
        _assert_equal(sums_s, want_sums, f'sga_bn_stats sums R={R} C={C} strided={strided}')
    _assert_equal(sums_g, want_sums, f'epilogue sums R={R} C={C}')
    if not exact_ok:
        return
    for act in (0, 1, 2):
        for with_resid in (False, True):
            y_ref, rm_ref, _ = PG.bn_lattice_reference(x, p, act, with_resid)
            for sums in (None, sums_g):
                for strided in (True, False):
                    what = f'R={R} C={C} act={act} resid={with_resid} path={"stats" if sums is None else "epilogue"} strided={strided}'
                    got = PG.run_bn(x if sums is None else xg, p, True, act, with_resid, sums, strided)
                    _assert_equal(got['y'], y_ref, 'y ' + what)
                    _assert_equal(got['running_mean'], rm_ref, 'running_mean ' + what)
                    assert got['num_batches_tracked'] == 4, what


# ------------------------------------------------------------------------------------------------ BatchNorm, gate
@pytest.mark.parametrize('case', PG.bn_cases(), ids=lambda c: f'{c[0]}-R{c[2]}-C{c[3]}')
def test_batchnorm_gate(case):
    """y, dx, dgamma, dbeta and the running statistics with the columns of one call at mean / std 0, 4 and 32, through sga_bn_stats, through
    the epilogue of sga_gemm_bnstats, and in eval mode: within r x the float32 two-pass yardstick."""
    family, path, R, C, training, act, with_resid = case
    res, guarded = PG.measure_bn(path, R, C, training, act, with_resid)
    print(f'[gate] guarded {guarded:.4%}')
    PG.check(res, family, f'{family} R={R} C={C} act={act}')


# ------------------------------------------------------------------------------------------------ the widest stage
@pytest.mark.parametrize('case', PG.head_cases(), ids=lambda c: f'{c[0]}-T{c[1]}-N{c[2]}-K{c[3]}-C{c[4]}-{"fused" if c[6] else "chain"}')
def test_head_gate(case):
    """conv + BatchNorm + LeakyReLU + point max as the fused node (algebraic backward) and as the chain of separate nodes, each against the
    independent fp64 reference: g, dcat, dW, dgamma, dbeta.  gamma of both signs, one all-equal object, C off the 64-channel blocks, N = 1,
    and the fused node at N = 1024, C = 1024 -- both caps of sga_pct_head_scatter."""
    family, T, N, K, C, training, fused = case
    res, guarded = PG.measure_head(T, N, K, C, training, fused)
    print(f'[gate] guarded {guarded:.4%}')
    PG.check(res, family, f'{family} T={T} N={N} K={K} C={C} {"fused" if fused else "chain"}')


@pytest.mark.parametrize('N,C', [(1025, 8), (8, 1025)])
def test_head_scatter_refuses_beyond_its_caps(N, C):
    """sga_pct_head_scatter above 1024 points per object or 1024 channels: an error code, and dcat untouched."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    K = 8
    coef = torch.ones(1, C, device='cuda')
    am = torch.zeros(1, C, device='cuda', dtype=torch.int32)
    w = torch.ones(C, K, device='cuda')
    dcat = torch.full((N, K), float('nan'), device='cuda')
    rc = _lib.lib().sga_pct_head_scatter(_p(coef), _p(am), _p(w), 1, N, C, K, _p(dcat), K, _stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert torch.isnan(dcat).all()


def test_naive_pct_above_the_point_cap_takes_the_chain(monkeypatch):
    """NaivePCT with 1025 points per object: the widest stage runs as separate nodes (the fused node is not called), forward and backward
    finite."""
    from sgaligner_amd import pct_ops
    from sgaligner_amd.aligner.networks.pct import NaivePCT
    calls = []
    real = pct_ops.segment_max
    monkeypatch.setattr(pct_ops, 'linear_bn_lrelu_max', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the fused node was called')))
    monkeypatch.setattr(pct_ops, 'segment_max', lambda *a, **k: (calls.append(a[1:]), real(*a, **k))[1])
    torch.manual_seed(0)
    net = NaivePCT().cuda().train()
    x = torch.randn(2, 3, 1025, device='cuda')
    out = net(x)
    out.sum().backward()
    torch.cuda.synchronize()
    assert calls == [(2, 1025)]
    assert torch.isfinite(out).all()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
