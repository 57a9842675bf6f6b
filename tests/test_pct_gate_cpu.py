"""Self-tests of tests/pct_gate.py that need no card: the lattice builders' conditions at every listed shape, the fp64 references against
oracle/pct_oracle.py, the guard's share and the yardstick's own standing in every gate case, the table of ratios against the committed
profile, and emulated defects that must FAIL at the ratios in use."""
import math

import pytest
import torch

import gemm_gate as G
import pct_gate as PG
from oracle import pct_oracle as O


# ------------------------------------------------------------------------------------------------ lattices
@pytest.mark.parametrize('N', PG.ATTN_N_EXACT)
def test_attention_lattice_conditions(N):
    """The builder's own assertions (power-of-two groups, partial sums below 2^24, the cross-group exponent below every subnormal) hold, groups
    straddle tiles where there are several, and the literal fp64 softmax gives the group means up to its own subnormal cross terms."""
    for T in (1, 3):
        q, v, dxs, exact = PG.attention_lattice('groups', T, N)
        ref = PG.attention_reference(q, v, dxs, T, N)
        assert (ref['xs'] - exact['xs']).abs().max() < 1e-300 and (ref['dv'] - exact['dv']).abs().max() < 1e-300
        assert (exact['xs'] * max(PG.group_sizes(N)) % 1 == 0).all()
    if N >= 64:
        g = q.view(3, N, PG.DA)[0].argmax(-1)
        tiles = {(int(a), int(i) // 32) for i, a in enumerate(g)}
        assert max(sum(1 for (a, _) in tiles if a == k) for k in set(g.tolist())) > 1, 'no group straddles two tiles'
    if N & (N - 1) == 0:
        PG.attention_lattice('uniform', 3, N)


def test_segmax_and_batchnorm_lattice_conditions():
    for N in PG.SEG_N:
        for C in PG.SEG_C:
            y, _ = PG.segmax_lattice(N, C)
            assert (y[[0, 2]][:, :, 1:] == y[[0, 2]][:, :, 1:].round()).all() and torch.isinf(y[0, :, 0]).all() and (y[1] == y[1, 0, 0]).all()
    for R in PG.BN_R_EXACT:
        for C in PG.BN_C_EXACT:
            x, p, exact_ok, (a, w) = PG.bn_lattice(R, C)
            assert exact_ok == (R in (2, 256)) and torch.equal(a @ w.t(), x)
            if exact_ok:                                     # rstd is a power of two: y = +-gamma + beta exactly
                y, rm, _ = PG.bn_lattice_reference(x, p, 0, False)
                assert torch.equal((y - p['beta']).abs(), p['gamma'].abs().expand_as(y))


# ------------------------------------------------------------------------------------------------ references against the oracle
def test_references_agree_with_the_oracle():
    gen = torch.Generator().manual_seed(5)
    T, N = 2, 9
    x = torch.randn(T, 128, N, generator=gen, dtype=torch.float64)
    wq = torch.randn(32, 128, 1, generator=gen, dtype=torch.float64) * 0.1
    wv = torch.randn(128, 128, 1, generator=gen, dtype=torch.float64) * 0.1
    eye = torch.eye(128, dtype=torch.float64)[:, :, None]
    one, zero = torch.ones(128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64)
    # trans_conv = identity and an eval BatchNorm that only adds 1000: sa_forward(x) = x + x_s + 1000
    sd = {'s.q_conv.weight': wq, 's.k_conv.weight': wq, 's.v_conv.weight': wv, 's.v_conv.bias': zero, 's.trans_conv.weight': eye,
          's.trans_conv.bias': zero, 's.after_norm.running_mean': zero, 's.after_norm.running_var': one - 1e-5, 's.after_norm.weight': one,
          's.after_norm.bias': one * 1000}
    xs_oracle = (O.sa_forward(x, sd, 's') - x - 1000).permute(0, 2, 1).reshape(T * N, 128)
    rows = x.permute(0, 2, 1).reshape(T * N, 128)
    q, v = (rows @ wq[:, :, 0].t()).float(), (rows @ wv[:, :, 0].t()).float()
    ref = PG.attention_reference(q, v, torch.zeros(T * N, 128), T, N)
    want = torch.softmax(q.double().view(T, N, 32) @ q.double().view(T, N, 32).transpose(1, 2) / math.sqrt(32), -1).transpose(1, 2) @ v.double().view(T, N, 128)
    assert torch.allclose(ref['xs'], want.reshape(T * N, 128), rtol=1e-13, atol=1e-13)
    assert torch.allclose(xs_oracle, want.reshape(T * N, 128), rtol=1e-5, atol=1e-5)           # (q, v rounded to float32 on the way)

    # BatchNorm (train) and the widest stage: oracle._bn_train / _conv / leaky_relu / max
    R, C, K = T * N, 7, 8
    cat = torch.randn(R, K, generator=gen)
    w = torch.randn(C, K, generator=gen)
    p = dict(gamma=torch.randn(C, generator=gen), beta=torch.randn(C, generator=gen), rm=torch.randn(C, generator=gen),
             rv=1 + torch.rand(C, generator=gen), dg=torch.randn(T, C, generator=gen), momentum=0.1, eps=1e-5)
    sd = {'b.weight': p['gamma'].double(), 'b.bias': p['beta'].double(), 'b.running_mean': p['rm'].double(), 'b.running_var': p['rv'].double()}
    ns = {}
    y3 = O._conv(cat.double().view(T, N, K).permute(0, 2, 1), w.double()[:, :, None])
    z = torch.nn.functional.leaky_relu(O._bn_train(y3, sd, 'b', ns), PG.HEAD_SLOPE)
    href = PG.head_reference(cat, w, p, T, N, True, guard=False)
    assert torch.allclose(href['g'], z.max(-1)[0], rtol=1e-12, atol=1e-12)
    assert torch.allclose(href['running_mean'], ns['b.running_mean'], rtol=1e-12, atol=1e-12)
    xb = (cat @ w.t())
    bp = dict(p, resid=None, dy=torch.randn(R, C, generator=gen))
    bref = PG.bn_reference(xb, bp, True, 0)
    ns = {}
    yb = O._bn_train(xb.double(), sd, 'b', ns)
    assert torch.allclose(bref['y'], yb, rtol=1e-12, atol=1e-12)
    assert torch.allclose(bref['running_var'], ns['b.running_var'], rtol=1e-12, atol=1e-12)
    assert torch.allclose(PG.bn_reference(xb, bp, False, 0)['y'], O._bn(xb.double(), sd, 'b'), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the gate's own standing
def test_gate_ratios_are_the_measured_ones():
    assert PG.R == PG.ratios_from_profile()
    fams = {c[0] for c in PG.attention_cases()} | {c[0] for c in PG.bn_cases()} | {c[0] for c in PG.head_cases()}
    assert set(PG.R) == fams


def _bn_cpu_case(path, R, C, training, act, with_resid):
    inp, p = PG.bn_gate_input(path, R, C)
    x = inp if path == 'stats' else (inp[0] @ inp[1].t())
    pp = dict(p, resid=p['resid'] if with_resid else None)
    ref = PG.bn_reference(x, pp, training, act)
    return x, dict(pp, dy=ref['dy']), ref


def test_guard_share_and_yardstick_in_every_gate_case():
    """Under the reference alone: at most 5 % of any case is guarded, and the float32 yardstick passes the gate it sets (finite errors, zero
    where the envelope is zero)."""
    for family, T, N, layout, outputs in PG.attention_cases():
        if layout != 'plain':
            continue
        q, v, dxs, ref = PG.attention_gate_input(family[5:], T, N)
        yard = PG.attention_yardstick(q, v, dxs, T, N)
        for k in outputs:
            e = PG.errors(yard[k], ref[k], ref['env'][k])
            assert G.gate_ok(e, e, PG.R[family][k])
    for family, path, R, C, training, act, with_resid in PG.bn_cases():
        x, pk, ref = _bn_cpu_case(path, R, C, training, act, with_resid)
        assert ref['guarded'] <= PG.GUARD_MAX
        yard = PG.bn_yardstick(x, pk, ref, training, act)
        for k in (PG.BN_OUT_TRAIN if training else PG.BN_OUT_EVAL):
            e = PG.errors(yard[k], ref[k], ref['env'][k])
            assert G.gate_ok(e, e, PG.R[family][k])
    for family, T, N, K, C, training, fused in PG.head_cases():
        cat, w, p = PG.head_gate_input(T, N, K, C)
        ref = PG.head_reference(cat, w, p, T, N, training)
        assert ref['guarded'] <= PG.GUARD_MAX
        yard = PG.head_yardstick(cat, w, p, ref, T, N, training)
        for k in PG.HEAD_OUT:
            e = PG.errors(yard[k], ref[k], ref['env'][k])
            assert G.gate_ok(e, e, PG.R[family][k])


# ------------------------------------------------------------------------------------------------ emulated defects must fail
@pytest.mark.parametrize('path', ['stats', 'gemm'])
@pytest.mark.parametrize('C', PG.BN_C_GATE)
@pytest.mark.parametrize('R', [257, 1025])
def test_gate_catches_one_pass_fp32_variance(R, C, path):
    """(i) var = sum x^2 / R - mean^2 from float32 partial sums -- sga_bn_stats' four row walkers per row block, the GEMM epilogue's lanes of
    64 rows -- at mean / std up to 32: running_var (and y, dx with it) FAILS at the r in use."""
    family = 'bn_train' if path == 'stats' else 'bn_train_gemm'
    x, pk, ref = _bn_cpu_case(path, R, C, True, 2, False)
    walkers = 4 * ((R + 255) // 256) if path == 'stats' else 2 * ((R + 127) // 128)
    bad = PG.bn_yardstick(x, pk, ref, True, 2, one_pass=True, walkers=walkers)
    yard = PG.bn_yardstick(x, pk, ref, True, 2)
    k = 'running_var'
    ke, ye = PG.errors(bad[k], ref[k], ref['env'][k]), PG.errors(yard[k], ref[k], ref['env'][k])
    print(f'one-pass variance R={R} C={C}: {ke[:2]} u against the yardstick {ye[:2]} u, r = {PG.R[family][k]}')
    assert not G.gate_ok(ke, ye, PG.R[family][k])


@pytest.mark.parametrize('N', [129, 160])
def test_gate_catches_a_dropped_softmax_rescale(N):
    """(ii) the online softmax without l exp(m - m_new) when the running maximum moves, on the late-maximum family: Xs and dV FAIL."""
    q, v, dxs, ref = PG.attention_gate_input('c', 2, N)
    bad = PG.attention_yardstick(q, v, dxs, 2, N, drop_rescale=True)
    yard = PG.attention_yardstick(q, v, dxs, 2, N)
    for k in ('xs', 'dv'):
        ke, ye = PG.errors(bad[k], ref[k], ref['env'][k]), PG.errors(yard[k], ref[k], ref['env'][k])
        assert not G.gate_ok(ke, ye, PG.R['attn_c'][k]), (k, ke, ye)


@pytest.mark.parametrize('family', ['a', 'c'])
def test_gate_catches_dq_without_the_key_role(family):
    """(iii) dQ without P[j,i] (dP[j,i] - delta_j) -- the gradient through the shared weight's key role: FAILS.  (Not in regime (b): with
    numerically one-hot rows dE vanishes, and with it both roles.)"""
    q, v, dxs, ref = PG.attention_gate_input(family, 2, 33)
    bad = PG.attention_yardstick(q, v, dxs, 2, 33, drop_key_role=True)
    yard = PG.attention_yardstick(q, v, dxs, 2, 33)
    ke, ye = PG.errors(bad['dq'], ref['dq'], ref['env']['dq']), PG.errors(yard['dq'], ref['dq'], ref['env']['dq'])
    assert not G.gate_ok(ke, ye, PG.R['attn_' + family]['dq']), (ke, ye)


@pytest.mark.parametrize('N', [3, 4, 5, 45])
def test_exact_comparison_catches_the_last_maximiser(N):
    """(iv) the LAST maximiser where torch.max takes the first: same G, another arg-max and another dY on the tie lattice."""
    y, dg = PG.segmax_lattice(N, 65)
    g, am = PG.segmax_reference(y)
    g2, am2 = PG.segmax_reference(y, last=True)
    assert torch.equal(g, g2) and not torch.equal(am, am2)
    assert not torch.equal(PG.segmax_bwd_reference(dg, am, N), PG.segmax_bwd_reference(dg, am2, N))
