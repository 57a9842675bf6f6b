"""The exact (lattice) and fp32-faithful (gate) checks of the offset-attention kernels (sga_pct_offset_attention, sga_pct_offset_attention_bwd;
csrc/pct.hip) and the plumbing they share (no tests in this module).  Built on pct_gate / gemm_gate: same metric, same rule for r.

Operation (OA.forward, pct.py:261-269, with the shared q/k weight; G = dL/dXr), per object:
    E = Q Q^T,  P = softmax(E, dim=-1),  c_j = sum_i P[i,j],  d_j = eps + c_j (eps = 1e-9f),  Xr[j] = (sum_i P[i,j] V[i]) / d_j
    Gh[j] = G[j] / d_j,  kappa_j = -<G[j], Xr[j]> / d_j,  dV[i] = sum_j P[i,j] Gh[j],  dP[i,j] = <V[i], Gh[j]> + kappa_j,
    delta_i = sum_j P[i,j] dP[i,j],  dE = P (dP - delta_i),  dQ[i] = sum_j (dE[i,j] + dE[j,i]) Q[j].

Reference.  fp64 torch on the CPU, literally: the forward as above, dV and dQ by autograd of <Xr, G>.

Metric.  gemm_gate.rel_errors: |out - ref| / envelope in u = 2^-24, the envelope propagated through the chain (running-error kind; |.| entrywise):
    eE = |Q||Q|^T;   eP = P (1 + eE + sum_k P[i,k] eE[i,k]) + FLUSH  (pct_gate's, with scale 1);   e_c = colsum(eP);
    env Xr[j] = (eP^T |V| + |Xr| e_c)[j] / d_j;
    eGh[j] = |Gh[j]| (1 + e_c[j] / d_j)                                           (one division, and d's own error);
    ek_j = <|G[j]|, env Xr[j] + |Xr[j]|> / d_j + |kappa_j| e_c[j] / d_j;
    env dV = eP |Gh| + P eGh;
    edP[i,j] = (|V||Gh|^T + |V| eGh^T)[i,j] + ek_j + |kappa_j|                    (the product's terms, kappa's error, the add's rounding);
    ed_i = sum_j (eP |dP| + P edP)[i,j];   edE = eP |dP - delta| + P (edP + ed);   env dQ = (edE + edE^T) |Q|.

Yardstick.  The same operation in plain float32 torch on the CPU -- never the library: every reduction over rows (the column sums, P^T V, P Gh,
the dQ product) takes 32 rows per product and adds the partial results one after the other (pointnet_gate.rows_tn); delta_i as
<V[i], dV[i]> + sum_j P[i,j] kappa_j.  No guard: nothing in the kernels is discontinuous.

Families.  a, b, c: pct_gate's inputs (scales 0.8 and 4, the late maximum).  d, 'shadowed': the upper half of the rows (ceil(N/2)) has
|q|^2 = 84 in random directions; lower row k is half of upper row k.  For a shadowed column j of upper row u:  E[j,j] = 21 against the row
maximum E[j,u] = 42, E[u,j] = 42 against 84, every other row further still -- so c_j ~ e^-21 = 7.6e-10, BELOW eps: d_j is more than half eps,
Xr[j] ~ 0.43 V[j], and leaving eps out (or adding it where float32 cannot see it) moves the output by its own size.  The builder asserts
7.5e-10 <= c_j <= 3.1e-9 on those columns.

Lattice.  pct_gate.attention_lattice's inputs (Q[i] = 64 e_g(i), power-of-two group sizes, integer V and G) and an integer X: across groups
exp(-4096) is exactly 0 in float32, every c_j is exactly 1 and fl32(1 + 1e-9f) = 1 (asserted), so Xr = group mean of V, dV = group mean of G
and Diff = X - Xr bit for bit; likewise Q = 0 at power-of-two N.  dQ (differences of equal numbers times 64) is gated at its measured r.

Gate.  gemm_gate.gate_ok at r per (family, output) from profiles/pct_oa_accuracy_vs_fp32.json (tools/pct_oa_accuracy.py writes it): "worst
measured kernel / yardstick ratio x 2, rounded up" (pct_gate.ratios).  tests/test_pct_oa_cpu.py keeps table and profile together and asserts
that the emulated defects FAIL at the r in use."""
import functools
import math
import os

import torch

import gemm_gate as G
import pct_gate as PG
from pointnet_gate import rows_tn

PROFILE = os.path.join(G.ROOT, 'profiles', 'pct_oa_accuracy_vs_fp32.json')
DA, DV = PG.DA, PG.DV
EPS32 = float(torch.tensor(1e-9, dtype=torch.float32))       # the float32 nearest 1e-9: what a float32 tensor + 1e-9 adds
N_EXACT = PG.ATTN_N_EXACT
N_GATE = PG.ATTN_N_GATE
FAMILIES = ('a', 'b', 'c', 'd')
LAYOUTS = PG.LAYOUTS
OUTPUTS = ('xr', 'dv', 'dq')
DEFECTS = ('no_eps', 'eps_rowsum', 'scaled', 'no_kappa', 'no_pkappa', 'rows_only')

# r per case family and output: ceil(2 x the worst ratio measured, rms or max) over the family's cases in profiles/pct_oa_accuracy_vs_fp32.json.
# test_pct_oa_cpu.py::test_gate_ratios_are_the_measured_ones keeps them together.
R = {
    'oa_a': {'xr': 4, 'dv': 4, 'dq': 1},
    'oa_b': {'xr': 1, 'dv': 1, 'dq': 1},
    'oa_c': {'xr': 4, 'dv': 3, 'dq': 1},
    'oa_d': {'xr': 5, 'dv': 5, 'dq': 1},
    'oa_lattice': {'dq': 0},            # measured exact (0 u): at r = 0 only gate_ok's floor of 1 u is left
}


def ratios_from_profile(path=PROFILE):
    return PG.ratios_from_profile(path)


# ================================================================================================ reference, yardstick
def reference(q, v, g, T, N):
    """fp64, literally.  q [T*N,32], v, g [T*N,128] float32.  Returns dict xr, dv, dq, d (column sums + eps) and env (xr, dv, dq)."""
    q64 = q.double().view(T, N, DA).clone().requires_grad_()
    v64 = v.double().view(T, N, DV).clone().requires_grad_()
    g64 = g.double().view(T, N, DV)
    p = torch.softmax(torch.bmm(q64, q64.transpose(1, 2)), dim=-1)
    d = EPS32 + p.sum(1)                                                        # [T, j]
    xr = torch.bmm(p.transpose(1, 2), v64) / d[:, :, None]
    (xr * g64).sum().backward()
    with torch.no_grad():
        p, d, xrd = p.detach(), d.detach()[:, :, None], xr.detach()             # d: [T, j, 1]
        aq, av, ag = q64.detach().abs(), v64.detach().abs(), g64.abs()
        ee = torch.bmm(aq, aq.transpose(1, 2))
        ep = p * (1.0 + ee + (p * ee).sum(-1, keepdim=True)) + PG.FLUSH
        ec = ep.sum(1)[:, :, None]                                              # [T, j, 1]
        exr = (torch.bmm(ep.transpose(1, 2), av) + xrd.abs() * ec) / d
        gh = g64 / d
        egh = gh.abs() * (1.0 + ec / d)
        kap = -(g64 * xrd).sum(-1, keepdim=True) / d                            # [T, j, 1]
        ek = (ag * (exr + xrd.abs())).sum(-1, keepdim=True) / d + kap.abs() * ec / d
        edv = torch.bmm(ep, gh.abs()) + torch.bmm(p, egh)
        kt, ekt = kap.transpose(1, 2), ek.transpose(1, 2)                       # [T, 1, j]
        dp = torch.bmm(v64.detach(), gh.transpose(1, 2)) + kt
        edp = torch.bmm(av, gh.abs().transpose(1, 2)) + torch.bmm(av, egh.transpose(1, 2)) + ekt + kt.abs()
        delta = (p * dp).sum(-1, keepdim=True)
        ed = (ep * dp.abs() + p * edp).sum(-1, keepdim=True)
        ede = ep * (dp - delta).abs() + p * (edp + ed)
        env = dict(xr=exr, dv=edv, dq=torch.bmm(ede + ede.transpose(1, 2), aq))
    flat = lambda t, w: t.detach().reshape(T * N, w)
    return dict(xr=flat(xr, DV), dv=flat(v64.grad, DV), dq=flat(q64.grad, DA), d=d.reshape(T * N), env={k: flat(e, e.shape[-1]) for k, e in env.items()})


def yardstick(q, v, g, T, N, defect=None):
    """Plain float32 on the CPU in the stated order (module text).  defect: one of DEFECTS, the emulated defects of the CPU self-tests --
    no_eps: d = c;  eps_rowsum: eps added to the softmax's row sum instead;  scaled: SA's 1/sqrt(32) on the logits;  no_kappa: dP without
    kappa_j;  no_pkappa: delta without sum_j P kappa_j;  rows_only: no column normalisation at all (d = 1, kappa = 0)."""
    assert defect is None or defect in DEFECTS
    eps = torch.tensor(EPS32, dtype=torch.float32)
    out = dict(xr=[], dv=[], dq=[])
    for t in range(T):
        qt, vt, gt = (x.float()[t * N:(t + 1) * N] for x in (q, v, g))
        e = qt @ qt.t()
        if defect == 'scaled':
            e = e * torch.tensor(1.0 / math.sqrt(DA), dtype=torch.float32)
        if defect == 'eps_rowsum':
            ex = torch.exp(e - e.amax(1, keepdim=True))
            p = ex / (ex.sum(1, keepdim=True) + eps)
        else:
            p = torch.softmax(e, dim=-1)
        c = rows_tn(p, torch.ones(N, 1))[:, 0]
        if defect == 'rows_only':
            d = torch.ones(N)
        else:
            d = c if defect in ('no_eps', 'eps_rowsum') else eps + c
        xr = rows_tn(p, vt) / d[:, None]
        gh = gt / d[:, None]
        kap = torch.zeros(N) if defect == 'rows_only' else -(gt * xr).sum(-1) / d
        dv = rows_tn(p.t().contiguous(), gh)
        dp = vt @ gh.t()
        if defect != 'no_kappa':
            dp = dp + kap[None, :]
        delta = (vt * dv).sum(-1)
        if defect != 'no_pkappa':
            delta = delta + (p * kap[None, :]).sum(-1)
        de = p * (dp - delta[:, None])
        out['xr'].append(xr)
        out['dv'].append(dv)
        out['dq'].append(rows_tn((de + de.t()).t().contiguous(), qt))
    return {k: torch.cat(x) for k, x in out.items()}


# ================================================================================================ inputs
@functools.lru_cache(maxsize=64)
def gate_input(family, T, N, seed=0):
    """(q, v, g, ref) of one gate case (module text)."""
    if family == 'lattice':
        q, v, g, _, _ = lattice('groups', T, N, seed)
    elif family in PG.ATTN_FAMILIES:
        q, v, g, _ = PG.attention_gate_input(family, T, N, seed)
    elif family == 'd':
        gen = PG._gen('oa', family, T, N, seed)
        v, g = PG._randn(gen, T * N, DV), PG._randn(gen, T * N, DV)
        nu = (N + 1) // 2
        up = PG._randn(gen, T, nu, DA)
        up = up * (math.sqrt(84.0) / up.norm(dim=-1, keepdim=True))
        q = torch.cat([up, 0.5 * up[:, :N - nu]], 1).reshape(T * N, DA)
        p = torch.softmax(torch.bmm(q.double().view(T, N, DA), q.double().view(T, N, DA).transpose(1, 2)), -1)
        c = p.sum(1)
        assert N - nu == 0 or (7.5e-10 <= c[:, nu:].min().item() and c[:, nu:].max().item() <= 3.1e-9), 'shadowed column sums outside [7.5e-10, 3.1e-9]'
        assert c[:, :nu].min().item() > 0.5
    else:
        raise ValueError(family)
    return q, v, g, reference(q, v, g, T, N)


@functools.lru_cache(maxsize=64)
def lattice(kind, T, N, seed=0):
    """(q, v, g, x, exact): pct_gate.attention_lattice's q, v and cotangent, an integer layer input x [T*N,128], and exact = dict(xr, dv, diff)
    in fp64.  Asserts what makes torch.equal legitimate (module text)."""
    q, v, g, ex = PG.attention_lattice(kind, T, N, seed)
    x = PG._ri(PG._gen('oa-lattice-x', kind, T, N, seed), -8, 8, T * N, DV)
    if kind == 'groups':
        # without SA's 1/sqrt(32) the exponent across groups is -4096 log2(e) = -5909: far below float32's smallest subnormal
        assert torch.exp(torch.tensor(-4096.0, dtype=torch.float32)).item() == 0.0 and 4096.0 * math.log2(math.e) > 149 + 24
    q3 = q.view(T, N, DA).double()
    p = torch.softmax(torch.bmm(q3, q3.transpose(1, 2)), -1)
    assert torch.equal(p, p.transpose(1, 2)) and torch.equal(p.sum(1), torch.ones(T, N, dtype=torch.float64)), 'a column sum is not exactly 1'
    assert (torch.tensor(1.0, dtype=torch.float32) + torch.tensor(EPS32, dtype=torch.float32)).item() == 1.0
    # Xr - X: multiples of 1/|g| below 2^24 / |g|
    assert (ex['xs'].abs().max().item() + 8) * N < PG.LIMIT
    return q, v, g, x, dict(xr=ex['xs'], dv=ex['dv'], diff=x.double() - ex['xs'])


# ================================================================================================ the kernels
def run(q, v, g, T, N, layout, x=None):
    """sga_pct_offset_attention and sga_pct_offset_attention_bwd through the C ABI.  layout 'plain': contiguous q, v, xr, dq, dv; 'train': q and
    v column slices of one [T*N, 160] buffer (PCTOffsetAttentionQVFn), dq and dv slices of another, xr, g, x and diff with a row stride of 132.
    Every buffer has GUARD_ROWS rows of NaN past T*N and NaN in its padding columns, stats and work a NaN tail: all of it must still be NaN
    afterwards.  x (optional): the layer input, for Diff.  Returns dict xr, dv, dq (and diff) on the device."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    rows, tot = T * N, T * N + PG.GUARD_ROWS
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    wide = DV + 4 if layout == 'train' else DV
    if layout == 'train':
        qv, dqv = nan(tot, 160), nan(tot, 160)
        qd, vd, dq, dv = qv[:rows, :DA], qv[:rows, DA:], dqv[:rows, :DA], dqv[:rows, DA:]
        guards = [qv, dqv]
    elif layout == 'plain':
        qb, vb, dqb, dvb = nan(tot, DA), nan(tot, DV), nan(tot, DA), nan(tot, DV)
        qd, vd, dq, dv = qb[:rows], vb[:rows], dqb[:rows], dvb[:rows]
        guards = [qb, vb, dqb, dvb]
    else:
        raise ValueError(layout)
    xrb, gb, xb, dfb = nan(tot, wide), nan(tot, wide), nan(tot, wide), nan(tot, wide)
    xr, gd, xd, df = xrb[:rows, :DV], gb[:rows, :DV], xb[:rows, :DV], dfb[:rows, :DV]
    qd.copy_(q)
    vd.copy_(v)
    gd.copy_(g)
    if x is not None:
        xd.copy_(x)
    stats, work = nan(3 * rows + 64), nan(130 * rows + 64)
    L = _lib.lib()
    ptr = lambda t: t.untyped_storage().data_ptr() + 4 * t.storage_offset()     # also of a view with no rows (T = 0)
    _lib.check(L.sga_pct_offset_attention(ptr(qd), qd.stride(0), ptr(vd), vd.stride(0), ptr(xd) if x is not None else None, xd.stride(0), T, N,
                                          _p(stats), ptr(xr), xr.stride(0), ptr(df) if x is not None else None, df.stride(0), _stream()),
               'sga_pct_offset_attention')
    _lib.check(L.sga_pct_offset_attention_bwd(ptr(qd), qd.stride(0), ptr(vd), vd.stride(0), ptr(xr), xr.stride(0), ptr(gd), gd.stride(0), 1.0, T, N,
                                              _p(stats), _p(work), ptr(dq), dq.stride(0), ptr(dv), dv.stride(0), _stream()),
               'sga_pct_offset_attention_bwd')
    torch.cuda.synchronize()
    isnan = lambda t: bool(torch.isnan(t).all())
    for b in (xrb, gb, xb, dfb):
        assert isnan(b[rows:]) and isnan(b[:, DV:]), 'a kernel wrote outside the rows / columns of Xr, G, X or Diff'
    assert x is not None or isnan(dfb), 'Diff written without being asked for'
    for b in guards:
        assert isnan(b[rows:]), 'a kernel wrote past T*N rows'
    assert isnan(stats[3 * rows:]) and isnan(work[130 * rows:]), 'stats / work written past their stated sizes'
    if rows:
        assert not torch.isnan(stats[:3 * rows]).any() and not torch.isnan(work[:130 * rows]).any(), 'NaN in the statistics / workspace'
    out = dict(xr=xr, dv=dv, dq=dq)
    if x is not None:
        out['diff'] = df
    return out


def measure(family, T, N, layout, outputs=OUTPUTS):
    """output -> (kernel errors, yardstick errors) on the card."""
    q, v, g, ref = gate_input(family, T, N)
    got = run(q, v, g, T, N, layout)
    yard = yardstick(q, v, g, T, N)
    return {k: (PG.errors(got[k], ref[k], ref['env'][k]), PG.errors(yard[k], ref[k], ref['env'][k])) for k in outputs}


def cases():
    """(family, T, N, layout, outputs) of the gate: what the tests run and the profile records."""
    out = [('oa_' + f, 2, n, lay, OUTPUTS) for f in FAMILIES for n in N_GATE for lay in LAYOUTS]
    return out + [('oa_lattice', 3, n, lay, ('dq',)) for n in N_EXACT for lay in LAYOUTS]


def check(results, family, what):
    """Print every figure, then assert gemm_gate.gate_ok per output at R[family][output]."""
    bad = []
    for k, (ke, ye) in results.items():
        r = R[family][k]
        print(f'[gate] {what} {k}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
        if not G.gate_ok(ke, ye, r):
            bad.append((k, ke[:2], ye[:2], r))
    assert not bad, f'{what}: (output, kernel (max, rms), yardstick (max, rms), r) beyond the gate: {bad}'
