"""The exact (lattice) and fp32-faithful (gate) checks of the PCT encoder kernels (csrc/pct.hip, csrc/bn.hip, the BatchNorm-statistics
epilogue of csrc/gemm.hip, pct_ops.py), and the plumbing they share (no tests in this module).

Reference.  fp64 torch on the CPU, literally:
  attention (pct.py:211-222, q_conv and k_conv share their weight)   E = Q Q^T / sqrt(32), P = softmax(E, dim=-1), Xs[j] = sum_i P[i,j] V[i];
      dV, dQ by autograd of <Xs, dXs>;
  point max (pct.py:308) with the FIRST maximiser as arg-max, its backward a scatter to that row;
  BatchNorm1d + activation + residual (pct.py:122-123, :226-229) in train mode (biased batch variance, unbiased running variance, momentum) and
      eval mode; dx, dgamma, dbeta by autograd;
  the widest stage (pct.py:282-286, :306-308)  g[t,c] = max_n LeakyReLU_0.2(BatchNorm(cat W^T)); dcat, dW, dgamma, dbeta by autograd through
      the reference's arg-max rows.

Metric.  gemm_gate.rel_errors: |out - ref| / envelope in u = 2^-24, the envelope PROPAGATED through the chain (running-error kind; |.| entrywise):
  attention   eE = |Q||Q|^T / sqrt(32);  eP = P (1 + eE + sum_k P[i,k] eE[i,k]) + 2^-126 / u  (softmax is 1-Lipschitz in its logits per unit
              of P; the last term is float32's underflow: fp64 keeps a weight of 1e-313 that every float32 evaluation flushes to zero);
              env Xs = eP^T |V|;  env dV = eP |dXs|;  with dP = V dXs^T, edP = |V||dXs|^T, delta = rowsum(P dP), ed = rowsum(eP |dP| + P edP),
              edE = eP |dP - delta| + P (edP + ed):   env dQ = (edE + edE^T) |Q| / sqrt(32).
  BatchNorm   env mean = mean|x|;  env var = var (a sum of squares: nothing cancels in the two-pass form, so a one-pass evaluation that cancels
              (mean/std)^2 of its digits is judged against what is left);  rstd inherits half of var's relative error;
              e_xhat = (|x| + mean|x|) rstd + |xhat| var / (2 (var + eps));  env y = act' (e_xhat |gamma| + |beta|) + |resid|;
              env running_mean = (1-m)|rm| + m mean|x|;  env running_var = (1-m)|rv| + m var R/(R-1);
              with g = dy act'(pre):  env dbeta = sum|g|;  env dgamma = sum |g| e_xhat;
              env dx = |gamma| rstd (|g| + mean|g| + e_xhat |mean(g xhat)| + |xhat| mean(|g| e_xhat)) + |dx| var / (2 (var + eps)).
              Eval mode: the same with the running statistics as exact constants (no var term, no batch means in dx).
  head        ey = |cat||W|^T;  env var = 2 mean(|y - mean| (ey + mean ey));  e_xhat, env g as for BatchNorm with ey for |x|, taken at the
              arg-max row;  dz = dg LeakyReLU'(z);  env dbeta = sum|dz|;  env dgamma = sum |dz| e_xhat;
              e_dy = |gamma| rstd (|D| + sum|dz|/R + e_xhat |S2|/R + |xhat| env dgamma / R) + |dy| env var / (2 (var + eps))  (D: dz at its row);
              env dW = e_dy^T |cat|;  env dcat = e_dy |W|.

Yardstick.  The same operation in plain float32 torch on the CPU -- never the library -- in a stated order: every reduction over rows takes
32 rows per product and adds the partial results one after the other (pointnet_gate.rows_tn); the softmax backward's row term as
delta_i = <V[i], dV[i]>; BatchNorm in the two-pass form (mean, then the
mean of squared deviations) and y = x scale + shift as the kernels apply it; the reference's masks and arg-max.

Guard.  A ReLU / LeakyReLU pre-activation within DELTA = 2^-16 of its envelope of zero, or an arg-max whose runner-up (among rows with other
inputs: equal rows tie exactly in any arithmetic) lies within DELTA of the envelopes, may flip between fp32 and fp64; the cotangent of such an
entry (BatchNorm) or (t, c) channel (head) is zeroed before kernel and reference see it.  At most GUARD_MAX of a case may be guarded.

Lattice.  Inputs for which every correct evaluation gives the reference bit for bit, whatever its order:
  attention   every row belongs to a group g(i), Q[i] = 64 e_g(i): E = 4096 inside a group, 0 across, and exp2((0 - 4096) log2(e)/sqrt(32))
              underflows to exactly 0; group sizes are powers of two, so l = |g| and 1/l are exact; V, dXs small integers, every partial sum
              below 2^24.  Xs[j] = mean of V over g(j), dV[i] = mean of dXs over g(i).  Q = 0 (uniform attention) at power-of-two N likewise.
  point max   integers; power-of-two scale, integer shift, slope 0.25 for the affine form.
  BatchNorm   x[r,c] = mean_c + s_r 2^j_c with integer mean_c and signs s_r that balance (R a power of two), eps = 0: var = 4^j, rstd = 2^-j;
              power-of-two gamma, integer beta and resid, momentum 1/2: y, running_mean, num_batches_tracked and the fp64 sums are exact.
The builders assert these conditions; they are what makes torch.equal legitimate.

Gate.  gemm_gate.gate_ok at r per (family, output) from profiles/pct_accuracy_vs_fp32.json (tools/pct_accuracy.py writes it): "worst
measured kernel / yardstick ratio x 2, rounded up", the yardstick's figure taken no smaller than the floor gate_ok grants (`ratios`).  tests/test_pct_gate_cpu.py keeps table and profile together and asserts that emulated
defects FAIL at the r in use."""
import functools
import json
import math
import os
import zlib

import torch

import gemm_gate as G
from pointnet_gate import first_argmax, rows_tn

ROOT = G.ROOT
PROFILE = os.path.join(ROOT, 'profiles', 'pct_accuracy_vs_fp32.json')
DELTA = 2.0 ** -16
GUARD_MAX = 0.05
LIMIT = 2.0 ** 24
DA, DV = 32, 128
SLOPE = {0: 1.0, 1: 0.0, 2: float(torch.tensor(0.2, dtype=torch.float32))}      # act: 0 none, 1 ReLU, 2 LeakyReLU(0.2f)
FLUSH = 2.0 ** -126 / G.U               # what float32 may flush to zero, as an envelope (in units of u) of every attention weight
GUARD_ROWS = 8                           # NaN rows past T*N in every buffer the attention kernels are given

# r per case family and output: ceil(2 x the worst ratio measured, rms or max) over the family's cases in profiles/pct_accuracy_vs_fp32.json.
# test_pct_gate_cpu.py::test_gate_ratios_are_the_measured_ones keeps them together.
R = {
    'attn_a': {'xs': 4, 'dv': 3, 'dq': 4},
    'attn_b': {'xs': 1, 'dv': 1, 'dq': 3},
    'attn_c': {'xs': 4, 'dv': 4, 'dq': 3},
    'attn_lattice': {'dq': 1},
    'bn_train': {'y': 2, 'dx': 2, 'dgamma': 2, 'dbeta': 3, 'running_mean': 3, 'running_var': 3},
    'bn_train_gemm': {'y': 2, 'dx': 2, 'dgamma': 2, 'dbeta': 3, 'running_mean': 4, 'running_var': 3},
    'bn_eval': {'y': 3, 'dx': 2, 'dgamma': 2, 'dbeta': 3},
    'head_train': {'g': 3, 'dcat': 4, 'dw': 3, 'dgamma': 3, 'dbeta': 2},
    'head_eval': {'g': 3, 'dcat': 3, 'dw': 3, 'dgamma': 3, 'dbeta': 2},
}


def ratios_from_profile(path=PROFILE):
    """family -> output -> ceil(2 x worst measured kernel / yardstick ratio), the derivation R states."""
    worst = {}
    for c in json.load(open(path))['cases']:
        w = worst.setdefault(c['family'], {})
        w[c['output']] = max(w.get(c['output'], 0.0), c['ratio_rms'], c['ratio_max'])
    return {f: {k: int(math.ceil(2.0 * v - 1e-9)) for k, v in w.items()} for f, w in worst.items()}


def ratios(ke, ye):
    """(max ratio, rms ratio) of kernel against yardstick errors (max, rms, n): kernel / max(yardstick, the floor gemm_gate.gate_ok grants that
    figure) -- FLOOR_U for the max, FLOOR_U / sqrt(n) for the rms.  Below its floor a figure is never compared, and a yardstick that happens to
    be exact (one term, or a lattice) would otherwise set a ratio that means nothing."""
    return ke[0] / max(ye[0], G.FLOOR_U), ke[1] / max(ye[1], G.FLOOR_U / max(ke[2], 1) ** 0.5)


def errors(out, ref, env):
    return G.rel_errors(out.detach().cpu(), ref, env)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _ri(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


# ================================================================================================ attention
ATTN_N_EXACT = (1, 2, 3, 4, 5, 31, 32, 33, 64, 127, 128, 129, 160)
ATTN_N_GATE = (5, 33, 129, 160)
ATTN_FAMILIES = ('a', 'b', 'c')
LAYOUTS = ('plain', 'train')


def attention_reference(q, v, dxs, T, N):
    """fp64, literally.  q [T*N,32], v, dxs [T*N,128] float32.  Returns dict xs, dv, dq and env (same keys)."""
    q64 = q.double().view(T, N, DA).clone().requires_grad_()
    v64 = v.double().view(T, N, DV).clone().requires_grad_()
    d64 = dxs.double().view(T, N, DV)
    energy = torch.bmm(q64, q64.transpose(1, 2)) / math.sqrt(DA)
    attention = torch.softmax(energy, dim=-1)
    xs = torch.bmm(attention.transpose(1, 2), v64)                  # x_s = x_v @ attention, point-major
    (xs * d64).sum().backward()
    with torch.no_grad():
        p = attention.detach()
        aq, av, ad = q64.detach().abs(), v64.detach().abs(), d64.abs()
        ee = torch.bmm(aq, aq.transpose(1, 2)) / math.sqrt(DA)
        ep = p * (1.0 + ee + (p * ee).sum(-1, keepdim=True)) + FLUSH
        dp = torch.bmm(v64.detach(), d64.transpose(1, 2))
        edp = torch.bmm(av, ad.transpose(1, 2))
        delta = (p * dp).sum(-1, keepdim=True)
        ed = (ep * dp.abs() + p * edp).sum(-1, keepdim=True)
        ede = ep * (dp - delta).abs() + p * (edp + ed)
        env = dict(xs=torch.bmm(ep.transpose(1, 2), av), dv=torch.bmm(ep, ad), dq=torch.bmm(ede + ede.transpose(1, 2), aq) / math.sqrt(DA))
    flat = lambda t, w: t.detach().reshape(T * N, w)
    return dict(xs=flat(xs, DV), dv=flat(v64.grad, DV), dq=flat(q64.grad, DA), env={k: flat(e, e.shape[-1]) for k, e in env.items()})


def attention_yardstick(q, v, dxs, T, N, drop_rescale=False, drop_key_role=False):
    """Plain float32 on the CPU, reductions over rows in 32-row tiles added in sequence.  drop_rescale / drop_key_role: the emulated defects of
    the CPU self-tests (the online softmax's row sum without its rescale when the running maximum moves; dQ without P[j,i] (dP[j,i] - delta_j))."""
    s = torch.tensor(1.0 / math.sqrt(DA), dtype=torch.float32)
    out = dict(xs=[], dv=[], dq=[])
    for t in range(T):
        qt, vt, dt = (x.float()[t * N:(t + 1) * N] for x in (q, v, dxs))
        e = (qt @ qt.t()) * s
        if drop_rescale:
            m = torch.full((N,), -math.inf)
            l = torch.zeros(N)
            for j0 in range(0, N, 32):
                mn = torch.maximum(m, e[:, j0:j0 + 32].amax(1))
                l = l + torch.exp(e[:, j0:j0 + 32] - mn[:, None]).sum(1)         # the kernel's is l exp(m - mn) + ...
                m = mn
            p = torch.exp(e - m[:, None]) / l[:, None]
        else:
            p = torch.softmax(e, dim=-1)
        out['xs'].append(rows_tn(p, vt))
        out['dv'].append(rows_tn(p.t().contiguous(), dt))
        dp = vt @ dt.t()
        # delta_i = sum_j P[i,j] dP[i,j] as <V[i], dV[i]>, the flash form.  (Taken as rowsum(P dP), a numerically one-hot row gives
        # delta_i = dP[i,i] to the bit and dE = 0 exactly: a yardstick 10^18 times more accurate than float32 owes anybody.)
        de = p * (dp - (vt * out['dv'][-1]).sum(-1, keepdim=True))
        g = (de if drop_key_role else de + de.t()) * s
        out['dq'].append(rows_tn(g.t().contiguous(), qt))
    return {k: torch.cat(x) for k, x in out.items()}


@functools.lru_cache(maxsize=64)
def attention_gate_input(family, T, N, seed=0):
    """(q, v, dxs, ref).  a: randn 0.8 (the existing tests' regime).  b: randn 4 -- logits of the order of +-100, rows numerically one-hot.
    c: 'late maximum' -- q[i] = a_i d + noise with |d|^2 = 32 and a_i growing with i: every row's maximum sits in the last tile and the running
    maximum of the online softmax jumps at every tile.  lattice: attention_lattice's inputs, for dQ (which carries the irrational scale)."""
    if family == 'lattice':
        q, v, dxs, _ = attention_lattice('groups', T, N, seed)
    else:
        gen = _gen('attn', family, T, N, seed)
        v, dxs = _randn(gen, T * N, DV), _randn(gen, T * N, DV)
        if family == 'a':
            q = _randn(gen, T * N, DA) * 0.8
        elif family == 'b':
            q = _randn(gen, T * N, DA) * 4.0
        elif family == 'c':
            d = _ri(gen, 0, 1, T, 1, DA) * 2 - 1
            a = 0.3 + 2.5 * (torch.arange(N).float() + 1) / N
            q = (a.view(1, N, 1) * d + 0.1 * _randn(gen, T, N, DA)).reshape(T * N, DA)
        else:
            raise ValueError(family)
    return q, v, dxs, attention_reference(q, v, dxs, T, N)


def group_sizes(N):
    """N as a sum of powers of two, at most 32 of them, split on until there are 8 (or all are 1)."""
    sizes = [1 << b for b in range(N.bit_length()) if N >> b & 1]
    while len(sizes) < 8 and max(sizes) > 1:
        m = max(sizes)
        sizes.remove(m)
        sizes += [m // 2, m // 2]
    assert sum(sizes) == N and len(sizes) <= 32 and all(s & (s - 1) == 0 for s in sizes)
    return sorted(sizes, reverse=True)


@functools.lru_cache(maxsize=64)
def attention_lattice(kind, T, N, seed=0):
    """(q, v, dxs, exact) with exact = dict(xs, dv) in fp64 (module text).  kind 'groups': the grouped one-hot lattice, members of a group
    spread by a seeded permutation over the 32-row tiles and 128-row blocks; 'uniform': Q = 0, N a power of two."""
    gen = _gen('lattice', kind, T, N, seed)
    v, dxs = _ri(gen, -8, 8, T, N, DV), _ri(gen, -8, 8, T, N, DV)
    q = torch.zeros(T, N, DA)
    grp = torch.zeros(T, N, dtype=torch.long)
    if kind == 'groups':
        sizes = group_sizes(N)
        for t in range(T):
            grp[t, torch.randperm(N, generator=gen)] = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        q.scatter_(2, grp[:, :, None], 64.0)
        # across groups the exponent is (0 - 4096) / sqrt(32) * log2(e) = -1044.6: below fp32's (and bf16's) smallest subnormal, 2^-149
        assert 4096.0 / math.sqrt(DA) * math.log2(math.e) > 149 + 24
    elif kind == 'uniform':
        assert N & (N - 1) == 0, 'uniform attention is exact only at power-of-two N'
    else:
        raise ValueError(kind)
    same = (grp[:, :, None] == grp[:, None, :]).double()                 # [T, i, j]
    size = same.sum(-1, keepdim=True)
    assert ((size.log2() % 1) == 0).all()
    p = same / size                                                      # row i: 1/|g(i)| on its group
    # every partial sum, in any order, is a multiple of 1/|g| bounded by the sum of the absolute terms
    assert max((same @ v.double().abs()).max().item(), (same @ dxs.double().abs()).max().item()) < LIMIT
    exact = dict(xs=(p.transpose(1, 2) @ v.double()).reshape(T * N, DV), dv=(p @ dxs.double()).reshape(T * N, DV))
    return q.reshape(T * N, DA), v.reshape(T * N, DV), dxs.reshape(T * N, DV), exact


def run_attention(q, v, dxs, T, N, layout):
    """sga_pct_attention and sga_pct_attention_bwd through the C ABI.  layout 'plain': contiguous q, v, xs, dq, dv; 'train': q and v column
    slices of one [T*N, 160] buffer (PCTAttentionQVFn), dq and dv slices of another, xs and dxs with a row stride of 132.  Every buffer has
    GUARD_ROWS rows of NaN past T*N and NaN in its padding columns, stats and work a NaN tail: all of it must still be NaN afterwards.
    Returns dict xs, dv, dq (device)."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    rows, tot = T * N, T * N + GUARD_ROWS
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    if layout == 'train':
        qv, dqv, xsb, dxb = nan(tot, 160), nan(tot, 160), nan(tot, 132), nan(tot, 132)
        qd, vd, dq, dv = qv[:rows, :DA], qv[:rows, DA:], dqv[:rows, :DA], dqv[:rows, DA:]
    elif layout == 'plain':
        qb, vb, dqb, dvb, xsb, dxb = nan(tot, DA), nan(tot, DV), nan(tot, DA), nan(tot, DV), nan(tot, DV), nan(tot, DV)
        qd, vd, dq, dv = qb[:rows], vb[:rows], dqb[:rows], dvb[:rows]
    else:
        raise ValueError(layout)
    xs, dxd = xsb[:rows, :DV], dxb[:rows, :DV]
    qd.copy_(q)
    vd.copy_(v)
    dxd.copy_(dxs)
    stats, work = nan(2 * rows + 64), nan(rows + 64)
    L = _lib.lib()
    # (the address of a view's first element, also of a view with no rows: T = 0 must not fail on a null pointer)
    ptr = lambda t: t.untyped_storage().data_ptr() + 4 * t.storage_offset()
    _lib.check(L.sga_pct_attention(ptr(qd), qd.stride(0), ptr(vd), vd.stride(0), T, N, _p(stats), ptr(xs), xs.stride(0), _stream()), 'sga_pct_attention')
    _lib.check(L.sga_pct_attention_bwd(ptr(qd), qd.stride(0), ptr(vd), vd.stride(0), ptr(dxd), dxd.stride(0), T, N, _p(stats), _p(work),
                                       ptr(dq), dq.stride(0), ptr(dv), dv.stride(0), _stream()), 'sga_pct_attention_bwd')
    torch.cuda.synchronize()
    isnan = lambda t: bool(torch.isnan(t).all())
    assert isnan(xsb[rows:]) and isnan(xsb[:, DV:]), 'the forward wrote outside Xs'
    assert isnan(stats[2 * rows:]) and isnan(work[rows:]), 'stats / work written past T*N'
    if layout == 'train':
        assert isnan(dqv[rows:]) and isnan(qv[rows:]) and isnan(dxb[rows:]) and isnan(dxb[:, DV:]), 'the backward wrote outside its rows'
    else:
        assert isnan(dqb[rows:]) and isnan(dvb[rows:]), 'the backward wrote outside its rows'
    if rows:
        assert not torch.isnan(stats[:2 * rows]).any(), 'NaN in the row statistics'
    return dict(xs=xs, dv=dv, dq=dq)


def measure_attention(family, T, N, layout, outputs=('xs', 'dv', 'dq')):
    """output -> (kernel errors, yardstick errors) on the card."""
    q, v, dxs, ref = attention_gate_input(family, T, N)
    got = run_attention(q, v, dxs, T, N, layout)
    yard = attention_yardstick(q, v, dxs, T, N)
    return {k: (errors(got[k], ref[k], ref['env'][k]), errors(yard[k], ref[k], ref['env'][k])) for k in outputs}


def attention_cases():
    """(family, T, N, layout, outputs) of the gate: what the tests run and the profile records."""
    cases = [('attn_' + f, 2, n, lay, ('xs', 'dv', 'dq')) for f in ATTN_FAMILIES for n in ATTN_N_GATE for lay in LAYOUTS]
    cases += [('attn_lattice', 3, n, lay, ('dq',)) for n in ATTN_N_EXACT for lay in LAYOUTS]
    return cases


# ================================================================================================ point max
SEG_N = (1, 3, 4, 5, 45)
SEG_C = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=32)
def segmax_lattice(N, C, T=3):
    """(y [T,N,C] integers, dg [T,C]).  The first maximiser of column c sits in row c % N -- every row walker n % 4 and every slot of the
    final fold takes its turn -- and is repeated in later rows; object 1 is all-equal; column 0 of object 0 is all -inf."""
    gen = _gen('segmax', N, C, T)
    y = _ri(gen, -5, 5, T, N, C)
    first = torch.arange(C) % N
    rows = torch.arange(N)[:, None]
    again = (torch.rand(T, N, C, generator=gen) < 0.4) & (rows > first[None, :])[None]
    y = torch.where((rows == first[None, :])[None] | again, torch.full_like(y, 9.0), y)
    if T > 1:
        y[1] = 3.0
    y[0, :, 0] = -math.inf
    return y, _ri(gen, -4, 4, T, C)


def segmax_reference(y, scale=None, shift=None, slope=None, last=False):
    """(g, first arg-max) in fp64; with scale / shift / slope the affine form act(scale y + shift) first.  last: the LAST maximiser (the
    emulated defect of the CPU self-test)."""
    z = y.double()
    if scale is not None:
        z = z * scale.double() + shift.double()
        z = torch.where(z > 0, z, z * slope)
    if last:
        mx, am = first_argmax(z.flip(1))
        return mx, z.shape[1] - 1 - am
    return first_argmax(z)


def run_segmax(y, dg, scale=None, shift=None, slope=None, pad=5):
    """sga_segment_max (or _affine) and sga_segment_max_bwd with row strides of C + pad, NaN in the padding.  Returns (g, am, dy [T*N, C])."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    T, N, C = y.shape
    yb = torch.full((T * N + 2, C + pad), float('nan'), device='cuda')
    yb[:T * N, :C] = y.reshape(T * N, C).cuda()
    yv = yb[:T * N, :C]
    g = torch.full((T * C + 8,), float('nan'), device='cuda')
    am = torch.full((T * C + 8,), -7, device='cuda', dtype=torch.int32)
    L = _lib.lib()
    if scale is None:
        _lib.check(L.sga_segment_max(_p(yv), yv.stride(0), T, N, C, _p(g), _p(am), _stream()), 'sga_segment_max')
    else:
        sc, sh = scale.float().cuda(), shift.float().cuda()
        _lib.check(L.sga_segment_max_affine(_p(yv), yv.stride(0), T, N, C, _p(sc), _p(sh), float(slope), _p(g), _p(am), _stream()), 'sga_segment_max_affine')
    torch.cuda.synchronize()
    assert torch.isnan(g[T * C:]).all() and (am[T * C:] == -7).all(), 'the point max wrote past its outputs'
    dyb = torch.full((T * N + 2, C + pad), float('nan'), device='cuda')
    dyv = dyb[:T * N, :C]
    dgd = dg.float().contiguous().cuda()
    _lib.check(L.sga_segment_max_bwd(_p(dgd), _p(am), T, N, C, _p(dyv), dyv.stride(0), _stream()), 'sga_segment_max_bwd')
    torch.cuda.synchronize()
    assert torch.isnan(dyb[T * N:]).all() and torch.isnan(dyb[:, C:]).all(), 'the point-max backward wrote outside dY'
    return g[:T * C].view(T, C), am[:T * C].view(T, C), dyv


def segmax_bwd_reference(dg, am, N):
    T, C = dg.shape
    dy = torch.zeros(T, N, C, dtype=torch.float64)
    dy.scatter_(1, am.long()[:, None, :], dg.double()[:, None, :])
    return dy.reshape(T * N, C)


# ================================================================================================ BatchNorm
BN_R_EXACT = (2, 7, 255, 256, 257, 1025)
BN_C_EXACT = (1, 63, 64, 65, 200)
BN_R_GATE = (7, 257, 1025)
BN_C_GATE = (65, 200)
BN_RATIOS = (0.0, 4.0, 32.0)             # column mean / std, mixed across the columns of one call
BN_OUT_TRAIN = ('y', 'dx', 'dgamma', 'dbeta', 'running_mean', 'running_var')
BN_OUT_EVAL = ('y', 'dx', 'dgamma', 'dbeta')
BN_K = 32                                # contraction length of the producing GEMM on the epilogue path


def act64(z, act):
    return z if act == 0 else torch.where(z > 0, z, z * SLOPE[act])


def bn_reference(x, p, training, act, guard=True):
    """fp64 from float32 x [R,C] and p = dict(gamma, beta, rm, rv, resid or None, dy, momentum, eps).  Returns dict with the outputs, env, the
    cotangent dy as the kernel must be given it (guarded), guarded (share of entries), and what yardstick and emulation need."""
    xd = x.double()
    R = x.shape[0]
    gamma = p['gamma'].double().clone().requires_grad_()
    beta = p['beta'].double().clone().requires_grad_()
    xg = xd.clone().requires_grad_()
    mom, eps = p['momentum'], p['eps']
    if training:
        mean = xg.mean(0)
        var = ((xg - mean) ** 2).mean(0)
    else:
        mean, var = p['rm'].double(), p['rv'].double()
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xg - mean) * rstd
    pre = xhat * gamma + beta
    y = act64(pre, act)
    if p['resid'] is not None:
        y = y + p['resid'].double()
    with torch.no_grad():
        ax = xd.abs()
        varc = var.detach()
        half = varc / (2.0 * (varc + eps)) if training else torch.zeros_like(varc)
        emean = ax.mean(0) if training else mean.abs()
        exh = (ax + emean) * rstd.detach() + xhat.detach().abs() * half
        epre = exh * gamma.detach().abs() + beta.detach().abs()
        dact = torch.ones_like(epre) if act == 0 else torch.where(pre.detach() > 0, torch.ones_like(epre), torch.full_like(epre, SLOPE[act]))
        env = dict(y=epre * (dact if act != 1 else 1.0) + (p['resid'].double().abs() if p['resid'] is not None else 0.0))
        near = (pre.detach().abs() <= DELTA * epre) if (act != 0 and guard) else torch.zeros_like(epre, dtype=torch.bool)
        dy = torch.where(near, torch.zeros_like(p['dy']), p['dy'])
    (y * dy.double()).sum().backward()
    out = dict(y=y.detach(), dx=xg.grad, dgamma=gamma.grad, dbeta=beta.grad, dy=dy, guarded=near.float().mean().item(), mask=pre.detach() > 0)
    with torch.no_grad():
        g = dy.double() * dact
        ag = g.abs()
        env['dbeta'] = ag.sum(0)
        env['dgamma'] = (ag * exh).sum(0)
        gr = (gamma.detach() * rstd.detach()).abs()
        if training:
            env['dx'] = gr * (ag + ag.mean(0) + exh * (g * xhat.detach()).mean(0).abs() + xhat.detach().abs() * (ag * exh).mean(0)) + xg.grad.abs() * half
            unb = R / max(R - 1, 1)
            out['running_mean'] = (1 - mom) * p['rm'].double() + mom * mean.detach()
            out['running_var'] = (1 - mom) * p['rv'].double() + mom * varc * unb
            env['running_mean'] = (1 - mom) * p['rm'].double().abs() + mom * ax.mean(0)
            env['running_var'] = (1 - mom) * p['rv'].double().abs() + mom * varc * unb
            out['sums'] = torch.cat([xd.sum(0), (xd * xd).sum(0)])
        else:
            env['dx'] = gr * ag
    out['env'] = env
    return out


def seq_mean(x):
    """Column means of x [R,C] in x's dtype, the rows in tiles of 32 added one after the other."""
    return rows_tn(torch.ones(x.shape[0], 1, dtype=x.dtype), x)[0] / x.shape[0]


def bn_yardstick(x, p, ref, training, act, one_pass=False, walkers=None):
    """Plain float32 on the CPU: two-pass statistics, y = act(x scale + shift) + resid, the backward by its formulas with the reference's mask.
    one_pass (the emulated defect): the variance as sum x^2 / R - mean^2 from float32 partial sums, one per row walker (`walkers` of them,
    each taking every walkers-th row in turn), folded in fp64 -- the arithmetic the statistics kernels had."""
    x = x.float()
    R = x.shape[0]
    gamma, beta = p['gamma'].float(), p['beta'].float()
    mom, eps = p['momentum'], p['eps']
    out = {}
    if training:
        if one_pass:
            s = torch.zeros(walkers, x.shape[1])
            q = torch.zeros(walkers, x.shape[1])
            for r0 in range(0, R, walkers):
                blk = x[r0:r0 + walkers]
                s[:blk.shape[0]] += blk
                q[:blk.shape[0]] += blk * blk
            m64 = s.double().sum(0) / R
            v64 = (q.double().sum(0) / R - m64 * m64).clamp_min(0)
            mean, var = m64.float(), v64.float()
            rstd = (1.0 / torch.sqrt(v64 + eps)).float()
        else:
            mean = seq_mean(x)
            var = seq_mean((x - mean) ** 2)
            rstd = 1.0 / torch.sqrt(var + eps)
        out['running_mean'] = (1 - mom) * p['rm'].float() + mom * mean
        out['running_var'] = (1 - mom) * p['rv'].float() + mom * (var * (R / max(R - 1, 1)))
    else:
        mean, var = p['rm'].float(), p['rv'].float()
        rstd = torch.rsqrt(var + eps)
    sc = gamma * rstd
    sh = beta - mean * sc
    pre = x * sc + sh
    y = pre if act == 0 else torch.where(ref['mask'], pre, pre * SLOPE[act])
    out['y'] = y + p['resid'].float() if p['resid'] is not None else y
    g = ref['dy'].float() * (1.0 if act == 0 else torch.where(ref['mask'], torch.tensor(1.0), torch.tensor(SLOPE[act])))
    xhat = (x - mean) * rstd
    out['dbeta'] = seq_mean(g) * R
    out['dgamma'] = seq_mean(g * xhat) * R
    out['dx'] = sc * (g - out['dbeta'] / R - xhat * (out['dgamma'] / R)) if training else sc * g
    return out


def bn_gate_params(R, C, seed=0):
    """Per-column std (a power of two in [1/4, 4]) and mean / std from BN_RATIOS by turns, and the parameters of the call."""
    gen = _gen('bn', R, C, seed)
    std = torch.ldexp(torch.ones(C), torch.randint(-2, 3, (C,), generator=gen))
    ratio_c = torch.tensor(BN_RATIOS)[torch.arange(C) % len(BN_RATIOS)]
    p = dict(gamma=_randn(gen, C), beta=_randn(gen, C), rm=_randn(gen, C) * 0.1 + std * ratio_c, rv=(1 + torch.rand(C, generator=gen)) * std * std,
             resid=_randn(gen, R, C), dy=_randn(gen, R, C), momentum=0.1, eps=1e-5)
    return gen, std, ratio_c, p


@functools.lru_cache(maxsize=32)
def bn_gate_input(path, R, C, seed=0):
    """path 'stats': x = std (randn + mean/std) for sga_bn_stats.  path 'gemm': (a [R,32], w [C,32]) whose product is such an x -- the last
    column of a is 1 and that of w the column's offset -- for sga_gemm_bnstats.  Returns (x or (a, w), p)."""
    gen, std, ratio_c, p = bn_gate_params(R, C, seed)
    if path == 'stats':
        return (_randn(gen, R, C) + ratio_c) * std, p
    a = torch.cat([_randn(gen, R, BN_K - 1), torch.ones(R, 1)], 1)
    w = torch.cat([_randn(gen, C, BN_K - 1) * (std / math.sqrt(BN_K - 1))[:, None], (std * ratio_c)[:, None]], 1)
    return (a, w), p


def bn_cases():
    """(family, path, R, C, training, act, with resid) of the gate."""
    cases = []
    for R_ in BN_R_GATE:
        for C in BN_C_GATE:
            act = (1, 2, 0)[(R_ + C) % 3]
            cases.append(('bn_train', 'stats', R_, C, True, act, act == 1))
            cases.append(('bn_train_gemm', 'gemm', R_, C, True, act, act == 1))
            cases.append(('bn_eval', 'stats', R_, C, False, act, act == 1))
    return cases


def _hold(t, strided):
    """A device copy of t [R,C]: contiguous, or a column slice (4 columns in) of a NaN-filled parent 12 columns wider and one row longer."""
    if not strided:
        return t.to('cuda').float().contiguous()
    parent = torch.full((t.shape[0] + 1, t.shape[1] + 12), float('nan'), device='cuda')
    view = parent[:t.shape[0], 4:4 + t.shape[1]]
    view.copy_(t)
    return view


def _outside_nan(view):
    par = view._base
    mask = torch.ones_like(par, dtype=torch.bool)
    mask[:view.shape[0], 4:4 + view.shape[1]] = False
    return bool(torch.isnan(par[mask]).all())


def run_gemm_bnstats(a, w, strided=True):
    """sga_gemm_bnstats: x = a w^T (device, a slice when strided) and the fp64 sums of its epilogue."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    a, w = (t.to('cuda').float().contiguous() for t in (a, w))
    R_, C = a.shape[0], w.shape[0]
    x = _hold(torch.zeros(R_, C), strided)
    sums = torch.full((2 * C + 4,), float('nan'), device='cuda', dtype=torch.float64)
    rc = _lib.lib().sga_gemm_bnstats(R_, C, a.shape[1], _p(a), a.stride(0), _p(w), w.stride(0), _p(x), x.stride(0), None, _p(sums), _stream())
    _lib.check(rc, 'sga_gemm_bnstats')
    torch.cuda.synchronize()
    assert torch.isnan(sums[2 * C:]).all() and (not strided or _outside_nan(x)), 'sga_gemm_bnstats wrote outside its outputs'
    return x, sums[:2 * C]


def run_bn_stats(x):
    """sga_bn_stats of a device tensor (any row stride): the fp64 sums."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    R_, C = x.shape
    sums = torch.full((2 * C + 4,), float('nan'), device='cuda', dtype=torch.float64)
    _lib.check(_lib.lib().sga_bn_stats(_p(x), x.stride(0), R_, C, _p(sums), _stream()), 'sga_bn_stats')
    torch.cuda.synchronize()
    assert torch.isnan(sums[2 * C:]).all()
    return sums[:2 * C]


def run_bn(x, p, training, act, with_resid, sums=None, strided=True):
    """BatchNormActFn on the card, forward and (when p has a cotangent dy) backward.  x: a CPU tensor (copied; strided: x, resid and out are
    column slices of wider NaN-filled buffers) or a device tensor taken as it is.  sums: the statistics of a producing sga_gemm_bnstats call
    (the `_sga_bn_sums` path); None: sga_bn_stats.  Returns the dict of outputs."""
    from sgaligner_amd import pct_ops
    dev = 'cuda'
    x = (x if x.is_cuda else _hold(x, strided)).detach()
    R_, C = x.shape
    x.requires_grad_()
    gamma, beta = p['gamma'].to(dev).float().requires_grad_(), p['beta'].to(dev).float().requires_grad_()
    rm, rv = p['rm'].to(dev).float().clone(), p['rv'].to(dev).float().clone()
    nbt = torch.tensor(3, device=dev, dtype=torch.int64)
    resid = _hold(p['resid'], strided) if with_resid else None
    out = _hold(torch.zeros(R_, C), True) if strided else None
    y = pct_ops.BatchNormActFn.apply(x, gamma, beta, rm, rv, nbt, training, p['momentum'], p['eps'], act, resid, out, sums if training else None)
    res = dict(y=y.detach().clone())
    if p.get('dy') is not None:
        y.backward(p['dy'].to(dev).float())
        res.update(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    torch.cuda.synchronize()
    if out is not None:
        assert _outside_nan(out), 'BatchNorm wrote outside its output slice'
    res.update(running_mean=rm, running_var=rv, num_batches_tracked=int(nbt.item()))
    return res


def measure_bn(path, R_, C, training, act, with_resid):
    """(output -> (kernel errors, yardstick errors), guarded share).  On the epilogue path x is what sga_gemm_bnstats wrote: the reference
    starts from the BatchNorm's own input on either path."""
    inp, p = bn_gate_input(path, R_, C)
    sums = None
    if path == 'gemm':
        x, sums = run_gemm_bnstats(*inp)
    else:
        x = _hold(inp, True)
    xc = x.cpu()
    pp = dict(p, resid=p['resid'] if with_resid else None)
    ref = bn_reference(xc, pp, training, act)
    assert ref['guarded'] <= GUARD_MAX
    pk = dict(pp, dy=ref['dy'])
    got = run_bn(x, pk, training, act, with_resid, sums)
    yard = bn_yardstick(xc, pk, ref, training, act)
    names = BN_OUT_TRAIN if training else BN_OUT_EVAL
    return {k: (errors(got[k], ref[k], ref['env'][k]), errors(yard[k], ref[k], ref['env'][k])) for k in names}, ref['guarded']


@functools.lru_cache(maxsize=64)
def bn_lattice(R_, C, seed=0):
    """The exact lattice (module text).  Returns (x, p, exact_ok, (a, w)): x [R,C] integers; exact_ok False when R is no power of two (then only
    the sums are claimed); (a, w) with K = 4 whose product is x exactly, for the epilogue path."""
    gen = _gen('bnlat', R_, C, seed)
    j = torch.randint(0, 4, (C,), generator=gen)
    mean = _ri(gen, -8, 8, C)
    exact_ok = R_ >= 2 and R_ & (R_ - 1) == 0
    if exact_ok:
        s = torch.cat([torch.ones(R_ // 2), -torch.ones(R_ // 2)])[torch.randperm(R_, generator=gen)]
    else:
        s = _ri(gen, -3, 3, R_)
    a = torch.stack([s, torch.ones(R_), torch.zeros(R_), torch.zeros(R_)], 1)
    w = torch.stack([torch.ldexp(torch.ones(C), j), mean, torch.zeros(C), torch.zeros(C)], 1)
    x = a @ w.t()
    gamma = torch.ldexp(torch.ones(C), torch.randint(-2, 3, (C,), generator=gen)) * (_ri(gen, 0, 1, C) * 2 - 1)
    p = dict(gamma=gamma, beta=_ri(gen, -4, 4, C), rm=_ri(gen, -6, 6, C), rv=torch.ones(C), resid=_ri(gen, -4, 4, R_, C), dy=None, momentum=0.5, eps=0.0)
    if exact_ok:
        xd = x.double()
        assert torch.equal(xd.mean(0), mean.double()) and torch.equal(((xd - xd.mean(0)) ** 2).mean(0), torch.ldexp(torch.ones(C), 2 * j).double())
    assert (x.double() ** 2).sum(0).max().item() < 2.0 ** 53 and x.abs().max() * R_ < LIMIT
    return x, p, exact_ok, (a, w)


def bn_lattice_reference(x, p, act, with_resid):
    """(y as float32 values, running_mean, sums) exactly: every step of the chain is exact on the lattice, except LeakyReLU's 0.2f v, which is
    one correctly rounded float32 product in kernel and reference alike."""
    xd = x.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    pre = (xd - mean) / torch.sqrt(var) * p['gamma'].double() + p['beta'].double()
    y = act64(pre, act).float()
    if with_resid:
        y = (y.double() + p['resid'].double()).float()
    return y, (0.5 * p['rm'].double() + 0.5 * mean).float(), torch.cat([xd.sum(0), (xd * xd).sum(0)])


# ================================================================================================ the widest stage (fused head / chain)
HEAD_SHAPES = ((3, 5, 8, 65), (4, 96, 64, 200), (2, 1, 4, 1))       # (T, N, K, C)
HEAD_OUT = ('g', 'dcat', 'dw', 'dgamma', 'dbeta')
HEAD_SLOPE = SLOPE[2]


def _row_ids(cat3):
    """[T,N]: for every row the index of the first row of its object with the same content."""
    T, N, _ = cat3.shape
    eq = (cat3[:, :, None, :] == cat3[:, None, :, :]).all(-1)           # [T, i, j]
    return eq.float().argmax(-1)


def head_reference(cat, w, p, T, N, training, guard=True):
    """fp64, literally: conv (cat W^T), BatchNorm, LeakyReLU(0.2), max over the points with the first maximiser; gradients by autograd through
    the arg-max rows.  p = dict(gamma, beta, rm, rv, dg, momentum, eps).  Returns outputs, env, dg (guarded), guarded, am and the rest."""
    R_, K = cat.shape
    C = w.shape[0]
    c64 = cat.double().clone().requires_grad_()
    w64 = w.double().clone().requires_grad_()
    gamma, beta = p['gamma'].double().clone().requires_grad_(), p['beta'].double().clone().requires_grad_()
    eps = p['eps']
    y = c64 @ w64.t()
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
    else:
        mean, var = p['rm'].double(), p['rv'].double()
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (y - mean) * rstd
    pre = xhat * gamma + beta
    z = torch.where(pre > 0, pre, pre * HEAD_SLOPE)
    with torch.no_grad():
        g0, am = first_argmax(z.detach().view(T, N, C))
    g = torch.gather(z.view(T, N, C), 1, am[:, None, :])[:, 0, :]
    with torch.no_grad():
        ey = cat.double().abs() @ w.double().abs().t()
        yd, md, vd, rd, xh = y.detach(), (mean.detach() if training else mean), (var.detach() if training else var), rstd.detach(), xhat.detach()
        if training:
            emean = ey.mean(0)
            evar = 2.0 * ((yd - md).abs() * (ey + emean)).mean(0)
            half = evar / (2.0 * (vd + eps))
        else:
            emean, half = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        exh = (ey + emean) * rd + xh.abs() * half
        epre = exh * gamma.detach().abs() + beta.detach().abs()
        dact = torch.where(pre.detach() > 0, torch.ones_like(epre), torch.full_like(epre, HEAD_SLOPE))
        ez = (epre * dact).view(T, N, C)
        pick = lambda t3: torch.gather(t3, 1, am[:, None, :])[:, 0, :]
        # guard: LeakyReLU's edge at the arg-max row, and a runner-up (among rows with other inputs) within DELTA of the two envelopes
        near = pick(pre.detach().view(T, N, C)).abs() <= DELTA * pick(epre.view(T, N, C))
        ids = _row_ids(cat.view(T, N, K))
        same = ids[:, :, None] == torch.gather(ids, 1, am.reshape(T, C)).view(T, 1, C)          # [T,N,C]: rows equal to the winner's
        zd = z.detach().view(T, N, C)
        other = torch.where(same, torch.full_like(zd, -math.inf), zd)
        ru, ru_i = other.max(1)
        gap_env = pick(ez) + torch.gather(ez, 1, ru_i[:, None, :])[:, 0, :]
        near = near | (torch.isfinite(ru) & (g0 - ru <= DELTA * gap_env))
        if not guard:
            near = torch.zeros_like(near)
        dg = torch.where(near, torch.zeros_like(p['dg']), p['dg'])
    (g * dg.double()).sum().backward()
    out = dict(g=g.detach(), dcat=c64.grad, dw=w64.grad, dgamma=gamma.grad, dbeta=beta.grad, dg=dg, am=am.int(), guarded=near.float().mean().item())
    with torch.no_grad():
        dz = dg.double() * pick(dact.view(T, N, C))
        adz = dz.abs()
        exh_w = pick(exh.view(T, N, C))
        env = dict(g=pick(ez), dbeta=adz.sum(0), dgamma=(adz * exh_w).sum(0))
        D = torch.zeros(T, N, C, dtype=torch.float64).scatter_(1, am[:, None, :], adz[:, None, :]).view(R_, C)
        gr = (gamma.detach() * rd).abs()
        if training:
            S2 = (dz * pick(xh.view(T, N, C))).sum(0)
            # dy of this stage, recovered from autograd's dcat is not needed: |dy| <= gr (|D| + ...) bounds the rstd term
            dyb = gr * (D + env['dbeta'] / R_ + xh.abs() * S2.abs() / R_)
            edy = gr * (D + env['dbeta'] / R_ + exh * S2.abs() / R_ + xh.abs() * env['dgamma'] / R_) + dyb * half
            out['running_mean'] = (1 - p['momentum']) * p['rm'].double() + p['momentum'] * md
        else:
            edy = gr * D
        env['dw'] = edy.t() @ cat.double().abs()
        env['dcat'] = edy @ w.double().abs()
    out['env'] = env
    out.update(mask=pre.detach() > 0, mean=md, var=vd)
    return out


def head_yardstick(cat, w, p, ref, T, N, training):
    """Plain float32 on the CPU with the reference's arg-max rows and LeakyReLU mask: two-pass statistics, the dense BatchNorm backward, the
    reductions over rows in 32-row tiles."""
    cat, w = cat.float(), w.float()
    R_, K = cat.shape
    C = w.shape[0]
    gamma, beta = p['gamma'].float(), p['beta'].float()
    y = G.yardstick(cat, w)
    if training:
        mean = seq_mean(y)
        var = seq_mean((y - mean) ** 2)
        rstd = 1.0 / torch.sqrt(var + p['eps'])
    else:
        mean, var = p['rm'].float(), p['rv'].float()
        rstd = torch.rsqrt(var + p['eps'])
    sc = gamma * rstd
    pre = y * sc + (beta - mean * sc)
    slope = torch.where(ref['mask'], torch.tensor(1.0), torch.tensor(HEAD_SLOPE))
    z = (pre * slope).view(T, N, C)
    am = ref['am'].long()
    pick = lambda t3: torch.gather(t3, 1, am[:, None, :])[:, 0, :]
    out = dict(g=pick(z))
    dz = ref['dg'].float() * pick(slope.view(T, N, C))
    xhat = (y - mean) * rstd
    out['dbeta'] = dz.sum(0)
    out['dgamma'] = (dz * pick(xhat.view(T, N, C))).sum(0)
    D = torch.zeros(T, N, C).scatter_(1, am[:, None, :], dz[:, None, :]).view(R_, C)
    dy = sc * (D - out['dbeta'] / R_ - xhat * (out['dgamma'] / R_)) if training else sc * D
    out['dw'] = rows_tn(dy, cat)
    out['dcat'] = G.yardstick(dy, w.t().contiguous())
    return out


@functools.lru_cache(maxsize=16)
def head_gate_input(T, N, K, C, seed=0):
    """(cat, w, p): random inputs, gamma of both signs bounded away from 0 (the fused node recovers x_hat as (z - beta) / gamma); object 1 (if
    there is one) has all its points equal -- every channel's arg-max in row 0."""
    gen = _gen('head', T, N, K, C, seed)
    cat = _randn(gen, T, N, K)
    if T > 1:
        cat[1] = cat[1, :1]
    w = _randn(gen, C, K) / math.sqrt(K)
    gamma = (0.5 + torch.rand(C, generator=gen)) * (_ri(gen, 0, 1, C) * 2 - 1)
    p = dict(gamma=gamma, beta=_randn(gen, C) * 0.5, rm=_randn(gen, C) * 0.1, rv=0.5 + torch.rand(C, generator=gen), dg=_randn(gen, T, C),
             momentum=0.1, eps=1e-5)
    return cat.reshape(T * N, K), w, p


def run_head(cat, w, p, T, N, training, fused):
    """pct_ops.linear_bn_lrelu_max (fused) or rows_linear(bn_stats=True) -> batch_norm_act(act=2) -> segment_max (the chain), forward and
    backward on the card.  Returns dict g, dcat, dw, dgamma, dbeta."""
    from sgaligner_amd import pct_ops as P
    C, K = w.shape
    bn = torch.nn.BatchNorm1d(C, eps=p['eps'], momentum=p['momentum']).cuda()
    with torch.no_grad():
        bn.weight.copy_(p['gamma'])
        bn.bias.copy_(p['beta'])
        bn.running_mean.copy_(p['rm'])
        bn.running_var.copy_(p['rv'])
    bn.train(training)
    cd = cat.float().cuda().requires_grad_()
    wd = w.float().cuda().reshape(C, K, 1).requires_grad_()
    if fused:
        g = P.linear_bn_lrelu_max(cd, wd, bn, T, N)
    else:
        g = P.segment_max(P.batch_norm_act(P.rows_linear(cd, wd, bn_stats=True), bn, act=2), T, N)
    g.backward(p['dg'].float().cuda())
    torch.cuda.synchronize()
    return dict(g=g.detach(), dcat=cd.grad, dw=wd.grad.reshape(C, K), dgamma=bn.weight.grad, dbeta=bn.bias.grad)


def head_cases():
    """(family, T, N, K, C, training, fused) of the gate; the last is the fused node at both caps of sga_pct_head_scatter."""
    cases = [(f'head_{"train" if tr else "eval"}', T, N, K, C, tr, fused) for (T, N, K, C) in HEAD_SHAPES for tr in (True, False) for fused in (True, False)]
    return cases + [('head_train', 1, 1024, 8, 1024, True, True)]


def measure_head(T, N, K, C, training, fused):
    cat, w, p = head_gate_input(T, N, K, C)
    ref = head_reference(cat, w, p, T, N, training)
    assert ref['guarded'] <= GUARD_MAX
    got = run_head(cat, w, dict(p, dg=ref['dg']), T, N, training, fused)
    yard = head_yardstick(cat, w, p, ref, T, N, training)
    return {k: (errors(got[k], ref[k], ref['env'][k]), errors(yard[k], ref[k], ref['env'][k])) for k in HEAD_OUT}, ref['guarded']


# ================================================================================================ the gate
def check(results, family, what):
    """Print every figure, then assert gemm_gate.gate_ok per output at R[family][output]."""
    bad = []
    for k, (ke, ye) in results.items():
        r = R[family][k]
        print(f'[gate] {what} {k}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
        if not G.gate_ok(ke, ye, r):
            bad.append((k, ke[:2], ye[:2], r))
    assert not bad, f'{what}: (output, kernel (max, rms), yardstick (max, rms), r) beyond the gate: {bad}'
