"""The exact (census) and fp32-faithful (gate) checks of the contrastive / alignment loss kernels, and the plumbing they share (no tests in
this module).  csrc/contrastive.hip, loss_anchor.hip, loss_pertable.hip, sweep3.hip, losshead.hip, loss_math.h behind include/sgaligner_hip.h.

Reference.  Every stage of the C ABI restated in fp64 torch on the CPU from oracle/sga_oracle.py:239-301 (reference src/aligner/losses.py), and
handed THE INPUTS THE KERNEL GETS (fp32 tables, the fp64 sums, the fp32 stash ...), so that a stage's error is its own:
    gather        E, idx -> Z = e / max(|e|, 1e-12), nrm
    neg_sums      Z -> sums8[fam * 2 + temp], fam = s11 (X1 N1), s12 (X1 N2), s22 (X2 N2), s21 (X2 N1), temp = (0.1, 1.0); the fused form adds
                  the joint row from S_J = sum_m beta_m S_m; an anchor shard [a_lo, a_hi) keeps those anchors' rows
    anchor_terms  Z, sums, alpha -> out = [NT icl | M ial_a | M ial_b]
                  qA[i,j] = g(exp(S[i,j] / t); s11, s12), qB[i,j] = g(exp(S[j,i] / t); s22, s21) -- qB indexed [i,j] UN-transposed, losses.py:54-56
    anchor_coef   ... and coef = dL/d(out) -> dL/dS_k[i,j] for every (i,j) (fused: M1[m] = dL/dS_m + beta_m dL/dS_J), gs = dL/d(sums8),
                  gamma = dL/dbeta through the A x A terms: fp64 autograd with the similarity blocks S and S^T as leaves
    stash_grad    M1 (M2), Z -> dZ on the anchor rows: GEMMs, by gemm_gate.reference / envelope
    neg_grad      Z, gs -> dZ on all rows and gamma through the negatives
    scatter       dZ, Z, nrm, idx -> dE = J_normalize^T dZ, duplicates summed; the two-part forms project the exact sum G + rho zbar
    head          the 3M+1 terms, both log_vars -> [loss, icl_uni, icl_multi, ial] and their gradients (losses.py:28-34,114-152)
Chained, they reproduce oracle.sga_oracle.overall_loss(...)['loss'].backward() in fp64 to 1e-12 (tests/test_loss_gate_cpu.py).

Metric.  gemm_gate.rel_errors: |out - ref| / envelope in u = 2^-24.  The envelope is a running-error bound from the fp64 reference alone:
    e_S = |Z||Z|^T      e_exp = exp(S/t) (1 + e_S / t)      e_sum = sum e_exp      (relative: eps_s = e_sum / sum)
    an element-wise output f of the A x A epilogue:  |f| + sum_x |df/dx| e_x  over x = S_m[i,j], S_m[j,i] (e_S) and the log of every sum
    (eps_s), the derivatives by a second fp64 autograd pass (every leaf is element-wise, the sums enter through a per-element log-scale);
    products c Z:  env(c) |Z|;   dE:  (env_g + |z| (env_g . |z|)) / n, scattered.
Scalars (sums, terms, gs, gamma, head outputs) are judged by their max alone and the YARDSTICK's error is floored at FLOOR_U = 1 u before
r is applied: a scalar is one draw, its float32 yardstick may land on the nearest float by luck (tests/eva_gate.py).

Yardstick.  The same stage in plain float32 torch on the CPU, never the library: products walk K (or the rows they contract) in chunks of
32 in a stated order (gemm_gate.yardstick), element-wise epilogues and their float32 autograd are order free, and the scalar sums add the
float32 terms in fp64 as the kernels' accumulators do.

Gate.  gemm_gate.gate_ok (FLOOR_U and its rms floor unchanged) at r per (stage output, tier) = ceil(2 x the worst kernel / yardstick ratio,
rms or max, measured on the MI355X over the gate cases): profiles/loss_accuracy_vs_fp32.json, written by tools/loss_accuracy.py;
test_loss_gate_cpu.py keeps R and the profile together and asserts that the seeded defects FAIL at the r in use.

Tier 'f16' (mode 'f16', tables wider than 128 columns: csrc/wide16.hip, the Zh forms of csrc/loss_pertable.hip's A x A kernels).  The stages
read fp16 copies of the unit rows: sga_wide16_prepare is pinned bit for bit (prepare_ref), the references are the fp64 stages on zh.double(),
and the yardstick restates the kernels' arithmetic in float32 torch -- fp32-chunked products of zh.float(), coefficients divided by their
family's bound and rounded to fp16, the stash scaled by a power of two and rounded to fp16 (the section at the end of this module).

Census.  Rows 2^s e_k: anchors take their class k from the low half of the columns, negatives from the high half, in every table.  Every
anchor x negative similarity -- fp32 MFMA, three bf16 planes, lite, fp16, and the derived joint -- is exactly 0, every term of the 8 NT global
sums is exp2(0) = 1 and every sum is the integer (anchors of the shard) x J: torch.equal is legitimate.  With at most CENSUS_COUNT = 8 rows per
class in a segment, every entry of the negatives' gradient is c_f1 n_1 + c_f2 n_2 with integer counts n <= 8 and ONE constant c_f per family
(c_f = gs[f,0]/t0 + gs[f,1]/t1, plus beta_m times the joint's): a lost or doubled pair moves an entry by >= 1/16 of its envelope.  A correct
kernel owes the rounding of c_f (formed from two products and, fused, one fma: <= 2 u), one of each product c_f n (n is exact; the MFMA's
fp32 accumulation of <= 8 equal terms rounds only when n c_f needs more bits: <= 1 u in all) and one of the final sum: CENSUS_U = 4 u."""
import functools
import json
import math
import os
import types
from unittest import mock

import torch

import gemm_gate as G

ROOT = G.ROOT
PROFILE = os.path.join(ROOT, 'profiles', 'loss_accuracy_vs_fp32.json')
TAU = (0.1, 1.0)                         # losses.py:39 (ICL), :63 (IAL)
ALPHA = 0.5
QEPS = 1e-9
NEPS = 1e-12                             # F.normalize's eps
DP = 104                                 # the fused path's row pitch
CENSUS_COUNT = 8
CENSUS_U = 4.0
SCALARS = ('sums', 'terms', 'gs', 'gamma', 'gamma_neg', 'head', 'dterms', 'dlv')          # (group.terms and group.gamma too: one scalar per group)

# r per 'stage.output|tier': ceil(2 x the worst measured kernel / yardstick ratio) over the gate cases of profiles/loss_accuracy_vs_fp32.json,
# at least 1 (the scalar head computes in fp64 and measures 0).
# Tiers: 'f32' (gather, scatter, the A x A kernels, the head: one arithmetic), and for the sweeps and stash products 'plain' (fp32 MFMA on the
# plain tables), 'centred' (fp32 MFMA on centred tables), 'planes' (three exact bf16 planes); 'f16' (mode 'f16', tables wider than 128 columns:
# fp16 inputs, fp32 accumulation -- csrc/wide16.hip and the Zh forms of the per-table A x A kernels, against a yardstick in the same arithmetic).
R = {
    'neg_grad.dZ|centred': 14, 'neg_grad.gamma_neg|centred': 2, 'neg_sums.sums|centred': 5, 'scatter.dE|centred': 3, 'stash_grad.dZ|centred': 9,
    'anchor_coef.dS|f32': 35, 'anchor_coef.gamma|f32': 1, 'anchor_coef.gs|f32': 3, 'anchor_terms.terms|f32': 6, 'gather.Z|f32': 3,
    'gather.nrm|f32': 3, 'head.dlv|f32': 2, 'head.dterms|f32': 2, 'head.head|f32': 1, 'scatter.dE|f32': 4, 'group.dE|mfma': 4, 'group.gamma|mfma': 1,
    'group.terms|mfma': 3, 'anchor_coef.dS|pertable': 7, 'anchor_coef.gs|pertable': 4, 'anchor_terms.terms|pertable': 4, 'neg_grad.dZ|pertable': 60,
    'neg_sums.sums|pertable': 8, 'neg_grad.dZ|plain': 19, 'neg_grad.gamma_neg|plain': 2, 'neg_sums.sums|plain': 5, 'stash_grad.dZ|plain': 31,
    'neg_grad.dZ|planes': 6, 'neg_grad.gamma_neg|planes': 1, 'neg_sums.sums|planes': 4, 'scatter.dE|planes': 3, 'stash_grad.dZ|planes': 3,
    'group.dE|valu': 4, 'group.gamma|valu': 1, 'group.terms|valu': 3, 'neg_grad.dZ|wide': 5,
    'anchor_coef.dS|f16': 10, 'anchor_coef.gs|f16': 2, 'anchor_terms.terms|f16': 4, 'neg_grad.dZ|f16': 3, 'neg_sums.sums|f16': 2, 'stash_grad.dZ|f16': 3,
}


# A condition on R, not a measurement: at the r in use the gate must fail a three-plane product that forgets one of its six partial products
# (test_loss_gate_cpu.py emulates it for every gate case).  Where it cannot -- the coefficients' own float32 error, exp(S / 0.1) amplifying the
# rounding of S, already sits within r of what the forgotten product adds -- the output is left ungated at that case and listed here;
# the census and the other cases still cover the kernel.  'output|tier' -> names of the gate cases left out.
# The tier 'f16' the same way: the three emulated wide16 defects of test_loss_gate_cpu.py (a lost K group in the sums; a lost anchor row and an
# un-zeroed straddling K group in the negatives' gradient) must fail at every gate case, or the case is listed.
UNGATED = {
    'neg_grad.dZ|planes': ('cluster-A1-1-1-D37-M4', 'cluster-A31-33-1-D37-M3', 'parallel-A31-33-1-D8-M4', 'parallel-A32-32-32-D8-M3',
                           'cluster-A33-31-65-D97-M4', 'cluster-A63-64-129-D97-M3', 'parallel-A63-64-129-D96-M4',
                           'cluster-A129-21-75-D37-M4', 'cluster-A33-31-65-D8-M2', 'cluster-A257-40-9-D100-M3',
                           'onehot-A65-127-63-D64-M3',),
    'stash_grad.dZ|planes': (),
    'neg_sums.sums|f16': (),
    'neg_grad.dZ|f16': ('f16-cluster-A2305-17-0-D136',),      # (one un-zeroed pad column among 2305 anchors; the census runs this shape too)
}


def ratios_from_profile(path=PROFILE):
    """'output|tier' -> ceil(2 x worst measured kernel / yardstick ratio), at least 1: the derivation R states."""
    worst = {}
    for c in json.load(open(path))['cases']:
        k = f"{c['output']}|{c['tier']}"
        worst[k] = max(worst.get(k, 0.0), c['ratio_rms'], c['ratio_max'])
    return {k: max(1, int(math.ceil(2.0 * v - 1e-9))) for k, v in worst.items()}      # (no kernel is asked to beat the yardstick: r >= 1)


def is_scalar(output):
    return output.split('.')[-1] in SCALARS


def gate_ok(kernel, yard, r, scalar):
    if scalar:
        return kernel[0] <= r * max(yard[0], G.FLOOR_U)
    return G.gate_ok(kernel, yard, r)


def ratio(kernel, yard, scalar):
    """(max ratio, rms ratio) kernel / yardstick as the profile records them, measured against the floors the gate uses: a scalar's
    yardstick error is floored at FLOOR_U, as its gate is; for the others a figure that gate_ok's floor admits whatever r is -- a max up to
    FLOOR_U, an rms up to FLOOR_U / sqrt(n) -- asks for no r and is recorded as 0 (a one-entry output whose yardstick drew 0.02 u by luck
    would otherwise set r for every shape)."""
    if scalar:
        v = kernel[0] / max(yard[0], G.FLOOR_U)
        return v, v
    n = max(kernel[2], 1)
    rmax = kernel[0] / max(yard[0], 1e-30) if kernel[0] > G.FLOOR_U else 0.0
    rrms = kernel[1] / max(yard[1], 1e-30) if kernel[1] > G.FLOOR_U / n ** 0.5 else 0.0
    return rmax, rrms


# ------------------------------------------------------------------------------------------------ arithmetic helpers
def mm(a, bt):
    """a bt^T: fp64 as one product, float32 in gemm_gate.yardstick's stated order (K in chunks of 32)."""
    if a.dtype == torch.float64:
        return a @ bt.t()
    return G.yardstick(a, bt)


def sum64(x):
    return x.double().sum()


def g_fn(d, sa, sb):
    """losses.py:5-15 per element."""
    a = d / (sa + QEPS)
    b = d / (sb + QEPS)
    return 1.0 / (1.0 + 1.0 / (a + QEPS) + 1.0 / (b + QEPS) + QEPS)


def segments(Z, A, J1, J2):
    return Z[:A], Z[A:2 * A], Z[2 * A:2 * A + J1], Z[2 * A + J1:2 * A + J1 + J2]


def sides(Z, A, J1, J2, D, centred=False):
    """(L, Rt, V): S = L Rt^T and the gradient's operand rows V.  A plain table: all three are Z[:, :D].  A centred table (z - zbar | b | 1):
    S_ij = z'_i . z'_j + b_i + b_j (the owner reads columns 100 / 101 swapped) and V = (z' | 1), the two parts of the gradient."""
    R = 2 * A + J1 + J2
    if not centred:
        z = Z[:R, :D]
        return z, z, z
    zc, b, one = Z[:R, :100], Z[:R, 100:101], Z[:R, 101:102]
    return torch.cat([zc, b, one], 1), torch.cat([zc, one, b], 1), torch.cat([Z[:R, :D], one], 1)


def neg_blocks(L, Rt, A, J1, J2):
    """[S11, S12, S22, S21]: the four anchors x negatives blocks of one table."""
    x1, x2, _, _ = segments(L, A, J1, J2)
    _, _, n1, n2 = segments(Rt, A, J1, J2)
    return [mm(x1, n1), mm(x1, n2), mm(x2, n2), mm(x2, n1)]


def with_joint(blocks, beta):
    """per-table lists of blocks + the joint's, S_J = sum_m beta_m S_m."""
    if beta is None:
        return blocks
    joint = [sum(beta[m].to(b[f].dtype) * b[f] for m, b in enumerate(blocks)) for f in range(len(blocks[0]))]
    return blocks + [joint]


# ------------------------------------------------------------------------------------------------ gather / scatter
def gather(E, idx, dt=torch.float64):
    e = E.to(dt)[idx.long()]
    if dt == torch.float64:
        n = e.pow(2).sum(1).sqrt()
    else:                                                  # squares added 32 columns at a time, in order
        sq = e * e
        pad = (-sq.shape[1]) % 32
        sq = torch.cat([sq, sq.new_zeros(sq.shape[0], pad)], 1).reshape(sq.shape[0], -1, 32)
        n = torch.zeros(sq.shape[0], dtype=dt)
        for c in range(sq.shape[1]):
            n = n + sq[:, c].sum(1)
        n = n.sqrt()
    return e / n.clamp_min(NEPS)[:, None], n


def scatter(G_, rho, Z, nrm, idx, T, zbar=None, dt=torch.float64, project=True, env_in=None):
    """dE [T, D] from the gradient of the unit rows.  One part: g = G_.  Two parts (zbar given): the true gradient is G + rho zbar; fp64
    projects that exact sum, float32 evaluates G - rho (z - zbar), equal under the projection (P z = 0) and free of the cancellation.
    Returns (dE, envelope)."""
    z, n = Z.to(dt), nrm.to(dt).clamp_min(NEPS)
    g = G_.to(dt)
    env_g = G_.double().abs() if env_in is None else env_in
    if zbar is not None:
        zb, rh = zbar.to(dt)[None, :], rho.to(dt)[:, None]
        g = g + rh * zb if dt == torch.float64 else g - rh * (z - zb)
        env_g = env_g + rho.double().abs()[:, None] * (Z.double().abs() + zbar.double().abs()[None, :])
    if project:
        out = (g - z * (g * z).sum(1, keepdim=True)) / n[:, None]
    else:
        out = g / n[:, None]
    za = Z.double().abs()
    env = (env_g + za * (env_g * za).sum(1, keepdim=True)) / nrm.double().clamp_min(NEPS)[:, None]
    dE = torch.zeros(T, g.shape[1], dtype=dt).index_add_(0, idx.long(), out)
    eE = torch.zeros(T, g.shape[1], dtype=torch.float64).index_add_(0, idx.long(), env)
    return dE, eE


# ------------------------------------------------------------------------------------------------ the global sums
def neg_sums(blocks, lo, hi):
    """blocks [NT][4] -> sums [NT, 8] (fp64 accumulation of the blocks' dtype terms) over the anchors [lo, hi)."""
    out = torch.zeros(len(blocks), 8, dtype=torch.float64)
    for k, b in enumerate(blocks):
        for f in range(4):
            for t in range(2):
                out[k, 2 * f + t] = sum64(torch.exp(b[f][lo:hi] / TAU[t]))
    return out


def neg_sums_envelope(blocks, eblocks, lo, hi):
    out = torch.zeros(len(blocks), 8, dtype=torch.float64)
    for k, (b, e) in enumerate(zip(blocks, eblocks)):
        for f in range(4):
            for t in range(2):
                out[k, 2 * f + t] = (torch.exp(b[f][lo:hi] / TAU[t]) * (1.0 + e[f][lo:hi] / TAU[t])).sum()
    return out


# ------------------------------------------------------------------------------------------------ anchors x anchors
def term_mats(X, Y, se, alpha, qb_transposed=False):
    """X[k] = S_k, Y[k] = S_k^T [A, A] for the NT tables (the joint last), se[k][8] the sums (scalars or [A, A]).  Returns the NT + 2M
    element-wise term matrices [icl_k | ial_a_m | ial_b_m]."""
    nt = len(X)
    m = nt - 1 if nt > 1 else 0
    q = []
    for k in range(nt):
        yk = X[k] if qb_transposed else Y[k]               # the seeded defect: qB taken transposed
        q.append([g_fn(torch.exp(X[k] / TAU[t]), se[k][0 + t], se[k][2 + t]) for t in range(2)] +
                 [g_fn(torch.exp(yk / TAU[t]), se[k][4 + t], se[k][6 + t]) for t in range(2)])
    icl = [-torch.log(alpha * q[k][0] + (1.0 - alpha) * q[k][2]) for k in range(nt)]
    ia = [torch.exp(q[i][1]) * (q[i][1] - torch.log(q[nt - 1][1])) for i in range(m)]
    ib = [torch.exp(q[i][3]) * (q[i][3] - torch.log(q[nt - 1][3])) for i in range(m)]
    return icl + ia + ib


def anchor_stage(S, beta, sums, alpha, coef, eS=None, esum=None, dt=torch.float64, qb_transposed=False):
    """S: the M modality blocks X1 X2^T (fused: beta given, the joint derived) or the NT tables' blocks (beta None).  Returns a dict:
    terms_rows [n_terms, A] (term k summed over the columns, per anchor row: a shard's share is a slice), dS [len(S)][A, A] = dL/dS (fused:
    M1[m] as the kernel defines it), gs_rows [NT, 8, A], gamma_rows [M, A]; with eS / esum also the envelopes env_*."""
    n = len(S)
    A = S[0].shape[0]
    X = [s.to(dt).clone().requires_grad_(True) for s in S]
    Y = [s.to(dt).t().clone().requires_grad_(True) for s in S]
    tabs_x, tabs_y = list(X), list(Y)
    zj = []
    if beta is not None:
        b = beta.to(dt).clone().requires_grad_(True)
        zj = [torch.zeros(A, A, dtype=dt, requires_grad=True) for _ in range(2)]
        tabs_x.append(sum(b[m] * X[m] for m in range(n)) + zj[0])
        tabs_y.append(sum(b[m] * Y[m] for m in range(n)) + zj[1])
    nt = len(tabs_x)
    th = [[torch.zeros(A, A, dtype=dt, requires_grad=True) for _ in range(8)] for _ in range(nt)]
    sm = sums.to(dt)
    se = [[sm[k, s] * torch.exp(th[k][s]) for s in range(8)] for k in range(nt)]
    mats = term_mats(tabs_x, tabs_y, se, alpha, qb_transposed)
    cf = coef.to(dt)
    T = sum(cf[k] * mats[k].sum() for k in range(len(mats)))
    leaves = X + Y + zj + [t for row in th for t in row]
    want_env = eS is not None
    W = torch.autograd.grad(T, leaves, create_graph=want_env, allow_unused=True)
    W = [w if w is not None else torch.zeros(A, A, dtype=dt) for w in W]
    out = {'terms_rows': torch.stack([m_.detach().double().sum(1) for m_ in mats])}
    WX, WY = W[:n], W[n:2 * n]
    out['dS'] = [(WX[m] + WY[m].t()).detach() for m in range(n)]
    o = 2 * n + len(zj)
    out['gs_rows'] = torch.stack([torch.stack([W[o + 8 * k + s].detach().double().sum(1) / sums[k, s].double() for s in range(8)]) for k in range(nt)])
    if beta is not None:
        WJ = W[2 * n:2 * n + 2]
        out['gamma_rows'] = torch.stack([(WJ[0].detach() * X[m].detach() + WJ[1].detach() * Y[m].detach()).double().sum(1) for m in range(n)])
    if not want_env:
        return out
    # ---- envelopes (fp64 only): e of every leaf, then |w| + sum_l' |dw/dl'| e_l' by one more pass per first derivative
    eps_s = (esum / sums).double()
    el = [e.double() for e in eS] + [e.double().t() for e in eS]
    if beta is not None:
        ej = sum(beta[m].double().abs() * (S[m].double().abs()) for m in range(n))          # the joint's own fma chain: |beta||S| per term
        el += [ej, ej.t()]
    el += [eps_s[k, s].expand(A, A) for k in range(nt) for s in range(8)]

    def env_of(w):
        if not w.requires_grad:
            return w.detach().abs()
        H = torch.autograd.grad(w.sum(), leaves, retain_graph=True, allow_unused=True)
        return w.detach().abs() + sum(h.abs() * e for h, e in zip(H, el) if h is not None)

    envW = [env_of(w) for w in W]
    out['env_dS'] = [envW[m] + envW[n + m].t() for m in range(n)]
    out['env_gs_rows'] = torch.stack([torch.stack([envW[o + 8 * k + s].sum(1) / sums[k, s].double() for s in range(8)]) for k in range(nt)])
    if beta is not None:
        xs, ys = [x.detach().abs() for x in X], [y.detach().abs() for y in Y]
        out['env_gamma_rows'] = torch.stack([(envW[2 * n] * xs[m] + WJ[0].detach().abs() * el[m] +
                                              envW[2 * n + 1] * ys[m] + WJ[1].detach().abs() * el[n + m]).sum(1) for m in range(n)])
    env_t = []
    for m_ in mats:
        H = torch.autograd.grad(m_.sum(), leaves, retain_graph=True, allow_unused=True)
        env_t.append((m_.detach().abs() + sum(h.abs() * e for h, e in zip(H, el) if h is not None)).sum(1))
    out['env_terms_rows'] = torch.stack(env_t)
    return out


# ------------------------------------------------------------------------------------------------ negatives' gradient
def neg_coefs(blocks, gs, beta, lo, hi, eblocks=None, env_gs=None):
    """c[m][f] = dL/dS_m,f over the anchors [lo, hi) (rows outside are zero), the joint's folded in (fused), its own c_J, and env(c)."""
    dt = blocks[0][0].dtype
    nt = len(blocks)

    def one(k, f, e=None):
        b = blocks[k][f]
        c = torch.zeros_like(b) if e is None else torch.zeros(b.shape, dtype=torch.float64)
        for t in range(2):
            w = (gs[k, 2 * f + t] / TAU[t])
            x = torch.exp(b[lo:hi] / TAU[t])
            if e is not None and env_gs is not None:
                w = w.abs() + env_gs[k, 2 * f + t] / TAU[t]
            c[lo:hi] += (w.to(dt) * x) if e is None else (w.abs() * x.double() * (1.0 + e[k][f][lo:hi] / TAU[t]))
        return c
    c = [[one(k, f) for f in range(4)] for k in range(nt)]
    env = None if eblocks is None else [[one(k, f, eblocks) for f in range(4)] for k in range(nt)]
    if beta is None:
        return c, None, env, None
    m = nt - 1
    cj, ej = c[m], (None if env is None else env[m])
    cm = [[c[i][f] + beta[i].to(dt) * cj[f] for f in range(4)] for i in range(m)]
    em = None if env is None else [[env[i][f] + beta[i].double().abs() * ej[f] for f in range(4)] for i in range(m)]
    return cm, cj, em, ej


def neg_grad_rows(c, V, A, J1, J2, absolute=False):
    """dZ [R, Dv] = the four blocks' coefficients times the other side's rows, in c's dtype; absolute: env(c) |V|."""
    v = V.double().abs() if absolute else V
    x1, x2, n1, n2 = segments(v, A, J1, J2)
    c11, c12, c22, c21 = c
    return torch.cat([mm(c11, n1.t()) + mm(c12, n2.t()), mm(c22, n2.t()) + mm(c21, n1.t()),
                      mm(c11.t(), x1.t()) + mm(c21.t(), x2.t()), mm(c12.t(), x1.t()) + mm(c22.t(), x2.t())])


# ------------------------------------------------------------------------------------------------ the scalar head
def head(terms, lv_ial, lv_icl, A, z_ial, alpha, zoom, dt=torch.float64):
    """losses.py:114-152 with CustomMultiLossLayer :28-34 on the raw terms [icl (M+1) | ial_a (M) | ial_b (M)]; A == 0 -> NaN (the mean of
    an empty matrix).  Returns [loss, icl_uni, icl_multi, ial]."""
    m = lv_ial.numel()
    t, la, lc = terms.to(dt), lv_ial.to(dt), lv_icl.to(dt)
    inv = 1.0 / float(A * A) if A else float('nan')
    icl = t[:m + 1] * inv
    ial = z_ial * (alpha * t[m + 1:2 * m + 1] + (1.0 - alpha) * t[2 * m + 1:])
    align = ((torch.exp(-la) * ial) + la).sum() * zoom
    uni = ((torch.exp(-lc) * icl[:m]) + lc).sum()
    return torch.stack([align + uni + icl[m], uni, icl[m], align])


# ------------------------------------------------------------------------------------------------ the stages chained: the whole loss
def chain_terms(E, beta, idx, A, J1, J2, coef, dt=torch.float64, envelopes=False, f16=None):
    """gather -> sums -> A x A terms and coefficients -> stash products -> negatives' gradient -> scatter in `dt` for tables E (beta given:
    the fused form, the joint derived; None: the tables as they are, the last one in the joint's place) and coef = dL/d(terms).  Returns
    terms, dE per table, gamma = dL/dbeta (fused); envelopes (fp64): every stage's envelope carried into the next one's input error.
    f16 (the float32 yardstick of mode 'f16', per-table form): one flag per table -- a flagged table takes the arithmetic of the tier 'f16':
    similarities and gradient products from the fp16 rounding of its unit rows, coefficients as f16_coefs, the stash as f16_stash_operand;
    its scatter reads the float32 rows, as the kernel's does."""
    T = E[0].shape[0]
    n = len(E)
    E = [e.to(dt) for e in E]
    Z, nrm = zip(*[gather(e, idx, dt) for e in E])
    f16 = list(f16) if f16 is not None else [False] * n
    assert not any(f16) or (dt == torch.float32 and beta is None and not envelopes)
    rows = Z                                               # the float32 rows (scatter); Z: what the products read
    Z = [z.to(torch.float16).to(dt) if h else z for z, h in zip(Z, f16)]
    bt = None if beta is None else beta.to(dt)
    blocks = with_joint([neg_blocks(z, z, A, J1, J2) for z in Z], bt)
    sums = neg_sums(blocks, 0, A)
    S = [mm(z[:A], z[A:2 * A]) for z in Z]
    eS = esum = eb = None
    if envelopes:
        eb = with_joint([neg_blocks(z.abs(), z.abs(), A, J1, J2) for z in Z], bt)
        esum = neg_sums_envelope(blocks, eb, 0, A)
        eS = [mm(z[:A].abs(), z[A:2 * A].abs()) for z in Z]
    an = anchor_stage(S, beta, sums, ALPHA, coef, eS=eS, esum=esum, dt=dt)
    gs = an['gs_rows'].sum(2)
    env_gs = an['env_gs_rows'].sum(2) if envelopes else None
    cm, cj, em, ej = neg_coefs(blocks, gs, bt, 0, A, eb, env_gs)
    dE, env_dE = [], []
    for m in range(n):
        if f16[m]:
            bounds = f16_bounds(gs[m])
            dz = f16_grad_rows(f16_coefs(cm[m], bounds), bounds, Z[m], A, J1, J2)
            dz[:2 * A] += f16_stash_rows(an['dS'][m], Z[m], A, 0, A, dt)
        else:
            dz = neg_grad_rows(cm[m], Z[m], A, J1, J2)
            dz[:A] += mm(an['dS'][m], Z[m][A:2 * A].t())
            dz[A:2 * A] += mm(an['dS'][m].t(), Z[m][:A].t())
        env_in = None
        if envelopes:
            env_in = neg_grad_rows(em[m], Z[m], A, J1, J2, True)
            env_in[:A] += an['env_dS'][m] @ Z[m][A:2 * A].abs()
            env_in[A:2 * A] += an['env_dS'][m].t() @ Z[m][:A].abs()
        de, ee = scatter(dz, None, rows[m], nrm[m], idx, T, dt=dt, env_in=env_in)
        dE.append(de)
        env_dE.append(ee)
    res = dict(terms=an['terms_rows'].sum(1), dE=dE)
    if envelopes:
        res.update(env_dE=env_dE, env_terms=an['env_terms_rows'].sum(1))
    if beta is not None:
        res['gamma'] = an['gamma_rows'].sum(1) + torch.stack([sum(sum64(cj[f] * blocks[m][f]) for f in range(4)) for m in range(n)])
        if envelopes:
            res['env_gamma'] = an['env_gamma_rows'].sum(1) + torch.stack([sum((ej[f] * blocks[m][f].abs() + cj[f].abs() * eb[m][f]).sum() for f in range(4))
                                                                          for m in range(n)])
    return res


def beta_of(weight):
    sw = torch.softmax(weight.reshape(-1), 0)
    return sw * sw / (sw * sw).sum()


def chain(E, weight, lv_ial, lv_icl, idx, A, J1, J2, dt=torch.float64, envelopes=False, z_ial=0.1, zoom=0.1):
    """chain_terms (fused) with the fusion weight in front and the scalar head behind: OverallLoss and the gradient of its 'loss' (M >= 2
    tables E [T, D], fusion weight [M, 1], the two log_vars)."""
    M = len(E)
    w = weight.detach().to(dt).clone().requires_grad_(True)
    beta_t = beta_of(w)
    one = torch.tensor([1.0, 0, 0, 0], dtype=dt)
    _, coef, _, _ = head_stage(torch.ones(3 * M + 1, dtype=dt), lv_ial, lv_icl, one, A, dt)     # does not depend on the term values
    ct = chain_terms(E, beta_t.detach(), idx, A, J1, J2, coef, dt, envelopes)
    (beta_t * ct['gamma'].to(dt)).sum().backward()
    out, _, dla, dlc = head_stage(ct['terms'], lv_ial, lv_icl, one, A, dt)
    res = dict(out=out, dE=ct['dE'], dw=w.grad.reshape(-1), dla=dla, dlc=dlc, terms=ct['terms'], gamma=ct['gamma'])
    if envelopes:
        # d beta / d weight is a handful of exact-to-rounding scalars: the weight gradient owes what gamma owes, through |d beta / d w|
        jac = torch.autograd.functional.jacobian(beta_of, weight.detach().double().reshape(-1))
        env_t = ct['env_terms']
        la, lc = lv_ial.double(), lv_icl.double()
        icl, ial = env_t[:M + 1] / float(A * A), z_ial * (ALPHA * env_t[M + 1:2 * M + 1] + (1 - ALPHA) * env_t[2 * M + 1:])
        al = ((torch.exp(-la) * ial) + la.abs()).sum() * zoom
        un = ((torch.exp(-lc) * icl[:M]) + lc.abs()).sum()
        res.update(env_dE=ct['env_dE'], env_dw=jac.abs().t() @ ct['env_gamma'], env_out=torch.stack([al + un + icl[M], un, icl[M], al]),
                   env_dla=zoom * (1.0 + torch.exp(-la) * ial), env_dlc=1.0 + torch.exp(-lc) * icl[:M])
    return res


# ------------------------------------------------------------------------------------------------ inputs
def index_sets(A, J1, J2, seed, dup=False):
    """(idx [2A + J1 + J2] int32 = e1i | e2i | e1j | e2j, T): distinct objects (no row is both anchor and negative), 5 unreferenced rows;
    dup: e1j and e2j each name one of their objects twice."""
    g = torch.Generator().manual_seed(seed)
    R = 2 * A + J1 + J2
    T = R + 5
    idx = torch.randperm(T, generator=g)[:R].to(torch.int32)
    if dup:
        if J1 > 1:
            idx[2 * A + J1 - 1] = idx[2 * A]
        if J2 > 1:
            idx[2 * A + J1 + J2 - 1] = idx[2 * A + J1]
    return idx, T


def tables(kind, T, D, M, seed, idx=None, A=0):
    """M embedding tables [T, D] float32 with row norms over 2^-20 .. 2^20.  'gauss': S / 0.1 ~ N(0, 1); 'cluster': 8 class centres + 0.05
    noise (S from about -0.2 to 0.99: a few pairs carry a sum); 'parallel': like gauss, but table 1's rows are nearly identical (centred);
    'onehot': the census with the centring ON -- two classes a side (|mean row|^2 >= 1/4), anchors x negatives similarities 0 up to the
    bookkeeping columns' rounding, judged at the gate."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for m in range(M):
        if kind == 'onehot':
            e = torch.zeros(T, D)
            ii = idx.long()
            e[ii[:2 * A], (torch.arange(2 * A) + m) % 2] = 1.0
            n = ii.numel() - 2 * A
            e[ii[2 * A:], D - 1 - (torch.arange(n) + m) % 2] = 1.0
            e[e.abs().sum(1) == 0, 0] = 1.0                 # the unreferenced rows
        elif kind == 'cluster':
            e = torch.randn(8, D, generator=g)[torch.randint(0, 8, (T,), generator=g)] + 0.05 * torch.randn(T, D, generator=g)
        elif kind == 'parallel' and m == 1:
            e = torch.randn(1, D, generator=g) + 0.05 * torch.randn(T, D, generator=g)
        else:
            e = torch.randn(T, D, generator=g)
        out.append((e * torch.ldexp(torch.ones(T), torch.randint(-20, 21, (T,), generator=g))[:, None]).float())
    return out


def fusion_weights(M, seed):
    """softmax(fusion.weight) of a case (sg_aligner.py:32)."""
    return torch.softmax(0.5 * torch.randn(M, generator=torch.Generator().manual_seed(77 + seed)), 0)


def fusion_beta(M, seed):
    w = fusion_weights(M, seed)
    return ((w * w) / (w * w).sum()).float()


def census(A, J1, J2, D, M, seed, count_limit=True, shards=None):
    """Census tables (module docstring): rows 2^s e_k, s in -20 .. 20.  Returns (tables [T, D] float32, idx, T, classes [M][R]).  The builder
    asserts >= 5 classes a side with even counts (|mean row|^2 < 1/4: the centring stays off) and, with count_limit, at most CENSUS_COUNT
    rows per class among the X1 and among the X2 anchors of every shard and in each negative segment."""
    g = torch.Generator().manual_seed(500 + seed)
    idx, T = index_sets(A, J1, J2, seed)
    half = D // 2
    assert half >= 5 and D - half >= 5, 'fewer than 5 classes a side'
    R = 2 * A + J1 + J2
    tabs, classes = [], []
    for m in range(M):
        cls = torch.empty(R, dtype=torch.long)
        for s0, n, c0, nc in ((0, A, 0, half), (A, A, 0, half), (2 * A, J1, half, D - half), (2 * A + J1, J2, half, D - half)):
            off = int(torch.randint(0, nc, (1,), generator=g))
            cls[s0:s0 + n] = c0 + (torch.arange(n) + off) % nc                       # round robin: even counts, a different start per table
        e = torch.zeros(T, D)
        sc = torch.ldexp(torch.ones(R), torch.randint(-20, 21, (R,), generator=g))
        e[idx.long(), cls] = sc
        z = e[idx.long()] / sc[:, None]
        assert float(z.mean(0).pow(2).sum()) < 0.25, 'the census would be centred'
        if count_limit:
            for lo, hi in (shards or [(0, A)]):
                for s0 in (0, A):
                    assert int(torch.bincount(cls[s0 + lo:s0 + hi], minlength=D).max()) <= CENSUS_COUNT
            for s0, n in ((2 * A, J1), (2 * A + J1, J2)):
                assert n == 0 or int(torch.bincount(cls[s0:s0 + n], minlength=D).max()) <= CENSUS_COUNT
        tabs.append(e)
        classes.append(cls)
    return tabs, idx, T, classes


def census_sums(A_shard, J1, J2, NT):
    """The 8 NT global sums of a census, fp64: integers."""
    row = torch.tensor([A_shard * J1] * 2 + [A_shard * J2] * 4 + [A_shard * J1] * 2, dtype=torch.float64)
    return row.expand(NT, 8).clone()


def packed(z, D, slack=32):
    """A unit-row table [R, D] as the fused kernels take it: float32 [R + 32, 104], zero padding and 32 readable zero rows."""
    out = torch.zeros(z.shape[0] + slack, DP)
    out[:z.shape[0], :D] = z.float()
    return out


# ------------------------------------------------------------------------------------------------ the gate cases
# (A, J1, J2) from the tile geometry: 32-row tiles, 64 / 128-row owner blocks, A x A blocks of 32 rows (16 staged at M = 4), the K tail at
# columns 96 .. 103; A = 257, 333 for the multi-block A x A walks; (300, 5500, 5500) for the split into work units of <= 160 tile steps.
EDGE_SHAPES = [(1, 1, 1), (31, 33, 1), (32, 32, 32), (33, 31, 65), (63, 64, 129), (65, 127, 63), (129, 21, 75)]
WIDTHS = [100, 97, 96, 64, 37, 8]
PLAIN_WIDTHS = [101, 104]


def gate_cases():
    """dict(name, A, J1, J2, D, M, kind, seed, dup): every shape, every width and every M at least once per tier; the edge shapes at M = 3, 4."""
    C = []
    kinds = ['gauss', 'cluster', 'parallel']
    for i, (a, j1, j2) in enumerate(EDGE_SHAPES):
        for M in (3, 4):
            C.append(dict(A=a, J1=j1, J2=j2, D=WIDTHS[(i + M) % len(WIDTHS)], M=M, kind=kinds[(i + M) % 3], seed=10 * i + M, dup=(i == 4)))
    C.append(dict(A=65, J1=127, J2=63, D=100, M=2, kind='parallel', seed=91, dup=True))
    C.append(dict(A=33, J1=31, J2=65, D=8, M=2, kind='cluster', seed=92, dup=False))
    C.append(dict(A=257, J1=40, J2=9, D=100, M=3, kind='cluster', seed=93, dup=False))
    C.append(dict(A=333, J1=17, J2=50, D=97, M=4, kind='gauss', seed=94, dup=False))
    C.append(dict(A=300, J1=5500, J2=5500, D=100, M=3, kind='gauss', seed=95, dup=False))
    C.append(dict(A=65, J1=127, J2=63, D=64, M=3, kind='onehot', seed=96, dup=False))
    for c in C:
        c['name'] = f"{c['kind']}-A{c['A']}-{c['J1']}-{c['J2']}-D{c['D']}-M{c['M']}"
    return C


def plain_cases():
    C = [dict(A=65, J1=127, J2=63, D=101, M=3, kind='gauss', seed=71, dup=False), dict(A=33, J1=31, J2=65, D=104, M=4, kind='cluster', seed=72, dup=False),
         dict(A=129, J1=21, J2=75, D=104, M=2, kind='gauss', seed=73, dup=True)]
    for c in C:
        c['name'] = f"{c['kind']}-A{c['A']}-{c['J1']}-{c['J2']}-D{c['D']}-M{c['M']}"
    return C


def shards3(A):
    """[0, A) in three shards cut off the 32-row grid (fewer for tiny A)."""
    cuts = sorted({0, A} | {c for c in (A // 3 + 1, 2 * A // 3 + 3) if 0 < c < A})
    return list(zip(cuts[:-1], cuts[1:]))


def shards8(A):
    """shards3 with the cuts moved down to multiples of 8 anchors: where a shard of the wide fp16 kernels may start."""
    cuts = sorted({0, A} | {lo // 8 * 8 for lo, _ in shards3(A) if 0 < lo // 8 * 8 < A})
    return list(zip(cuts[:-1], cuts[1:]))


@functools.lru_cache(maxsize=None)
def _case_inputs(name):
    c = {k['name']: k for k in gate_cases() + plain_cases()}[name]
    idx, T = index_sets(c['A'], c['J1'], c['J2'], c['seed'], c['dup'])
    E = tables(c['kind'], T, c['D'], c['M'], c['seed'], idx, c['A'])
    beta = fusion_beta(c['M'], c['seed'])
    g = torch.Generator().manual_seed(c['seed'])
    coef = ((torch.rand(3 * c['M'] + 1, generator=g) + 0.5) * 1e-2).float()
    Z = [gather(e, idx)[0].float() for e in E]                       # what every later stage is handed: the fp32 rounding of the exact rows
    return dict(c, idx=idx, T=T, E=E, beta=beta, coef=coef, Z=Z)


def case_inputs(case):
    return _case_inputs(case if isinstance(case, str) else case['name'])


def errors(out, ref, env):
    return G.rel_errors(out.detach().cpu(), ref, env)


def centre_image(z, D):
    """What sga_loss_centre_tables / sga_loss_split3_tables make of a unit-row table z [R, D <= 100] float32: (Zc [R + 32, 104] float32 =
    (z - zbar | b = zbar . (z - zbar) + |zbar|^2 / 2 | 1 | 0 0), zbar [100] float32, centred?), zbar = 0 unless |mean row|^2 >= 1/4."""
    R = z.shape[0]
    zb = torch.zeros(100)
    zb[:D] = (z.double().sum(0) / max(R, 1)).float()
    tot = float(zb.double().pow(2).sum())
    centred = tot >= 0.25
    if not centred:
        zb.zero_()
    out = torch.zeros(R + 32, DP)
    out[:R, :D] = z.float() - zb[:D]
    nbh = torch.tensor(0.5 * tot if centred else 0.0).float().double()
    out[:R, 100] = ((zb.double()[None, :] * out[:R, :100].double()).sum(1) + nbh).float()
    out[:R, 101] = 1.0
    return out, zb, centred


# ------------------------------------------------------------------------------------------------ the references of a case, once per session
@functools.lru_cache(maxsize=None)
def anchor_refs(name):
    """The A x A stages of a case (one arithmetic for every tier: the kernels take the plain tables): inputs, fp64 reference with envelopes,
    float32 yardstick."""
    c = _case_inputs(name)
    A, D = c['A'], c['D']
    X = [(z[:A, :D], z[A:2 * A, :D]) for z in c['Z']]
    S64 = [mm(x1.double(), x2.double()) for x1, x2 in X]
    eS = [mm(x1.double().abs(), x2.double().abs()) for x1, x2 in X]
    S32 = [mm(x1, x2) for x1, x2 in X]
    # the sums the stage is handed: the fp64 reference sums of the plain tables (any positive numbers of the right size would do)
    sd = [sides(z.double(), A, c['J1'], c['J2'], D) for z in c['Z']]
    blocks = with_joint([neg_blocks(L, Rt, A, c['J1'], c['J2']) for L, Rt, _ in sd], c['beta'].double())
    sums = neg_sums(blocks, 0, A)
    eb = with_joint([neg_blocks(L.abs(), Rt.abs(), A, c['J1'], c['J2']) for L, Rt, _ in sd], c['beta'].double())
    esum = neg_sums_envelope(blocks, eb, 0, A)
    ref = anchor_stage(S64, c['beta'], sums, ALPHA, c['coef'], eS=eS, esum=esum)
    yard = anchor_stage(S32, c['beta'], sums, ALPHA, c['coef'], dt=torch.float32)
    return dict(sums=sums, ref=ref, yard=yard)


@functools.lru_cache(maxsize=None)
def sweep_refs(name, tier):
    """The anchors x negatives stages of a case in one tier, the stash products and the scatter: inputs (the table images the kernels take),
    fp64 references with envelopes, float32 yardsticks.  gs and the stashes are the A x A reference's (fp64 / rounded to fp32)."""
    c = _case_inputs(name)
    A, J1, J2, D, M = c['A'], c['J1'], c['J2'], c['D'], c['M']
    beta = c['beta']
    cen = tier != 'plain'
    if cen:
        made = [centre_image(z, D) for z in c['Z']]
        img, zbar, flag = [m_[0] for m_ in made], [m_[1][:D] for m_ in made], [m_[2] for m_ in made]
    else:
        img, zbar, flag = [packed(z, D) for z in c['Z']], [None] * M, [False] * M
    an = anchor_refs(name)
    gs = an['ref']['gs_rows'].sum(2)
    out = dict(img=img, zbar=zbar, centred=flag, gs=gs, shards=shards3(A))
    sd = {dt: [sides(i.to(dt), A, J1, J2, D, cen) for i in img] for dt in (torch.float64, torch.float32)}
    bl = {dt: with_joint([neg_blocks(L, Rt, A, J1, J2) for L, Rt, _ in sd[dt]], beta.to(dt)) for dt in sd}
    eb = with_joint([neg_blocks(L.abs(), Rt.abs(), A, J1, J2) for L, Rt, _ in sd[torch.float64]], beta.double())
    cols = list(range(D)) + ([101] if cen else [])
    out['cols'] = cols
    for lo, hi in [(0, A)] + (out['shards'] if len(out['shards']) > 1 else []):
        r = {}
        r['sums'] = (neg_sums(bl[torch.float64], lo, hi), neg_sums_envelope(bl[torch.float64], eb, lo, hi), neg_sums(bl[torch.float32], lo, hi))
        cm, cj, em, ej = neg_coefs(bl[torch.float64], gs, beta, lo, hi, eb)
        ym, yj, _, _ = neg_coefs(bl[torch.float32], gs, beta, lo, hi)
        r['dZ'] = [(neg_grad_rows(cm[m], sd[torch.float64][m][2], A, J1, J2), neg_grad_rows(em[m], sd[torch.float64][m][2], A, J1, J2, True),
                    neg_grad_rows(ym[m], sd[torch.float32][m][2], A, J1, J2)) for m in range(M)]
        b64, b32 = bl[torch.float64], bl[torch.float32]
        r['gamma_neg'] = (torch.stack([sum(sum64(cj[f] * b64[m][f]) for f in range(4)) for m in range(M)]),
                          torch.stack([sum((ej[f] * b64[m][f].abs() + cj[f].abs() * eb[m][f]).sum() for f in range(4)) for m in range(M)]),
                          torch.stack([sum(sum64(yj[f] * b32[m][f]) for f in range(4)) for m in range(M)]))
        out[(lo, hi)] = r
    # ---- stash products: dX1 = dS B[X2 rows], dX2 = dS^T B[X1 rows] on the tier's B operand, all 104 columns
    m1 = [d.float() for d in an['ref']['dS']]
    out['m1'] = m1
    st = []
    for m in range(M):
        b1, b2 = img[m][:A], img[m][A:2 * A]
        ref = torch.cat([G.reference(m1[m], b2.t()), G.reference(m1[m].t(), b1.t())])
        env = torch.cat([G.envelope(m1[m], b2.t()), G.envelope(m1[m].t(), b1.t())])
        yard = torch.cat([G.yardstick(m1[m], b2.t().contiguous()), G.yardstick(m1[m].t().contiguous(), b1.t().contiguous())])
        st.append((ref, env, yard))
    out['stash'] = st
    # ---- scatter: the rows' gradient as the stages above deliver it (rounded to fp32), projected and scattered
    nrm = [gather(e, c['idx'])[1].float() for e in c['E']]
    out['nrm'] = nrm
    sc, dzin = [], []
    Rr = 2 * A + J1 + J2
    for m in range(M):
        full = out[(0, A)]['dZ'][m][0].clone()
        dz = torch.zeros(Rr, DP, dtype=torch.float64)
        dz[:, cols] = full
        dz[:2 * A] += st[m][0]
        dz = dz.float()
        dzin.append(dz)
        zb = zbar[m] if flag[m] else None
        rho = dz[:, 101] if flag[m] else None
        ref, env = scatter(dz[:, :D], rho, c['Z'][m][:, :D], nrm[m], c['idx'], c['T'], zb)
        yard, _ = scatter(dz[:, :D], rho, c['Z'][m][:, :D], nrm[m], c['idx'], c['T'], zb, dt=torch.float32)
        sc.append((ref, env, yard))
    out['dz_in'], out['scatter'] = dzin, sc
    return out


@functools.lru_cache(maxsize=None)
def gather_refs(name, m=0):
    c = _case_inputs(name)
    z, n = gather(c['E'][m], c['idx'])
    zy, ny = gather(c['E'][m], c['idx'], torch.float32)
    return dict(Z=(z, z.abs(), zy), nrm=(n, n.abs(), ny))


# ------------------------------------------------------------------------------------------------ launches at the C ABI (GPU)
NAN = float('nan')


def _abi():
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _ptr_array, _stream
    return _lib, _lib.lib(), _p, _ptr_array, _stream()


def _slots():
    return 1 + _abi()[1].sga_loss_slots()


def run_gather(E, idx, Dp):
    lib, L, p, _, st = _abi()
    e, ix = E.cuda().contiguous(), idx.cuda().contiguous()
    R, D = ix.numel(), e.shape[1]
    z = torch.full((R, Dp), NAN, device='cuda')
    n = torch.full((R,), NAN, device='cuda')
    lib.check(L.sga_loss_gather(p(e), e.shape[0], D, p(ix), R, p(z), Dp, p(n), st), 'sga_loss_gather')
    return z.cpu(), n.cpu()


class Tier:
    """A case's tables in one tier, launched through the product's own tier object (sgaligner_amd.loss_ops.TIERS), with what is the test's:
    outputs pre-filled with NaN; centred: the CPU-made centred images (the stage's stated input) in place of the library's.  made_zc: the
    centred rows the library itself produced, for the check against centre_image."""

    def __init__(self, tier, Z, img, A, J1, J2, D):
        from sgaligner_amd import loss_ops, ops
        self.ops = ops
        self.tier, self.M, self.A, self.J1, self.J2, self.D = tier, len(Z), A, J1, J2, D
        self.R = 2 * A + J1 + J2
        self.zs = [packed(z, D).cuda() for z in Z]
        self.index = types.SimpleNamespace(A=A, J1=J1, J2=J2, R=self.R, idx=None)          # what the tier reads of ops.IndexSets
        t = self.t = loss_ops.TIERS[tier](self.index, self.zs, D)
        for zc in getattr(t, 'zc', []):
            zc[:-32].fill_(NAN)
        t.prepare()
        self.stat = getattr(t, 'stat', None)
        self.made_zc = [zc[:-32] for zc in getattr(t, 'zc', [])]
        if tier == 'centred':
            t.zc = [i.cuda().contiguous() for i in img]

    def sums(self, beta, lo, hi, lite=0):
        buf = torch.full((_slots(), self.M + 1, 8), NAN, device='cuda', dtype=torch.float64)
        with mock.patch.object(self.ops, 'BF16X6_SUMS_LITE', bool(lite)):
            self.t.sums(beta.cuda(), buf, lo, hi)
        return buf[0].cpu()

    def grad(self, beta, gs, lo, hi, dz=None):
        """dZ [M][R, 104] (accumulated into dz when given) and gamma [M]."""
        if dz is None:
            dz = [torch.zeros(self.R + 32, DP, device='cuda') for _ in range(self.M)]
        gam = torch.full((_slots(), self.M), NAN, device='cuda', dtype=torch.float64)
        self.t.grad(beta.cuda(), gs.cuda().contiguous(), dz, gam, lo, hi)
        return dz, gam[0].cpu()

    def stash(self, m, dS, jobs, entry):
        """The stash products of table m over a walk of `jobs` (lo, hi, j_lo, j_hi, mir): the float32 coefficients dS [A, A] cut into the
        launches' stashes M1[(j - j_lo), (i - lo)] = dS[i, j], M2[(j - mir), (i - lo)] = dS[j, i].  entry: 'stash_grad' (ordered blocks, jobs
        (lo, hi, 0, A, A)), 'symx', 'symx_bf16x6' (the planes tier's own) -- chosen here, through the tier's arguments.  Returns dZ [2A, 104]."""
        dz = torch.zeros(self.R + 32, DP, device='cuda')
        d = dS.cuda()
        assert entry != 'symx_bf16x6' or self.tier == 'planes'
        with mock.patch.object(self.ops, 'BF16X6_STASH', entry == 'symx_bf16x6'):
            for lo, hi, jl, jh, mir in jobs:
                m1 = d[lo:hi, jl:jh].t().contiguous()
                m2 = d[mir:jh, lo:hi].contiguous() if mir < jh else None
                assert entry != 'stash_grad' or ((jl, jh) == (0, self.A) and mir >= self.A)
                self.t.stash(m, m1, m2, dz, (lo, hi, jl, jh, mir), entry != 'stash_grad')
        return dz[:2 * self.A].cpu()

    def scatter(self, m, dz_in, nrm, idx, T, stat=None):
        """dE [T, D] by the tier's scatter; centred: stat = a statistics block to hand over instead of the library's own."""
        de = torch.zeros(T, self.D, device='cuda')
        self.index.idx = idx.cuda()
        self.t.stat = self.stat if stat is None else {m: stat}
        self.t.scatter(m, dz_in.cuda().contiguous(), nrm.cuda(), self.D, de)
        return de.cpu()


def run_anchor_fwd(zs, beta, A, sums, lo, hi):
    lib, L, p, pa, st = _abi()
    M = len(zs)
    n = 3 * M + 1
    out = torch.full((_slots() * n,), NAN, device='cuda', dtype=torch.float64)
    s, b = sums.cuda().contiguous(), beta.cuda()
    lib.check(L.sga_loss_anchor_multi_fwd(pa(zs), M, p(b), A, p(s), ALPHA, TAU[0], TAU[1], p(out), lo, hi, st), 'sga_loss_anchor_multi_fwd')
    return out[:n].cpu()


AA_ORDERED, AA_SYMX, AA_PLANES = 'sga_loss_anchor_multi_bwd', 'sga_loss_anchor_multi_bwd_symx', 'sga_loss_anchor_multi_bwd_symx_bf16x6'


def run_anchor_bwd(entry, tables, geom, beta, sums, coef, jobs, terms=True):
    """A whole walk of the A x A backward through `entry`: jobs (lo, hi, j_lo, j_hi, mir).  AA_ORDERED takes the packed tables, geom = (A,) and
    ordered jobs (lo, hi, 0, A, A); AA_SYMX the packed tables and geom = (A,); AA_PLANES the three-plane images and geom = (A, J1, J2).  terms:
    with out_terms (a symmetric launch always).  A job without mirrored elements (mir >= j_hi) passes M2 == NULL.  Stashes are pre-filled with
    NaN and written into NaN-filled [A, A] matrices dS[m][i, j] -- an element no launch produced stays NaN, an element produced twice must
    agree.  Returns (dS [M][A, A], terms, gs [NT, 8], gamma [M]), summed over the walk."""
    lib, L, p, pa, st = _abi()
    A = geom[0]
    M, nt = len(tables), len(tables) + 1
    n = 3 * M + 1
    s, b, cf = sums.cuda().contiguous(), beta.cuda(), coef.cuda()
    dS = [torch.full((A, A), NAN, device='cuda') for _ in range(M)]
    acc = [torch.zeros(n, dtype=torch.float64), torch.zeros(nt, 8, dtype=torch.float64), torch.zeros(M, dtype=torch.float64)]
    for lo, hi, jl, jh, mir in jobs:
        ns = hi - lo
        out = torch.full((_slots() * n,), NAN, device='cuda', dtype=torch.float64)
        gsc = torch.full((_slots() + 1, nt, 8), NAN, device='cuda', dtype=torch.float64)
        gam = torch.full((_slots(), M), NAN, device='cuda', dtype=torch.float64)
        m1 = [torch.full(((jh - jl) * ns,), NAN, device='cuda') for _ in range(M)]
        m2 = [torch.full(((jh - mir) * ns,), NAN, device='cuda') for _ in range(M)] if mir < jh else None
        if entry == AA_ORDERED:
            assert (jl, jh) == (0, A) and m2 is None
            stash2, where = (), (lo, hi)
        else:
            stash2, where = (pa(m2) if m2 else None,), (lo, hi, jl, jh, mir)
        lib.check(getattr(L, entry)(pa(tables), M, p(b), *geom, p(s), ALPHA, TAU[0], TAU[1], p(cf), pa(m1), *stash2, p(gsc), p(gam), *where,
                                    p(out) if terms else None, st), entry)
        for m in range(M):
            new = [(slice(lo, hi), slice(jl, jh), m1[m].view(jh - jl, ns).t())]
            if m2:
                new.append((slice(mir, jh), slice(lo, hi), m2[m].view(jh - mir, ns)))
            for ri, ci, v in new:
                old = dS[m][ri, ci]
                seen = ~torch.isnan(old)
                assert torch.equal(old[seen], v[seen]), 'an element written by two launches of a walk differs'
                dS[m][ri, ci] = v
        if terms:
            acc[0] += out[:n].cpu()
        acc[1] += gsc[0].cpu()
        acc[2] += gam[0].cpu()
    return [d.cpu() for d in dS], acc[0], acc[1], acc[2]


def ordered_jobs(A, rows):
    return [(lo, min(lo + rows, A), 0, A, A) for lo in range(0, A, rows)]


def sym_jobs(A, M, stash_bytes, cuts=None):
    """ops._sym_jobs for every rank of `cuts` (one rank: [0, A]) under a stash bound."""
    from sgaligner_amd import ops
    cuts = cuts or [0, A]
    with mock.patch.object(ops, 'STASH_BYTES', stash_bytes):
        return [j for r in range(len(cuts) - 1) for j in ops._sym_jobs(list(cuts), r, M)]


def run_head(terms, lv_ial, lv_icl, A, z_ial, alpha, zoom, f64, gout):
    """(out [4], dterms [3M+1], dlv_ial [M], dlv_icl [M]) of sga_loss_head_fwd / _bwd; terms in fp64 (f64) or float32."""
    lib, L, p, pa, st = _abi()
    M = lv_ial.numel()
    t = (terms.double() if f64 else terms.float()).cuda().contiguous()
    la, lc, go = lv_ial.float().cuda(), lv_icl.float().cuda(), gout.double().cuda()
    inv = 1.0 / float(A * A) if A else NAN
    out = torch.full((4,), NAN, device='cuda', dtype=torch.float64)
    lib.check(L.sga_loss_head_fwd(p(t), int(f64), p(la), p(lc), M, inv, z_ial, alpha, zoom, p(out), st), 'sga_loss_head_fwd')
    d = torch.full_like(t, NAN)
    da, dc = torch.full_like(la, NAN), torch.full_like(lc, NAN)
    lib.check(L.sga_loss_head_bwd(p(go), p(t), int(f64), p(la), p(lc), M, inv, z_ial, alpha, zoom, p(d), p(da), p(dc), st), 'sga_loss_head_bwd')
    return out.cpu(), d.cpu(), da.cpu(), dc.cpu()


# ------------------------------------------------------------------------------------------------ measurements (GPU): what the tests gate and the profile records
def tier_for(case):
    """The tiers a case runs in: tables wider than 100 columns take the plain fp32 sweeps, the others the centred and three-plane ones
    (and the plain sweeps too: the kernels accept any width up to 104)."""
    return ['plain'] if case['D'] > 100 else ['plain', 'centred', 'planes']


@functools.lru_cache(maxsize=4)
def tier_images(name, tier):
    c = _case_inputs(name)
    return Tier(tier, c['Z'], sweep_refs(name, tier)['img'], c['A'], c['J1'], c['J2'], c['D'])


def _row(output, tier, out, ref, env, yard):
    return output, tier, errors(out, ref, env), errors(yard, ref, env)


def measure_gather(name):
    c = _case_inputs(name)
    D = c['D']
    ref = gather_refs(name)
    for Dp in sorted({DP, (D + 7) // 8 * 8}):
        z, n = run_gather(c['E'][0], c['idx'], Dp)
        assert torch.equal(z[:, D:], torch.zeros_like(z[:, D:])), 'padding columns not zeroed'
        yield _row('gather.Z', 'f32', z[:, :D], *ref['Z'])
        yield _row('gather.nrm', 'f32', n, *ref['nrm'])


def measure_centring(name, tier):
    """The centred rows the library makes (sga_loss_centre_tables; the anchor rows of sga_loss_split3_tables) against centre_image: the
    images the sweep stages are handed must be the library's own, to a unit in the last place of the mean row."""
    c = _case_inputs(name)
    T, sr = tier_images(name, tier), sweep_refs(name, tier)
    for m, made in enumerate(T.made_zc):
        n = made.shape[0]
        img, got = sr['img'][m][:n].clone(), made[:n].cpu()
        if tier == 'planes':                               # (the anchor rows' copy carries no b: the stash products never read column 100)
            img[:, 100] = 0.0
        assert torch.isfinite(got).all()
        tol = 2.0 ** -23 * (c['Z'][m].abs().amax() + 1.0)
        assert (got - img).abs().max() <= tol, (name, tier, m)


def measure_sums(name, tier):
    c = _case_inputs(name)
    T, sr = tier_images(name, tier), sweep_refs(name, tier)
    A = c['A']
    whole = T.sums(c['beta'], 0, A)
    yield _row('neg_sums.sums', tier, whole, *sr[(0, A)]['sums'])
    if len(sr['shards']) > 1:
        for lo, hi in sr['shards']:
            yield _row('neg_sums.sums', tier, T.sums(c['beta'], lo, hi), *sr[(lo, hi)]['sums'])


def measure_grad(name, tier):
    c = _case_inputs(name)
    T, sr = tier_images(name, tier), sweep_refs(name, tier)
    A, R, cols = c['A'], T.R, sr['cols']
    runs = [[(0, A)]] + ([sr['shards']] if len(sr['shards']) > 1 else [])
    for parts in runs:                                     # unsharded, then the shards replayed into the same buffers
        dz, gam = None, torch.zeros(c['M'], dtype=torch.float64)
        for lo, hi in parts:
            dz, g1 = T.grad(c['beta'], sr['gs'], lo, hi, dz)
            gam += g1
        ref = sr[(0, A)]
        for m in range(c['M']):
            out = dz[m].cpu()
            if tier == 'plain':
                assert torch.equal(out[:R, c['D']:], torch.zeros(R, DP - c['D'])), 'gradient in the padding columns'
            assert torch.equal(out[R:], torch.zeros(32, DP)), 'gradient in the slack rows'
            yield _row('neg_grad.dZ', tier, out[:R][:, cols], *ref['dZ'][m])
        yield _row('neg_grad.gamma_neg', tier, gam, *ref['gamma_neg'])


def aa_walks(A, M):
    """(label, jobs, sym): ordered blocks of 32 k rows with a ragged last one; the symmetric walk of one rank under a stash bound that
    forces >= 3 blocks of growing height; the same for 3 ranks (wrapped columns)."""
    W = [('ordered', ordered_jobs(A, 32 if A < 200 else 96), False)]
    if A >= 96:
        bound = 4 * M * 2 * A * 32
        W.append(('sym', sym_jobs(A, M, bound), True))
        c1 = (A // 3 + 31) // 32 * 32
        W.append(('sym3', sym_jobs(A, M, bound, [0, c1, min(A, 2 * c1), A]), True))
    return W


def measure_anchor(name):
    c = _case_inputs(name)
    an = anchor_refs(name)
    A, M = c['A'], c['M']
    T = tier_images(name, 'plain')
    ref, yard = an['ref'], an['yard']
    tot = lambda k, d: d[k].sum(-1)
    t3 = (tot('terms_rows', ref), tot('env_terms_rows', ref), tot('terms_rows', yard))
    yield _row('anchor_terms.terms', 'f32', run_anchor_fwd(T.zs, c['beta'], A, an['sums'], 0, A), *t3)
    sh = shards3(A)
    if len(sh) > 1:
        yield _row('anchor_terms.terms', 'f32', sum(run_anchor_fwd(T.zs, c['beta'], A, an['sums'], lo, hi) for lo, hi in sh), *t3)
    for label, jobs, sym in aa_walks(A, M):
        dS, terms, gs, gam = run_anchor_bwd(AA_SYMX if sym else AA_ORDERED, T.zs, (A,), c['beta'], an['sums'], c['coef'], jobs)
        yield _row('anchor_terms.terms', 'f32', terms, *t3)
        for m in range(M):
            yield _row('anchor_coef.dS', 'f32', dS[m], ref['dS'][m], ref['env_dS'][m], yard['dS'][m])
        yield _row('anchor_coef.gs', 'f32', gs, tot('gs_rows', ref), tot('env_gs_rows', ref), tot('gs_rows', yard))
        yield _row('anchor_coef.gamma', 'f32', gam, tot('gamma_rows', ref), tot('env_gamma_rows', ref), tot('gamma_rows', yard))


def measure_stash(name, tier):
    c = _case_inputs(name)
    T, sr = tier_images(name, tier), sweep_refs(name, tier)
    A, M = c['A'], c['M']
    cols = list(range(DP)) if tier == 'plain' else sr['cols']
    for label, jobs, sym in aa_walks(A, M):
        entry = 'symx_bf16x6' if tier == 'planes' else ('symx' if sym else 'stash_grad')
        for m in range(M):
            out = T.stash(m, sr['m1'][m], jobs, entry)
            ref, env, yard = sr['stash'][m]
            yield _row('stash_grad.dZ', tier, out[:, cols], ref[:, cols], env[:, cols], yard[:, cols])


def measure_scatter(name, tier):
    c = _case_inputs(name)
    T, sr = tier_images(name, tier), sweep_refs(name, tier)
    for m in range(c['M']):
        de = T.scatter(m, sr['dz_in'][m], sr['nrm'][m], c['idx'], c['T'])
        yield _row('scatter.dE', 'f32' if tier == 'plain' else tier, de, *sr['scatter'][m])


HEAD_CASES = [(2, 75, 1), (3, 800, 2), (4, 33, 3)]         # (M, anchors, seed)


def head_refs(M, A, seed):
    g = torch.Generator().manual_seed(seed)
    terms = (torch.rand(3 * M + 1, generator=g, dtype=torch.float64) + 0.5) * float(max(A, 1) ** 2)
    la, lc = 0.3 * torch.randn(M, generator=g), 0.3 * torch.randn(M, generator=g)
    gout = torch.tensor([1.0, 0.25, -0.5, 2.0], dtype=torch.float64)
    return terms, la, lc, gout


def head_stage(terms, la, lc, gout, A, dt):
    t = terms.detach().to(dt).clone().requires_grad_(True)
    a, c_ = la.detach().to(dt).clone().requires_grad_(True), lc.detach().to(dt).clone().requires_grad_(True)
    out = head(t, a, c_, A, 0.1, ALPHA, 0.1, dt)
    (out * gout.to(dt)).sum().backward()
    return out.detach(), t.grad, a.grad, c_.grad


def measure_head(M, A, seed, f64):
    terms, la, lc, gout = head_refs(M, A, seed)
    if not f64:
        terms = terms.float().double()                     # the float32 terms are the stage's input
    ref = head_stage(terms, la, lc, gout, A, torch.float64)
    yard = head_stage(terms, la, lc, gout, A, torch.float32)
    out = run_head(terms, la, lc, A, 0.1, ALPHA, 0.1, f64, gout)
    m = la.numel()
    icl = terms[:m + 1].abs() / float(A * A)
    ial = 0.1 * (ALPHA * terms[m + 1:2 * m + 1].abs() + (1 - ALPHA) * terms[2 * m + 1:].abs())
    al = ((torch.exp(-la.double()) * ial) + la.double().abs()).sum() * 0.1
    un = ((torch.exp(-lc.double()) * icl[:m]) + lc.double().abs()).sum()
    env_out = torch.stack([al + un + icl[m], un, icl[m], al])
    yield _row('head.head', 'f32', out[0], ref[0], env_out, yard[0])
    yield _row('head.dterms', 'f32', out[1], ref[1], ref[1].abs(), yard[1])
    gu, ga = (gout[0] + gout[1]).abs(), ((gout[0] + gout[3]) * 0.1).abs()
    yield _row('head.dlv', 'f32', torch.cat([out[2], out[3]]), torch.cat([ref[2], ref[3]]),
               torch.cat([ga * (1.0 + torch.exp(-la.double()) * ial), gu * (1.0 + torch.exp(-lc.double()) * icl[:m])]), torch.cat([yard[2], yard[3]]))


def measure_all(name, tier):
    """Every gated stage of a case in one tier ('f32'-tier stages ride with the plain tier)."""
    if tier == 'plain':
        yield from measure_gather(name)
        yield from measure_anchor(name)
    else:
        measure_centring(name, tier)
    yield from measure_sums(name, tier)
    yield from measure_grad(name, tier)
    yield from measure_stash(name, tier)
    yield from measure_scatter(name, tier)


def assert_gate(rows, what='', case=None):
    """Print and gate measured rows (output, tier, kernel, yardstick) at R; an output listed in UNGATED for `case` is printed only."""
    bad = []
    for output, tier, ke, ye in rows:
        key = f'{output}|{tier}'
        r = R[key]
        if case in UNGATED.get(key, ()):
            print(f'[loss gate] {what} {key}: NOT GATED here (UNGATED): kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u')
            continue
        print(f'[loss gate] {what} {key}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | fp32 yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
        if not gate_ok(ke, ye, r, is_scalar(output)):
            bad.append((key, ke[:2], ye[:2], r))
    assert not bad, f'{what}: beyond the gate: {bad}'


# ------------------------------------------------------------------------------------------------ the per-table kernels (any joint table; tier 'pertable')
def pertable_cases():
    """The edge shapes at M = 3 (NT = 4 tables of their own widths, the last one standing for the joint) and NT = 1."""
    return [c['name'] for c in gate_cases() if c['M'] == 3 and c['J1'] < 1000]


@functools.lru_cache(maxsize=None)
def pertable_refs(name, nt):
    """NT = 1: the case's first table alone (ICL only); NT = M + 1: its M tables and one more of width D + 8 in the joint's place."""
    c = _case_inputs(name)
    A, J1, J2, D = c['A'], c['J1'], c['J2'], c['D']
    Z = [c['Z'][0]] if nt == 1 else list(c['Z']) + [gather(tables(c['kind'] if c['kind'] != 'onehot' else 'gauss', c['T'], D + 8, 1, c['seed'] + 500)[0], c['idx'])[0].float()]
    m = nt - 1
    coef = ((torch.rand(nt + 2 * m, generator=torch.Generator().manual_seed(c['seed'])) + 0.5) * 1e-2).float()
    out = dict(Z=Z, coef=coef, shards=shards3(A))
    bl = {dt: [neg_blocks(z.to(dt), z.to(dt), A, J1, J2) for z in Z] for dt in (torch.float64, torch.float32)}
    eb = [neg_blocks(z.double().abs(), z.double().abs(), A, J1, J2) for z in Z]
    for lo, hi in [(0, A)] + (out['shards'] if len(out['shards']) > 1 else []):
        out[('sums', lo, hi)] = (neg_sums(bl[torch.float64], lo, hi), neg_sums_envelope(bl[torch.float64], eb, lo, hi), neg_sums(bl[torch.float32], lo, hi))
    sums, esum = out[('sums', 0, A)][:2]
    S64 = [mm(z[:A].double(), z[A:2 * A].double()) for z in Z]
    eS = [mm(z[:A].double().abs(), z[A:2 * A].double().abs()) for z in Z]
    out['sums'] = sums
    out['ref'] = anchor_stage(S64, None, sums, ALPHA, coef, eS=eS, esum=esum)
    out['yard'] = anchor_stage([mm(z[:A], z[A:2 * A]) for z in Z], None, sums, ALPHA, coef, dt=torch.float32)
    gs = out['ref']['gs_rows'].sum(2)
    out['gs'] = gs
    c64, _, e64, _ = neg_coefs(bl[torch.float64], gs, None, 0, A, eb)
    c32, _, _, _ = neg_coefs(bl[torch.float32], gs, None, 0, A)
    out['dZ'] = [(neg_grad_rows(c64[k], Z[k].double(), A, J1, J2), neg_grad_rows(e64[k], Z[k].double(), A, J1, J2, True),
                  neg_grad_rows(c32[k], Z[k], A, J1, J2)) for k in range(nt)]
    return out


def measure_pertable(name, nt):
    """sga_loss_neg_sums_shard, sga_loss_anchor_fwd_f16 / _bwd_f16 with Zh = NULL (exact fp32) and sga_loss_neg_grad_shard on tables of
    pitch Dp = D padded to 8, whole and as three shards."""
    import ctypes
    lib, L, p, pa, st = _abi()
    c, pr = _case_inputs(name), pertable_refs(name, nt)
    A, J1, J2 = c['A'], c['J1'], c['J2']
    R, m = 2 * A + J1 + J2, nt - 1
    dps = [(z.shape[1] + 7) // 8 * 8 for z in pr['Z']]
    zs = []
    for z, dp in zip(pr['Z'], dps):
        t = torch.zeros(R + 32, dp)
        t[:R, :z.shape[1]] = z
        zs.append(t.cuda())
    parts = [[(0, A)]] + ([pr['shards']] if len(pr['shards']) > 1 else [])
    for k in range(nt):
        for lo, hi in parts[0] + (parts[1] if len(parts) > 1 else []):
            buf = torch.full((_slots() * 8,), NAN, device='cuda', dtype=torch.float64)
            lib.check(L.sga_loss_neg_sums_shard(p(zs[k]), dps[k], A, J1, J2, TAU[0], TAU[1], p(buf), lo, hi, st), 'sga_loss_neg_sums_shard')
            ref, env, yard = pr[('sums', lo, hi)]
            yield _row('neg_sums.sums', 'pertable', buf[:8].cpu(), ref[k], env[k], yard[k])
    n = nt + 2 * m
    sums, cf = pr['sums'].cuda().contiguous(), pr['coef'].cuda()
    dparr = (ctypes.c_int * nt)(*dps)
    nullh = (ctypes.c_void_p * nt)()
    ref, yard = pr['ref'], pr['yard']
    tot = lambda key, d: d[key].sum(-1)
    for ps in parts:
        terms = torch.zeros(n, dtype=torch.float64)
        gs = torch.zeros(nt, 8, dtype=torch.float64)
        dS = [torch.full((A, A), NAN) for _ in range(nt)]
        for lo, hi in ps:
            out = torch.full((_slots() * n,), NAN, device='cuda', dtype=torch.float64)
            lib.check(L.sga_loss_anchor_fwd_f16(pa(zs), nullh, dparr, nt, A, p(sums), ALPHA, TAU[0], TAU[1], p(out), lo, hi, None, 0, st), 'sga_loss_anchor_fwd_f16')
            terms += out[:n].cpu()
            m1 = [torch.full((A * (hi - lo),), NAN, device='cuda') for _ in range(nt)]
            gsc = torch.full((_slots() + 1, nt, 8), NAN, device='cuda', dtype=torch.float64)
            lib.check(L.sga_loss_anchor_bwd_f16(pa(zs), nullh, dparr, nt, A, p(sums), ALPHA, TAU[0], TAU[1], p(cf), pa(m1), p(gsc), lo, hi, None, 0, st),
                      'sga_loss_anchor_bwd_f16')
            gs += gsc[0].cpu()
            for k in range(nt):
                dS[k][lo:hi] = m1[k].view(A, hi - lo).t().cpu()
        yield _row('anchor_terms.terms', 'pertable', terms, tot('terms_rows', ref), tot('env_terms_rows', ref), tot('terms_rows', yard))
        yield _row('anchor_coef.gs', 'pertable', gs, tot('gs_rows', ref), tot('env_gs_rows', ref), tot('gs_rows', yard))
        for k in range(nt):
            yield _row('anchor_coef.dS', 'pertable', dS[k], ref['dS'][k], ref['env_dS'][k], yard['dS'][k])
        g = pr['gs'].cuda().contiguous()
        for k in range(nt):
            dz = torch.zeros(R + 32, dps[k], device='cuda')
            for lo, hi in ps:
                lib.check(L.sga_loss_neg_grad_shard(p(zs[k]), dps[k], A, J1, J2, TAU[0], TAU[1], g[k].data_ptr(), p(dz), lo, hi, st), 'sga_loss_neg_grad_shard')
            o = dz.cpu()
            d = pr['Z'][k].shape[1]
            assert torch.equal(o[R:], torch.zeros(32, dps[k])) and torch.equal(o[:R, d:], torch.zeros(R, dps[k] - d))
            yield _row('neg_grad.dZ', 'pertable', o[:R, :d], *pr['dZ'][k])


# ------------------------------------------------------------------------------------------------ loss_group = b and the wide per-table sweep
GROUP_CASES = [(1, 1, 0), (2, 2, 0), (3, 2, 1), (4, 3, 0), (3, 1, 1)]         # (M, pairs per group, use_valu)


def group_batch(seed):
    """A hand-made batch of 5 pairs with ragged counts -- one pair has a single anchor, so b = 1 makes a group of one anchor, b = 2 and 3
    make groups of ragged size: (data_dict of index arrays and per-pair counts, T)."""
    import numpy as np
    ca, c1, c2 = [1, 5, 33, 2, 17], [3, 9, 40, 1, 21], [2, 11, 31, 4, 35]
    A, J1, J2 = sum(ca), sum(c1), sum(c2)
    idx, T = index_sets(A, J1, J2, seed)
    i = idx.numpy()
    return dict(e1i=i[:A], e2i=i[A:2 * A], e1j=i[2 * A:2 * A + J1], e2j=i[2 * A + J1:], e1i_count=np.array(ca), e1j_count=np.array(c1), e2j_count=np.array(c2)), T


@functools.lru_cache(maxsize=None)
def group_refs(M, b, seed=7):
    from sgaligner_amd.loss_ops import group_data_dicts
    dd, T = group_batch(seed)
    E = tables('cluster' if M % 2 else 'gauss', T, 100 if M != 2 else 37, M, seed)
    beta = fusion_beta(M, seed) if M > 1 else None
    groups = group_data_dicts(dd, b)
    n = (M + 1 + 2 * M) if M > 1 else 1
    coef = ((torch.rand(len(groups), n, generator=torch.Generator().manual_seed(seed)) + 0.5) * 1e-2).float()
    acc = {}
    for dt, env in ((torch.float64, True), (torch.float32, False)):
        terms, dE, gam, e_t, e_dE, e_g = [], None, 0, [], None, 0
        for g, d in enumerate(groups):
            ix = torch.cat([torch.as_tensor(d[k].astype('int32')) for k in ('e1i', 'e2i', 'e1j', 'e2j')])
            r = chain_terms(E, beta, ix, len(d['e1i']), len(d['e1j']), len(d['e2j']), coef[g], dt, env)
            terms.append(r['terms'])
            dE = r['dE'] if dE is None else [x + y for x, y in zip(dE, r['dE'])]
            gam = gam + r.get('gamma', 0)
            if env:
                e_t.append(r['env_terms'])
                e_dE = r['env_dE'] if e_dE is None else [x + y for x, y in zip(e_dE, r['env_dE'])]
                e_g = e_g + r.get('env_gamma', 0)
        acc[dt] = dict(terms=torch.stack(terms), dE=dE, gamma=gam, env_terms=torch.stack(e_t) if env else None, env_dE=e_dE, env_gamma=e_g)
    return dict(dd=dd, E=E, beta=beta, coef=coef, b=b, ref=acc[torch.float64], yard=acc[torch.float32])


def measure_group(M, b, valu):
    """sga_group_loss_fwd / _bwd through ops.GroupedContrastiveFn (MFMA or VALU forms): every group's raw terms, dE per table and dL/dbeta
    against the stages restricted to each group's own anchors and negatives."""
    from sgaligner_amd import ops
    from sgaligner_amd.loss_ops import GroupedContrastiveFn, LossGroups
    gr_ = group_refs(M, b)
    tier = 'valu' if valu else 'mfma'
    keep = ops.GROUP_LOSS_VALU
    ops.GROUP_LOSS_VALU = bool(valu)
    try:
        tabs = [e.cuda().requires_grad_(True) for e in gr_['E']]
        beta = gr_['beta'].cuda().requires_grad_(True) if M > 1 else None
        s = ops.IndexSets.of(gr_['dd'], tabs[0].device, int(tabs[0].shape[0]))
        gr = LossGroups.of(gr_['dd'], b, tabs[0].device)
        out = GroupedContrastiveFn.apply(s, gr, ALPHA, beta, *tabs)
        (out * gr_['coef'].cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.GROUP_LOSS_VALU = keep
    ref, yard = gr_['ref'], gr_['yard']
    yield _row('group.terms', tier, out.detach().double().cpu(), ref['terms'], ref['env_terms'], yard['terms'])
    for m in range(M):
        yield _row('group.dE', tier, tabs[m].grad, ref['dE'][m], ref['env_dE'][m], yard['dE'][m])
    if M > 1:
        yield _row('group.gamma', tier, beta.grad, ref['gamma'], ref['env_gamma'], yard['gamma'])


def wide_cases():
    return ['gauss-A33-31-65-D100-M3', 'cluster-A63-64-129-D97-M3', 'gauss-A129-21-75-D64-M3']


@functools.lru_cache(maxsize=None)
def wide_refs(name, D=136):
    c = _case_inputs(name)
    A, J1, J2 = c['A'], c['J1'], c['J2']
    z = gather(tables(c['kind'], c['T'], D, 1, c['seed'] + 900)[0], c['idx'])[0].float()
    gs = ((torch.rand(1, 8, generator=torch.Generator().manual_seed(c['seed']), dtype=torch.float64) + 0.5) * 1e-3)
    bl = {dt: [neg_blocks(z.to(dt), z.to(dt), A, J1, J2)] for dt in (torch.float64, torch.float32)}
    eb = [neg_blocks(z.double().abs(), z.double().abs(), A, J1, J2)]
    c64, _, e64, _ = neg_coefs(bl[torch.float64], gs, None, 0, A, eb)
    c32, _, _, _ = neg_coefs(bl[torch.float32], gs, None, 0, A)
    return dict(z=z, gs=gs, dZ=(neg_grad_rows(c64[0], z.double(), A, J1, J2), neg_grad_rows(e64[0], z.double(), A, J1, J2, True), neg_grad_rows(c32[0], z, A, J1, J2)))


def measure_wide(name):
    """sga_loss_neg_grad_wide on a 136-column table: everything in one block, and a stash bound that forces several anchor-row blocks."""
    lib, L, p, pa, st = _abi()
    c, w = _case_inputs(name), wide_refs(name)
    A, J1, J2 = c['A'], c['J1'], c['J2']
    R, dp = 2 * A + J1 + J2, w['z'].shape[1]
    z, g = w['z'].cuda().contiguous(), w['gs'].cuda().contiguous()
    for floats in (int(L.sga_loss_neg_grad_wide_floats(A, J1, J2)), 2 * (J1 + J2) * min(A, 32)):
        dz = torch.zeros(R, dp, device='cuda')
        stash = torch.full((floats,), NAN, device='cuda')
        lib.check(L.sga_loss_neg_grad_wide(p(z), dp, A, J1, J2, TAU[0], TAU[1], p(g), p(dz), p(stash), floats, st), 'sga_loss_neg_grad_wide')
        yield _row('neg_grad.dZ', 'wide', dz.cpu(), *w['dZ'])


# ------------------------------------------------------------------------------------------------ tier 'f16': csrc/wide16.hip and the Zh forms of the per-table A x A kernels
# Reference: the fp64 stage on what the kernel gets -- zh.double(), the tables AFTER the fp16 rounding (sga_wide16_prepare is pinned bit
# for bit on its own), the fp32 M1.  Yardstick: float32 torch restating the arithmetic csrc/wide16.hip's header states: fp32-chunked products of
# zh.float(); coefficients divided by the family's bound and rounded to fp16; M1 scaled by a power of two into [2^13, 2^14) and rounded to
# fp16.  (Against a plain-fp32 yardstick every ratio would be about 2^13 and gate nothing: hence a tier of its own.)
# (A, J1, J2, Dp) from the 256 x 256 tile, the 8-row-tile groups of the tile remap, K chunks of 64 and 16-byte K groups, 128-row anchor blocks.
F16_SHAPES = [
    dict(A=33, J1=31, J2=65, Dp=136, shards=((0, 8), (8, 24), (24, 33))),     # two K chunks, the second holding one group; shards3 moved to the 8-grid
    dict(A=129, J1=21, J2=75, Dp=192),                                        # K exactly three chunks; the wave-row split at 128
    dict(A=257, J1=40, J2=9, Dp=200, forms=('four', 'one', 'rows128', 'one128')),   # row tile edge 256 / 257; the stash-limited forms of the gradient
    dict(A=65, J1=520, J2=63, Dp=136),                                        # K = J1 > 512 in the anchors' GEMM: a K split is possible
    dict(A=24, J1=2305, J2=40, Dp=264),                                       # negatives' GEMM: 10 row tiles (groups of 8 and 2) x 2 column tiles, batched with one tile
    dict(A=2305, J1=17, J2=0, Dp=136, anchors=False),                         # S / COEF passes with 10 row tiles in ONE column of tiles; J2 = 0; no A x A epilogue (2305^2 fp64 autograd)
    dict(A=2305, J1=257, J2=0, Dp=136, anchors=False),                        # the same with two column tiles: the short group of the remap is a 2 x 2 patch
    dict(A=40, J1=33, J2=31, Dp=136, shards=((40, 40), (8, 40))),             # an empty shard at a_lo == A, and one that starts off the 32-grid
]
F16_ALL_WIDE = (200, 264)                       # the case's own table first: NT = 3, every table with a copy
F16_MIXED = (100, 136, 64, 264)                 # Zh = (NULL, zh, NULL, zh)


def f16_cases():
    C = []
    for i, s in enumerate(F16_SHAPES):
        for kind in ('gauss', 'cluster'):
            c = dict(s, kind=kind, seed=300 + 10 * i + (kind == 'cluster'))
            c['name'] = f"f16-{kind}-A{c['A']}-{c['J1']}-{c['J2']}-D{c['Dp']}"
            C.append(c)
    return C


def f16_case(name):
    return {c['name']: c for c in f16_cases()}[name]


def f16_runs(c):
    """The anchor ranges a case runs on: whole, then the shards it names."""
    return [(0, c['A'])] + list(c.get('shards', ()))


def f16_partition(c):
    """The shards a case names, completed to a partition of [0, A) (the A x A terms and dL/d(sums) are judged by the shards' sum)."""
    out, at = [], 0
    for lo, hi in sorted(c.get('shards', ())):
        if lo > at:
            out.append((at, lo))
        out.append((lo, hi))
        at = max(at, hi)
    return out + ([(at, c['A'])] if at < c['A'] else [])


def pad8(n):
    return (n + 7) // 8 * 8


def seg_cols(A, J1, J2):
    """First padded column of the segments X1 | X2 | N1 | N2 in ZhT and its pitch (csrc/wide16.hip, seg_cols)."""
    x2 = pad8(A)
    n1 = x2 + pad8(A)
    n2 = n1 + pad8(J1)
    return (0, x2, n1, n2), max(n2 + pad8(J2), 8)


def prepare_ref(z, A, J1, J2):
    """What sga_wide16_prepare makes of z [R, Dp] float32: Zh = fp16(z), round to nearest even, subnormals kept; ZhT [Dp, ldt] its transpose with
    every segment starting at a multiple of 8 columns and zeros everywhere else."""
    zh = z.to(torch.float16)
    starts, ldt = seg_cols(A, J1, J2)
    zt = torch.zeros(z.shape[1], ldt, dtype=torch.float16)
    for s0, n, c0 in zip((0, A, 2 * A, 2 * A + J1), (A, A, J1, J2), starts):
        zt[:, c0:c0 + n] = zh[s0:s0 + n].t()
    return zh, zt


def f16_bounds(gs_row):
    """The coefficient bound of each sum family, float32: 1.02 (|g0| / tau0 e^(1 / tau0) + |g1| / tau1 e^(1 / tau1))."""
    g = gs_row.double()
    e = [torch.exp(torch.tensor(1.0 / t, dtype=torch.float32)) for t in TAU]
    return [(1.02 * ((g[2 * f] / TAU[0]).float().abs() * e[0] + (g[2 * f + 1] / TAU[1]).float().abs() * e[1])).clamp_min(1e-30) for f in range(4)]


def f16_coefs(c32, bounds):
    """The four families' float32 coefficients as the matrix cores get them: c / bound rounded to fp16."""
    return [(c / b).to(torch.float16).float() for c, b in zip(c32, bounds)]


def f16_grad_rows(ch, bounds, V, A, J1, J2):
    """neg_grad_rows on the fp16 coefficients, every family's product scaled back by its bound."""
    x1, x2, n1, n2 = segments(V, A, J1, J2)
    c11, c12, c22, c21 = ch
    b11, b12, b22, b21 = bounds
    return torch.cat([b11 * mm(c11, n1.t()) + b12 * mm(c12, n2.t()), b22 * mm(c22, n2.t()) + b21 * mm(c21, n1.t()),
                      b11 * mm(c11.t(), x1.t()) + b21 * mm(c21.t(), x2.t()), b12 * mm(c12.t(), x1.t()) + b22 * mm(c22.t(), x2.t())])


def f16_stash_operand(m1):
    """(fp16(2^e M1) as float32, 2^-e): 2^e the power of two that puts the block's largest magnitude into [2^13, 2^14)."""
    amax = float(m1.abs().max()) if m1.numel() else 0.0
    if amax == 0.0:
        return m1.clone(), 1.0
    ex = math.frexp(amax)[1]
    return (m1 * 2.0 ** (14 - ex)).to(torch.float16).float(), 2.0 ** (ex - 14)


def f16_stash_rows(ds_block, zq, A, lo, hi, dt):
    """The stash products of the anchor rows [lo, hi): dX1[lo:hi] = dS[lo:hi] X2, dX2 = dS[lo:hi]^T X1[lo:hi] -> [2A, Dp] in dt; float32: on the fp16
    operand of f16_stash_operand, K walked in chunks of 32."""
    out = torch.zeros(2 * A, zq.shape[1], dtype=dt)
    x1, x2 = zq[lo:hi].to(dt), zq[A:2 * A].to(dt)
    if dt == torch.float64:
        out[lo:hi] = ds_block.double() @ x2
        out[A:] = ds_block.double().t() @ x1
    else:
        mh, back = f16_stash_operand(ds_block)
        out[lo:hi] = G.yardstick(mh, x2.t().contiguous()) * back
        out[A:] = G.yardstick(mh.t().contiguous(), x1.t().contiguous()) * back
    return out


@functools.lru_cache(maxsize=None)
def f16_inputs(name):
    c = f16_case(name)
    A, J1, J2, Dp = c['A'], c['J1'], c['J2'], c['Dp']
    idx, T = index_sets(A, J1, J2, c['seed'])
    z = gather(tables(c['kind'], T, Dp, 1, c['seed'])[0], idx)[0].float()
    zh, zt = prepare_ref(z, A, J1, J2)
    g = torch.Generator().manual_seed(c['seed'])
    gs = (torch.rand(1, 8, generator=g, dtype=torch.float64) + 0.5) * 1e-3
    return dict(c, idx=idx, T=T, z=z, zh=zh, zt=zt, gs=gs, R=2 * A + J1 + J2)


@functools.lru_cache(maxsize=None)
def f16_anchor_refs(name, mixed):
    """The A x A stage of a case's anchors on NT tables: all wide (the case's own table and two more, every one with a copy) or the mixed set
    (Zh = (NULL, zh, NULL, zh)).  S of a table with a copy is formed from its fp16 rounding, of the others from the float32 rows."""
    c = f16_inputs(name)
    A, J1, J2 = c['A'], c['J1'], c['J2']
    if mixed:
        widths, Z = F16_MIXED, []
    else:
        widths, Z = F16_ALL_WIDE, [c['z']]
    for k, w in enumerate(widths):
        Z.append(gather(tables(c['kind'], c['T'], w, 1, c['seed'] + 40 * (k + 1) + int(mixed))[0], c['idx'])[0].float())
    copy = [z.shape[1] > 128 for z in Z]
    Zq = [z.to(torch.float16).float() if h else z for z, h in zip(Z, copy)]
    nt = len(Z)
    coef = ((torch.rand(nt + 2 * (nt - 1), generator=torch.Generator().manual_seed(c['seed'] + 1)) + 0.5) * 1e-2).float()
    bl = [neg_blocks(z.double(), z.double(), A, J1, J2) for z in Zq]
    eb = [neg_blocks(z.double().abs(), z.double().abs(), A, J1, J2) for z in Zq]
    sums, esum = neg_sums(bl, 0, A), neg_sums_envelope(bl, eb, 0, A)
    sums = sums.clamp_min(1.0)                             # (J2 == 0 never gets here; any positive numbers of the right size would do)
    S64 = [mm(z[:A].double(), z[A:2 * A].double()) for z in Zq]
    eS = [mm(z[:A].double().abs(), z[A:2 * A].double().abs()) for z in Zq]
    ref = anchor_stage(S64, None, sums, ALPHA, coef, eS=eS, esum=esum)
    yard = anchor_stage([mm(z[:A], z[A:2 * A]) for z in Zq], None, sums, ALPHA, coef, dt=torch.float32)
    return dict(Z=Z, copy=copy, coef=coef, sums=sums, ref=ref, yard=yard)


def f16_m1(name):
    """dL/dS [A, A] float32 the stash products are handed: the A x A reference's for the case's own table; without an A x A stage a matrix of the
    same make, signed coefficients exp(S / tau0) of the case's own similarities."""
    c = f16_inputs(name)
    A = c['A']
    if c.get('anchors', True):
        return f16_anchor_refs(name, False)['ref']['dS'][0].float()
    zq = c['zh'].float()
    sgn = torch.randint(0, 2, (A, A), generator=torch.Generator().manual_seed(c['seed'] + 2)).float() * 2.0 - 1.0
    return 1e-4 * sgn * torch.exp(mm(zq[:A], zq[A:2 * A]) / TAU[0])


@functools.lru_cache(maxsize=None)
def f16_refs(name):
    """Sums, negatives' gradient and stash products of a case, per anchor range: (fp64 reference, envelope, float32 yardstick)."""
    c = f16_inputs(name)
    A, J1, J2 = c['A'], c['J1'], c['J2']
    zq = c['zh'].float()
    z64 = zq.double()
    bl = {dt: [neg_blocks(zq.to(dt), zq.to(dt), A, J1, J2)] for dt in (torch.float64, torch.float32)}
    eb = [neg_blocks(z64.abs(), z64.abs(), A, J1, J2)]
    bounds = f16_bounds(c['gs'][0])
    m1 = f16_m1(name)
    out = dict(m1=m1, bounds=bounds)
    for lo, hi in f16_runs(c):
        r = {}
        r['sums'] = (neg_sums(bl[torch.float64], lo, hi)[0], neg_sums_envelope(bl[torch.float64], eb, lo, hi)[0], neg_sums(bl[torch.float32], lo, hi)[0])
        c64, _, e64, _ = neg_coefs(bl[torch.float64], c['gs'], None, lo, hi, eb)
        c32, _, _, _ = neg_coefs(bl[torch.float32], c['gs'], None, lo, hi)
        r['c32'] = c32[0]
        r['dZ'] = (neg_grad_rows(c64[0], z64, A, J1, J2), neg_grad_rows(e64[0], z64, A, J1, J2, True),
                   f16_grad_rows(f16_coefs(c32[0], bounds), bounds, zq, A, J1, J2))
        blk = m1[lo:hi]
        env = torch.zeros(2 * A, zq.shape[1], dtype=torch.float64)
        env[lo:hi] = blk.double().abs() @ z64[A:2 * A].abs()
        env[A:] = blk.double().abs().t() @ z64[lo:hi].abs()
        r['stash'] = (f16_stash_rows(blk, zq, A, lo, hi, torch.float64), env, f16_stash_rows(blk, zq, A, lo, hi, torch.float32))
        out[(lo, hi)] = r
    return out


def f16_defect(name, defect):
    """A CPU emulation of a wide16 kernel with a seeded defect, on the whole anchor range: (output key, out, ref, env, yard), or None where the
    defect has nothing to act on.
    'k_group'   S without the last 8-column K group of the table (columns 128 .. 135 of 136), in the sums;
    'last_row'  the negatives' gradient without the last anchor row of the row block (the C^T products lose their last K index);
    'straddle'  the straddling K group of the C^T products not zeroed: the column behind the block's last anchor holds a copy of that anchor's
                coefficients and meets the next packed row of the table (A % 8 == 0: no group straddles)."""
    c, fr = f16_inputs(name), f16_refs(name)
    A, J1, J2, Dp = c['A'], c['J1'], c['J2'], c['Dp']
    r = fr[(0, A)]
    zq = c['zh'].float()
    if defect == 'k_group':
        cut = zq[:, :Dp - 8]
        return ('neg_sums.sums|f16', neg_sums([neg_blocks(cut, cut, A, J1, J2)], 0, A)[0]) + r['sums']
    ch = f16_coefs(r['c32'], fr['bounds'])
    ref, env, yard = r['dZ']
    bad = yard.clone()
    b11, b12, b22, b21 = fr['bounds']
    c11, c12, c22, c21 = ch
    x1, x2, _, _ = segments(zq, A, J1, J2)
    if defect == 'last_row':
        sign, row1, row2 = -1.0, x1[A - 1], x2[A - 1]
    else:
        if A % 8 == 0:
            return None
        sign, row1, row2 = 1.0, zq[A], zq[2 * A]           # the packed rows behind the last X1 / X2 anchor
    n1, n2 = slice(2 * A, 2 * A + J1), slice(2 * A + J1, 2 * A + J1 + J2)
    bad[n1] += sign * (b11 * c11[A - 1][:, None] * row1[None, :] + b21 * c21[A - 1][:, None] * row2[None, :])
    bad[n2] += sign * (b12 * c12[A - 1][:, None] * row1[None, :] + b22 * c22[A - 1][:, None] * row2[None, :])
    return 'neg_grad.dZ|f16', bad, ref, env, yard


# ---- launches (GPU)
def run_prepare(z, A, J1, J2):
    """sga_wide16_prepare on z [R, Dp] float32: (Zh, ZhT) on the device, both pre-filled with NaN."""
    lib, L, p, _, st = _abi()
    zc = z.cuda().contiguous()
    R, Dp = zc.shape
    ldt = int(L.sga_wide16_ldt(A, J1, J2))
    zh = torch.full((max(R, 1), Dp), NAN, device='cuda', dtype=torch.float16)
    zt = torch.full((Dp, ldt), NAN, device='cuda', dtype=torch.float16)
    lib.check(L.sga_wide16_prepare(p(zc), Dp, A, J1, J2, p(zh), p(zt), st), 'sga_wide16_prepare')
    return zh, zt


@functools.lru_cache(maxsize=2)
def f16_device(name):
    """A case's fp16 operands as the library makes them -- and they are prepare_ref's, bit for bit: the references stand on zh.double()."""
    c = f16_inputs(name)
    zh, zt = run_prepare(c['z'], c['A'], c['J1'], c['J2'])
    assert torch.equal(zh.cpu(), c['zh']) and torch.equal(zt.cpu(), c['zt']), 'sga_wide16_prepare differs from prepare_ref'
    return zh, zt


def f16_stash_forms(c):
    """(label, bytes) of the coefficient stash sga_loss_neg_grad_f16 is given: 'four' holds four stash pairs of all anchors (the families share
    their launches); 'one' a single pair of all anchors (family by family); 'rows128' four pairs of 128 rows and 'one128' one pair of 128 rows
    (several anchor-row blocks)."""
    L = _abi()[1]
    need = lambda r: int(L.sga_loss_neg_grad_f16_bytes(r, c['J1'], c['J2'])) // 4
    size = {'four': 4 * need(c['A']), 'one': need(c['A']), 'rows128': 4 * need(128), 'one128': need(128)}
    return [(f, size[f]) for f in c.get('forms', ('four',))]


def _outside_zero(out, A, lo, hi, what):
    """Anchor rows of X1 / X2 outside the shard hold no gradient of it."""
    for s0 in (0, A):
        rows = torch.cat([out[s0:s0 + lo], out[s0 + hi:s0 + A]])
        assert not rows.any(), f'{what}: anchor rows outside [{lo}, {hi}) written'


def measure_f16_sums(name):
    lib, L, p, _, st = _abi()
    c, fr = f16_inputs(name), f16_refs(name)
    zh, _ = f16_device(name)
    for lo, hi in f16_runs(c):
        buf = torch.full((_slots() * 8,), NAN, device='cuda', dtype=torch.float64)
        lib.check(L.sga_loss_neg_sums_f16(p(zh), c['Dp'], c['A'], c['J1'], c['J2'], TAU[0], TAU[1], p(buf), lo, hi, st), 'sga_loss_neg_sums_f16')
        out = buf[:8].cpu()
        if hi == lo:
            assert torch.equal(out, torch.zeros(8, dtype=torch.float64)), 'sums of an empty shard'
        yield _row('neg_sums.sums', 'f16', out, *fr[(lo, hi)]['sums'])


def measure_f16_grad(name):
    lib, L, p, _, st = _abi()
    c, fr = f16_inputs(name), f16_refs(name)
    zh, zt = f16_device(name)
    A, R, Dp = c['A'], c['R'], c['Dp']
    g = c['gs'].cuda().contiguous()
    for form, nbytes in f16_stash_forms(c):
        for lo, hi in f16_runs(c):
            dz = torch.zeros(R, Dp, device='cuda')
            stash = torch.full((nbytes,), 255, device='cuda', dtype=torch.uint8)          # (0xffff: an fp16 NaN)
            lib.check(L.sga_loss_neg_grad_f16(p(zh), p(zt), Dp, A, c['J1'], c['J2'], TAU[0], TAU[1], p(g), p(dz), p(stash), nbytes, lo, hi, st),
                      'sga_loss_neg_grad_f16')
            out = dz.cpu()
            _outside_zero(out, A, lo, hi, f'{name} {form}')
            if hi == lo:
                assert not out.any(), 'gradient of an empty shard'
            yield _row('neg_grad.dZ', 'f16', out, *fr[(lo, hi)]['dZ'])


def measure_f16_stash(name):
    lib, L, p, _, st = _abi()
    c, fr = f16_inputs(name), f16_refs(name)
    _, zt = f16_device(name)
    A, R, Dp = c['A'], c['R'], c['Dp']
    for lo, hi in f16_runs(c):
        dz = torch.zeros(R, Dp, device='cuda')
        m1 = fr['m1'][lo:hi].t().contiguous().cuda() if hi > lo else torch.zeros(4, device='cuda')
        nbytes = int(L.sga_loss_stash_grad_f16_bytes(A, hi - lo))
        ws = torch.full((nbytes,), 255, device='cuda', dtype=torch.uint8)
        lib.check(L.sga_loss_stash_grad_f16(p(m1), p(zt), Dp, A, c['J1'], c['J2'], p(dz), lo, hi, p(ws), nbytes, st), 'sga_loss_stash_grad_f16')
        out = dz.cpu()
        assert not out[2 * A:].any(), 'stash products in the negatives\' rows'
        assert not out[:lo].any() and not out[hi:A].any(), 'stash products in X1 rows outside the shard'       # (every X2 row is written)
        if hi == lo:
            assert not out.any(), 'stash products of an empty shard'
        yield _row('stash_grad.dZ', 'f16', out[:2 * A], *fr[(lo, hi)]['stash'])


def measure_f16_anchor(name, mixed, use_ws):
    """sga_loss_anchor_fwd_f16 / _bwd_f16 with fp16 copies: the K-loop form (ws = NULL) or the workspace form (similarity blocks first), on
    the all-wide or the mixed table set, per anchor range."""
    import ctypes
    lib, L, p, pa, st = _abi()
    c, ar = f16_inputs(name), f16_anchor_refs(name, mixed)
    A, R = c['A'], c['R']
    nt = len(ar['Z'])
    n = nt + 2 * (nt - 1)
    dps = [pad8(z.shape[1]) for z in ar['Z']]
    zs, zhs = [], []
    for z, dp, h in zip(ar['Z'], dps, ar['copy']):
        t = torch.zeros(R + 32, dp)
        t[:R, :z.shape[1]] = z
        zs.append(t.cuda())
        zhs.append(run_prepare(t[:R], A, c['J1'], c['J2'])[0] if h else None)
    dparr = (ctypes.c_int * nt)(*dps)
    sums, cf = ar['sums'].cuda().contiguous(), ar['coef'].cuda()
    ref, yard = ar['ref'], ar['yard']
    tot = lambda key, d: d[key].sum(-1)
    for parts in [[(0, A)]] + ([f16_partition(c)] if c.get('shards') else []):
        terms, gs = torch.zeros(n, dtype=torch.float64), torch.zeros(nt, 8, dtype=torch.float64)
        for lo, hi in parts:
            ns = hi - lo
            nbytes = int(L.sga_loss_anchor_f16_ws_bytes(nt, A, max(ns, 1))) if use_ws else 0
            ws = torch.full((nbytes,), 255, device='cuda', dtype=torch.uint8) if use_ws else None
            out = torch.full((_slots() * n,), NAN, device='cuda', dtype=torch.float64)
            lib.check(L.sga_loss_anchor_fwd_f16(pa(zs), pa(zhs), dparr, nt, A, p(sums), ALPHA, TAU[0], TAU[1], p(out), lo, hi, p(ws), nbytes, st), 'sga_loss_anchor_fwd_f16')
            m1 = [torch.full((A * max(ns, 1),), NAN, device='cuda') for _ in range(nt)]
            gsc = torch.full((_slots() + 1, nt, 8), NAN, device='cuda', dtype=torch.float64)
            lib.check(L.sga_loss_anchor_bwd_f16(pa(zs), pa(zhs), dparr, nt, A, p(sums), ALPHA, TAU[0], TAU[1], p(cf), pa(m1), p(gsc), lo, hi, p(ws), nbytes, st),
                      'sga_loss_anchor_bwd_f16')
            if ns == 0:
                assert not out[:n].any() and not gsc[0].any(), 'terms or dL/d(sums) of an empty shard'
                assert all(bool(torch.isnan(m).all()) for m in m1), 'a stash written by an empty shard'
            terms += out[:n].cpu()
            gs += gsc[0].cpu()
            for k in range(nt if ns else 0):
                yield _row('anchor_coef.dS', 'f16', m1[k].view(A, ns).t().cpu(), ref['dS'][k][lo:hi], ref['env_dS'][k][lo:hi], yard['dS'][k][lo:hi])
        # (a shard's share of a term or of dL/d(sums) is the kernel's own split -- the B direction rides with S[i, j], not with row i -- and
        # is all-reduced: the shards are judged by their sum)
        yield _row('anchor_terms.terms', 'f16', terms, tot('terms_rows', ref), tot('env_terms_rows', ref), tot('terms_rows', yard))
        yield _row('anchor_coef.gs', 'f16', gs, tot('gs_rows', ref), tot('env_gs_rows', ref), tot('gs_rows', yard))


def measure_f16(name):
    """Every gated stage of a case in the tier 'f16'."""
    yield from measure_f16_sums(name)
    yield from measure_f16_grad(name)
    yield from measure_f16_stash(name)
    if f16_case(name).get('anchors', True):
        for mixed in (False, True):
            for use_ws in (False, True):
                yield from measure_f16_anchor(name, mixed, use_ws)
