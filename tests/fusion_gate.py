"""The exact (lattice) and fp32-faithful (gate) checks of the fusion kernels (csrc/fusion.hip) and of the three element-wise kernels
(sga_elu_fwd / sga_elu_bwd / sga_relu_bwd), and the inputs tests and profile share (no tests in this module).  Metric and convention are those
of gemm_gate / pointnet_gate / eva_gate.

Reference.  The module's own text, joint = cat_m softmax(weight)[m] * x_m / max(||x_m||, 1e-12), in fp64 torch with gradients by fp64 autograd.

Yardstick.  The same text in float32 torch on the CPU -- never the library.

Lattice.  Row t of table m holds exactly 4^j non-zero entries +-2^e (j uniform over the values with 4^j <= D_m, at most 3; e uniform in
[-3, 3]; random places and signs), all fusion weights are one common value and the cotangent is integer-valued in [-2, 2].  For M in
{1, 2, 4, 8} every quantity is then a small dyadic number -- the softmax weight 1 / M, every norm 2^(j+e), every scale, x . g, c1 g - c2 x, the
sums a_m (a row adds a multiple of 1/8 of at most 16: no partial sum of fewer than 2^17 rows leaves float32's integers) and the weight
gradient -- so any correct evaluation, contracted or not, in any order, gives the reference bit for bit.  The builder asserts that every fp64
reference value round-trips through float32.  All-zero rows are not part of the family (their gradient w g / 1e-12 may round differently in two correct evaluations).

Gate inputs.  Gaussian rows at norms spread over 1e-3 .. 1e3; on every third row the cotangent's component along x is removed to within 2^-10
of |g| (the cancellation c1 g - c2 x lives on); on every fifth row (that is no third one) the cotangents are scaled so that the a_m = sum_t
g . xhat of all tables agree to within 1 % (the cancellation a_m - sum_k w_k a_k of the softmax Jacobian lives on); weights from N(0, 1); two
all-zero rows, whose output must be exactly 0 and whose gradient is judged as test_linear_fusion_gpu.py::test_fusion_zero_row_and_large judges
it -- they are left out of the enveloped comparison, and never more than ZERO_ROWS_MAX rows are.

Metric.  gemm_gate.rel_errors, |out - ref| / envelope in u = 2^-24, with xhat = x / n:
    out   |ref|
    gx    (w_m / n) (|g| + |xhat| sum_d |xhat_d| |g_d|)
    gw    w_m (A_m + sum_k w_k A_k),  A_m = sum_t sum_d |g| |xhat|

Gate.  eva_gate.gate_ok at r per output from profiles/fusion_accuracy_vs_fp32.json (tools/fusion_accuracy.py writes it on the card):
r = ceil(2 x the worst measured kernel / yardstick ratio, rms or max); the factor 2 is for seeds and for the order of the wave reduction
against the CPU's.  No r may exceed R_CAP (a condition, not a measurement).  tests/test_fusion_gate_cpu.py keeps table and profile together
and shows that four emulated defects fail both checks.

Element-wise.  ELU for x <= 0 is judged in ulps of the fp64 result (expm1(x); gy exp(x)) on stratified inputs -- +-0, -2^k (1 + i / 64) for
k in [-40, 6], -inf -- next to torch's float32 F.elu on the CPU; the bound per kernel is ceil(2 x the worst figure measured on the card) ulps
(the profile's 'elementwise' key) and may not exceed ULP_CAP.  Everything else about the three kernels is exact."""
import functools
import json
import math
import os

import torch
import torch.nn.functional as F

import eva_gate as EG
import gemm_gate as G

ROOT = G.ROOT
PROFILE = os.path.join(ROOT, 'profiles', 'fusion_accuracy_vs_fp32.json')
FU_MAXM = 8
WAVES_PER_CU = 32                        # rows of one pass of the row loop per CU: 8 workgroups of four waves (fusion.hip: grid_for_rows)
CUS_MI355X = 256                         # the CPU self-tests build the inputs the GPU tests build on a 256-CU card
OUTPUTS = ('out', 'gx', 'gw')
R_CAP = 8
ULP_CAP = 4
ZERO_ROWS_MAX = 2

LATTICE_MS = (1, 2, 4, 8)
LATTICE_DS = (1, 3, 63, 64, 65, 100, 257)
LATTICE_BIG_DS = (3, 65)                 # the widths that also run at the row counts around one pass of the row loop
LATTICE_VAR_WIDTHS = ((1, 64, 65, 257), (400, 200, 100, 100), (1, 2, 3, 4, 5, 6, 7, 8))
GATE_MS = (1, 2, 3, 5, 7, 8)
RAGGED = (65, 257, 3, 100, 64, 130, 7, 33)       # the ragged mix of the gate: its first M widths

# r per output: ceil(2 x the worst ratio measured, rms or max) over the cases of profiles/fusion_accuracy_vs_fp32.json.
R = {'out': 5, 'gx': 5, 'gw': 6}
# ulps per kernel: ceil(2 x the worst error measured on the card), the profile's 'elementwise' rows.
ULP = {'elu_fwd': 2, 'elu_bwd': 3}


def ratios_from_profile(path=PROFILE):
    """output -> ceil(2 x worst measured kernel / yardstick ratio), the derivation R states."""
    worst = {}
    for c in json.load(open(path))['cases']:
        worst[c['output']] = max(worst.get(c['output'], 0.0), c['ratio_rms'], c['ratio_max'])
    return {k: int(math.ceil(2.0 * v - 1e-9)) for k, v in worst.items()}


def ulps_from_profile(path=PROFILE):
    """kernel -> ceil(2 x worst measured error in ulps), the derivation ULP states."""
    worst = {}
    for c in json.load(open(path))['elementwise']:
        worst[c['kernel']] = max(worst.get(c['kernel'], 0.0), c['kernel_ulp'])
    return {k: int(math.ceil(2.0 * v - 1e-9)) for k, v in worst.items()}


def rows_per_pass(cus=CUS_MI355X):
    """P: the rows one pass of the four row kernels' grid-stride loop covers."""
    return WAVES_PER_CU * int(cus)


def device_rows_per_pass():
    from sgaligner_amd import _lib
    return rows_per_pass(_lib.lib().sga_device_cus())


# ------------------------------------------------------------------------------------------------ reference, yardstick, emulation
def fusion_text(weight, tabs):
    """MultiModalFusion.forward as the module writes it, in the dtype of its arguments."""
    w = F.softmax(weight, dim=0)
    return torch.cat([w[m] * F.normalize(t) for m, t in enumerate(tabs)], dim=1)


def evaluate(weight, tabs, gj, dtype):
    """(out, gx [T, sum D], gw [M]) of the module text in `dtype` on the CPU, gradients by autograd."""
    w = weight.detach().to(dtype).requires_grad_(True)
    xs = [t.detach().to(dtype).requires_grad_(True) for t in tabs]
    out = fusion_text(w, xs)
    grads = torch.autograd.grad(out, [w] + xs, gj.to(dtype))
    return out.detach(), torch.cat(grads[1:], dim=1), grads[0].reshape(-1)


DEFECTS = ('tail', 'c2', 'jacobian', 'rows')


def emulate(weight, tabs, gj, defect=None, P=None):
    """The kernels' formulas in float32 torch on the CPU (a_m summed in fp64, as the kernels do), with one defect:
    'tail'     the norm without the columns past the last full 64 (tables with D > 64 and D % 64 != 0)
    'c2'       gx without the c2 term
    'jacobian' gw without - sum_k w_k a_k
    'rows'     rows >= P left unwritten (zero here) and out of the sums a_m
    None is the faithful text: the CPU tests assert that it equals the lattice bit for bit and passes the gate."""
    w = F.softmax(weight.float(), dim=0).reshape(-1)
    outs, gxs, a = [], [], []
    off = 0
    for m, x in enumerate(tabs):
        x = x.float()
        D = x.shape[1]
        g = gj[:, off:off + D].float()
        off += D
        xs = x[:, :D // 64 * 64] if defect == 'tail' and D > 64 and D % 64 else x
        n = xs.pow(2).sum(1, keepdim=True).sqrt()
        inv = 1.0 / n.clamp_min(1e-12)
        dot = (x * g).sum(1, keepdim=True) * inv
        c2 = torch.where(n < 1e-12, torch.zeros_like(n), w[m] * dot * inv * inv)
        if defect == 'c2':
            c2 = torch.zeros_like(c2)
        out, gx = x * (w[m] * inv), (w[m] * inv) * g - c2 * x
        if defect == 'rows':
            out[P:], gx[P:], dot = 0.0, 0.0, dot[:P]
        outs.append(out)
        gxs.append(gx)
        a.append(dot.double().sum())
    a = torch.stack(a)
    wd = w.double()
    gw = wd * a if defect == 'jacobian' else wd * (a - (wd * a).sum())
    return torch.cat(outs, dim=1), torch.cat(gxs, dim=1), gw.float()


def run(weight, tabs, gj, route='auto'):
    """The kernels on the card: (out, gx [T, sum D], gw [M]) on the host.  route: 'equal' (ops.FusionFn), 'var' (ops.FusionVarFn), 'auto'
    (ops.fusion)."""
    from sgaligner_amd import ops
    w = weight.float().cuda().requires_grad_(True)
    xs = [t.float().cuda().requires_grad_(True) for t in tabs]
    out = {'equal': ops.FusionFn.apply, 'var': ops.FusionVarFn.apply, 'auto': lambda w_, *e: ops.fusion(w_, list(e))}[route](w, *xs)
    grads = torch.autograd.grad(out, [w] + xs, gj.float().cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), torch.cat([g.cpu() for g in grads[1:]], dim=1), grads[0].reshape(-1).cpu()


# ------------------------------------------------------------------------------------------------ the exact family
def _seed(T, widths, seed):
    return (1000003 * seed + 7919 * T + 31 * sum(widths) + len(widths)) % (2 ** 31)


@functools.lru_cache(maxsize=4)
def lattice(T, widths, seed=0, common=0.7):
    """dict(weight [M, 1], tabs, gj, out, gx, gw): the exact family (module docstring) with its fp64 reference; out / gx / gw are float32
    tensors that hold the reference's values exactly."""
    widths = tuple(int(d) for d in widths)
    M = len(widths)
    assert M in LATTICE_MS, 'the softmax weight 1 / M must be dyadic'
    gen = torch.Generator().manual_seed(_seed(T, widths, seed))
    tabs = []
    for D in widths:
        jmax = max(j for j in range(4) if 4 ** j <= D)
        count = 4 ** torch.randint(0, jmax + 1, (T, 1), generator=gen)
        places = torch.rand(T, D, generator=gen).argsort(dim=1)                       # a random permutation of the columns per row
        mask = torch.zeros(T, D).scatter_(1, places, (torch.arange(D)[None, :] < count).float())
        sign = torch.randint(0, 2, (T, D), generator=gen).float() * 2 - 1
        e = torch.randint(-3, 4, (T, 1), generator=gen)
        tabs.append(mask * sign * torch.ldexp(torch.ones(T, 1), e))
    gj = torch.randint(-2, 3, (T, sum(widths)), generator=gen).float()
    weight = torch.full((M, 1), float(common))
    ref = evaluate(weight, tabs, gj, torch.float64)
    for r in ref:
        assert torch.equal(r.float().double(), r), 'a reference value of the lattice is no float32 number: narrow the cotangent'
    out, gx, gw = [r.float() for r in ref]
    return dict(weight=weight, tabs=tabs, gj=gj, out=out, gx=gx, gw=gw)


def assert_lattice_equal(got, lat, what=''):
    """Bit-equality (as numbers: +0 and -0 are one value) of (out, gx, gw) with the lattice's reference."""
    bad = [k for k, g in zip(OUTPUTS, got) if g.shape != lat[k].shape or not torch.equal(g, lat[k])]
    assert not bad, (what, bad, [(g - lat[k]).abs().max().item() for k, g in zip(OUTPUTS, got) if g.shape == lat[k].shape])


def lattice_equal(got, lat):
    return all(g.shape == lat[k].shape and torch.equal(g, lat[k]) for k, g in zip(OUTPUTS, got))


# ------------------------------------------------------------------------------------------------ the gate
def judge_inputs(weight, tabs, gj):
    """dict(ref, env, keep, zero) for any inputs: the fp64 reference of (out, gx, gw), their envelopes, the rows that are compared (a row with
    an all-zero table row is not) and the (table, row) pairs of the all-zero rows."""
    w = F.softmax(weight.double(), dim=0).reshape(-1)
    ref = dict(zip(OUTPUTS, evaluate(weight, tabs, gj, torch.float64)))
    T = tabs[0].shape[0]
    keep = torch.ones(T, dtype=torch.bool)
    zero, e_gx, A = [], [], []
    off = 0
    for m, x in enumerate(tabs):
        x = x.double()
        D = x.shape[1]
        g = gj[:, off:off + D].double().abs()
        off += D
        n = x.norm(dim=1, keepdim=True)
        for t in torch.nonzero(n.reshape(-1) == 0).reshape(-1).tolist():
            zero.append((m, t))
            keep[t] = False
        xh = (x / n.clamp_min(1e-12)).abs()
        e_gx.append(w[m] / n.clamp_min(1e-12) * (g + xh * (xh * g).sum(1, keepdim=True)))
        A.append((g * xh).sum())
    A = torch.stack(A)
    assert int((~keep).sum()) <= ZERO_ROWS_MAX, 'more rows left out of the comparison than the gate family has all-zero rows'
    env = dict(out=ref['out'].abs(), gx=torch.cat(e_gx, dim=1), gw=w * (A + (w * A).sum()))
    return dict(ref=ref, env=env, keep=keep, zero=zero, widths=tuple(int(t.shape[1]) for t in tabs), w=w)


def errors(got, judged):
    """output -> gemm_gate.rel_errors of (out, gx, gw) on the rows compared."""
    keep, ref, env = judged['keep'], judged['ref'], judged['env']
    out, gx, gw = [g.detach().cpu() for g in got]
    return dict(out=G.rel_errors(out[keep], ref['out'][keep], env['out'][keep]), gx=G.rel_errors(gx[keep], ref['gx'][keep], env['gx'][keep]),
                gw=G.rel_errors(gw.reshape(-1), ref['gw'], env['gw']))


def zero_rows_ok(got, judged, gj):
    """The all-zero rows: the output exactly 0, the gradient w g / 1e-12 within 1e-4 of the reference's, relative to max(|ref|, 1) (the check
    and the bound of test_linear_fusion_gpu.py::test_fusion_zero_row_and_large)."""
    out, gx = got[0].detach().cpu(), got[1].detach().cpu()
    offs = [0]
    for d in judged['widths']:
        offs.append(offs[-1] + d)
    ok = True
    for m, t in judged['zero']:
        sl = slice(offs[m], offs[m + 1])
        ref = judged['ref']['gx'][t, sl]
        err = ((gx[t, sl].double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
        ok = ok and bool((out[t, sl] == 0).all()) and err < 1e-4
    return ok


def assert_gate(meas, what=''):
    """meas: output -> (kernel errors, yardstick errors); every figure is printed before it is judged."""
    bad = []
    for k, (ke, ye) in meas.items():
        print(f'[fusion gate] {what} {k}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {R[k]}')
        if not EG.gate_ok(ke, ye, R[k]):
            bad.append((k, ke, ye, R[k]))
    assert not bad, (what, bad)


def ratio(kernel, yard):
    """(max ratio, rms ratio) kernel / yardstick as the profile records them.  A single-entry output: eva_gate.ratio (the yardstick floored
    at FLOOR_U, as its gate is).  Otherwise a max up to FLOOR_U, which gate_ok admits whatever r is, asks for no r and counts as 0."""
    if kernel[2] <= 1:
        return EG.ratio(kernel, yard)
    assert yard[1] > 0 or kernel[1] == 0, 'an exact yardstick: the case measures nothing'
    return (0.0 if kernel[0] <= G.FLOOR_U else kernel[0] / yard[0]), (kernel[1] / yard[1] if kernel[1] > 0 else 0.0)


def measure(got, weight, tabs, gj, judged=None):
    """output -> (kernel errors, yardstick errors) of `got` = (out, gx, gw) on these inputs."""
    judged = judged or judge_inputs(weight, tabs, gj)
    ke, ye = errors(got, judged), errors(evaluate(weight, tabs, gj, torch.float32), judged)
    return {k: (ke[k], ye[k]) for k in OUTPUTS}


def gate_widths(M, kind):
    return (100,) * M if kind == 'equal' else RAGGED[:M]


def gate_cases(P):
    """(name, T, widths) of every gate case for a card whose row loop covers P rows a pass."""
    return [(f'M{M}-{kind}-T{T}', T, gate_widths(M, kind)) for M in GATE_MS for kind in ('equal', 'ragged') for T in (33, P + 1)]


@functools.lru_cache(maxsize=2)
def gate_case(T, widths, seed=0):
    """dict(weight, tabs, gj, judged): the gate family (module docstring)."""
    widths = tuple(int(d) for d in widths)
    M = len(widths)
    assert T >= 11 and 1 <= M <= FU_MAXM
    gen = torch.Generator().manual_seed(_seed(T, widths, seed) + 1)
    rows = torch.arange(T)
    third = rows % 3 == 0
    fifth = (rows % 5 == 0) & ~third
    free = torch.nonzero(~third & (rows % 5 != 0)).reshape(-1)
    zero = ((0, int(free[0])), (M - 1, int(free[-1])))
    tabs, gs, xhs = [], [], []
    for m, D in enumerate(widths):
        x = torch.randn(T, D, generator=gen, dtype=torch.float64)
        x = x / x.norm(dim=1, keepdim=True) * 10.0 ** (torch.rand(T, 1, generator=gen, dtype=torch.float64) * 6 - 3)
        for zm, zt in zero:
            if zm == m:
                x[zt] = 0.0
        x = x.float()
        xh = F.normalize(x.double())
        g = torch.randn(T, D, generator=gen, dtype=torch.float64)
        dot = (g * xh).sum(1, keepdim=True)
        perp = g - dot * xh
        side = torch.randint(0, 2, (T, 1), generator=gen).double() * 2 - 1
        g = torch.where(third[:, None], perp + 2.0 ** -10 * perp.norm(dim=1, keepdim=True) * side * xh, g)
        g = torch.where(fifth[:, None] & (dot < 0), -g, g)                              # every fifth row pulls a_m the same way
        tabs.append(x)
        gs.append(g)
        xhs.append(xh)
    a = torch.stack([(g * xh).sum() for g, xh in zip(gs, xhs)])
    b = torch.stack([(g * xh)[fifth].sum() for g, xh in zip(gs, xhs)])
    assert (b > 0).all()
    rest = a - b
    target = (rest.max() + b.max()) * (1 + 0.005 * (torch.rand(M, generator=gen, dtype=torch.float64) * 2 - 1))
    for m in range(M):
        gs[m][fifth] *= (target[m] - rest[m]) / b[m]
    gj = torch.cat(gs, dim=1).float()
    weight = torch.randn(M, 1, generator=gen)
    # the family's three properties, on the float32 numbers the kernels see
    off = 0
    a32 = []
    for m, D in enumerate(widths):
        g = gj[:, off:off + D].double()
        off += D
        dots = (g * xhs[m]).sum(1)
        if D > 1:
            assert (dots[third].abs() <= 2.0 ** -9 * g.norm(dim=1)[third]).all()
        a32.append(dots.sum())
    a32 = torch.stack(a32)
    assert (a32.max() - a32.min()) <= 0.01 * a32.abs().min(), 'the a_m of the tables do not agree to within 1 %'
    judged = judge_inputs(weight, tabs, gj)
    assert sorted(judged['zero']) == sorted(set(zero)) and int((~judged['keep']).sum()) == len({t for _, t in zero})
    return dict(weight=weight, tabs=tabs, gj=gj, judged=judged)


def large_inputs():
    """The inputs of test_linear_fusion_gpu.py::test_fusion_zero_row_and_large: (weight, tabs, cotangent)."""
    torch.manual_seed(0)
    embs = [torch.randn(5000, 100) for _ in range(3)]
    embs[1][17] = 0.0                                    # F.normalize eps branch
    w = torch.tensor([[0.3], [1.2], [-0.4]])
    cot = torch.randn(5000, 300)
    return w, embs, cot


# ------------------------------------------------------------------------------------------------ element-wise kernels
EW_SIZES = (1, 255, 256, 257, 2097152, 2097153, 2097152 + 65793)
EW_STRIDE = 8192 * 256                   # elements of one trip of the three kernels' grid-stride loop
ELU_GY = (1.0, -3.0, 2.0 ** -20)


def elu_strata():
    """The x <= 0 of the ELU tests: +-0, -2^k (1 + i / 64) for k in [-40, 6] and i in [0, 63], -inf (float32, 3011 values)."""
    k = torch.arange(-40, 7, dtype=torch.float64)[:, None]
    i = torch.arange(64, dtype=torch.float64)[None, :]
    neg = -(2.0 ** k * (1 + i / 64)).reshape(-1)
    return torch.cat([torch.tensor([0.0, -0.0], dtype=torch.float64), neg, torch.tensor([-math.inf], dtype=torch.float64)]).float()


@functools.lru_cache(maxsize=1)
def _ew_pattern():
    """One period of the element-wise inputs: the strata and as many x > 0 (2^k (1 + i / 64), k in [-40, 6], and +inf's neighbour the largest
    float), in a fixed random order; its length is no multiple of 3, so a tiled x meets every gy of ELU_GY."""
    neg = elu_strata()
    pos = torch.cat([-neg[2:-1], torch.tensor([torch.finfo(torch.float32).max, torch.finfo(torch.float32).tiny, 1.0])])
    pat = torch.cat([neg, pos])
    assert pat.numel() % 3 != 0 and pat.numel() < 65793
    return pat[torch.randperm(pat.numel(), generator=torch.Generator().manual_seed(5))]


@functools.lru_cache(maxsize=8)
def ew_inputs(n):
    """(x, gy): n float32 each.  x tiles the pattern (every branch in the first trip of the stride loop and, at n >= EW_STRIDE + its length,
    in the second); gy cycles ELU_GY."""
    pat = _ew_pattern()
    idx = torch.arange(n)
    return pat[idx % pat.numel()].clone(), torch.tensor(ELU_GY)[idx % 3].clone()


def relu_inputs(n):
    """(y, gy): y tiles a pattern of positive values, +0, -0 and negative ones (what a ReLU output never holds, but the kernel's contract
    covers); gy is Gaussian with a -0 and a +0 in every period of 7."""
    pat = _ew_pattern()
    idx = torch.arange(n)
    y = pat[idx % pat.numel()].clone()
    gy = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000003))
    gy[idx % 7 == 3] = -0.0
    gy[idx % 7 == 5] = 0.0
    return y, gy


def ulp_errors(got, ref):
    """|got - ref| in float32 ulps of the fp64 value ref (the spacing of float32 at |ref|, denormal spacing below the normal range); where
    ref is 0 or infinite the result must equal it.  Returns the per-entry errors (fp64)."""
    got, ref = got.double(), ref.double()
    special = (ref == 0) | torch.isinf(ref)
    _, e = torch.frexp(torch.where(special, torch.ones_like(ref), ref.abs()))
    ulp = torch.ldexp(torch.ones_like(ref), (e - 24).clamp_min(-149))
    err = (got - ref).abs() / ulp
    return torch.where(special, torch.where(got == ref, torch.zeros_like(err), torch.full_like(err, math.inf)), err)


def elu_reference(x, gy):
    """fp64: (expm1(x), gy exp(x)) -- for the x <= 0 entries."""
    x = x.double()
    return torch.expm1(x), gy.double() * torch.exp(x)


def elu_yardstick(x, gy):
    """torch's float32 F.elu and its backward on the CPU."""
    xr = x.clone().requires_grad_(True)
    y = F.elu(xr)
    gx, = torch.autograd.grad(y, xr, gy)
    return y.detach(), gx


def elu_worst_ulps(y, gx, x, gy):
    """(forward, backward): the worst error in ulps over the x <= 0 entries."""
    neg = x <= 0
    ry, rg = elu_reference(x[neg], gy[neg])
    return ulp_errors(y[neg], ry).max().item(), ulp_errors(gx[neg], rg).max().item()


def elu_run(x, gy):
    """sga_elu_fwd and sga_elu_bwd called directly on the card: (y, gx) on the host."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    xd, gd = x.cuda(), gy.cuda()
    y, gx = torch.full_like(xd, math.nan), torch.full_like(xd, math.nan)
    _lib.check(_lib.lib().sga_elu_fwd(_p(xd), _p(y), xd.numel(), _stream()), 'sga_elu_fwd')
    _lib.check(_lib.lib().sga_elu_bwd(_p(xd), _p(gd), _p(gx), xd.numel(), _stream()), 'sga_elu_bwd')
    torch.cuda.synchronize()
    return y.cpu(), gx.cpu()


def relu_run(y, gy):
    """sga_relu_bwd called directly on the card."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    yd, gd = y.cuda(), gy.cuda()
    gx = torch.full_like(yd, math.nan)
    _lib.check(_lib.lib().sga_relu_bwd(_p(yd), _p(gd), _p(gx), yd.numel(), _stream()), 'sga_relu_bwd')
    torch.cuda.synchronize()
    return gx.cpu()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
