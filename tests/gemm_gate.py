"""The accuracy gate of the GEMM tests, and the plumbing they share (no tests in this module).

Metric.  The error of an output entry is taken relative to its ENVELOPE, e_ij = |C_ij - ref_ij| / (|A| |B| + |bias| + |C0|)_ij with `ref` and
the envelope in fp64, and is quoted in units of u = 2^-24 (half an fp32 ulp at 1).  Against the envelope -- not against max|ref| -- an entry
that cancels to nearly nothing is judged like any other, and scaling a row of A or of B by a power of two changes nothing at all.  Inputs are
zero mean: with a common offset the products stop cancelling and a dropped low-order product hides behind the rounding of the large sum.

Yardstick.  Plain fp32 arithmetic of the same blocking, by torch on the CPU (never by the library under test):
    acc = 0;  for each 32-wide chunk of K:  acc = acc + A[:, chunk] @ B[:, chunk].T        (all float32)
then bias and C0 are added in fp32.  Its max and rms e stand next to the kernel's.

Gate.  kernel_rms <= r * yardstick_rms and kernel_max <= r * yardstick_max, r per route and K band (R_LOW, R below): "the measured ratio x 2, rounded up", the
measurement being profiles/gemm_accuracy_vs_fp32.json (tools/gemm_accuracy.py writes it; the factor 2 is for seeds and for the MFMA's
accumulation order against the CPU's).  For the three-plane routes (NT3_*) r must stay below 8 in rms whatever is measured: the weakest
realistic defect of that arithmetic (one of the six partial products forgotten) sits >= 15 x above the yardstick in rms, and
tests/test_gemm_plan_cpu.py::test_gate_would_catch_a_dropped_plane asserts that five, four and three products FAIL the gate at the r in use.

Floor, on the max alone.  The max of a handful of entries is one draw: at K = 1 the CPU's product and the kernel's are both exactly rounded, yet
one may show 0.2 u where the other shows 0.5 u, and r x a lucky draw admits no correct kernel.  One rounding of the sum (0.5 u of |C| <= 0.5 u
of the envelope) and one of the bias / C0 addition (0.5 u again) are owed by every correct fp32 evaluation, so a MAX error up to FLOOR_U = 1 u of
the envelope passes regardless of the yardstick's.  The rms is judged by r x the yardstick's rms; it is granted only what that max floor grants
ONE entry, FLOOR_U / sqrt(n) over n entries -- the whole floor for a 1 x 1 output, whose rms is a single draw like its max, 0.003 u at 10^5
entries.  That keeps a forgotten partial product visible at large K, where the defect falls like 1 / sqrt(K) with the yardstick (self-test up to
K = 16 384).
"""
import json
import math
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'gemm_accuracy_vs_fp32.json')
U = 2.0 ** -24
FLOOR_U = 1.0
KC = 32                                  # the K chunk of every tiled kernel (SGA_KC)
NT3_RMS_CAP = 8.0                        # condition, not measurement (see above)

# r per route and K band: ceil(2 x the worst ratio measured for the route in the band, rms or max), from profiles/gemm_accuracy_vs_fp32.json.
# Two bands, K <= 256 and above, because the fp32 MFMA routes' ratio grows with K (their rounding per two products against the yardstick's per
# 32): one r over all K would leave the short shapes, where most tests run, gated at several times their measurement.  A band holds the worst of
# ALL its measured K, so a test at a K between two measured ones is covered by the larger.  R is the high band (the worst over every K) where a
# route has one.  test_gemm_plan_cpu.py::test_gate_ratios_are_the_measured_ones keeps these tables and the profile together.
K_BAND = 256
R_LOW = {
    'TN_NARROW': 3, 'TN_SPLIT': 3, 'TN_BIG': 9, 'NN': 8, 'NT_128': 6, 'NT_64': 5, 'NT3_128': 3, 'NT3_64': 4,
    'SMALL_F32': 3, 'SMALL_F64': 3, 'GENERIC_F32': 8, 'GENERIC_F64': 8,
}
R = {
    'TN_NARROW': 3, 'TN_SPLIT': 3, 'TN_BIG': 13, 'NN': 8, 'NT_128': 6, 'NT_64': 5, 'NT3_128': 5, 'NT3_64': 4,
    'SMALL_F32': 3, 'SMALL_F64': 3, 'GENERIC_F32': 11, 'GENERIC_F64': 8,
}


def r_for(route, k):
    """The gate ratio of a route at contraction length k."""
    return R_LOW[route] if k <= K_BAND else R[route]


def ratios_from_profile(path=PROFILE, kmax=None):
    """route -> ceil(2 x worst measured kernel / yardstick ratio) over the cases with K <= kmax (all of them: None), the derivation R states."""
    rows = json.load(open(path))['cases']
    worst = {}
    for c in rows:
        if kmax is None or c['K'] <= kmax:
            worst[c['route']] = max(worst.get(c['route'], 0.0), c['ratio_rms'], c['ratio_max'])
    return {k: int(math.ceil(2.0 * v - 1e-9)) for k, v in worst.items()}


# ------------------------------------------------------------------------------------------------ metric, yardstick, gate
def envelope(a, bt, bias=None, c0=None):
    """(|A| |B| + |bias| + |C0|) in fp64 for logical A [M,K] and B^T [N,K] (any device)."""
    env = a.double().abs() @ bt.double().abs().t()
    if bias is not None:
        env = env + bias.double().abs()
    if c0 is not None:
        env = env + c0.double().abs()
    return env


def reference(a, bt, bias=None, c0=None):
    ref = a.double() @ bt.double().t()
    if bias is not None:
        ref = ref + bias.double()
    if c0 is not None:
        ref = ref + c0.double()
    return ref


def rel_errors(c, ref, env):
    """(max, rms, number of entries) of |c - ref| / env in units of u.  An entry with an empty envelope (K = 0, no bias) must be exact."""
    d = (c.double() - ref).abs()
    assert torch.isfinite(d).all(), 'non-finite output'
    zero = env == 0
    assert not (d[zero] != 0).any(), 'non-zero output where every term is zero'
    e = torch.where(zero, torch.zeros_like(d), d / torch.where(zero, torch.ones_like(env), env)) / U
    if e.numel() == 0:
        return 0.0, 0.0, 0
    return e.max().item(), e.pow(2).mean().sqrt().item(), e.numel()


def yardstick(a, bt, bias=None, c0=None):
    """Plain fp32, K walked in chunks of 32, on the CPU."""
    a = a.detach().float().cpu()
    bt = bt.detach().float().cpu()
    acc = torch.zeros(a.shape[0], bt.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], KC):
        acc = acc + a[:, k0:k0 + KC] @ bt[:, k0:k0 + KC].t()
    if bias is not None:
        acc = acc + bias.detach().float().cpu()
    if c0 is not None:
        acc = acc + c0.detach().float().cpu()
    return acc


def gate_ok(kernel, yard, r):
    """kernel, yard: (max, rms, n) of rel_errors, in u."""
    return kernel[0] <= max(r * yard[0], FLOOR_U) and kernel[1] <= max(r * yard[1], FLOOR_U / max(kernel[2], 1) ** 0.5)


def assert_gate(c, a, bt, r, bias=None, c0=None, what='', yard_c=None, ref=None, env=None, rows=None):
    """Gate `c` (device or host) against fp64 on the logical operands; returns (kernel, yardstick) errors.  rows: judge this row subset only
    (a tensor of indices) -- the yardstick is then computed for those rows alone."""
    if rows is not None:
        rows_d = rows.to(c.device)
        c, a = c[rows_d], a[rows.to(a.device)]
        c0 = None if c0 is None else c0[rows.to(c0.device)]
    if ref is None:
        ref = reference(a, bt, bias, c0)
    if env is None:
        env = envelope(a, bt, bias, c0)
    if yard_c is None:
        yard_c = yardstick(a, bt, bias, c0)
    ke = rel_errors(c.to(ref.device), ref, env)
    ye = rel_errors(yard_c.to(ref.device), ref, env)
    print(f'[gate] {what}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | fp32 yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
    assert gate_ok(ke, ye, r), f'{what}: kernel (max, rms) = {ke[:2]} u against yardstick {ye[:2]} u exceeds r = {r}'
    return ke, ye


# ------------------------------------------------------------------------------------------------ the three-plane arithmetic, emulated (CPU)
def split3(x):
    """x = h + m + l, each a bf16 value (round to nearest), held in float32."""
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = (x - h - m).bfloat16().float()
    return h, m, l


# (plane of A, plane of B); the kernel's six, then what is left when products are forgotten
PRODUCTS = {
    6: [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)],
    5: [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2)],              # l h' forgotten
    4: [(0, 0), (0, 1), (1, 0), (1, 1)],                      # no l plane
    3: [(0, 0), (0, 1), (1, 0)],
}


def planes_product(a, bt, nprod):
    """A B^T by `nprod` partial products of the bf16 planes: exact products (fp64), h h' and the small ones in two fp32 accumulators that take one
    addition per 32-wide K chunk each -- gemm_nt3_kernel's arithmetic without the MFMA's internal alignment."""
    pa, pb = split3(a.float().cpu()), split3(bt.float().cpu())
    acc = torch.zeros(a.shape[0], bt.shape[0], dtype=torch.float32)
    accs = torch.zeros_like(acc)
    for k0 in range(0, a.shape[1], KC):
        sl = slice(k0, k0 + KC)
        small = torch.zeros(acc.shape, dtype=torch.float64)
        for (i, j) in PRODUCTS[nprod]:
            pr = pa[i][:, sl].double() @ pb[j][:, sl].double().t()
            if (i, j) == (0, 0):
                acc = acc + pr.float()
            else:
                small = small + pr
        accs = accs + small.float()
    return acc + accs


# ------------------------------------------------------------------------------------------------ operands and launches (GPU)
def zero_mean(shape, gen, device='cuda'):
    return torch.randn(shape, generator=gen, device=device)


def pow2_scales(n, gen, device='cuda', span=20):
    """2^e, e uniform integer in [-span, span]."""
    e = torch.randint(-span, span + 1, (n,), generator=gen, device=device)
    return torch.ldexp(torch.ones(n, device=device), e)


def logical_operands(m, n, k, seed, grade=None, device='cuda'):
    """Zero-mean logical A [m,k] and B^T [n,k].  grade 'rows': rows of A and of B^T scaled by random powers of two in 2^+-20;
    grade 'k': column kk of A and of B^T each by its own random power of two in 2^+-20, so every product of a sum sits at its own exponent
    (2^+-40 apart at most: inside fp32's range for unit-variance entries and K <= 2^16)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    a = zero_mean((m, k), gen, device)
    bt = zero_mean((n, k), gen, device)
    if grade == 'rows':
        a = a * pow2_scales(m, gen, device)[:, None]
        bt = bt * pow2_scales(n, gen, device)[:, None]
    elif grade == 'k':
        a = a * pow2_scales(k, gen, device)[None, :]
        bt = bt * pow2_scales(k, gen, device)[None, :]
    elif grade is not None:
        raise ValueError(grade)
    return a, bt


def store(x, layout='plain', fill=0.0, dtype=None):
    """A device copy of the 2-d tensor x in the asked memory layout: 'plain' (contiguous), 'slice' (a column slice, 8 columns in, of a
    parent 20 columns wider: a leading dimension of its own, 16-byte alignment kept when the width is a multiple of 4), 'off1' (contiguous
    but starting one element into its allocation: 4-byte aligned only)."""
    dtype = dtype or x.dtype
    r, c = x.shape
    if layout == 'plain':
        return x.to(dtype).contiguous().clone()
    if layout == 'slice':
        parent = torch.full((r, c + 20), fill, device=x.device, dtype=dtype)
        v = parent[:, 8:8 + c]
        v.copy_(x)
        return v
    if layout == 'off1':
        buf = torch.full((r * c + 4,), fill, device=x.device, dtype=dtype)
        v = buf[1:1 + r * c].view(r, c)
        v.copy_(x)
        return v
    raise ValueError(layout)


def stored_pair(a, bt, ta, tb, la='plain', lb='plain', a_f64=False):
    """The operands as sga_gemm wants them: A [m,k] (ta: [k,m]), B [k,n] (tb: [n,k])."""
    sa = a.t() if ta else a
    if a_f64:
        # fp64 values that are NOT fp32 numbers: the loader's conversion has something to round
        gen = torch.Generator(device=a.device)
        gen.manual_seed(7)
        sa = sa.double() * (1.0 + 1e-8 * torch.randn(sa.shape, generator=gen, device=a.device, dtype=torch.float64))
    sa = store(sa, la)
    sb = store(bt if tb else bt.t(), lb)
    return sa, sb


def nan_window(m, n, device='cuda'):
    """(parent, view): an m x n window inside a NaN-filled parent with a margin on every side."""
    parent = torch.full((m + 3, n + 11), float('nan'), device=device)
    return parent, parent[1:1 + m, 4:4 + n]


def outside_still_nan(parent, m, n):
    mask = torch.ones_like(parent, dtype=torch.bool)
    mask[1:1 + m, 4:4 + n] = False
    return bool(torch.isnan(parent[mask]).all())


def plan_of(ta, tb, m, n, k, a, b, c, bias=None, accumulate=False, act=0, resid=None, colstats=False, ncu=0):
    from sgaligner_amd import ops
    return ops.gemm_plan(ta, tb, m, n, k, lda=a.stride(0), ldb=b.stride(0), ldc=c.stride(0), ldr=resid.stride(0) if resid is not None else 0,
                         a_is_f64=a.dtype == torch.float64, a_aligned16=a.data_ptr() % 16 == 0, b_aligned16=b.data_ptr() % 16 == 0,
                         has_bias=bias is not None, accumulate=accumulate, act=act, has_resid=resid is not None, has_colstats=colstats, ncu=ncu)


def launch(ta, tb, m, n, k, a, b, c=None, bias=None, accumulate=False, act=0, resid=None, expect=None, ex=None):
    """sga_gemm (or sga_gemm_ex when an activation / a residual is asked for, or ex=True) on stored operands; the plan on this card is
    asserted first when `expect` names a route.  Returns (c, plan)."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    if c is None:
        c = torch.empty((m, n), device=b.device, dtype=torch.float32)
    plan = plan_of(ta, tb, m, n, k, a, b, c, bias, accumulate, act, resid)
    if expect is not None:
        assert plan[0] == expect, f'this shape no longer reaches {expect}: ({ta},{tb}) {m} x {n} x {k} is planned as {plan}'
    if ex is None:
        ex = act != 0 or resid is not None
    if ex:
        assert not accumulate and a.dtype == torch.float32
        rc = _lib.lib().sga_gemm_ex(int(ta), int(tb), m, n, k, _p(a), a.stride(0), _p(b), b.stride(0), _p(c), c.stride(0), _p(bias), act,
                                    _p(resid), resid.stride(0) if resid is not None else 0, _stream())
        _lib.check(rc, 'sga_gemm_ex')
    else:
        rc = _lib.lib().sga_gemm(int(ta), int(tb), m, n, k, _p(a), a.stride(0), int(a.dtype == torch.float64), _p(b), b.stride(0), _p(c),
                                 c.stride(0), _p(bias), int(accumulate), _stream())
        _lib.check(rc, 'sga_gemm')
    return c, plan


def activation64(z, act):
    """act on an fp64 tensor with the kernel's fp32 slope."""
    if act == 0:
        return z
    if act == 1:
        return z.clamp_min(0)
    return torch.where(z > 0, z, z * float(torch.tensor(0.2, dtype=torch.float32)))


# ------------------------------------------------------------------------------------------------ the cases both the gate tests and the profile run
# One shape per (route, K) of the K sweep {32, 128, 256, 1024, 4096, 40000} that the route's conditions admit at 256 CUs, kept small enough for a
# CPU yardstick.  (ta, tb, m, n, k, options).  Options: la / lb layouts, a_f64, bias, resid0 (an all-zero residual: keeps a K >= 4096 call of few
# rows off the split-K rule without touching the numbers), rows (judge a sample of rows), grade.
def accuracy_cases():
    C = []

    def add(route, ta, tb, m, n, k, **o):
        C.append(dict(route=route, ta=ta, tb=tb, m=m, n=n, k=k, **o))

    for k in (32, 128):
        add('NT_128', 0, 1, 384, 256, k, bias=True)
        add('NT_64', 0, 1, 163840, 128, k, bias=True, rows=8192)
    for k in (256, 1024):
        add('NT3_128', 0, 1, 384, 256, k, bias=True)
    add('NT3_128', 0, 1, 300, 128, 256)
    for k in (4096, 40000):
        add('NT3_128', 0, 1, 384, 256, k, bias=True, resid0=True)
    add('NT3_128', 0, 1, 384, 256, 1024, grade='rows')
    add('NT3_128', 0, 1, 384, 256, 1024, grade='k')
    add('NT3_64', 0, 1, 163840, 128, 256, bias=True, rows=8192)
    add('NT3_64', 0, 1, 163840, 32, 1024, bias=True, rows=8192)
    add('NT3_64', 0, 1, 163840, 128, 256, grade='rows', rows=8192)
    for k in (32, 128, 256):
        add('SMALL_F32', 0, 1, 384, 256, k, la='off1', bias=True)
        add('SMALL_F64', 0, 1, 384, 256, k, a_f64=True, bias=True)
        add('GENERIC_F32', 0, 1, 384, 260, k, la='off1', bias=True)
        add('GENERIC_F64', 0, 1, 384, 260, k, a_f64=True, bias=True)
    for k in (1024, 4096, 40000):
        add('GENERIC_F32', 0, 1, 384, 256, k, la='off1', bias=True)                 # K >= 4096: split over K, atomics
        add('GENERIC_F64', 0, 1, 384, 256, k, a_f64=True, bias=True)
    add('GENERIC_F32', 0, 1, 384, 256, 4096, la='off1', bias=True, resid0=True)     # unsplit
    add('GENERIC_F32', 0, 1, 384, 256, 1024, la='off1', grade='rows')
    for k in (32, 128, 256, 1024, 4096, 40000):
        add('NN', 0, 0, 384, 256, k)
    add('NN', 0, 0, 384, 256, 1024, grade='k')
    for k in (128, 256, 1024, 4096, 40000):
        add('TN_SPLIT', 1, 0, 384, 256, k)
        add('TN_NARROW', 1, 0, 5000, 8, k)
    add('TN_NARROW', 1, 0, 5000, 3, 64)
    for k in (256, 1024):
        add('TN_BIG', 1, 0, 2048, 2048, k, rows=512)
    add('TN_BIG', 1, 0, 2048, 2048, 1024, grade='rows', rows=512)
    return C


def run_accuracy_case(case, seed=0):
    """Runs one case on the card; returns dict(kernel=(max, rms), yard=(max, rms), plan=...).  The plan is asserted first."""
    ta, tb, m, n, k = case['ta'], case['tb'], case['m'], case['n'], case['k']
    a, bt = logical_operands(m, n, k, seed + m + n + k, case.get('grade'))
    sa, sb = stored_pair(a, bt, ta, tb, case.get('la', 'plain'), case.get('lb', 'plain'), case.get('a_f64', False))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed + 1)
    bias = torch.randn(n, generator=gen, device='cuda') if case.get('bias') else None
    if bias is not None and case.get('grade') == 'rows':
        bias = bias * bt.abs().amax(dim=1)
    resid = torch.zeros(m, n, device='cuda') if case.get('resid0') else None
    c, plan = launch(ta, tb, m, n, k, sa, sb, bias=bias, resid=resid, expect=case['route'])
    rows = None
    if case.get('rows'):
        # a sample that keeps both ends of the row range and of a tile
        rows = torch.cat([torch.arange(0, 130), torch.arange(m - 130, m), torch.randperm(m, generator=torch.Generator().manual_seed(seed))[:case['rows']]]).unique()
    if case.get('a_f64'):
        a = sa.t().float() if ta else sa.float()                    # what the loader's conversion makes of the fp64 values
    ke, ye = assert_gate(c, a, bt, float('inf'), bias=bias, rows=rows, what=f"{case['route']} {m}x{n}x{k} {case.get('grade') or ''}")
    return dict(kernel=ke, yard=ye, plan=plan)
