"""Every route of the GEMM launcher (csrc/gemm.hip, enum sga_gemm_route) against torch fp64 on the same inputs.

Each case first asserts, through sga_gemm_plan on this card, that its shape reaches the route it is there for -- when a threshold moves the
test fails with "this shape no longer reaches X" instead of going quietly blind -- and then judges the numbers by the accuracy gate of
tests/gemm_gate.py: the envelope-relative error against fp64 may be at most r_for(route, K) times that of plain fp32 arithmetic computed by torch
on the CPU (zero-mean inputs).  The bit-invariance promises of the launcher (64-row against 128-row tiles, row chunks against the whole
batch for K < 4096, run to run on every route without atomics) are tested with torch.equal."""
import pytest
import torch

import gemm_gate as G
from gemm_gate import launch, r_for

pytestmark = pytest.mark.gpu

NT, NN, TN, TT = (0, 1), (0, 0), (1, 0), (1, 1)
EPILOGUE_ROUTES = ('NT_128', 'NT_64', 'NT3_128', 'NT3_64', 'SMALL_F32', 'GENERIC_F32')
ATOMIC_ROUTES = ('TN_NARROW', 'TN_SPLIT', 'TN_BIG')            # + any route planned with splits > 1


def _gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------ one shape (or two) per route, four variants each
# (route, (ta, tb), m, n, k, options): bias where the route takes one; a_f64; grade.  Routes at 256 CUs; the plan on the card is asserted.
ROUTE_CASES = [
    ('TN_NARROW', TN, 5000, 8, 333, {}),
    ('TN_NARROW', TN, 128, 3, 40000, {}),
    ('TN_SPLIT', TN, 3072, 1024, 300, {}),
    ('TN_SPLIT', TN, 100, 256, 9000, {}),
    ('TN_BIG', TN, 2048, 2048, 512, {}),
    ('NN', NN, 300, 256, 100, {}),
    ('NN', NN, 300, 104, 4096, {}),                                  # split over K
    ('NT_128', NT, 300, 100, 128, dict(bias=True)),
    ('NT_64', NT, 163840, 128, 128, dict(bias=True)),
    ('NT3_128', NT, 300, 100, 1024, dict(bias=True)),
    ('NT3_128', NT, 384, 256, 256, dict(bias=True, grade='rows')),
    ('NT3_128', NT, 384, 256, 1024, dict(grade='k')),
    ('NT3_64', NT, 163840, 128, 256, dict(bias=True)),
    ('NT3_64', NT, 163840, 128, 256, dict(grade='rows')),
    ('NT_64', NT, 163840, 128, 128, dict(grade='rows')),
    ('SMALL_F32', NT, 300, 100, 41, dict(bias=True)),
    ('SMALL_F32', TT, 65, 200, 70, dict(bias=True)),
    ('SMALL_F64', NT, 300, 100, 164, dict(bias=True, a_f64=True)),
    ('GENERIC_F32', NT, 300, 300, 515, dict(bias=True)),
    ('GENERIC_F32', NT, 64, 100, 4096, dict(bias=True)),            # split over K: the case of test_rows_split_over_k_from_4096_on
    ('GENERIC_F32', TT, 65, 200, 700, dict(bias=True)),
    ('GENERIC_F32', TN, 102, 256, 9000, {}),                         # M % 4 != 0 falls off the TN kernel, split over K
    ('GENERIC_F64', NT, 300, 100, 700, dict(bias=True, a_f64=True)),
    ('GENERIC_F64', NT, 300, 300, 164, dict(bias=True, a_f64=True, grade='rows')),
]
# the two routes that launch nothing: (route, m, n, k) of test_empty_outputs_with_null_pointers, (route, m, n, k, layout of A) of
# test_bnstats_refused_shape_writes_nothing -- each asserted there through the plan
EMPTY_CASES = [('EMPTY', 0, 5, 7), ('EMPTY', 5, 0, 7), ('EMPTY', 0, 0, 7)]
REFUSED_CASES = [('REFUSED', 300, 100, 130, 'plain'), ('REFUSED', 300, 100, 128, 'off1')]
CLAIMED = {c[0] for c in ROUTE_CASES + EMPTY_CASES + REFUSED_CASES}


def test_every_route_is_claimed_by_a_case():
    from sgaligner_amd import _lib
    assert CLAIMED == set(_lib.GEMM_ROUTES), set(_lib.GEMM_ROUTES) ^ CLAIMED


@pytest.mark.parametrize('route,tt,m,n,k,o', ROUTE_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_route_variants(route, tt, m, n, k, o):
    """plain | accumulate on a random C | a strided C inside a NaN-filled parent (everything outside the window must still be NaN: the zeroing of the
    atomic routes and every mask) | A and B as column slices of wider parents."""
    ta, tb = tt
    r = r_for(route, k)
    a, bt = G.logical_operands(m, n, k, 11 + m + n + k, o.get('grade'))
    f64 = o.get('a_f64', False)
    sa, sb = G.stored_pair(a, bt, ta, tb, a_f64=f64)
    if f64:
        a = (sa.t() if ta else sa).float()                           # the loader's conversion is part of the operation (.float() of the features)
    g = _gen(m + k)
    bias = torch.randn(n, generator=g, device='cuda') if o.get('bias') else None
    if bias is not None and o.get('grade') == 'rows':
        bias = bias * bt.abs().amax(dim=1)
    ref, env, yard = G.reference(a, bt, bias), G.envelope(a, bt, bias), G.yardstick(a, bt, bias).cuda()
    what = f'{route} ({ta},{tb}) {m}x{n}x{k}'

    c, plan = launch(ta, tb, m, n, k, sa, sb, bias=bias, expect=route)
    G.assert_gate(c, a, bt, r, what=what + ' plain', yard_c=yard, ref=ref, env=env)
    atomic = plan[1] > 1 or route in ATOMIC_ROUTES
    if not atomic:                                                   # run to run: the same bits on every route without atomics
        c2, _ = launch(ta, tb, m, n, k, sa, sb, bias=bias, expect=route)
        assert torch.equal(c, c2), what + ': two runs differ'

    # C0 of the size of the product itself (its envelope over sqrt(K): what a gradient accumulated into a gradient looks like).  The atomic routes
    # add `splits` partial sums into C one by one, each rounded at the magnitude of C0 + partial: under a C0 that dwarfs the product the metric
    # would read sqrt(splits) ulps of C0 and say nothing about the kernel.
    c0 = torch.randn(m, n, generator=g, device='cuda') * (env / max(k, 1) ** 0.5).float()
    c1, _ = launch(ta, tb, m, n, k, sa, sb, c=c0.clone(), bias=bias, accumulate=True, expect=route)
    G.assert_gate(c1, a, bt, r, what=what + ' accumulate', yard_c=yard + c0, ref=ref + c0.double(), env=env + c0.double().abs())

    parent, win = G.nan_window(m, n)
    launch(ta, tb, m, n, k, sa, sb, c=win, bias=bias, expect=route)
    G.assert_gate(win, a, bt, r, what=what + ' strided C', yard_c=yard, ref=ref, env=env)
    assert G.outside_still_nan(parent, m, n), what + ': wrote outside the M x N window of a strided C'
    # the same with accumulate: a window of C0 inside the NaN parent, nothing zeroed, nothing outside touched
    parent, win = G.nan_window(m, n)
    win.copy_(c0)
    launch(ta, tb, m, n, k, sa, sb, c=win, bias=bias, accumulate=True, expect=route)
    G.assert_gate(win, a, bt, r, what=what + ' strided C accumulate', yard_c=yard + c0, ref=ref + c0.double(), env=env + c0.double().abs())
    assert G.outside_still_nan(parent, m, n)

    ssa, ssb = G.store(sa, 'slice'), G.store(sb, 'slice')            # the same values (fp64 ones included) in strided parents
    cs, _ = launch(ta, tb, m, n, k, ssa, ssb, bias=bias, expect=route)
    G.assert_gate(cs, a, bt, r, what=what + ' sliced A, B', yard_c=yard, ref=ref, env=env)
    if not atomic:
        assert torch.equal(cs, c), what + ': strided operands change the bits'


# ------------------------------------------------------------------------------------------------ edges
E9 = (31, 32, 33, 63, 64, 65, 127, 128, 129)
EDGE_K = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260)


EDGE_ROUTES = {NT: {'SMALL_F32', 'NT_128', 'NT3_128'}, NN: {'SMALL_F32', 'NN'}, TN: {'SMALL_F32', 'GENERIC_F32', 'TN_SPLIT'}, TT: {'SMALL_F32'}}


@pytest.mark.parametrize('tt', [NT, NN, TN, TT], ids=['NT', 'NN', 'TN', 'TT'])
def test_tile_edges(tt):
    """M, N, K one below, at and one above the 32 / 64 / 128 tile sizes and the 32-wide K chunk (and the K = 256 switch of the NT arithmetic), into a
    NaN-framed strided C; whatever route the launcher plans for a shape, its numbers pass that route's gate and nothing outside the window is
    written.  The set of routes met is asserted."""
    ta, tb = tt
    pairs = sorted({(m, n) for m in E9 for n in (32, 33, 128)} | {(m, n) for n in E9 for m in (32, 33, 128)})
    met = {}
    for k in EDGE_K:
        a_all, bt_all = G.logical_operands(129, 129, k, 100 + k)
        for (m, n) in pairs:
            a, bt = a_all[:m].contiguous(), bt_all[:n].contiguous()
            sa, sb = G.stored_pair(a, bt, ta, tb)
            parent, win = G.nan_window(m, n)
            _, plan = launch(ta, tb, m, n, k, sa, sb, c=win)
            met[plan[0]] = met.get(plan[0], 0) + 1
            ref, env = G.reference(a, bt), G.envelope(a, bt)
            ke, ye = G.rel_errors(win, ref, env), G.rel_errors(G.yardstick(a, bt).cuda(), ref, env)
            assert G.gate_ok(ke, ye, r_for(plan[0], k)), f'({ta},{tb}) {m}x{n}x{k} on {plan}: kernel {ke} u, yardstick {ye} u'
            assert G.outside_still_nan(parent, m, n), f'({ta},{tb}) {m}x{n}x{k} on {plan}: wrote outside the window'
    print('routes met:', met)
    assert set(met) == EDGE_ROUTES[tt], f'({ta},{tb}): the edge shapes no longer reach {EDGE_ROUTES[tt] - set(met)} (met {met})'


def test_k_zero_writes_bias_or_leaves_c():
    """K == 0: C = bias (0 without one), or C untouched under accumulate -- on the route each transpose pair takes."""
    for (ta, tb), route, n in ((NT, 'NT_128', 40), (TN, 'SMALL_F32', 40), (NN, 'NN', 40), (TT, 'SMALL_F32', 40), (TT, 'GENERIC_F32', 300)):
        m = 70
        a = torch.zeros(4, m, device='cuda')[:0] if ta else torch.zeros(m, 4, device='cuda')[:, :0]      # no elements, a real pointer and pitch
        b = torch.zeros(n, 4, device='cuda')[:, :0] if tb else torch.zeros(4, n, device='cuda')[:0]
        bias = torch.randn(n, device='cuda') if route != 'NN' else None
        parent, win = G.nan_window(m, n)
        launch(ta, tb, m, n, 0, a, b, c=win, bias=bias, expect=route)
        want = bias.expand(m, n) if bias is not None else torch.zeros(m, n, device='cuda')
        assert torch.equal(win, want), (ta, tb)
        assert G.outside_still_nan(parent, m, n)
        c0 = torch.randn(m, n, device='cuda')
        c1, _ = launch(ta, tb, m, n, 0, a, b, c=c0.clone(), accumulate=True)
        assert torch.equal(c1, c0), (ta, tb)
        if bias is not None:
            c1, _ = launch(ta, tb, m, n, 0, a, b, c=c0.clone(), bias=bias, accumulate=True, expect=route)
            assert torch.equal(c1, c0 + bias), (ta, tb)
    # sga_gemm_ex: act(bias) + resid
    bias, resid = torch.randn(40, device='cuda'), torch.randn(70, 40, device='cuda')
    a, b = torch.zeros(70, 4, device='cuda'), torch.zeros(40, 4, device='cuda')
    y, _ = launch(0, 1, 70, 40, 0, a, b, bias=bias, act=2, resid=resid, expect='NT_128')
    ab = torch.where(bias > 0, bias, 0.2 * bias).expand(70, 40)
    assert ((y.double() - (ab.double() + resid.double())).abs() <= 2 * G.U * (ab.abs() + resid.abs()).double()).all()


def test_empty_outputs_with_null_pointers():
    """M == 0 or N == 0: SGA_OK, nothing launched, null pointers allowed (a zero-row shard)."""
    from sgaligner_amd import _lib, ops
    L = _lib.lib()
    for (route, m, n, k) in EMPTY_CASES:
        assert k == 7 and ops.gemm_plan(0, 1, m, n, k)[0] == route
        assert L.sga_gemm(0, 1, m, n, 7, None, 7, 0, None, 7, None, max(n, 1), None, 0, ops._stream()) == 0
        assert L.sga_gemm(1, 0, m, n, 7, None, 7, 1, None, 7, None, max(n, 1), None, 1, ops._stream()) == 0
        assert L.sga_gemm_ex(0, 1, m, n, 7, None, 7, None, 7, None, max(n, 1), None, 1, None, 0, ops._stream()) == 0
    # ... and a live output next to it is not touched
    guard = torch.full((16,), float('nan'), device='cuda')
    assert L.sga_gemm(0, 1, 0, 4, 4, None, 4, 0, None, 4, guard.data_ptr(), 4, None, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(guard).all()
    # a non-empty output with null operands is an argument error, not a launch
    assert L.sga_gemm(0, 1, 4, 4, 4, None, 4, 0, None, 4, guard.data_ptr(), 4, None, 0, ops._stream()) != 0
    assert torch.isnan(guard).all()


def test_bnstats_refused_shape_writes_nothing():
    """REFUSED: sga_gemm_bnstats on a shape the NT kernels do not take returns an argument error and leaves C alone."""
    from sgaligner_amd import _lib, ops
    L = _lib.lib()
    for (route, m, n, k, layout) in REFUSED_CASES:                   # K % 4 != 0; 4-byte aligned rows
        x, w = G.store(torch.randn(m, k, device='cuda'), layout), torch.randn(n, k, device='cuda')
        y = torch.full((m, n), float('nan'), device='cuda')
        sums = torch.empty(2 * n, device='cuda', dtype=torch.float64)
        assert G.plan_of(0, 1, m, n, k, x, w, y, colstats=True)[0] == route
        assert L.sga_gemm_bnstats(m, n, k, x.data_ptr(), k, w.data_ptr(), k, y.data_ptr(), n, None, sums.data_ptr(), ops._stream()) != 0
        assert b'NT kernel' in L.sga_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(y).all()


@pytest.mark.parametrize('tt,m,n,k,aligned,off', [(NT, 300, 100, 128, 'NT_128', 'SMALL_F32'), (NT, 300, 100, 1024, 'NT3_128', 'GENERIC_F32'),
                                                  (NN, 300, 256, 100, 'NN', 'SMALL_F32'), (TN, 100, 256, 9000, 'TN_SPLIT', 'GENERIC_F32'),
                                                  (TN, 2048, 2048, 512, 'TN_BIG', 'GENERIC_F32')])
def test_four_byte_aligned_operand_falls_off_the_vector_kernels(tt, m, n, k, aligned, off):
    """An operand whose first element sits 4 bytes into a 16-byte line (a view starting one element in): the launcher must leave the kernels
    that load 16 bytes at a time, and the result agrees with the aligned call's within the gate (both are judged against fp64)."""
    ta, tb = tt
    a, bt = G.logical_operands(m, n, k, 3)
    ref, env, yard = G.reference(a, bt), G.envelope(a, bt), G.yardstick(a, bt).cuda()
    sa, sb = G.stored_pair(a, bt, ta, tb)
    c, _ = launch(ta, tb, m, n, k, sa, sb, expect=aligned)
    G.assert_gate(c, a, bt, r_for(aligned, k), what=f'{aligned} aligned', yard_c=yard, ref=ref, env=env)
    for la, lb in (('off1', 'plain'), ('plain', 'off1'), ('off1', 'off1')):
        oa, ob = G.stored_pair(a, bt, ta, tb, la, lb)
        assert (oa.data_ptr() % 16 != 0) == (la == 'off1') and oa.data_ptr() % 4 == 0
        co, _ = launch(ta, tb, m, n, k, oa, ob, expect=off)
        G.assert_gate(co, a, bt, r_for(off, k), what=f'{off} A {la} B {lb}', yard_c=yard, ref=ref, env=env)


def test_narrow_walk():
    """gemm_tn_narrow_kernel at N in {1, 3, 8}, K in {64, 65, 333, 40000}, M in {1, 63, 64, 65, 5000}: a strided C in a NaN frame, then accumulate
    on top of it."""
    for k in (64, 65, 333, 40000):
        for m in (1, 63, 64, 65, 5000):
            a, bt8 = G.logical_operands(m, 8, k, m + k)
            sa = G.store(a.t(), 'plain')
            ref8, env8, yard8 = G.reference(a, bt8), G.envelope(a, bt8), G.yardstick(a, bt8).cuda()
            for n in (1, 3, 8):
                bt = bt8[:n].contiguous()
                sb = G.store(bt.t(), 'plain')
                ref, env, yard = ref8[:, :n], env8[:, :n], yard8[:, :n]
                parent, win = G.nan_window(m, n)
                _, plan = launch(1, 0, m, n, k, sa, sb, c=win, expect='TN_NARROW')
                what = f'narrow {m}x{n}x{k} {plan}'
                assert plan[1] * plan[2] >= k
                ke, ye = G.rel_errors(win, ref, env), G.rel_errors(yard, ref, env)
                assert G.gate_ok(ke, ye, r_for('TN_NARROW', k)), f'{what}: kernel {ke} u, yardstick {ye} u'
                assert G.outside_still_nan(parent, m, n), what
                c0 = win.clone()
                launch(1, 0, m, n, k, sa, sb, c=win, accumulate=True, expect='TN_NARROW')
                ref2, env2 = ref + c0.double(), env + c0.double().abs()
                ke, ye = G.rel_errors(win, ref2, env2), G.rel_errors(yard + c0, ref2, env2)
                assert G.gate_ok(ke, ye, r_for('TN_NARROW', k)), f'{what} accumulate: kernel {ke} u, yardstick {ye} u'
                assert G.outside_still_nan(parent, m, n), what


# ------------------------------------------------------------------------------------------------ sga_gemm_ex
EX_SHAPES = {'NT_128': (300, 100, 128), 'NT_64': (163840, 128, 128), 'NT3_128': (300, 100, 512), 'NT3_64': (163840, 128, 256),
             'SMALL_F32': (300, 100, 41), 'GENERIC_F32': (300, 300, 515)}
assert set(EX_SHAPES) == set(EPILOGUE_ROUTES)


@pytest.mark.parametrize('route', EPILOGUE_ROUTES)
def test_gemm_ex_epilogues(route):
    """act in {none, ReLU, LeakyReLU(0.2)} x {bias, none} x {residual, none} on every route that takes an epilogue.  The pre-activation is judged
    by the gate through act = 0; the activation and the residual are then two fp32 operations on it: |y - (act(z) + resid)| <= 2 u (|act(z)| +
    |resid|) (one rounding of 0.2 z, one of the sum; z is the kernel's own pre-activation, these routes are bit-stable).  The residual has a leading
    dimension of its own (ldr != ldc)."""
    m, n, k = EX_SHAPES[route]
    a, bt = G.logical_operands(m, n, k, 21 + k)
    sa, sb = G.stored_pair(a, bt, 0, 1)
    g = _gen(5)
    resid = G.store(torch.randn(m, n, generator=g, device='cuda'), 'slice')
    assert resid.stride(0) != n
    sample = None if m < 10000 else torch.cat([torch.arange(0, 200), torch.arange(m - 200, m), torch.arange(0, m, 37)]).unique()
    for with_bias in (True, False):
        bias = torch.randn(n, generator=g, device='cuda') if with_bias else None
        z, _ = launch(0, 1, m, n, k, sa, sb, bias=bias, expect=route, ex=True)
        G.assert_gate(z, a, bt, r_for(route, k), bias=bias, rows=sample, what=f'{route} pre-activation bias={with_bias}')
        assert (z < 0).any() and (z > 0).any()
        z64 = z.double()
        for act in (0, 1, 2):
            for with_resid in (False, True):
                rs = resid if with_resid else None
                y, _ = launch(0, 1, m, n, k, sa, sb, bias=bias, act=act, resid=rs, expect=route, ex=True)
                az = G.activation64(z64, act)
                want = az + (rs.double() if with_resid else 0)
                bound = 2 * G.U * (az.abs() + (rs.double().abs() if with_resid else 0))
                bad = (y.double() - want).abs() > bound
                assert not bad.any(), f'{route} act={act} bias={with_bias} resid={with_resid}: {int(bad.sum())} entries off'
                if act == 1:
                    assert (y[z <= 0] == (rs[z <= 0] if with_resid else 0)).all()
                if not with_resid and act != 2:
                    assert torch.equal(y, az.float())


@pytest.mark.parametrize('route', EPILOGUE_ROUTES)
def test_gemm_ex_exact_zero_and_negative_preactivations(route):
    """Small integers: A W^T + b is an exact integer on every route (three bf16 planes included), built to be exactly 0 along row 0, along
    column 0 and wherever the integers cancel.  There relu(0) = leaky(0) = 0 exactly; everywhere else the output is the exact integer, its ReLU, or
    fp32(0.2) x the negative integer rounded once."""
    m, n, k = EX_SHAPES[route]
    g = _gen(9)
    a = torch.randint(-2, 3, (m, k), generator=g, device='cuda').float()
    w = torch.randint(-2, 3, (n, k), generator=g, device='cuda').float()
    w[0] = 0
    bias = -(a[0].double() @ w.double().t()).float()                # row 0 of A W^T + b is exactly zero; bias[0] = 0 and column 0 is zero as well
    z_exact = (a.double() @ w.double().t() + bias.double())
    assert (z_exact[0] == 0).all() and (z_exact[:, 0] == 0).all() and (z_exact < 0).any() and z_exact.abs().max() < 2 ** 24
    sa, sb = G.stored_pair(a, w, 0, 1)
    for act in (0, 1, 2):
        y, _ = launch(0, 1, m, n, k, sa, sb, bias=bias, act=act, expect=route, ex=True)
        want = G.activation64(z_exact, act).float()
        assert torch.equal(y, want), f'{route} act={act}: {(y != want).sum().item()} entries differ from exact integer arithmetic'
        assert (y[0] == 0).all() and (y[:, 0] == 0).all() and not torch.isnan(y).any()


# ------------------------------------------------------------------------------------------------ sga_gemm_bnstats on the half-tile routes
@pytest.mark.parametrize('rows', [163840, 163841])
@pytest.mark.parametrize('k,route', [(128, 'NT_64'), (256, 'NT3_64')])
def test_bnstats_on_half_tiles(rows, k, route):
    """The statistics epilogue on the 64-row tile kernels, at the PCT production row count and one row more (a last tile of one row): fp64 column sums
    and sums of squares of the y that was written, to 1e-6 of their largest; y itself under the accuracy gate."""
    from sgaligner_amd import _lib, ops
    n = 128
    a, bt = G.logical_operands(rows, n, k, rows + k)
    bt = bt * 0.1
    bias = torch.randn(n, generator=_gen(1), device='cuda')
    y = torch.empty(rows, n, device='cuda')
    sums = torch.full((2 * n,), float('nan'), device='cuda', dtype=torch.float64)
    assert G.plan_of(0, 1, rows, n, k, a, bt, y, bias=bias, colstats=True)[0] == route, f'this shape no longer reaches {route}'
    rc = _lib.lib().sga_gemm_bnstats(rows, n, k, a.data_ptr(), k, bt.data_ptr(), k, y.data_ptr(), n, bias.data_ptr(), sums.data_ptr(), ops._stream())
    _lib.check(rc, 'sga_gemm_bnstats')
    yd = y.double()
    exact = torch.cat([yd.sum(0), (yd * yd).sum(0)])
    assert (sums - exact).abs().max() <= 1e-6 * exact.abs().max(), ((sums - exact).abs().max().item(), exact.abs().max().item())
    sample = torch.cat([torch.arange(0, 200), torch.arange(rows - 200, rows), torch.arange(0, rows, 41)]).unique()
    G.assert_gate(y, a, bt, r_for(route, k), bias=bias, rows=sample, what=f'bnstats y {route} {rows} rows')
    y2, _ = launch(0, 1, rows, n, k, a, bt, bias=bias, expect=route)
    assert torch.equal(y, y2)                                        # the statistics do not change what is written


# ------------------------------------------------------------------------------------------------ sga_colsum, sga_cast_f64_f32
@pytest.mark.parametrize('m', [1, 2048, 2049, 131072, 131073, 300000])
def test_colsum(m):
    """Column sums against fp64: plain store up to 2048 rows, atomics above, the grid capped at 512 row groups above 131 072 rows (rows wrap).
    Tolerance per column: 4 x sqrt(M) 2^-23 sum|x| -- one rounding per addition with random signs grows like sqrt(M) ulps of the running
    sum (<= sum|x|); the factor 4 covers the four-walker fold and the order of the atomics."""
    from sgaligner_amd import _lib, ops
    g = _gen(m)
    for n in (1, 64, 65, 1000):
        parent = torch.randn(m, n + 7, generator=g, device='cuda')
        for x in (parent[:, :n].contiguous(), parent[:, 3:3 + n]):
            exact, mass = x.double().sum(0), x.double().abs().sum(0)
            tol = 4 * (m ** 0.5) * 2.0 ** -23 * mass
            out = torch.full((n + 2,), float('nan'), device='cuda')
            _lib.check(_lib.lib().sga_colsum(x.data_ptr(), x.stride(0), m, n, out[1:].data_ptr(), 0, ops._stream()), 'sga_colsum')
            assert torch.isnan(out[0]) and torch.isnan(out[n + 1])
            err = (out[1:n + 1].double() - exact).abs()
            print(f'[colsum] M={m} N={n} ld={x.stride(0)}: worst err / tol {(err / tol).max().item():.4f}')
            assert (err <= tol).all(), (m, n, (err / tol).max().item())
            o0 = torch.randn(n, generator=g, device='cuda') * (mass / m ** 0.5).float()      # the size of a column sum; one more summand of the bound
            o1 = o0.clone()
            _lib.check(_lib.lib().sga_colsum(x.data_ptr(), x.stride(0), m, n, o1.data_ptr(), 1, ops._stream()), 'sga_colsum')
            err = (o1.double() - (exact + o0.double())).abs()
            assert (err <= 4 * ((m + 1) ** 0.5) * 2.0 ** -23 * (mass + o0.double().abs())).all(), (m, n, 'accumulate')


def test_colsum_no_rows_and_no_columns():
    from sgaligner_amd import _lib, ops
    out = torch.full((5,), float('nan'), device='cuda')
    assert _lib.lib().sga_colsum(None, 3, 0, 3, out[1:].data_ptr(), 0, ops._stream()) == 0
    assert torch.equal(out[1:4], torch.zeros(3, device='cuda')) and torch.isnan(out[0]) and torch.isnan(out[4])
    out = torch.full((5,), 2.0, device='cuda')
    assert _lib.lib().sga_colsum(None, 3, 0, 3, out.data_ptr(), 1, ops._stream()) == 0
    assert _lib.lib().sga_colsum(out.data_ptr(), 3, 7, 0, None, 0, ops._stream()) == 0
    assert (out == 2).all()


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 10 ** 7])
def test_cast_f64_f32_is_float(n):
    """Bit-equal to .float(): normals, subnormals (of fp32, and fp64 values below them), +-0, +-inf, NaN, values that round up across a binade,
    ties, |x| > FLT_MAX (-> inf)."""
    from sgaligner_amd import _lib, ops
    fmax = float(torch.finfo(torch.float32).max)
    special = torch.tensor([0.0, -0.0, float('inf'), float('-inf'), float('nan'), fmax, -fmax, fmax * (1 + 2.0 ** -26), fmax * (1 + 2.0 ** -24),
                            -fmax * (1 + 2.0 ** -24), 1e39, -1e300, 2.0 - 2.0 ** -25, 2.0 - 2.0 ** -24, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50,
                            1 + 3 * 2.0 ** -24, 2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -30), 2.0 ** -151, 1e-310,
                            -(2.0 ** -149), 3 * 2.0 ** -150, 0.1, -1 / 3], dtype=torch.float64)
    gen = torch.Generator().manual_seed(n)
    body = torch.randn(max(n, 1), generator=gen, dtype=torch.float64) * torch.exp2(torch.randint(-160, 130, (max(n, 1),), generator=gen).double())
    x = torch.cat([special, body])[:n] if n else torch.empty(0, dtype=torch.float64)
    if n >= 256:
        x[-special.numel():] = special                             # the tail block too
    xd = x.cuda()
    out = torch.full((n + 2,), float('nan'), device='cuda')
    rc = _lib.lib().sga_cast_f64_f32(xd.data_ptr() if n else None, out[1:].data_ptr() if n else None, n, ops._stream())
    assert rc == 0
    want = x.float()
    got = out[1:n + 1].cpu()
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    diff = got[ok].view(torch.int32) != want[ok].view(torch.int32)
    assert not diff.any(), f'{int(diff.sum())} values differ from .float(), first: {x[ok][diff][:4].tolist()} -> {got[ok][diff][:4].tolist()}'
    assert torch.isnan(out[0]) and torch.isnan(out[n + 1])


# ------------------------------------------------------------------------------------------------ LinearFn
def _linear_grads(t, k, dtype, seed):
    from sgaligner_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t, k, generator=g, dtype=torch.float64)
    if dtype == torch.float32:
        x = x.float().double()
    w = torch.randn(100, k, generator=g).double() * 0.1
    b = torch.randn(100, generator=g).double() * 0.1
    cot = torch.randn(t, 100, generator=g).double()
    xd = x.to(dtype).cuda().requires_grad_(dtype == torch.float32)
    wd, bd = w.float().cuda().requires_grad_(True), b.float().cuda().requires_grad_(True)
    y = ops.linear(xd, wd, bd)
    (y * cot.float().cuda()).sum().backward()
    return dict(x=x, w=w, b=b, cot=cot, y=y.detach(), gw=wd.grad, gb=bd.grad, gx=xd.grad)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('t,k', [(4095, 41), (4096, 41), (5000, 3), (4096, 164)])
def test_linear_fn_padding_branch(t, k, dtype):
    """LinearFn forward and its three gradients against fp64 (the operands are the fp32 values the op sees; an fp64 x is first rounded like
    .float()).  Weight gradients with k % 4 != 0 take the zero-padded TN route from t = 4096 on and the unpadded one below: both are judged by
    the gate of the route they run, the envelope being |dY|^T |X|."""
    from sgaligner_amd import ops
    o = _linear_grads(t, k, dtype, t + k)
    x32 = o['x'].float().cuda()
    w32, b32, cot32 = o['w'].float().cuda(), o['b'].float().cuda(), o['cot'].float().cuda()
    fwd = ops.gemm_plan(0, 1, t, 100, k, a_is_f64=dtype == torch.float64, has_bias=True)[0]
    G.assert_gate(o['y'], x32, w32, r_for(fwd, k), bias=b32, what=f'linear forward {fwd}')
    padded = k % 4 != 0 and t >= 4096
    kp = (k + 3) // 4 * 4 if padded else k
    gw_route = ops.gemm_plan(1, 0, 100, kp, t)[0]
    assert gw_route == ('TN_NARROW' if kp <= 8 else 'TN_SPLIT' if kp % 4 == 0 else 'GENERIC_F32'), gw_route
    G.assert_gate(o['gw'], cot32.t(), x32.t(), r_for(gw_route, t), what=f'linear dW {gw_route} padded={padded}')
    # dB: the column-sum bound of test_colsum
    exact, mass = cot32.double().sum(0), cot32.double().abs().sum(0)
    assert ((o['gb'].double() - exact).abs() <= 4 * t ** 0.5 * 2.0 ** -23 * mass).all()
    if dtype == torch.float32:
        gx_route = ops.gemm_plan(0, 1, t, k, 100)[0]
        G.assert_gate(o['gx'], cot32, w32.t(), r_for(gx_route, 100), what=f'linear dX {gx_route}')
    else:
        assert o['gx'] is None


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_linear_fn_padded_and_unpadded_branches_agree(dtype):
    """t = 4095 (unpadded: generic kernel) against t = 4096 (padded to k = 44: TN kernel) on the same first 4095 rows with a zero cotangent in the
    last: the two weight gradients are the same sum and must agree to the gate of either route against fp64."""
    from sgaligner_amd import ops
    k = 41
    g = torch.Generator().manual_seed(8)
    x = torch.randn(4096, k, generator=g, dtype=torch.float64).to(dtype)
    w = (torch.randn(100, k, generator=g) * 0.1).cuda()
    b = torch.zeros(100).cuda()
    cot = torch.randn(4096, 100, generator=g)
    cot[4095] = 0
    grads = []
    for t in (4095, 4096):
        wd = w.clone().requires_grad_(True)
        (ops.linear(x[:t].cuda(), wd, b) * cot[:t].cuda()).sum().backward()
        grads.append(wd.grad)
    assert ops.gemm_plan(1, 0, 100, 41, 4095)[0] == 'GENERIC_F32' and ops.gemm_plan(1, 0, 100, 44, 4096)[0] == 'TN_SPLIT'
    a, bt = cot[:4095].t().contiguous().cuda(), x[:4095].float().t().contiguous().cuda()
    ref, env, yard = G.reference(a, bt), G.envelope(a, bt), G.yardstick(a, bt).cuda()
    G.assert_gate(grads[0], a, bt, r_for('GENERIC_F32', 4095), what='dW unpadded', yard_c=yard, ref=ref, env=env)
    G.assert_gate(grads[1], a, bt, r_for('TN_SPLIT', 4096), what='dW padded', yard_c=yard, ref=ref, env=env)
    ye, rsum = G.rel_errors(yard, ref, env), r_for('GENERIC_F32', 4095) + r_for('TN_SPLIT', 4096)
    diff = G.rel_errors(grads[0], grads[1].double(), env)
    assert diff[0] <= rsum * ye[0] and diff[1] <= rsum * ye[1], (diff, ye)


# ------------------------------------------------------------------------------------------------ bit invariance
@pytest.mark.parametrize('k,whole,quarter', [(128, 'NT_64', 'NT_128'), (256, 'NT3_64', 'NT3_128')])
def test_half_tiles_and_full_tiles_give_equal_bits(k, whole, quarter):
    """163 840 x 128 rows take the 64-row tile kernel, their four 40 960-row quarters the 128-row one (256 CUs): equal bits, with bias + ReLU +
    residual."""
    m, n = 163840, 128
    a, bt = G.logical_operands(m, n, k, 77)
    g = _gen(3)
    bias, resid = torch.randn(n, generator=g, device='cuda'), torch.randn(m, n, generator=g, device='cuda')
    y, _ = launch(0, 1, m, n, k, a, bt, bias=bias, act=1, resid=resid, expect=whole)
    q = m // 4
    parts = [launch(0, 1, q, n, k, a[i * q:(i + 1) * q], bt, bias=bias, act=1, resid=resid[i * q:(i + 1) * q], expect=quarter)[0] for i in range(4)]
    assert torch.equal(y, torch.cat(parts))
    assert (y != resid).any()


CHUNK_ROUTES = {3: {'SMALL_F32', 'GENERIC_F32'}, 64: {'NT_128', 'SMALL_F32', 'GENERIC_F32'}, 128: {'NT_128', 'SMALL_F32', 'GENERIC_F32'},
                256: {'NT3_128', 'SMALL_F32', 'GENERIC_F32'}, 1024: {'NT3_128', 'GENERIC_F32'}}


@pytest.mark.parametrize('k', [3, 64, 128, 256, 1024])
def test_row_chunks_give_the_bits_of_the_whole_batch(k):
    """K < 4096: C = act(A W^T + b) + resid walked in chunks of 1, 37, 128 and 1000 rows equals the unchunked call bit for bit, on every route that
    takes an epilogue (N and alignment choose the route; the rows must not)."""
    m = 2600
    g = _gen(k)
    met = set()
    for n, la in ((100, 'plain'), (100, 'off1'), (300, 'off1'), (128, 'plain')):
        a, bt = G.logical_operands(m, n, k, 5 + k + n)
        sa, sb = G.store(a, la if k % 4 == 0 else 'plain'), G.store(bt, 'plain')
        bias, resid = torch.randn(n, generator=g, device='cuda'), torch.randn(m, n, generator=g, device='cuda')
        for act in (0, 2):
            y, plan = launch(0, 1, m, n, k, sa, sb, bias=bias, act=act, resid=resid)
            assert plan[0] in EPILOGUE_ROUTES and plan[1] == 1
            met.add(plan[0])
            for chunk in (1, 37, 128, 1000):
                out = torch.full((m, n), float('nan'), device='cuda')
                for r0 in (range(0, m, chunk) if chunk > 1 else (0, 1, 127, 128, m - 1)):
                    r1 = min(m, r0 + chunk)
                    _, p = launch(0, 1, r1 - r0, n, k, sa[r0:r1], sb, c=out[r0:r1], bias=bias, act=act, resid=resid[r0:r1])
                    assert p[:2] == plan[:2], (p, plan)
                done = ~torch.isnan(out[:, 0])
                assert torch.equal(out[done], y[done]), f'K={k} N={n} {plan[0]} act={act} chunk={chunk}'
    assert met == CHUNK_ROUTES[k], f'K = {k}: these shapes no longer reach {CHUNK_ROUTES[k] - met} (met {met})'


@pytest.mark.parametrize('k,whole,part', [(128, 'NT_64', 'NT_128'), (256, 'NT3_64', 'NT3_128')])
def test_row_chunks_of_the_half_tile_batch(k, whole, part):
    """The PCT production shape: 163 840 x 128 rows run on the 64-row tile kernels; walked in chunks of 1000, 128 and 37 rows (128-row tile kernel
    of the same arithmetic) and as single rows (a sample) the batch must come out with the same bits, bias + LeakyReLU + residual included."""
    m, n = 163840, 128
    a, bt = G.logical_operands(m, n, k, 78)
    g = _gen(4)
    bias, resid = torch.randn(n, generator=g, device='cuda'), torch.randn(m, n, generator=g, device='cuda')
    y, _ = launch(0, 1, m, n, k, a, bt, bias=bias, act=2, resid=resid, expect=whole)
    for chunk in (1000, 128, 37, 1):
        out = torch.full((m, n), float('nan'), device='cuda')
        starts = range(0, m, chunk) if chunk > 1 else (0, 1, 63, 64, 127, 128, 40959, 40960, 100001, m - 2, m - 1)
        for r0 in starts:
            r1 = min(m, r0 + chunk)
            _, p = launch(0, 1, r1 - r0, n, k, a[r0:r1], bt, c=out[r0:r1], bias=bias, act=2, resid=resid[r0:r1])
            assert p[:2] == (part, 1), f'a chunk of {r1 - r0} rows no longer reaches {part}: {p}'
        done = ~torch.isnan(out[:, 0])
        assert int(done.sum()) == (m if chunk > 1 else len(starts))
        assert torch.equal(out[done], y[done]), f'K={k} {whole} against {part} in chunks of {chunk}'


def test_rows_split_over_k_from_4096_on():
    """The documented end of the row-chunk promise: from K = 4096 on a plain A W^T + b of few rows is split over K (atomics on the generic
    kernel) while many rows take the NT kernel.  The launcher was left as it is (a K = 65 536 weight-gradient-like NT product of few rows needs
    the split); the header and INTEGRATION.md state the domain K < 4096.  Both forms pass their gates; with an epilogue there is no split and the
    bits are those of the whole batch again."""
    from sgaligner_amd import _lib
    k, n = 4096, 100
    ncu = _lib.lib().sga_device_cus()
    m = 128 * ncu
    a, bt = G.logical_operands(m, n, k, 1)
    bias = torch.randn(n, generator=_gen(2), device='cuda')
    y, plan = launch(0, 1, m, n, k, a, bt, bias=bias, expect='NT3_128')
    ys, plans = launch(0, 1, 64, n, k, a[:64], bt, bias=bias, expect='GENERIC_F32')
    assert plan[1] == 1 and plans[1] > 1
    G.assert_gate(ys, a[:64], bt, r_for('GENERIC_F32', k), bias=bias, what='64 rows, split')
    G.assert_gate(y[:4096], a[:4096], bt, r_for('NT3_128', k), bias=bias, what='whole batch (first 4096 rows)')
    z = torch.zeros(m, n, device='cuda')
    y1, _ = launch(0, 1, m, n, k, a, bt, bias=bias, resid=z, expect='NT3_128')
    y2, _ = launch(0, 1, 64, n, k, a[:64], bt, bias=bias, resid=z[:64], expect='NT3_128')
    assert torch.equal(y1[:64], y2) and torch.equal(y1, y)
