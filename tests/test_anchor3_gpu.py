"""GPU: sga_loss_anchor_multi_bwd_symx_bf16x6 (csrc/anchor3.hip) -- the anchors x anchors backward with its similarities formed from the
three-plane image on the bf16 matrix pipe.  It is held to what the fp32 kernel is held to: the gate of tests/loss_gate.py at the fp32
kernel's own r (references: the fp64 chain and the float32 yardstick, never a kernel), the fp32 entry on edge shapes at the tolerances
tests/test_onepass_gpu.py uses between walks, refusals, and the product routes that take it."""
import functools
from unittest import mock

import pytest
import torch

import loss_gate as LG

pytestmark = pytest.mark.gpu

ENTRY = LG.AA_PLANES
GATE = [c['name'] for c in LG.gate_cases() if c['D'] <= 100 and c['M'] in (2, 3)]
NAN = LG.NAN


@pytest.mark.parametrize('name', GATE)
def test_gate_at_the_fp32_kernel_s_r(name):
    """Every gate case with D <= 100 and M in {2, 3}, every walk of loss_gate.aa_walks (ordered blocks with a ragged last one, the symmetric
    walk under a stash bound that forces >= 3 blocks, the three-rank walk with wrapped columns): terms, EVERY element of dL/dS_m + beta_m
    dL/dS_J, dL/d(sums), dL/dbeta at R['anchor_*|f32'].  No stash element stays NaN, none is produced twice with two values."""
    c = LG.case_inputs(name)
    an = LG.anchor_refs(name)
    A, M = c['A'], c['M']
    T = LG.tier_images(name, 'planes')
    ref, yard = an['ref'], an['yard']
    tot = lambda k, d: d[k].sum(-1)
    t3 = (tot('terms_rows', ref), tot('env_terms_rows', ref), tot('terms_rows', yard))

    def rows():
        for label, jobs, sym in LG.aa_walks(A, M):
            dS, terms, gs, gam = LG.run_anchor_bwd(ENTRY, T.t.planes, (A, c['J1'], c['J2']), c['beta'], an['sums'], c['coef'], jobs)
            yield LG._row('anchor_terms.terms', 'f32', terms, *t3)
            for m in range(M):
                yield LG._row('anchor_coef.dS', 'f32', dS[m], ref['dS'][m], ref['env_dS'][m], yard['dS'][m])
            yield LG._row('anchor_coef.gs', 'f32', gs, tot('gs_rows', ref), tot('env_gs_rows', ref), tot('gs_rows', yard))
            yield LG._row('anchor_coef.gamma', 'f32', gam, tot('gamma_rows', ref), tot('env_gamma_rows', ref), tot('gamma_rows', yard))

    LG.assert_gate(rows(), f'{name} anchor3')


@functools.lru_cache(maxsize=None)
def _edge(A, M):
    """Random unit rows of width 100 (negatives: a handful, the image needs the segments), both entries' inputs."""
    J1, J2, D = 33, 17, 100
    g = torch.Generator().manual_seed(7 * A + M)
    R = 2 * A + J1 + J2
    Z = [torch.nn.functional.normalize(torch.randn(R, D, generator=g, dtype=torch.float64), dim=1).float() for _ in range(M)]
    T = LG.Tier('planes', Z, None, A, J1, J2, D)
    sums = torch.rand(M + 1, 8, generator=g, dtype=torch.float64) * 1e3 + 1e3
    beta = torch.softmax(torch.randn(M, generator=g), 0)
    coef = ((torch.rand(3 * M + 1, generator=g) + 0.5) * 1e-2).float()
    return T, sums, beta, coef


def _against_fp32(A, M, jobs, sym):
    """The new entry against the fp32 entry on the same inputs and jobs: terms 1e-6, stashes 2e-5 of the maximum, the same elements produced."""
    T, sums, beta, coef = _edge(A, M)
    want = LG.run_anchor_bwd(LG.AA_SYMX if sym else LG.AA_ORDERED, T.zs, (A,), beta, sums, coef, jobs)
    got = LG.run_anchor_bwd(ENTRY, T.t.planes, (A, T.J1, T.J2), beta, sums, coef, jobs)
    for m in range(M):
        assert torch.equal(torch.isnan(got[0][m]), torch.isnan(want[0][m])), 'the two entries produce different elements'
        ok = ~torch.isnan(want[0][m])
        d, mx = (got[0][m][ok] - want[0][m][ok]).abs().max().item(), want[0][m][ok].abs().max().item()
        print(f'[anchor3] A={A} M={M} table {m}: stash max diff {d:.3e} of max {mx:.3e}')
        assert d <= 2e-5 * mx
    for k, what in ((1, 'terms'), (2, 'gs'), (3, 'gamma')):
        d, mx = (got[k] - want[k]).abs().max().item(), want[k].abs().max().item()
        print(f'[anchor3] A={A} M={M} {what}: max diff {d:.3e} of max {mx:.3e}')
        assert d <= (1e-6 if what == 'terms' else 2e-5) * mx
    return got, want


@pytest.mark.parametrize('M', [2, 3])
@pytest.mark.parametrize('A', [97, 127])
def test_edge_walks_against_the_fp32_entry(A, M):
    """A = 97: the smallest A with a symmetric walk and a one-row last block; A = 127; both with a_hi == A off the grid, and the ordered walk
    with M2 == NULL."""
    for label, jobs, sym in LG.aa_walks(A, M):
        got, _ = _against_fp32(A, M, jobs, sym)
        assert not any(torch.isnan(d).any() for d in got[0]), label


@pytest.mark.parametrize('M', [2, 3])
@pytest.mark.parametrize('job', [(32, 96, 32, 160, 96), (0, 64, 96, 160, 96), (128, 160, 128, 160, 160)])
def test_edge_rectangles_against_the_fp32_entry(job, M):
    """A = 160: a block with its square and mirrored columns, a rectangle with no own square, and a symmetric job whose mirror start is its
    column end (M2 == NULL)."""
    _against_fp32(160, M, [job], True)


def test_exact_similarities_give_the_fp32_entry_s_stashes():
    """The onehot gate case: the similarities are exact in both arithmetics, so the stashes equal the fp32 entry's to 1 ulp elementwise, with
    identical NaN coverage."""
    name = next(n for n in GATE if n.startswith('onehot'))
    c = LG.case_inputs(name)
    an = LG.anchor_refs(name)
    A, M = c['A'], c['M']
    T = LG.tier_images(name, 'planes')
    P = LG.tier_images(name, 'plain')
    for label, jobs, sym in LG.aa_walks(A, M):
        want = LG.run_anchor_bwd(LG.AA_SYMX if sym else LG.AA_ORDERED, P.zs, (A,), c['beta'], an['sums'], c['coef'], jobs)[0]
        got = LG.run_anchor_bwd(ENTRY, T.t.planes, (A, c['J1'], c['J2']), c['beta'], an['sums'], c['coef'], jobs)[0]
        for m in range(M):
            assert torch.equal(torch.isnan(got[m]), torch.isnan(want[m]))
            ok = ~torch.isnan(want[m])
            g, w = got[m][ok], want[m][ok]
            inf = torch.full_like(w, float('inf'))
            ulp = torch.maximum(torch.nextafter(w, inf) - w, w - torch.nextafter(w, -inf))
            worst = ((g - w).abs() / ulp).max().item()
            print(f'[anchor3] onehot {label} table {m}: worst {worst:.2f} ulp')
            assert worst <= 1.0


@pytest.mark.parametrize('bad', ['a_lo', 'mir', 'M4'])
def test_refusals_launch_nothing(bad):
    lib, L, p, pa, st = LG._abi()
    A, M = 160, (4 if bad == 'M4' else 3)
    T, sums, beta, coef = _edge(A, 3)
    planes = (T.t.planes * 2)[:M]
    job = {'a_lo': (8, 64, 0, 160, 160), 'mir': (0, 64, 0, 160, 72), 'M4': (0, 64, 0, 160, 160)}[bad]
    nt = M + 1
    gsc = torch.full((LG._slots() + 1, nt, 8), NAN, device='cuda', dtype=torch.float64)
    gam = torch.full((LG._slots(), M), NAN, device='cuda', dtype=torch.float64)
    out = torch.full((LG._slots() * (3 * M + 1),), NAN, device='cuda', dtype=torch.float64)
    m1 = [torch.full((160 * 64,), NAN, device='cuda') for _ in range(M)]
    m2 = [torch.full((160 * 64,), NAN, device='cuda') for _ in range(M)]
    b = torch.full((M,), 1.0 / M, device='cuda')
    cf = torch.full((3 * M + 1,), 1e-2, device='cuda')
    s = torch.full((nt, 8), 1e3, device='cuda', dtype=torch.float64)
    rc = getattr(L, ENTRY)(pa(planes), M, p(b), A, T.J1, T.J2, p(s), 0.5, 0.1, 1.0, p(cf), pa(m1), pa(m2), p(gsc), p(gam), *job, p(out), st)
    torch.cuda.synchronize()
    assert rc != 0 and ENTRY.encode() in L.sga_last_error()
    for t in [gsc, gam, out] + m1 + m2:
        assert torch.isnan(t).all(), 'a refused call wrote something'


NEW_PLANES = {'sga_loss_split3_tables', 'sga_loss_multi_sums_bf16x6', ENTRY, 'sga_loss_stash_grad_symx_bf16x6', 'sga_loss_multi_grad_bf16x6',
              'sga_loss_scatter_tangent'}
ROUTES = {
    # name: (the route of test_loss_gate_gpu.ROUTES it starts from, more switches, the loss entry points that must run -- exactly)
    'sym': ('planes-onepass-sym', dict(AA_PLANES_MIN_ANCHORS=0), NEW_PLANES),
    'sym-default-constant': ('planes-onepass-sym', dict(), None),                       # None: the old route's own set -- the fp32 entry runs
    'ordered': ('planes-onepass-ordered', dict(AA_PLANES_MIN_ANCHORS=0), NEW_PLANES),
    'twopass': ('planes-twopass', dict(AA_PLANES_MIN_ANCHORS=0), NEW_PLANES | {'sga_loss_anchor_multi_fwd'}),
    'switched-off': ('planes-onepass-sym', dict(AA_PLANES_MIN_ANCHORS=0, AA_PLANES=False), None),
}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_routes_end_to_end(route):
    """test_loss_gate_gpu.test_overall_loss_end_to_end itself (its batch, its recorder, its gate rows at its r) on the routes that take the new
    entry once AA_PLANES_MIN_ANCHORS admits the batch, symmetric, ordered and two-pass; with the default constant, or switched off, the old
    entry runs."""
    import test_loss_gate_gpu as TG
    from sgaligner_amd import ops
    base, switches, expect = ROUTES[route]
    D, mode, sw, old = TG.ROUTES[base]
    assert ops.AA_PLANES and ops.AA_PLANES_MIN_ANCHORS >= 1024
    with mock.patch.dict(TG.ROUTES, {base: (D, mode, dict(sw, **switches), old if expect is None else expect)}):
        TG.test_overall_loss_end_to_end(base)
