"""Self-tests of tests/loss_gate.py (no card): the stage references chained together ARE the oracle's loss and its autograd, the gate ratios
are the measured ones, the gate has teeth -- each seeded defect of the float32 yardstick (or of the emulated three-plane products) fails at
the r in use while the clean arithmetic passes -- and the census builder's conditions hold for every input the GPU tests build."""
import numpy as np
import pytest
import torch

import gemm_gate as G
import loss_gate as LG
from oracle import sga_oracle as O

F64, F32 = torch.float64, torch.float32


def _chain(E, weight, lv_ial, lv_icl, dd):
    """loss_gate.chain (M >= 2), or for a single table the same stages without joint, fusion weight and head."""
    idx = torch.cat([torch.as_tensor(np.asarray(dd[k]), dtype=torch.int32) for k in ('e1i', 'e2i', 'e1j', 'e2j')])
    A, J1, J2 = len(dd['e1i']), len(dd['e1j']), len(dd['e2j'])
    if len(E) > 1:
        r = LG.chain(E, weight, lv_ial, lv_icl, idx, A, J1, J2)
        return dict(loss=r['out'][0], icl_loss_unimodal=r['out'][1], icl_loss_multimodal=r['out'][2], ial_loss=r['out'][3], dE=r['dE'], dw=r['dw'],
                    dla=r['dla'], dlc=r['dlc'])
    z, nrm = LG.gather(E[0], idx)
    blocks = [LG.neg_blocks(z, z, A, J1, J2)]
    sums = LG.neg_sums(blocks, 0, A)
    an = LG.anchor_stage([z[:A] @ z[A:2 * A].t()], None, sums, LG.ALPHA, torch.tensor([1.0 / (A * A)], dtype=F64))
    cm, _, _, _ = LG.neg_coefs(blocks, an['gs_rows'].sum(2), None, 0, A)
    dz = LG.neg_grad_rows(cm[0], z, A, J1, J2)
    dz[:A] += an['dS'][0] @ z[A:2 * A]
    dz[A:2 * A] += an['dS'][0].t() @ z[:A]
    return dict(loss=an['terms_rows'].sum() / (A * A), dE=[LG.scatter(dz, None, z, nrm, idx, E[0].shape[0])[0]])


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('M,ragged', [(1, False), (2, False), (3, True), (4, False)])
def test_stage_chain_is_the_oracle(M, ragged):
    """fp64 round-off over a few thousand terms: 1e-12 relative, for the four loss values and every gradient."""
    from sgaligner_amd.synthetic import make_batch
    dd = make_batch(3, 9, 1, seed=M, ragged=ragged)
    T = int(np.asarray(dd['tot_obj_count']).sum())
    g = torch.Generator().manual_seed(M)
    mods = ['point', 'gat', 'rel', 'attr'][:M]
    E = [torch.randn(T, 11 + m, generator=g, dtype=F64) for m in range(M)]
    weight = 0.5 * torch.randn(M, 1, generator=g, dtype=F64)
    lv1, lv2 = 0.3 * torch.randn(M, generator=g, dtype=F64), 0.3 * torch.randn(M, generator=g, dtype=F64)
    leaves = [e.clone().requires_grad_(True) for e in E]
    w, la, lc = (t.clone().requires_grad_(True) for t in (weight, lv1, lv2))
    od = dict(zip(mods, leaves))
    if M > 1:
        od['joint'] = O.fusion(leaves, w)
    res = O.overall_loss(od, dd, mods, la, lc)
    res['loss'].backward()
    got = _chain(E, weight, lv1, lv2, dd)
    for k in ('loss', 'icl_loss_unimodal', 'icl_loss_multimodal', 'ial_loss'):
        if k in got:
            assert abs(float(got[k]) - float(res[k].detach())) <= 1e-12 * abs(float(res[k].detach())), k
    for m in range(M):
        assert _rel(got['dE'][m], leaves[m].grad) <= 1e-12, m
    if M > 1:
        assert _rel(got['dw'].reshape(-1), w.grad.reshape(-1)) <= 1e-12
        assert _rel(got['dla'], la.grad) <= 1e-12 and _rel(got['dlc'], lc.grad) <= 1e-12


def test_head_without_anchors_is_nan_like_the_reference():
    t, la, lc, _ = LG.head_refs(3, 0, 5)
    out = LG.head(t, la, lc, 0, 0.1, 0.5, 0.1)
    assert torch.isnan(out[:3]).all() and torch.isfinite(out[3])


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' of profiles/loss_accuracy_vs_fp32.json, per stage output and tier."""
    assert LG.ratios_from_profile() == LG.R
    tiers = ('plain', 'centred', 'planes')
    want = {f'{o}|{t}' for o in ('neg_sums.sums', 'neg_grad.dZ', 'neg_grad.gamma_neg', 'stash_grad.dZ') for t in tiers}
    want |= {f'{o}|f32' for o in ('gather.Z', 'gather.nrm', 'anchor_terms.terms', 'anchor_coef.dS', 'anchor_coef.gs', 'anchor_coef.gamma', 'scatter.dE',
                                  'head.head', 'head.dterms', 'head.dlv')}
    want |= {'scatter.dE|centred', 'scatter.dE|planes'}
    want |= {f'{o}|pertable' for o in ('neg_sums.sums', 'anchor_terms.terms', 'anchor_coef.dS', 'anchor_coef.gs', 'neg_grad.dZ')}
    want |= {f'group.{o}|{t}' for o in ('terms', 'dE', 'gamma') for t in ('mfma', 'valu')} | {'neg_grad.dZ|wide'}
    want |= {f'{o}|f16' for o in ('neg_sums.sums', 'neg_grad.dZ', 'stash_grad.dZ', 'anchor_terms.terms', 'anchor_coef.dS', 'anchor_coef.gs')}
    assert set(LG.R) == want


# ------------------------------------------------------------------------------------------------ the seeded defects
DEFECT_CASES = [c['name'] for c in LG.gate_cases()]          # every gate case: every shape, width, M and input kind


def _passes(key, out, ref, env, yard):
    ke, ye = LG.errors(out, ref, env), LG.errors(yard, ref, env)
    return LG.gate_ok(ke, ye, LG.R[key], LG.is_scalar(key.split('|')[0])), ke[:2], ye[:2]


@pytest.mark.parametrize('name', DEFECT_CASES)
def test_gate_catches_a_transposed_qb(name):
    """Defect 1: qB taken transposed in the A x A epilogue (the reference's quirk 'fixed')."""
    c, an = LG.case_inputs(name), LG.anchor_refs(name)
    A, D = c['A'], c['D']
    S32 = [LG.mm(z[:A, :D], z[A:2 * A, :D]) for z in c['Z']]
    bad = LG.anchor_stage(S32, c['beta'], an['sums'], LG.ALPHA, c['coef'], dt=F32, qb_transposed=True)
    ref, yard = an['ref'], an['yard']
    if A == 1 or c['kind'] == 'onehot':                    # S = S^T (one anchor; the one-hot classes alternate alike on both sides): transposing changes nothing
        assert all(torch.allclose(b, y, rtol=1e-5, atol=0) for b, y in zip(bad['dS'], yard['dS']))
        return
    for m in range(c['M']):
        assert _passes('anchor_coef.dS|f32', yard['dS'][m], ref['dS'][m], ref['env_dS'][m], yard['dS'][m])[0]
        ok, ke, ye = _passes('anchor_coef.dS|f32', bad['dS'][m], ref['dS'][m], ref['env_dS'][m], yard['dS'][m])
        assert not ok, (m, ke, ye)
    t = lambda d, k: d[k].sum(-1)
    ok, ke, ye = _passes('anchor_terms.terms|f32', t(bad, 'terms_rows'), t(ref, 'terms_rows'), t(ref, 'env_terms_rows'), t(yard, 'terms_rows'))
    assert not ok, (ke, ye)


@pytest.mark.parametrize('name', DEFECT_CASES)
@pytest.mark.parametrize('tier', ['plain', 'planes'])
def test_gate_catches_a_scatter_without_the_tangent_projection(name, tier):
    """Defect 2: dE = dZ / n, the component along the row not projected out."""
    c, sr = LG.case_inputs(name), LG.sweep_refs(name, tier)
    D = c['D']
    key = 'scatter.dE|' + ('f32' if tier == 'plain' else tier)
    for m in range(c['M']):
        ref, env, yard = sr['scatter'][m]
        assert _passes(key, yard, ref, env, yard)[0]
        dz = sr['dz_in'][m]
        zb, rho = (sr['zbar'][m], dz[:, 101]) if sr['centred'][m] else (None, None)
        bad, _ = LG.scatter(dz[:, :D], rho, c['Z'][m][:, :D], sr['nrm'][m], c['idx'], c['T'], zb, dt=F32, project=False)
        ok, ke, ye = _passes(key, bad, ref, env, yard)
        assert not ok, (m, ke, ye)


@pytest.mark.parametrize('name', DEFECT_CASES)
@pytest.mark.parametrize('tier', ['plain', 'centred', 'planes'])
def test_gate_catches_an_unnormalised_beta(name, tier):
    """Defect 3: the joint similarity with w^2 instead of beta = w^2 / sum w^2."""
    c, sr = LG.case_inputs(name), LG.sweep_refs(name, tier)
    A, J1, J2, D = c['A'], c['J1'], c['J2'], c['D']
    w2 = LG.fusion_weights(c['M'], c['seed']).pow(2).float()                  # w^2 without the division by sum w^2 (< 1 for softmax weights)
    assert float(w2.sum()) < 0.999
    sd = [LG.sides(i, A, J1, J2, D, tier != 'plain') for i in sr['img']]
    bad = LG.neg_sums(LG.with_joint([LG.neg_blocks(L, Rt, A, J1, J2) for L, Rt, _ in sd], w2), 0, A)
    ref, env, yard = sr[(0, A)]['sums']
    key = f'neg_sums.sums|{tier}'
    assert _passes(key, yard, ref, env, yard)[0]
    if c['kind'] == 'onehot':                               # every anchor x negative similarity is 0 (to the centring's rounding), and so is any weighted sum of them
        assert torch.allclose(bad, ref, rtol=1e-6)
        return
    ok, ke, ye = _passes(key, bad, ref, env, yard)
    assert not ok, (ke, ye)


def _planes_rows(c, V, A, J1, J2, nprod):
    """loss_gate.neg_grad_rows with every product on the emulated bf16 planes."""
    pp = lambda a, bt: G.planes_product(a, bt.contiguous(), nprod)
    x1, x2, n1, n2 = LG.segments(V, A, J1, J2)
    c11, c12, c22, c21 = c
    return torch.cat([pp(c11, n1.t()) + pp(c12, n2.t()), pp(c22, n2.t()) + pp(c21, n1.t()),
                      pp(c11.t(), x1.t()) + pp(c21.t(), x2.t()), pp(c12.t(), x1.t()) + pp(c22.t(), x2.t())])


PLANE_CASES = [c['name'] for c in LG.gate_cases()]


def plane_defect_verdicts(name, which):
    """(the six-product emulation passes for every table, five products pass for SOME table) at the r in use; which: 'neg_grad' or 'stash_grad'."""
    c, sr = LG.case_inputs(name), LG.sweep_refs(name, 'planes')
    A, J1, J2, D = c['A'], c['J1'], c['J2'], c['D']
    six_ok, five_ok = True, False
    if which == 'neg_grad':
        sd = [LG.sides(i, A, J1, J2, D, True) for i in sr['img']]
        bl = LG.with_joint([LG.neg_blocks(L, Rt, A, J1, J2) for L, Rt, _ in sd], c['beta'])
        cm, _, _, _ = LG.neg_coefs(bl, sr['gs'], c['beta'], 0, A)
    cols = sr['cols']
    for m in range(c['M']):
        if which == 'neg_grad':
            ref, env, yard = sr[(0, A)]['dZ'][m]
            emu = lambda n: _planes_rows(cm[m], sd[m][2], A, J1, J2, n)
        else:
            ref, env, yard = (t[:, cols] for t in sr['stash'][m])
            m1, b1, b2 = sr['m1'][m], sr['img'][m][:A][:, cols], sr['img'][m][A:2 * A][:, cols]
            emu = lambda n: torch.cat([G.planes_product(m1, b2.t().contiguous(), n), G.planes_product(m1.t().contiguous(), b1.t().contiguous(), n)])
        key = f'{which}.dZ|planes'
        six_ok &= _passes(key, emu(6), ref, env, yard)[0]
        five_ok |= _passes(key, emu(5), ref, env, yard)[0]
    return six_ok, five_ok


@pytest.mark.parametrize('which', ['neg_grad', 'stash_grad'])
@pytest.mark.parametrize('name', PLANE_CASES)
def test_gate_catches_a_dropped_plane_product(name, which):
    """Defects 4 and 5: c Z (the negatives' gradient) and the A x A stash products on five of the six partial products of the bf16 planes,
    at every gate case, the smallest J included.  Six products pass; five FAIL -- or the case is listed in loss_gate.UNGATED for that
    output, and only then: the list holds exactly the cases where the gate at the r in use is blind to the omission."""
    six_ok, five_ok = plane_defect_verdicts(name, which)
    listed = name in LG.UNGATED[f'{which}.dZ|planes']
    assert six_ok, 'the six-product emulation misses the gate'
    if LG.case_inputs(name)['A'] == 1 and listed:           # three rows: the verdict hangs on single roundings of the host's fp64 products (seen to differ between two machines)
        return
    assert five_ok == listed, f'five products {"pass" if five_ok else "fail"} the gate here, but the case is {"" if listed else "not "}listed in UNGATED'


# ------------------------------------------------------------------------------------------------ the tier 'f16'
F16_CASES = [c['name'] for c in LG.f16_cases()]
F16_DEFECTS = {'neg_sums.sums|f16': ('k_group',), 'neg_grad.dZ|f16': ('last_row', 'straddle')}


def f16_defect_verdicts(name, key):
    """(the clean yardstick passes its own gate, SOME seeded defect of this output passes too) at the r in use."""
    clean_ok, slipped = True, []
    for defect in F16_DEFECTS[key]:
        v = LG.f16_defect(name, defect)
        if v is None:                                       # no K group straddles the end of a block of A % 8 == 0 anchors
            assert defect == 'straddle' and LG.f16_case(name)['A'] % 8 == 0
            continue
        k, bad, ref, env, yard = v
        assert k == key
        clean_ok &= _passes(key, yard, ref, env, yard)[0]
        ok, ke, ye = _passes(key, bad, ref, env, yard)
        if ok:
            slipped.append((defect, ke, ye))
    return clean_ok, slipped


@pytest.mark.parametrize('key', sorted(F16_DEFECTS))
@pytest.mark.parametrize('name', F16_CASES)
def test_f16_gate_catches_the_seeded_defects(name, key):
    """Three emulated wide16 kernels, at every gate case of the tier 'f16': (a) S without the last 8-column K group of the table (columns
    128 .. 135 of 136) in the sums; (b) the negatives' gradient without the last anchor row of the row block; (c) the straddling K group of
    the C^T product not zeroed -- a copy of the last anchor's coefficients meets the next packed row.  The clean arithmetic passes; each
    defect FAILS at the r in use -- or the case is listed in loss_gate.UNGATED for that output, and only then."""
    clean_ok, slipped = f16_defect_verdicts(name, key)
    listed = name in LG.UNGATED.get(key, ())
    assert clean_ok, 'the clean yardstick misses its own gate'
    assert bool(slipped) == listed, f'{slipped or "every defect fails the gate"}, but the case is {"" if listed else "not "}listed in UNGATED'


def test_f16_ungated_cases_are_few():
    """At most one third of the gate cases of an output may go ungated; the census covers the rest."""
    for key in F16_DEFECTS:
        listed = LG.UNGATED.get(key, ())
        assert set(listed) <= set(F16_CASES) and 3 * len(listed) <= len(F16_CASES), key


def test_f16_yardstick_operands():
    """The float32 restatement of csrc/wide16.hip's operands: ZhT keeps every segment on the 8-column grid with zeros between them; the
    stash operand's largest magnitude lies in [2^13, 2^14) and the scaling is undone exactly; the coefficients are at most 1 in magnitude."""
    c = LG.f16_inputs('f16-cluster-A33-31-65-D136')
    A, J1, J2 = c['A'], c['J1'], c['J2']
    starts, ldt = LG.seg_cols(A, J1, J2)
    assert starts == (0, 40, 80, 112) and ldt == 184 and tuple(c['zt'].shape) == (136, ldt)
    used = torch.zeros(ldt, dtype=torch.bool)
    for s0, n in zip(starts, (A, A, J1, J2)):
        used[s0:s0 + n] = True
    assert not c['zt'][:, ~used].any() and torch.equal(c['zt'][:, :A].t(), c['zh'][:A]) and torch.equal(c['zt'][:, 112:112 + J2].t(), c['zh'][2 * A + J1:])
    m1 = LG.f16_m1(c['name'])
    mh, back = LG.f16_stash_operand(m1)
    assert 2.0 ** 13 <= float(mh.abs().max()) < 2.0 ** 14 + 8 and back == 2.0 ** round(np.log2(back))
    fr = LG.f16_refs(c['name'])
    ch = LG.f16_coefs(fr[(0, A)]['c32'], fr['bounds'])
    assert all(float(x.abs().max()) <= 1.0 for x in ch) and any(float(x.abs().max()) > 0 for x in ch)


# ------------------------------------------------------------------------------------------------ the census
CENSUS_SHAPES = [(33, 31, 65, 37), (129, 21, 75, 64), (65, 127, 63, 97), (257, 40, 9, 100), (333, 17, 50, 100), (32, 32, 32, 104), (63, 64, 129, 101)]


@pytest.mark.parametrize('A,J1,J2,D', CENSUS_SHAPES)
@pytest.mark.parametrize('M', [2, 3, 4])
def test_census_conditions_and_integer_sums(A, J1, J2, D, M):
    """The builder's assertions hold (>= 5 even classes a side, centring off, counts <= 8 in every shard and segment), the rows normalise
    exactly, and the reference sums -- fp64 and the float32 yardstick alike -- are the integers."""
    tabs, idx, T, cls = LG.census(A, J1, J2, D, M, seed=A + M, shards=[(0, A)] + LG.shards3(A))
    beta = LG.fusion_beta(M, A)
    for dt in (F64, F32):
        Z = [LG.gather(e, idx, dt)[0] for e in tabs]
        for z in Z:
            assert torch.equal(z, (z != 0).to(dt)) and torch.equal(z.sum(1), torch.ones(z.shape[0], dtype=dt))
        bl = LG.with_joint([LG.neg_blocks(z, z, A, J1, J2) for z in Z], beta.to(dt))
        assert all(not b.any() for k in bl for b in k)
        for lo, hi in [(0, A)] + LG.shards3(A):
            assert torch.equal(LG.neg_sums(bl, lo, hi), LG.census_sums(hi - lo, J1, J2, M + 1))
    if D <= 100:
        assert not LG.centre_image(Z[0].float(), D)[2]


@pytest.mark.parametrize('A,J1,J2', [(33, 31, 65), (129, 21, 75), (65, 127, 63), (257, 40, 9), (333, 17, 50), (63, 64, 129), (24, 2305, 40), (2305, 17, 0), (2305, 257, 0)])
def test_census_of_136_columns_for_the_fp16_kernels(A, J1, J2):
    """The 136-column census of the wide fp16 kernels: one-hot rows are their own fp16 rounding, the sums are the integers in whole and in
    shards on the 8-anchor grid, and where the segments are short enough the counts stay <= 8 in every such shard (J2 = 0 included)."""
    limited = max(A, J1) <= 400
    tabs, idx, _, _ = LG.census(A, J1, J2, 136, 1, seed=A + 1, count_limit=limited, shards=[(0, A)] + LG.shards8(A))
    z = LG.gather(tabs[0], idx)[0]
    assert torch.equal(z.to(torch.float16).double(), z) and torch.equal(LG.prepare_ref(z.float(), A, J1, J2)[0].double(), z)
    bl = [LG.neg_blocks(z, z, A, J1, J2)]
    sh = LG.shards8(A)
    assert sh[0][0] == 0 and sh[-1][1] == A and all(lo % 8 == 0 and lo < hi for lo, hi in sh) and all(a[1] == b[0] for a, b in zip(sh, sh[1:]))
    for lo, hi in [(0, A)] + sh:
        assert torch.equal(LG.neg_sums(bl, lo, hi), LG.census_sums(hi - lo, J1, J2, 1))


def test_census_of_the_work_unit_shape_has_integer_sums_only():
    """(300, 5500, 5500): the sums are integers; the count condition cannot hold (5500 rows over 50 classes) and is not asked."""
    LG.census(300, 5500, 5500, 100, 3, seed=1, count_limit=False)
    with pytest.raises(AssertionError):
        LG.census(300, 5500, 5500, 100, 3, seed=1)
    assert float(LG.census_sums(300, 5500, 5500, 4).max()) < 2.0 ** 53
