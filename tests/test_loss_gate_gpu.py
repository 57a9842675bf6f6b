"""GPU: the loss kernels at the C ABI against the fp64 stage references of tests/loss_gate.py -- every stage output of the fused path gated
at r x the float32 yardstick's envelope-relative error (gate), and the census: exact inputs on which every global sum is an integer and
every entry of the negatives' gradient a small count times one constant, so that one lost, doubled or misplaced pair shows.  Shapes sit on
the tile geometry's edges (loss_gate.gate_cases); outputs a kernel must write are pre-filled with NaN.  The wide fp16 kernels (mode 'f16':
csrc/wide16.hip and the Zh forms of the per-table A x A kernels) have a tier of their own, 'f16' (loss_gate.f16_cases), their operands
pinned bit for bit, and their routes through ops.contrastive_terms pinned end to end, a batch in shards included."""
import pytest
import torch

import gemm_gate as G
import loss_gate as LG

pytestmark = pytest.mark.gpu

CASES = LG.gate_cases() + LG.plain_cases()
NAMES = [c['name'] for c in CASES]
TIERED = [(c['name'], t) for c in CASES for t in LG.tier_for(c)]
CENTRED = [(n, t) for n, t in TIERED if t != 'plain']


@pytest.mark.parametrize('name', NAMES)
def test_gather_gate(name):
    """sga_loss_gather at Dp = 104 and at D padded to 8: rows of norm 2^-20 .. 2^20, the padding columns zero."""
    LG.assert_gate(LG.measure_gather(name), name)


@pytest.mark.parametrize('name', NAMES)
def test_anchor_terms_and_coefficients_gate(name):
    """sga_loss_anchor_multi_fwd (whole and as three shards), and sga_loss_anchor_multi_bwd in ordered blocks with a ragged last one,
    sga_loss_anchor_multi_bwd_symx over the symmetric walk of one rank and of three ranks (wrapped columns) under a stash bound that forces
    >= 3 blocks: the terms, EVERY element of dL/dS_m + beta_m dL/dS_J, dL/d(sums) and dL/dbeta.  No stash element stays NaN, none is
    produced twice with two values."""
    LG.assert_gate(LG.measure_anchor(name), name)


@pytest.mark.parametrize('name,tier', CENTRED)
def test_centred_images_are_the_library_s(name, tier):
    """sga_loss_centre_tables / sga_loss_split3_tables make the centred rows loss_gate.centre_image states (the sweeps' stated input)."""
    LG.measure_centring(name, tier)


@pytest.mark.parametrize('name,tier', TIERED)
def test_neg_sums_gate(name, tier):
    """sga_loss_multi_sums / _centred / _bf16x6 (lite = 0): the 8 (M + 1) sums, whole and per shard of three cut off the 32-row grid."""
    LG.assert_gate(LG.measure_sums(name, tier), f'{name} {tier}')


@pytest.mark.parametrize('name,tier', TIERED)
def test_neg_grad_gate(name, tier):
    """sga_loss_multi_grad / _centred / _bf16x6: dZ of every row and dL/dbeta through the negatives, unsharded and as three shards replayed
    into the same buffers; nothing outside the rows and columns the kernel owns."""
    LG.assert_gate(LG.measure_grad(name, tier), f'{name} {tier}', case=name)


@pytest.mark.parametrize('name,tier', TIERED)
def test_stash_grad_gate(name, tier):
    """sga_loss_stash_grad (ordered blocks), sga_loss_stash_grad_symx with the plain and the centred B operand, and
    sga_loss_stash_grad_symx_bf16x6, over the same walks as the A x A kernels."""
    LG.assert_gate(LG.measure_stash(name, tier), f'{name} {tier}', case=name)


@pytest.mark.parametrize('name,tier', TIERED)
def test_scatter_gate(name, tier):
    """sga_loss_scatter, sga_loss_scatter_tangent_stat, sga_loss_scatter_tangent: the normalisation's Jacobian and the row scatter
    (one case repeats an object inside e1j / e2j: duplicates are summed)."""
    LG.assert_gate(LG.measure_scatter(name, tier), f'{name} {tier}')


@pytest.mark.parametrize('name', LG.pertable_cases())
@pytest.mark.parametrize('nt', [1, 4])
def test_per_table_kernels_gate(name, nt):
    """The per-table route (any joint table): sga_loss_neg_sums_shard, sga_loss_anchor_fwd_f16 / _bwd_f16 with Zh = NULL and
    sga_loss_neg_grad_shard on tables of pitch D padded to 8, NT = 1 and NT = M + 1, whole and as three shards."""
    LG.assert_gate(LG.measure_pertable(name, nt), f'{name} NT={nt}')


@pytest.mark.parametrize('M,b,valu', LG.GROUP_CASES)
def test_group_loss_gate(M, b, valu):
    """sga_group_loss_fwd / _bwd, MFMA and VALU forms, M = 1 .. 4: groups of ragged size, one of a single anchor; every group's terms, dE and
    dL/dbeta against the stages restricted to the group's own rows."""
    LG.assert_gate(LG.measure_group(M, b, valu), f'group M={M} b={b} valu={valu}')


@pytest.mark.parametrize('name', LG.wide_cases())
def test_wide_neg_grad_gate(name):
    """sga_loss_neg_grad_wide (136 columns): one block, and a stash bound that forces several anchor-row blocks."""
    LG.assert_gate(LG.measure_wide(name), name)


# ------------------------------------------------------------------------------------------------ the wide fp16 kernels (tier 'f16')
PREPARE_SHAPES = [(1, 1, 1, 136), (33, 31, 65, 136), (63, 64, 129, 200), (65, 0, 7, 264)]


@pytest.mark.parametrize('A,J1,J2,Dp', PREPARE_SHAPES)
def test_wide16_prepare_is_exact(A, J1, J2, Dp):
    """sga_wide16_prepare, bit for bit: Zh = fp16(z) rounded to nearest even -- ties, values below 2^-14 (fp16 subnormals, kept, not flushed) and
    below 2^-25 (zero) among the entries --, ZhT[d, r + shift of r's segment] = Zh[r, d] with every segment starting at a multiple of 8 columns,
    and every other column of ZhT zero (both outputs pre-filled with NaN)."""
    R = 2 * A + J1 + J2
    g = torch.Generator().manual_seed(A + Dp)
    z = torch.randn(R, Dp, generator=g) * torch.ldexp(torch.ones(R, Dp), torch.randint(-27, 1, (R, Dp), generator=g))
    special = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                            3.0 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, -(2.0 ** -24), 0.0, -0.0, 1.0, 65504.0, 2.0 ** -26])
    z.view(-1)[:special.numel()] = special[:z.numel()]
    z.view(-1)[-special.numel():] = special[:z.numel()].flip(0)
    zh, zt = LG.run_prepare(z, A, J1, J2)
    want_h, want_t = LG.prepare_ref(z, A, J1, J2)
    assert int(((want_h != 0) & (want_h.abs() < 2.0 ** -14)).sum()) >= 3, 'no fp16 subnormal among the expected values'
    assert tuple(zt.shape) == tuple(want_t.shape)
    assert torch.equal(zh.cpu().view(torch.int16), want_h.view(torch.int16)), 'Zh is not the round-to-nearest-even fp16 of z'
    assert torch.equal(zt.cpu().view(torch.int16), want_t.view(torch.int16)), 'ZhT: a transposed entry misplaced, or padding not zero'


F16_NAMES = [c['name'] for c in LG.f16_cases()]
F16_ANCHORED = [c['name'] for c in LG.f16_cases() if c.get('anchors', True)]


@pytest.mark.parametrize('name', F16_NAMES)
def test_f16_neg_sums_gate(name):
    """sga_loss_neg_sums_f16, whole and per shard; an empty shard returns exact zeros."""
    LG.assert_gate(LG.measure_f16_sums(name), name, case=name)


@pytest.mark.parametrize('name', F16_NAMES)
def test_f16_neg_grad_gate(name):
    """sga_loss_neg_grad_f16 per anchor range into a zeroed buffer, with a coefficient stash that holds four pairs -- and at A = 257 one pair
    (family by family) and 128-row blocks, batched and family by family: anchor rows outside the shard stay zero, an empty shard writes nothing."""
    LG.assert_gate(LG.measure_f16_grad(name), name, case=name)


@pytest.mark.parametrize('name', F16_NAMES)
def test_f16_stash_grad_gate(name):
    """sga_loss_stash_grad_f16 per anchor range: the fp32 M1 against zh.double()."""
    LG.assert_gate(LG.measure_f16_stash(name), name, case=name)


@pytest.mark.parametrize('name', F16_ANCHORED)
@pytest.mark.parametrize('mixed', [False, True])
@pytest.mark.parametrize('use_ws', [False, True])
def test_f16_anchor_gate(name, mixed, use_ws):
    """sga_loss_anchor_fwd_f16 / _bwd_f16 with fp16 copies, in the K-loop form (ws = NULL) and the workspace form, NT = 3 all wide and the
    mixed set Zh = (NULL, zh, NULL, zh) on widths (100, 136, 64, 264): every element of dL/dS per anchor range; the terms and dL/d(sums) whole
    and as the sum over the case's shards; an empty shard adds exact zeros and writes no stash."""
    LG.assert_gate(LG.measure_f16_anchor(name, mixed, use_ws), f'{name} mixed={mixed} ws={use_ws}', case=name)


@pytest.mark.parametrize('M,A,seed', LG.HEAD_CASES)
@pytest.mark.parametrize('f64', [1, 0])
def test_head_gate(M, A, seed, f64):
    LG.assert_gate(LG.measure_head(M, A, seed, f64), f'head M={M} f64={f64}')


def test_head_without_anchors_is_nan_like_the_reference():
    terms, la, lc, gout = LG.head_refs(3, 0, 5)
    out, d, _, _ = LG.run_head(terms, la, lc, 0, 0.1, 0.5, 0.1, 1, gout)
    ref = LG.head(terms, la, lc, 0, 0.1, 0.5, 0.1)
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.isnan(out[:3]).all() and torch.isnan(d[:4]).all()
    assert abs(float(out[3]) - float(ref[3])) <= 1e-12 * abs(float(ref[3]))


# ------------------------------------------------------------------------------------------------ the census
CENSUS = [(33, 31, 65, 37, 3), (129, 21, 75, 64, 4), (65, 127, 63, 97, 2), (257, 40, 9, 100, 3), (333, 17, 50, 100, 4), (63, 64, 129, 100, 4)]
CENSUS_PLAIN = [(32, 32, 32, 104, 3), (63, 64, 129, 101, 4)]


def _census_tier(A, J1, J2, D, M, tier, count_limit=True):
    tabs, idx, T, _ = LG.census(A, J1, J2, D, M, seed=A + M, count_limit=count_limit, shards=[(0, A)] + LG.shards3(A))
    Z = [LG.gather(e, idx)[0].float() for e in tabs]
    img = [LG.centre_image(z, D)[0] for z in Z] if tier != 'plain' else None
    return tabs, idx, T, Z, LG.Tier(tier, Z, img, A, J1, J2, D)


def _census_params():
    P = [(s, t) for s in CENSUS for t in ('plain', 'centred', 'planes', 'lite')] + [(s, 'plain') for s in CENSUS_PLAIN]
    return P + [((300, 5500, 5500, 100, 3), t) for t in ('centred', 'planes', 'lite')]


@pytest.mark.parametrize('shape,tier', _census_params())
def test_census_sums_are_the_integers(shape, tier):
    """Every term is exp2(0) = 1: sga_loss_multi_sums, _centred, _bf16x6 with lite 0 and 1 return (anchors of the shard) x J exactly, and three
    shards cut off the 32-row grid add up to the unsharded integers."""
    A, J1, J2, D, M = shape
    _, _, _, _, T = _census_tier(A, J1, J2, D, M, 'planes' if tier == 'lite' else tier, count_limit=J1 <= 400)
    beta = LG.fusion_beta(M, A)
    lite = int(tier == 'lite')
    assert torch.equal(T.sums(beta, 0, A, lite), LG.census_sums(A, J1, J2, M + 1))
    parts = [T.sums(beta, lo, hi, lite) for lo, hi in LG.shards3(A)]
    for (lo, hi), s in zip(LG.shards3(A), parts):
        assert torch.equal(s, LG.census_sums(hi - lo, J1, J2, M + 1)), (lo, hi)
    assert torch.equal(sum(parts), LG.census_sums(A, J1, J2, M + 1))


@pytest.mark.parametrize('shape', CENSUS[:3])
def test_census_sums_per_table(shape):
    """sga_loss_neg_sums_shard (the per-table kernels, Dp = D padded to 8): the same integers, whole and in shards."""
    A, J1, J2, D, M = shape
    lib, L, p, _, st = LG._abi()
    tabs, idx, _, _ = LG.census(A, J1, J2, D, 1, seed=A + M)
    dp = (D + 7) // 8 * 8
    z = torch.zeros(2 * A + J1 + J2 + 32, dp)
    z[:2 * A + J1 + J2, :D] = LG.gather(tabs[0], idx)[0].float()
    z = z.cuda()
    for lo, hi in [(0, A)] + LG.shards3(A):
        buf = torch.full((LG._slots() * 8,), LG.NAN, device='cuda', dtype=torch.float64)
        lib.check(L.sga_loss_neg_sums_shard(p(z), dp, A, J1, J2, LG.TAU[0], LG.TAU[1], p(buf), lo, hi, st), 'sga_loss_neg_sums_shard')
        assert torch.equal(buf[:8].cpu(), LG.census_sums(hi - lo, J1, J2, 1)[0]), (lo, hi)


CENSUS_F16 = CENSUS + [(2305, 17, 0, 136, 1), (2305, 257, 0, 136, 1)]             # S pass of 10 row tiles (a full group of 8 and a short one) x 1 and x 2 column tiles; J2 = 0


@pytest.mark.parametrize('shape', CENSUS_F16)
def test_census_sums_fp16(shape):
    """sga_loss_neg_sums_f16 (mode 'f16', tables wider than 128 columns): one-hot rows are exact in fp16 too, the sums are the integers --
    whole, in three shards cut anywhere and in shards on the 8-anchor grid, which add up to the unsharded integers."""
    A, J1, J2, _, M = shape
    D = 136
    lib, L, p, _, st = LG._abi()
    tabs, idx, _, _ = LG.census(A, J1, J2, D, 1, seed=A + M, count_limit=A <= 400)          # (2305 anchors over 68 classes: integer sums only)
    R = 2 * A + J1 + J2
    z = LG.gather(tabs[0], idx)[0].float().cuda().contiguous()
    zh = torch.zeros(R, D, device='cuda', dtype=torch.float16)
    zt = torch.zeros(D, int(L.sga_wide16_ldt(A, J1, J2)), device='cuda', dtype=torch.float16)
    lib.check(L.sga_wide16_prepare(p(z), D, A, J1, J2, p(zh), p(zt), st), 'sga_wide16_prepare')
    for parts in ([(0, A)], LG.shards3(A), LG.shards8(A)):
        tot = torch.zeros(8, dtype=torch.float64)
        for lo, hi in parts:
            buf = torch.full((LG._slots() * 8,), LG.NAN, device='cuda', dtype=torch.float64)
            lib.check(L.sga_loss_neg_sums_f16(p(zh), D, A, J1, J2, LG.TAU[0], LG.TAU[1], p(buf), lo, hi, st), 'sga_loss_neg_sums_f16')
            assert torch.equal(buf[:8].cpu(), LG.census_sums(hi - lo, J1, J2, 1)[0]), (lo, hi)
            tot += buf[:8].cpu()
        assert torch.equal(tot, LG.census_sums(A, J1, J2, 1)[0]), parts


@pytest.mark.parametrize('shape', CENSUS[:4])
@pytest.mark.parametrize('wide', [False, True])
def test_census_gradient_counts_per_table(shape, wide):
    """sga_loss_neg_grad_shard (Dp = D padded to 8; unsharded and as three shards) and sga_loss_neg_grad_wide (136 columns, several row
    blocks): every entry a constant per family times a count <= 8, against fp64 at CENSUS_U = 4 u."""
    A, J1, J2, D, M = shape
    D = 136 if wide else D
    lib, L, p, _, st = LG._abi()
    tabs, idx, _, _ = LG.census(A, J1, J2, D, 1, seed=A + M, shards=[(0, A)] + LG.shards3(A))
    R, dp = 2 * A + J1 + J2, (D + 7) // 8 * 8
    z64 = LG.gather(tabs[0], idx)[0]
    z = torch.zeros(R + 32, dp)
    z[:R, :D] = z64.float()
    z = z.cuda()
    gs = (torch.rand(1, 8, generator=torch.Generator().manual_seed(A), dtype=torch.float64) + 0.5) * 1e-3
    bl = [LG.neg_blocks(z64, z64, A, J1, J2)]
    cm, _, _, _ = LG.neg_coefs(bl, gs, None, 0, A)
    ref = LG.neg_grad_rows(cm[0], z64, A, J1, J2)
    env = LG.neg_grad_rows([c.abs() for c in cm[0]], z64, A, J1, J2, True)
    g = gs.cuda().contiguous()
    for parts in ([(0, A)],) if wide else ([(0, A)], LG.shards3(A)):
        dz = torch.zeros(R + 32, dp, device='cuda')
        for lo, hi in parts:
            if wide:
                floats = 2 * (J1 + J2) * min(A, 32)
                stash = torch.full((floats,), LG.NAN, device='cuda')
                lib.check(L.sga_loss_neg_grad_wide(p(z), dp, A, J1, J2, LG.TAU[0], LG.TAU[1], p(g), p(dz), p(stash), floats, st), 'sga_loss_neg_grad_wide')
            else:
                lib.check(L.sga_loss_neg_grad_shard(p(z), dp, A, J1, J2, LG.TAU[0], LG.TAU[1], p(g), p(dz), lo, hi, st), 'sga_loss_neg_grad_shard')
        out = dz.cpu()[:R, :D]
        e = LG.errors(out, ref, env)
        print(f'[census] per-table {shape} wide={wide} shards={len(parts)}: max {e[0]:.3f} u')
        assert e[0] <= LG.CENSUS_U, e
        assert torch.equal(out != 0, ref != 0)


@pytest.mark.parametrize('shape', CENSUS[:4] + [(24, 2305, 40, 136, 1), (2305, 17, 0, 136, 1), (2305, 257, 0, 136, 1)])
def test_census_gradient_counts_fp16(shape):
    """The third form of test_census_gradient_counts_per_table: sga_loss_neg_grad_f16 on 136-column census tables, unsharded and as shards on
    the 8-anchor grid replayed into the same buffer ((24, 2305, 40): the negatives' GEMM of 10 row tiles, and (2305, 17, 0), (2305, 257, 0): the coefficient
    pass of 10 row tiles by one and by two column tiles, J2 = 0; their counts exceed 8, which the fp32 accumulation of equal fp16 terms still holds exactly).  dL/d(sums) is non-zero for ONE sum family at a time, so every non-zero entry is
    n x c: an integer count n (the fp64 reference's) times one constant c for the whole family.  The zero pattern is the reference's; all
    entries agree on c to CENSUS_U = 4 u; c is within one fp16 step (2^-10) of gs[f,0] / tau0 + gs[f,1] / tau1 -- the coefficient enters the
    matrix cores rounded to fp16.  A lost or doubled pair moves an entry by at least 1/8 of itself (1/n of it where the counts are not limited)."""
    A, J1, J2, _, M = shape
    D = 136
    lib, L, p, _, st = LG._abi()
    limited = max(A, J1) <= 400
    tabs, idx, _, _ = LG.census(A, J1, J2, D, 1, seed=A + M, count_limit=limited, shards=[(0, A)] + LG.shards8(A))
    R = 2 * A + J1 + J2
    z64 = LG.gather(tabs[0], idx)[0]
    zh, zt = LG.run_prepare(z64.float(), A, J1, J2)
    assert torch.equal(zh.cpu().double(), z64)
    nbytes = int(L.sga_loss_neg_grad_f16_bytes(A, J1, J2))
    bl = [LG.neg_blocks(z64, z64, A, J1, J2)]
    g0 = (torch.rand(4, 2, generator=torch.Generator().manual_seed(A), dtype=torch.float64) + 0.5) * 1e-3
    for f in range(4):
        gs = torch.zeros(1, 8, dtype=torch.float64)
        gs[0, 2 * f:2 * f + 2] = g0[f] * (-1.0 if f % 2 else 1.0)
        c_exact = float(gs[0, 2 * f] / LG.TAU[0] + gs[0, 2 * f + 1] / LG.TAU[1])
        cm, _, _, _ = LG.neg_coefs(bl, gs, None, 0, A)
        ref = LG.neg_grad_rows(cm[0], z64, A, J1, J2)
        count = torch.round(ref / c_exact)
        assert torch.equal(count * c_exact != 0, ref != 0) and float((ref - count * c_exact).abs().max()) <= 1e-12 * abs(c_exact) * float(count.max())
        g = gs.cuda().contiguous()
        for parts in ([(0, A)], LG.shards8(A)):
            dz = torch.zeros(R, D, device='cuda')
            for lo, hi in parts:
                stash = torch.full((nbytes,), 255, device='cuda', dtype=torch.uint8)
                lib.check(L.sga_loss_neg_grad_f16(p(zh), p(zt), D, A, J1, J2, LG.TAU[0], LG.TAU[1], p(g), p(dz), p(stash), nbytes, lo, hi, st), 'sga_loss_neg_grad_f16')
            out = dz.cpu().double()
            assert torch.isfinite(out).all()
            assert torch.equal(out != 0, ref != 0), (f, parts)
            nz = ref != 0
            if not nz.any():                               # (a family without negatives: J2 = 0)
                continue
            c = out[nz] / count[nz]
            mid = float(c.median())
            spread = float((c - mid).abs().max()) / abs(mid) / G.U
            step = abs(mid - c_exact) / abs(c_exact) * 2.0 ** 10
            print(f'[census] fp16 {shape} family {f} shards={len(parts)}: c spread {spread:.3f} u, c off the exact constant by {step:.3f} fp16 steps, max count {int(count.max())}')
            assert spread <= LG.CENSUS_U, (f, parts, spread)
            assert step <= 1.0, (f, parts, step)


@pytest.mark.parametrize('shape,tier', [(s, t) for s in CENSUS for t in ('plain', 'centred', 'planes')] + [(s, 'plain') for s in CENSUS_PLAIN])
def test_census_gradient_counts(shape, tier):
    """Every entry of the negatives' gradient is (a constant per family) x (a count <= 8): against fp64 at CENSUS_U = 4 u of the entry's
    envelope (loss_gate's docstring derives the 4), unsharded and as three shards; then through the tier's scatter every referenced object
    has a gradient and every unreferenced one has none."""
    A, J1, J2, D, M = shape
    tabs, idx, Tn, Z, T = _census_tier(A, J1, J2, D, M, tier)
    beta = LG.fusion_beta(M, A)
    g = torch.Generator().manual_seed(A)
    gs = (torch.rand(M + 1, 8, generator=g, dtype=torch.float64) + 0.5) * 1e-3
    z64 = [z.double() for z in Z]
    bl = LG.with_joint([LG.neg_blocks(z, z, A, J1, J2) for z in z64], beta.double())
    cm, _, _, _ = LG.neg_coefs(bl, gs, beta.double(), 0, A)
    R = 2 * A + J1 + J2
    for parts in ([(0, A)], LG.shards3(A)):
        dz = None
        for lo, hi in parts:
            dz, _ = T.grad(beta, gs, lo, hi, dz)
        for m in range(M):
            ref = LG.neg_grad_rows(cm[m], z64[m], A, J1, J2)
            env = LG.neg_grad_rows([c.abs() for c in cm[m]], z64[m], A, J1, J2, True)
            out = dz[m].cpu()[:R, :D]
            e = LG.errors(out, ref, env)
            print(f'[census] {shape} {tier} shards={len(parts)} table {m}: max {e[0]:.3f} u')
            assert e[0] <= LG.CENSUS_U, (m, e)
            assert torch.equal(out != 0, ref != 0)
    nrm = [LG.gather(e, idx)[1].float() for e in tabs]
    for m in range(M):
        de = T.scatter(m, dz[m][:R], nrm[m], idx, Tn)
        has = torch.zeros(Tn, dtype=torch.bool)
        has[idx.long()] = True
        assert torch.equal(de.abs().sum(1) > 0, has)


# ------------------------------------------------------------------------------------------------ end to end, one test per product route
class _Recorder:
    """A stand-in for the loaded library that notes which entry points are called (ops.KERNEL_EVENTS covers only some)."""

    def __init__(self, real):
        self._real, self.called = real, set()

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self._real, name)


FUSED_COMMON = {'sga_loss_gather', 'sga_loss_check_norms', 'sga_loss_head_fwd', 'sga_loss_head_bwd'}
ROUTES = {
    # name: (D, mfma mode, switches, the loss entry points that must run -- exactly)
    'planes-onepass-sym': (100, 'bf16x6', dict(STASH_BYTES=1 << 19), {'sga_loss_split3_tables', 'sga_loss_multi_sums_bf16x6', 'sga_loss_anchor_multi_bwd_symx',
                           'sga_loss_stash_grad_symx_bf16x6', 'sga_loss_multi_grad_bf16x6', 'sga_loss_scatter_tangent'}),
    'planes-onepass-ordered': (97, 'bf16x6', dict(AA_SYMMETRIC=False, STASH_BYTES=1 << 19), {'sga_loss_split3_tables', 'sga_loss_multi_sums_bf16x6',
                               'sga_loss_anchor_multi_bwd', 'sga_loss_stash_grad_symx_bf16x6', 'sga_loss_multi_grad_bf16x6', 'sga_loss_scatter_tangent'}),
    'planes-twopass': (100, 'bf16x6', dict(FUSED_AA_ONEPASS=False), {'sga_loss_split3_tables', 'sga_loss_multi_sums_bf16x6', 'sga_loss_anchor_multi_fwd',
                       'sga_loss_anchor_multi_bwd', 'sga_loss_stash_grad_symx_bf16x6', 'sga_loss_multi_grad_bf16x6', 'sga_loss_scatter_tangent'}),
    'planes-fp32-stash': (100, 'bf16x6', dict(BF16X6_STASH=False, STASH_BYTES=1 << 19), {'sga_loss_split3_tables', 'sga_loss_multi_sums_bf16x6',
                          'sga_loss_anchor_multi_bwd_symx', 'sga_loss_stash_grad_symx', 'sga_loss_multi_grad_bf16x6', 'sga_loss_scatter_tangent'}),
    'centred-onepass-sym': (100, 'f32', dict(STASH_BYTES=1 << 19), {'sga_loss_centre_tables', 'sga_loss_multi_sums_centred', 'sga_loss_anchor_multi_bwd_symx',
                            'sga_loss_stash_grad_symx', 'sga_loss_multi_grad_centred', 'sga_loss_scatter_tangent_stat'}),
    'centred-twopass': (64, 'f32', dict(FUSED_AA_ONEPASS=False), {'sga_loss_centre_tables', 'sga_loss_multi_sums_centred', 'sga_loss_anchor_multi_fwd',
                        'sga_loss_anchor_multi_bwd', 'sga_loss_stash_grad', 'sga_loss_multi_grad_centred', 'sga_loss_scatter_tangent_stat'}),
    'plain-onepass-sym': (104, 'bf16x6', dict(STASH_BYTES=1 << 19), {'sga_loss_multi_sums', 'sga_loss_anchor_multi_bwd_symx', 'sga_loss_stash_grad_symx',
                          'sga_loss_multi_grad', 'sga_loss_scatter'}),
    'plain-twopass': (104, 'bf16x6', dict(FUSED_AA_ONEPASS=False), {'sga_loss_multi_sums', 'sga_loss_anchor_multi_fwd', 'sga_loss_anchor_multi_bwd',
                      'sga_loss_stash_grad', 'sga_loss_multi_grad', 'sga_loss_scatter'}),
}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_overall_loss_end_to_end(route):
    """OverallLoss through ops.fused_contrastive_terms and the scalar head on one product route: the four loss values, dE of every table,
    d fusion weight and both d log_vars against the fp64 chain (== the oracle, test_loss_gate_cpu.py), each at the largest r of the stages
    that feed it; the route is pinned by the set of loss entry points that ran."""
    import numpy as np
    from sgaligner_amd import _lib, ops
    from sgaligner_amd.aligner import losses as L
    from sgaligner_amd.aligner.sg_aligner import MultiModalFusion
    from sgaligner_amd.synthetic import make_batch
    D, mode, switches, expect = ROUTES[route]
    mods = ['point', 'gat', 'rel']
    M = len(mods)
    dd = make_batch(24, 40, 1, seed=3, ragged=True)
    idx = torch.cat([torch.as_tensor(np.asarray(dd[k]), dtype=torch.int32) for k in ('e1i', 'e2i', 'e1j', 'e2j')])
    A, J1, J2 = len(dd['e1i']), len(dd['e1j']), len(dd['e2j'])
    assert A >= ops.ONEPASS_MIN_ANCHORS
    T = int(np.asarray(dd['tot_obj_count']).sum())
    g = torch.Generator().manual_seed(len(route))
    E = [torch.randn(T, D, generator=g) for _ in mods]
    E[2] = torch.randn(1, D, generator=g) + 0.05 * torch.randn(T, D, generator=g)            # nearly parallel rows, like meta_embedding_rel
    w0 = 0.5 * torch.randn(M, 1, generator=g)
    lv1, lv2 = 0.3 * torch.randn(M, generator=g), 0.3 * torch.randn(M, generator=g)
    ref = LG.chain(E, w0, lv1, lv2, idx, A, J1, J2, envelopes=True)
    yard = LG.chain(E, w0, lv1, lv2, idx, A, J1, J2, dt=torch.float32)

    e = {k: E[i].cuda().requires_grad_(True) for i, k in enumerate(mods)}
    fus = MultiModalFusion(M).cuda()
    ial, icl = L.CustomMultiLossLayer(M).cuda(), L.CustomMultiLossLayer(M).cuda()
    with torch.no_grad():
        fus.weight.copy_(w0.cuda()); ial.log_vars.copy_(lv1.cuda()); icl.log_vars.copy_(lv2.cuda())
    keep = {k: getattr(ops, k) for k in switches}
    keep_mode = ops.get_mfma_mode()
    real = _lib.lib()
    rec = _Recorder(real)
    try:
        for k, v in switches.items():
            setattr(ops, k, v)
        ops.set_mfma_mode(mode)
        _lib._lib = rec
        out = dict(e)
        out['joint'] = fus([e[k] for k in mods])
        fn = L.OverallLoss(ial, icl, 'cuda', {'zoom': 0.1, 'wt_align_loss': 1.0, 'wt_contrastive_loss': 1.0, 'modules': mods})
        res = fn(out, dd)
        res['loss'].backward()
        torch.cuda.synchronize()
        ops.DEFERRED_CHECKS.flush()
    finally:
        _lib._lib = real
        ops.set_mfma_mode(keep_mode)
        for k, v in keep.items():
            setattr(ops, k, v)
    ran = {n for n in rec.called if n.startswith('sga_loss_') and not n.endswith(('_slots', '_bytes', '_floats'))}          # (size queries launch nothing)
    assert ran == expect | FUSED_COMMON, (sorted(ran - expect - FUSED_COMMON), sorted((expect | FUSED_COMMON) - ran))

    tier = 'plain' if D > 100 else ('centred' if mode == 'f32' else 'planes')
    stier = tier if expect & {'sga_loss_stash_grad_symx_bf16x6'} else ('plain' if tier == 'plain' else 'centred')
    r = lambda *keys: max(LG.R[k] for k in keys)
    r_terms = r('anchor_terms.terms|f32', f'neg_sums.sums|{tier}', 'head.head|f32')
    r_de = r('anchor_coef.dS|f32', 'anchor_coef.gs|f32', f'neg_grad.dZ|{tier}', f'stash_grad.dZ|{stier}', 'scatter.dE|' + ('f32' if tier == 'plain' else tier),
             'gather.Z|f32', f'neg_sums.sums|{tier}')
    r_w = r('anchor_coef.gamma|f32', f'neg_grad.gamma_neg|{tier}', 'anchor_coef.gs|f32', f'neg_sums.sums|{tier}')
    vals = torch.stack([res[k].detach().double().cpu() for k in ('loss', 'icl_loss_unimodal', 'icl_loss_multimodal', 'ial_loss')])
    rows = [('e2e.head', vals, ref['out'], ref['env_out'], yard['out'], r_terms, True)]
    rows += [(f'e2e.dE[{m}]', e[k].grad, ref['dE'][m], ref['env_dE'][m], yard['dE'][m], r_de, False) for m, k in enumerate(mods)]
    rows += [('e2e.dweight', fus.weight.grad.reshape(-1), ref['dw'], ref['env_dw'], yard['dw'], r_w, True),
             ('e2e.dlv_ial', ial.log_vars.grad, ref['dla'], ref['env_dla'], yard['dla'], max(r_terms, LG.R['head.dlv|f32']), True),
             ('e2e.dlv_icl', icl.log_vars.grad, ref['dlc'], ref['env_dlc'], yard['dlc'], max(r_terms, LG.R['head.dlv|f32']), True)]
    bad = []
    for what, got, rf, env, yd, rr, scalar in rows:
        ke, ye = LG.errors(got, rf, env), LG.errors(yd, rf, env)
        print(f'[loss gate] {route} {what}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | fp32 yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {rr}')
        if not LG.gate_ok(ke, ye, rr, scalar):
            bad.append((what, ke[:2], ye[:2], rr))
    assert not bad, bad


F16_MIXED_ENTRIES = {'sga_loss_gather', 'sga_loss_neg_sums_shard', 'sga_loss_neg_sums_f16', 'sga_loss_anchor_fwd_f16', 'sga_loss_anchor_bwd_f16', 'sga_loss_stash_grad',
                     'sga_loss_stash_grad_f16', 'sga_loss_neg_grad_shard', 'sga_loss_neg_grad_f16', 'sga_loss_scatter'}
PER_TABLE_ROUTES = {
    # name: (table widths, the last standing for the joint; ops.WIDE_STASH; the loss entry points that must run -- exactly)
    'narrow': ((100, 37, 64, 120), True, {'sga_loss_gather', 'sga_loss_neg_sums_shard', 'sga_loss_anchor_fwd_f16', 'sga_loss_anchor_bwd_f16', 'sga_loss_stash_grad',
                                          'sga_loss_neg_grad_shard', 'sga_loss_scatter'}),
    'wide': ((100, 97, 300), True, {'sga_loss_gather', 'sga_loss_neg_sums_shard', 'sga_loss_anchor_fwd_f16', 'sga_loss_anchor_bwd_f16', 'sga_loss_stash_grad',
                                    'sga_loss_neg_grad_shard', 'sga_loss_neg_grad_wide', 'sga_loss_scatter'}),
    'wide-multipass': ((100, 97, 300), False, {'sga_loss_gather', 'sga_loss_neg_sums_shard', 'sga_loss_anchor_fwd_f16', 'sga_loss_anchor_bwd_f16',
                                               'sga_loss_stash_grad', 'sga_loss_neg_grad_shard', 'sga_loss_scatter'}),
    # mode 'f16' (a fourth entry: the mfma mode): tables wider than 128 columns take their fp16 copies through csrc/wide16.hip
    'f16-all-wide': ((136, 264, 400), True, {'sga_loss_gather', 'sga_loss_neg_sums_f16', 'sga_loss_anchor_fwd_f16', 'sga_loss_anchor_bwd_f16', 'sga_loss_stash_grad_f16',
                                             'sga_loss_neg_grad_f16', 'sga_loss_scatter'}, 'f16'),
    'f16-mixed': ((100, 120, 220), True, F16_MIXED_ENTRIES, 'f16'),                     # two narrow tables and their wide joint
    'f16-mixed-first-wide': ((264, 100, 364), True, F16_MIXED_ENTRIES, 'f16'),
}
F16_KEYS = ('anchor_terms.terms|f16', 'neg_sums.sums|f16', 'anchor_coef.dS|f16', 'anchor_coef.gs|f16', 'neg_grad.dZ|f16', 'stash_grad.dZ|f16')


def _route_gates(f16):
    """(r of the terms, r of dE): the largest r of the stages that feed each output on a per-table route."""
    r = lambda *keys: max(LG.R[k] for k in keys)
    r_terms = r('anchor_terms.terms|pertable', 'neg_sums.sums|pertable')
    r_de = r('anchor_coef.dS|pertable', 'anchor_coef.gs|pertable', 'neg_grad.dZ|pertable', 'neg_grad.dZ|wide', 'stash_grad.dZ|plain', 'scatter.dE|f32', 'gather.Z|f32',
             'neg_sums.sums|pertable')
    if f16:
        r_terms = max(r_terms, r(*F16_KEYS[:2]))
        r_de = max(r_de, r(*F16_KEYS[1:]))
    return r_terms, r_de


def _gate_rows(what, rows):
    bad = []
    for name, got, rf, env, yd, rr, scalar in rows:
        ke, ye = LG.errors(got, rf, env), LG.errors(yd, rf, env)
        print(f'[loss gate] per-table {what} {name}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | fp32 yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {rr}')
        if not LG.gate_ok(ke, ye, rr, scalar):
            bad.append((name, ke[:2], ye[:2], rr))
    assert not bad, bad


@pytest.mark.parametrize('route', sorted(PER_TABLE_ROUTES))
def test_contrastive_terms_end_to_end(route):
    """ops.contrastive_terms (any joint table) on the narrow route, the wide one (coefficient stash + GEMMs), the wide multi-pass sweep and,
    in mode 'f16', all tables wide and the two mixed sets (a narrow table beside a wide one: fp16 copies for some tables only): the raw terms
    and dE of every table against the fp64 chain of the per-table stages, at the largest r of the stages that feed them.  The yardstick of a
    table with an fp16 copy is the float32 chain in the arithmetic of the tier 'f16'."""
    import numpy as np
    from sgaligner_amd import _lib, ops
    from sgaligner_amd.synthetic import make_batch
    widths, wide_stash, expect, *mode = PER_TABLE_ROUTES[route]
    mode = mode[0] if mode else ops.get_mfma_mode()
    dd = make_batch(6, 30, 1, seed=4, ragged=True)
    idx = torch.cat([torch.as_tensor(np.asarray(dd[k]), dtype=torch.int32) for k in ('e1i', 'e2i', 'e1j', 'e2j')])
    A, J1, J2 = len(dd['e1i']), len(dd['e1j']), len(dd['e2j'])
    T = int(np.asarray(dd['tot_obj_count']).sum())
    g = torch.Generator().manual_seed(len(route))
    E = [torch.randn(T, d, generator=g) for d in widths]
    nt = len(E)
    coef = (torch.rand(nt + 2 * (nt - 1), generator=g) + 0.5) * 1e-2
    copies = [mode == 'f16' and d > 128 for d in widths]
    ref = LG.chain_terms(E, None, idx, A, J1, J2, coef, envelopes=True)
    yard = LG.chain_terms(E, None, idx, A, J1, J2, coef, dt=torch.float32, f16=copies)
    tabs = [e.cuda().requires_grad_(True) for e in E]
    keep, keep_mode, real = ops.WIDE_STASH, ops.get_mfma_mode(), _lib.lib()
    rec = _Recorder(real)
    try:
        ops.WIDE_STASH = wide_stash
        ops.set_mfma_mode(mode)
        _lib._lib = rec
        out, _ = ops.contrastive_terms(tabs, dd)
        (out * coef.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
        ops.set_mfma_mode(keep_mode)
        ops.WIDE_STASH = keep
    ran = {n for n in rec.called if n.startswith('sga_loss_') and not n.endswith(('_slots', '_bytes', '_floats'))}
    assert ran == expect, (sorted(ran - expect), sorted(expect - ran))
    r_terms, r_de = _route_gates(any(copies))
    rows = [('e2e.terms', out.detach().double().cpu(), ref['terms'], ref['env_terms'], yard['terms'], r_terms, True)]
    rows += [(f'e2e.dE[{k}]', tabs[k].grad, ref['dE'][k], ref['env_dE'][k], yard['dE'][k], r_de, False) for k in range(nt)]
    _gate_rows(route, rows)


def test_contrastive_terms_f16_mixed_in_shards():
    """The route 'f16-mixed' with the anchors of a batch (A = 55: not a multiple of 8) in three shards, (0, 32), (32, A) and the empty (A, A)
    -- the few-anchors case of the trainer's shard cuts --, the all-reduce emulated by evaluating the shards one after another with the
    totals of the earlier passes: the shares of the terms add up to the unsharded terms and the table gradients to the unsharded
    gradients, within the route's gate against the fp64 chain; the empty shard's shares are exact zeros; a wide table with a non-empty
    shard that starts off the 8-anchor grid raises."""
    import numpy as np
    from sgaligner_amd import ops
    from sgaligner_amd.synthetic import make_batch
    widths = PER_TABLE_ROUTES['f16-mixed'][0]
    dd = make_batch(5, 40, 1, seed=4, ragged=True)
    idx = torch.cat([torch.as_tensor(np.asarray(dd[k]), dtype=torch.int32) for k in ('e1i', 'e2i', 'e1j', 'e2j')])
    A, J1, J2 = len(dd['e1i']), len(dd['e1j']), len(dd['e2j'])
    assert A > 32 and A % 8
    T = int(np.asarray(dd['tot_obj_count']).sum())
    g = torch.Generator().manual_seed(55)
    E = [torch.randn(T, d, generator=g) for d in widths]
    nt = len(E)
    coef = (torch.rand(nt + 2 * (nt - 1), generator=g) + 0.5) * 1e-2
    copies = [d > 128 for d in widths]
    ref = LG.chain_terms(E, None, idx, A, J1, J2, coef, envelopes=True)
    yard = LG.chain_terms(E, None, idx, A, J1, J2, coef, dt=torch.float32, f16=copies)
    shards = [(0, 32), (32, A), (A, A)]

    def run(shard, reduce):
        tabs = [e.cuda().requires_grad_(True) for e in E]
        out, _ = ops.contrastive_terms(tabs, dd, shard=shard, reduce=reduce)
        (out * coef.cuda()).sum().backward()
        torch.cuda.synchronize()
        return out.detach().double().cpu(), [t.grad.cpu() for t in tabs]

    keep_mode = ops.get_mfma_mode()
    try:
        ops.set_mfma_mode('f16')
        whole = run(None, None)
        # the in-place SUM all-reduce of three ranks, one rank after another: pass p knows the totals of the reductions before the p-th
        # (forward: the sums, the terms; backward: dL/d(sums)) and collects the ranks' shares of the p-th
        totals, shares = [], []
        for _ in range(4):
            pending, results = [], []
            for rank, shard in enumerate(shards):
                calls = [0]

                def reduce(t, rank=rank, calls=calls):
                    k = calls[0]
                    calls[0] += 1
                    if k == len(totals):
                        pending.append(t.detach().clone())
                    if k < len(totals):
                        t.copy_(totals[k])
                results.append(run(shard, reduce))
            if pending:
                assert len(pending) == len(shards)
                shares.append(pending)
                totals.append(sum(pending))
        assert len(totals) == 3, 'contrastive_terms reduces the sums, the terms and dL/d(sums)'
        with pytest.raises(RuntimeError, match='multiple of 8'):
            run((5, A), None)
    finally:
        ops.set_mfma_mode(keep_mode)
    r_terms, r_de = _route_gates(True)
    n = nt + 2 * (nt - 1)
    terms = totals[1][:n].double().cpu()
    dE = [sum(res[1][k] for res in results) for k in range(nt)]
    rows = [('whole.terms', whole[0], ref['terms'], ref['env_terms'], yard['terms'], r_terms, True), ('shards.terms', terms, ref['terms'], ref['env_terms'], yard['terms'], r_terms, True)]
    rows += [(f'whole.dE[{k}]', whole[1][k], ref['dE'][k], ref['env_dE'][k], yard['dE'][k], r_de, False) for k in range(nt)]
    rows += [(f'shards.dE[{k}]', dE[k], ref['dE'][k], ref['env_dE'][k], yard['dE'][k], r_de, False) for k in range(nt)]
    _gate_rows('f16-mixed in shards', rows)
    for res in results:                                    # every rank returns the all-reduced terms
        assert torch.equal(res[0], results[0][0])
    empty = len(shards) - 1
    assert all(not share[empty].any() for share in shares), 'the empty shard adds to a global sum, a term or dL/d(sums)'
    assert all(not d.any() for d in results[empty][1]), 'the empty shard has a table gradient'
