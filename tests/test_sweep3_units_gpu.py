"""The three-plane sweeps' tile transport and work split at the shapes where they can go wrong (csrc/sweep3.hip: the buffer-form LDS copies
-- one descriptor per table and segment, tile and chunk in the scalar offset -- and the per-group choice of the kernel body: the negative-
owner groups of the gradient sweep run the body that never forms Gamma).  Nothing in either changes a product or a sum, so everything is
compared with the exact-fp32 MFMA sweeps (ops.set_mfma_mode('f32')) at the tolerances of
test_bf16x6_gpu.py::test_sweeps_vs_fp32_sweeps_and_anchor_shards: sums rtol 2e-6, table gradients 5e-6 of their maximum, dL/dbeta (the
fusion weight's gradient, which Gamma feeds) 5e-5.

Shapes (A anchors per side, J1 / J2 negatives; a tile = 32 rows, an owner block = 64 rows in the gradient sweep, 128 in the sums):
  edge        A = 70, J1 = 21, J2 = 75: no count a multiple of 32 / 64, a partial last owner block, and J1 a segment of ONE tile -- its first copy
              is also its last tile (the tile re-copies itself into the idle buffer);
  one_anchor_tile  A = 23: the negative-owner groups meet a single anchor tile per segment, the anchor owners a single partial block;
  split       A = 300 against 2 x 5 500 negatives: 344 tile steps per anchor-owner group -> nsplit = 3 (work units of <= 160 steps), several
              work units per owner block, the two-buffer ring wraps ~57 times per unit and a unit's tiles are nsplit apart;
  shards      the edge shape's anchors cut at rows that are not multiples of 32 (what the ranks of a multi-GPU job own)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {'edge': (70, 21, 75), 'one_anchor_tile': (23, 130, 33), 'split': (300, 5500, 5500)}
_cache = {}


def _case(M, A, J1, J2, seed):
    # As in a real batch every index set names its own objects (a row that is anchor AND negative would meet itself: S = 1, a term e^10 that no
    # batch of the reference contains), in scattered order, and some rows are named by nobody.  Tables: plain random rows, as in the test whose
    # tolerances these are (the centred form of nearly parallel rows has tests of its own, with their own bars: test_bf16x6_gpu.py).
    rng = np.random.RandomState(seed)
    T = 2 * A + J1 + J2 + 17
    perm = rng.permutation(T).astype(np.int32)
    dd = {'e1i': perm[:A], 'e2i': perm[A:2 * A], 'e1j': perm[2 * A:2 * A + J1], 'e2j': perm[2 * A + J1:2 * A + J1 + J2]}
    g = torch.Generator(device='cuda').manual_seed(seed)
    base = [torch.randn(T, 100, device='cuda', generator=g) for _ in range(M)]
    w0 = torch.tensor([[0.3], [1.1], [-0.4]], device='cuda')[:M].contiguous()
    cot = torch.randn(M + 1 + 2 * M, device='cuda', generator=g)
    return dd, base, w0, cot


def _run(mode, dd, base, w0, cot):
    from sgaligner_amd import ops
    old = ops.set_mfma_mode(mode)
    try:
        tabs = [b.clone().requires_grad_(True) for b in base]
        w = w0.clone().requires_grad_(True)
        sums, _ = ops.fused_contrastive_terms(tabs, w, dd)
        (sums * cot).sum().backward()
        torch.cuda.synchronize()
        return sums.detach().clone(), [t.grad.clone() for t in tabs], w.grad.clone()
    finally:
        ops.set_mfma_mode(old)


def _both(M, name):
    """(three-plane result, fp32-MFMA result) of a shape, computed once per session and shared"""
    key = (M, name)
    if key not in _cache:
        case = _case(M, *SHAPES[name], seed=100 + 7 * M + len(name))
        _cache[key] = (case, _run('bf16x6', *case), _run('f32', *case))
    return _cache[key]


def _check(b, f, M):
    sb, gb, wb = b
    sf, gf, wf = f
    print('sums max rel diff', ((sb - sf).abs() / sf.abs().clamp_min(1e-30)).max().item())
    assert torch.allclose(sb, sf, rtol=2e-6, atol=1e-7), (sb, sf)
    for m in range(M):
        sc = gf[m].abs().max().item()
        d = (gb[m] - gf[m]).abs().max().item()
        print('table', m, 'gradient diff / max', d / sc)
        assert d < 5e-6 * sc, (m, d, sc)
    dw = (wb - wf).abs().max().item()
    print('d beta diff', dw, 'of', wf.abs().max().item())
    assert dw < 5e-5 * max(1e-3, wf.abs().max().item()), (wb, wf)


@pytest.mark.parametrize('M', [3, 2])
@pytest.mark.parametrize('name', ['edge', 'one_anchor_tile', 'split'])
def test_sums_gradients_and_dbeta_equal_the_fp32_sweeps(M, name):
    """Sums, every table gradient and dL/dbeta (Gamma from the anchor-owner groups only; the negative-owner groups on the GAM = false body)."""
    _, b, f = _both(M, name)
    _check(b, f, M)


@pytest.mark.parametrize('M', [3, 2])
def test_split_shape_runs_more_than_one_work_unit_per_owner_block_and_every_negative_gets_gradient(M):
    """The split shape really is split (the host's rule: work units of 160 .. 640 tile steps), and a dropped or misplaced tile would show: every
    referenced negative row carries gradient, rows nobody references carry none."""
    A, J1, J2 = SHAPES['split']
    steps = (J1 + 31) // 32 + (J2 + 31) // 32
    assert steps > 320 and (steps + 159) // 160 >= 2
    (dd, base, _, _), b, f = _both(M, 'split')
    used = torch.zeros(base[0].shape[0], dtype=torch.bool, device='cuda')
    used[torch.as_tensor(np.concatenate([dd[k] for k in ('e1i', 'e2i', 'e1j', 'e2j')]).astype(np.int64), device='cuda')] = True
    for m in range(M):
        assert (b[1][m][used].abs().amax(dim=1) > 0).all()
        assert float(b[1][m][~used].abs().max()) == 0.0


@pytest.mark.parametrize('M', [3, 2])
def test_anchor_shards_off_the_tile_grid_sum_to_the_fp32_sweeps_shards(M):
    """Three anchor shards cut at rows 27 and 45 of 70 (no cut a multiple of 32): the negative-owner groups then meet anchor segments whose
    first and last tiles are partly foreign.  Summed over the shards, in both arithmetics, with the same replayed all-reduces."""
    from sgaligner_amd import ops
    from test_c3_gpu import _replay_sharded
    (dd, base, w0, cot), b, _ = _both(M, 'edge')
    cuts = [0, 27, 45, SHAPES['edge'][0]]
    res = {}
    for mode in ('bf16x6', 'f32'):
        old = ops.set_mfma_mode(mode)
        try:
            _, gs, gw, all_sums = _replay_sharded(base, w0, cot, dd, cuts)
            torch.cuda.synchronize()
        finally:
            ops.set_mfma_mode(old)
        res[mode] = (all_sums, gs, gw)
    for sb, sf in zip(res['bf16x6'][0], res['f32'][0]):
        _check((sb, res['bf16x6'][1], res['bf16x6'][2]), (sf, res['f32'][1], res['f32'][2]), M)
    # and the shards add up to the unsharded sweep (different summation order: the bars of test_sweeps_vs_fp32_sweeps_and_anchor_shards)
    for sr in res['bf16x6'][0]:
        assert torch.allclose(sr, b[0], rtol=1e-5, atol=1e-6)
    for m in range(M):
        sc = b[1][m].abs().max().item()
        assert (res['bf16x6'][1][m] - b[1][m]).abs().max().item() < 2e-5 * sc, m
    assert (res['bf16x6'][2] - b[2]).abs().max().item() < 2e-4 * max(1e-3, b[2].abs().max().item())


def test_dbeta_vs_fp64_oracle_with_gamma_from_the_anchor_owner_groups_only():
    """The fusion weight's gradient of the product OverallLoss against the fp64 oracle (5 pairs x 50 objects: 75 anchors per side, counts
    off the tile grid): the three-plane sweeps' error is that of fp32 arithmetic -- at most 1.25 x the fp32-MFMA sweeps' own
    error + 5e-7, and within 1e-3 (the bars of test_error_vs_fp64_oracle_no_larger_than_the_fp32_mfma_paths)."""
    from test_bf16x6_gpu import _overall_vs_fp64
    errs = _overall_vs_fp64(5, 50, 17)
    a, b = errs['f32'], errs['bf16x6']
    print('errors vs fp64:', a, b)
    for k in ('dw', 'loss', 'dE_point', 'dE_gat', 'dE_rel'):
        assert b[k] <= 1.25 * a[k] + 5e-7, (k, a[k], b[k])
        assert b[k] < (1e-4 if k == 'loss' else 1e-3), (k, b[k])


@pytest.mark.parametrize('M', [3, 2])
def test_lite_forward_sums_at_the_split_shape(M):
    """The LITE forward sums (h and m planes only: 14 of a block's 20 chunks are copied, the last copy slot of a table is remapped to the tail
    image's chunks) at the split shape, against the full forward sums.  Bound: each similarity carries an unbiased rounding of ~2^-16, i.e.
    each term exp(S / tau0) a relative eps <= 1e-4 (sweep3.hip, LITE); a sum of n such terms moves by eps sqrt(sum t^2) / sum t.  Unit rows of
    100 random columns give S / tau0 ~ N(0, 1), sum t^2 / (sum t)^2 = e / n, and n = 300 x 5 500 per family: 1.3e-7 -- the 1e-6 of
    test_lite_forward_sums_* is > 7 such deviations."""
    from sgaligner_amd import ops
    (dd, base, w0, cot), b, _ = _both(M, 'split')
    keep = ops.BF16X6_SUMS_LITE
    try:
        ops.BF16X6_SUMS_LITE = True
        lite = _run('bf16x6', dd, base, w0, cot)
    finally:
        ops.BF16X6_SUMS_LITE = keep
    rel = ((lite[0].double() - b[0].double()).abs() / b[0].double().abs().clamp_min(1e-300)).max().item()
    print('lite vs full sums, max rel', rel)
    assert rel < 1e-6, rel
