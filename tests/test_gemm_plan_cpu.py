"""CPU: the GEMM launcher's dispatch, written down.  sga_gemm_plan is the decision gemm_launch itself runs (one copy of the conditions); with a CU
count passed in it touches no device, so the table below pins every route and every threshold on a machine without a card.  A threshold
change edits this table on purpose.  Also here, because they need no GPU: the accuracy gate's self-test (defective three-plane arithmetic
must FAIL the gate at the ratios in use) and the check that those ratios are the ones the committed measurement gives."""
import os
import re

import pytest
import torch

import gemm_gate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT, NN, TN, TT = (0, 1), (0, 0), (1, 0), (1, 1)
L26 = 1 << 26


def _plan(args, kw, ncu):
    from sgaligner_amd import ops
    return ops.gemm_plan(*args, ncu=ncu, **kw)


# (transposes, M, N, K, options) -> (route, splits) at 256 CUs | at 64 CUs (None: the same).  splits is the number of workgroups along K.
TABLE = [
    # every route once (starting points: the product's own shapes)
    ((*NT, 163840, 128, 128), {}, ('NT_64', 1), ('NT_128', 1)),                    # PCT per-point layer, K = 128: half tiles at 256 CUs
    ((*NT, 163840, 128, 256), {}, ('NT3_64', 1), ('NT3_128', 1)),
    ((*NT, 40960, 128, 256), {}, ('NT3_128', 1), ('NT3_64', 1)),                   # a quarter of the batch
    ((*NT, 40960, 128, 128), {}, ('NT_128', 1), ('NT_64', 1)),
    ((*TN, 2048, 2048, 512), {}, ('TN_BIG', 1), None),
    ((*TN, 3072, 1024, 300), {}, ('TN_SPLIT', 5), ('TN_BIG', 1)),
    ((*NT, 64, 100, 4096), dict(has_bias=True), ('GENERIC_F32', 16), None),
    ((*NT, 300, 300, 515), dict(has_bias=True, act=2, has_resid=True, ldr=300), ('GENERIC_F32', 1), None),
    ((*NT, 300, 100, 700), dict(a_is_f64=True), ('GENERIC_F64', 1), None),
    ((*NT, 300, 100, 164), dict(a_is_f64=True), ('SMALL_F64', 1), None),
    ((*NT, 300, 64, 3), dict(has_bias=True, act=1), ('SMALL_F32', 1), None),
    ((*TT, 65, 200, 70), {}, ('SMALL_F32', 1), None),
    ((*TT, 65, 200, 700), {}, ('GENERIC_F32', 1), None),
    ((*NN, 300, 256, 100), {}, ('NN', 1), None),
    ((*TN, 5000, 8, 333), {}, ('TN_NARROW', 11), ('TN_NARROW', 4)),
    ((*NT, 0, 5, 5), {}, ('EMPTY', 1), None),
    ((*NT, 5, 0, 5), {}, ('EMPTY', 1), None),
    ((*NT, 300, 100, 130), dict(has_colstats=True), ('REFUSED', 1), None),        # has_colstats with K % 4 != 0
    # K == 0: the NT kernel writes the bias
    ((*NT, 70, 40, 0), dict(has_bias=True), ('NT_128', 1), None),
    ((*TN, 70, 40, 0), {}, ('SMALL_F32', 1), None),
    ((*NN, 70, 40, 0), {}, ('NN', 1), None),
    # K = 255 | 256: fp32 MFMA against three bf16 planes (K % 4 == 0 on the NT route: 252 | 256)
    ((*NT, 300, 100, 252), {}, ('NT_128', 1), None),
    ((*NT, 300, 100, 255), {}, ('SMALL_F32', 1), None),
    ((*NT, 300, 100, 256), {}, ('NT3_128', 1), None),
    # the narrow walk: N = 8 | 9, K = 63 | 64, a K chunk that does not divide K
    ((*TN, 5000, 9, 333), {}, ('GENERIC_F32', 6), None),
    ((*TN, 5000, 3, 63), {}, ('SMALL_F32', 1), None),
    ((*TN, 5000, 3, 64), {}, ('TN_NARROW', 2), None),
    ((*TN, 128, 3, 40000), {}, ('TN_NARROW', 507), ('TN_NARROW', 128)),
    ((*TN, 5000, 8, 40000), {}, ('TN_NARROW', 13), ('TN_NARROW', 4)),
    ((*TN, 5000, 8, 333), dict(has_bias=True), ('SMALL_F32', 1), None),
    # K = 4095 | 4096 with an output grid smaller than the chip: the split-K rule
    ((*NT, 64, 100, 4092), dict(has_bias=True), ('NT3_128', 1), None),
    ((*NT, 64, 100, 4095), dict(has_bias=True), ('GENERIC_F32', 1), None),
    ((*NT, 64, 100, 4096), dict(has_bias=True, act=1), ('NT3_128', 1), None),      # an epilogue cannot be split
    ((*NT, 64, 100, 4096), dict(has_resid=True, ldr=100), ('NT3_128', 1), None),
    ((*NT, 64, 100, 4096), dict(has_colstats=True), ('NT3_128', 1), None),
    ((*NT, 128 * 256, 100, 4096), dict(has_bias=True), ('NT3_128', 1), None),      # ... and a grid that fills 256 CUs is not
    ((*NT, 128 * 64, 100, 4096), dict(has_bias=True), ('GENERIC_F32', 16), ('NT3_128', 1)),
    ((*NN, 300, 104, 4092), {}, ('NN', 1), None),
    ((*NN, 300, 104, 4096), {}, ('NN', 16), None),
    # gx * gy = 255 | 256 for the unsplit TN form
    ((*TN, 2048, 1920, 512), {}, ('TN_SPLIT', 4), ('TN_BIG', 1)),
    ((*TN, 128 * 255, 128, 512), {}, ('TN_SPLIT', 4), ('TN_BIG', 1)),
    ((*TN, 128 * 256, 128, 512), {}, ('TN_BIG', 1), None),
    ((*TN, 2048, 2048, 252), {}, ('GENERIC_F32', 1), None),                        # tn_big needs K >= 256
    ((*TN, 2048, 2048, 512), dict(has_colstats=True), ('REFUSED', 1), None),
    ((*TN, 256, 256, 127), {}, ('SMALL_F32', 1), None),                            # the 64-row splits start at K = 128
    ((*TN, 256, 256, 128), {}, ('TN_SPLIT', 2), None),
    # M % 4 / N % 4 != 0 and a bias fall off the TN kernel, a bias off the NN kernel
    ((*TN, 100, 256, 9000), {}, ('TN_SPLIT', 36), None),
    ((*TN, 102, 256, 9000), {}, ('GENERIC_F32', 36), None),
    ((*TN, 100, 254, 9000), {}, ('GENERIC_F32', 36), None),
    ((*TN, 100, 256, 9000), dict(has_bias=True), ('GENERIC_F32', 36), None),
    ((*TN, 100, 256, 300), dict(has_bias=True), ('SMALL_F32', 1), None),
    ((*NN, 300, 256, 100), dict(has_bias=True), ('SMALL_F32', 1), None),
    ((*NN, 300, 254, 100), {}, ('SMALL_F32', 1), None),
    # the leading-dimension limit of the NT epilogue's 32-bit row offsets
    ((*NT, 300, 100, 128), dict(ldc=L26 - 1), ('NT_128', 1), None),
    ((*NT, 300, 100, 128), dict(ldc=L26), ('SMALL_F32', 1), None),
    ((*NT, 300, 100, 128), dict(has_resid=True, ldr=L26 - 1), ('NT_128', 1), None),
    ((*NT, 300, 100, 128), dict(has_resid=True, ldr=L26), ('SMALL_F32', 1), None),
    # an operand that is not 16-byte aligned (pointer or leading dimension) falls off the vector kernels
    ((*NT, 300, 100, 128), dict(a_aligned16=False), ('SMALL_F32', 1), None),
    ((*NT, 300, 100, 128), dict(b_aligned16=False), ('SMALL_F32', 1), None),
    ((*NT, 300, 100, 128), dict(lda=130), ('SMALL_F32', 1), None),
    ((*NT, 300, 300, 128), dict(a_aligned16=False), ('GENERIC_F32', 1), None),
    ((*NT, 300, 100, 1024), dict(a_aligned16=False), ('GENERIC_F32', 1), None),
    ((*NT, 300, 100, 1024), dict(a_aligned16=False, has_colstats=True), ('REFUSED', 1), None),
    ((*TN, 100, 256, 9000), dict(b_aligned16=False), ('GENERIC_F32', 36), None),
    ((*NN, 300, 256, 100), dict(a_aligned16=False), ('SMALL_F32', 1), None),
]
# the half-tile rule: 64-row tiles when the 128-row grid is between one and three rounds of 4 workgroups per CU and ends in a round less than
# half full.  tiles = M / 128 at N = 128; 1024 slots at 256 CUs, 256 at 64.
for tiles, half256, half64 in [(1024, False, False), (1025, True, False), (1280, True, False), (1535, True, False), (1536, False, False),
                               (3071, False, False), (3072, False, False), (2049, True, False), (257, False, True), (320, False, True),
                               (384, False, False), (768, False, False)]:
    TABLE.append(((*NT, 128 * tiles, 128, 128), {}, ('NT_64' if half256 else 'NT_128', 1), ('NT_64' if half64 else 'NT_128', 1)))
    TABLE.append(((*NT, 128 * tiles, 128, 256), {}, ('NT3_64' if half256 else 'NT3_128', 1), ('NT3_64' if half64 else 'NT3_128', 1)))


def _id(row):
    args, kw = row[0], row[1]
    return '-'.join(str(a) for a in args) + ''.join(f'-{k}{v}' for k, v in kw.items())


@pytest.mark.parametrize('row', TABLE, ids=_id)
def test_dispatch_table(row):
    args, kw, at256, at64 = row
    assert _plan(args, kw, 256)[:2] == at256, f'256 CUs: {_plan(args, kw, 256)}'
    assert _plan(args, kw, 64)[:2] == (at64 or at256), f'64 CUs: {_plan(args, kw, 64)}'


def test_table_holds_every_route():
    from sgaligner_amd import _lib
    seen = {r[2][0] for r in TABLE} | {r[3][0] for r in TABLE if r[3]}
    assert seen == set(_lib.GEMM_ROUTES), set(_lib.GEMM_ROUTES) ^ seen


def test_route_names_are_the_header_enum():
    from sgaligner_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'sgaligner_hip.h')).read()
    body = re.search(r'enum\s+sga_gemm_route\s*\{(.*?)\}', txt, flags=re.S).group(1)
    names = re.findall(r'SGA_GEMM_(\w+)', body)
    assert tuple(names) == _lib.GEMM_ROUTES


def test_k_per_split_covers_k():
    """splits x k_per_split covers K with no empty split, k_per_split a multiple of the 32-wide chunk on the tiled routes."""
    for args, kw, _, _ in TABLE:
        for ncu in (256, 64, 304):
            route, splits, kper = _plan(args, kw, ncu)
            k = args[4]
            if route == 'EMPTY':
                continue
            assert splits >= 1 and kper >= 1 and splits * kper >= k and (splits - 1) * kper < max(k, 1), (args, kw, ncu, route, splits, kper)
            if route != 'TN_NARROW':
                assert kper % 32 == 0
            if route in ('NT_128', 'NT_64', 'NT3_128', 'NT3_64', 'TN_BIG', 'SMALL_F32', 'SMALL_F64', 'REFUSED'):
                assert splits == 1


def test_plan_rejects_bad_arguments():
    from sgaligner_amd import _lib
    with pytest.raises(RuntimeError, match='negative size'):
        _plan((*NT, -1, 4, 4), {}, 256)
    with pytest.raises(RuntimeError, match='act=3'):
        _plan((*NT, 4, 4, 4), dict(act=3), 256)
    # null output pointers are allowed
    assert _lib.lib().sga_gemm_plan(0, 1, 8, 8, 8, 8, 8, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 256, None, None, None) == 0


def test_forward_route_is_independent_of_rows_below_k_4096():
    """The row-chunk promise in its stated domain: for K < 4096 the route of C = act(A W^T + b) (+ resid) depends on M only through the NT tile
    height (whose two forms give equal bits: tests/test_gemm_routes_gpu.py).  From K = 4096 on the split-K rule looks at the grid: documented,
    and pinned here so that the domain cannot widen or narrow unnoticed."""
    fam = {'NT_128': 'NT', 'NT_64': 'NT', 'NT3_128': 'NT3', 'NT3_64': 'NT3'}
    rows = (1, 37, 128, 1000, 40960, 163840, 400000)
    for ncu in (64, 256, 304):
        for n in (1, 32, 100, 128, 256, 300, 1024):
            for k in (3, 41, 64, 128, 164, 256, 515, 1024, 4092, 4095):
                for kw in ({}, dict(has_bias=True), dict(has_bias=True, act=1), dict(has_bias=True, act=2, has_resid=True, ldr=n),
                           dict(a_aligned16=False, has_bias=True), dict(a_is_f64=True, has_bias=True)):
                    got = set()
                    for m in rows:
                        route, splits, _ = _plan((*NT, m, n, k), kw, ncu)
                        got.add((fam.get(route, route), splits))
                    assert len(got) == 1 and next(iter(got))[1] == 1, (ncu, n, k, kw, got)
    # outside the domain: few rows are split over K (atomics), many rows are not
    assert _plan((*NT, 64, 100, 4096), dict(has_bias=True), 256)[:2] == ('GENERIC_F32', 16)
    assert _plan((*NT, 163840, 100, 4096), dict(has_bias=True), 256)[:2] == ('NT3_64', 1)


# ------------------------------------------------------------------------------------------------ the gate, tested without a card
def test_gate_ratios_are_the_measured_ones():
    """R is 'the measured ratio x 2, rounded up' of profiles/gemm_accuracy_vs_fp32.json, per route; the three-plane routes stay under the cap."""
    assert G.ratios_from_profile() == G.R
    assert G.ratios_from_profile(kmax=G.K_BAND) == G.R_LOW
    assert G.R['NT3_128'] < G.NT3_RMS_CAP and G.R['NT3_64'] < G.NT3_RMS_CAP


@pytest.mark.parametrize('m,n,k', [(300, 128, 256), (384, 256, 1024), (384, 256, 4096), (192, 128, 16384)])
def test_gate_would_catch_a_dropped_plane(m, n, k):
    """The three-plane arithmetic emulated on the CPU (bf16 round-to-nearest splits, exact plane products, fp32 accumulation per 32-wide K chunk):
    all six partial products pass the gate at the NT3 routes' r; five (l h' forgotten), four (no l plane) and three products fail it, in rms, up to K = 16 384.  Raise r
    far enough and this test says which defect became invisible."""
    a, bt = G.logical_operands(m, n, k, seed=5, device='cpu')
    ref, env = G.reference(a, bt), G.envelope(a, bt)
    yard = G.rel_errors(G.yardstick(a, bt), ref, env)
    r = max(G.r_for('NT3_128', k), G.r_for('NT3_64', k))
    six = G.rel_errors(G.planes_product(a, bt, 6), ref, env)
    assert G.gate_ok(six, yard, r), (six, yard)
    for nprod in (5, 4, 3):
        bad = G.rel_errors(G.planes_product(a, bt, nprod), ref, env)
        assert not G.gate_ok(bad, yard, r), f'{nprod} products pass the gate: {bad} against {yard}, r = {r}'
        assert bad[1] > r * yard[1], f'{nprod} products are not caught by the rms: {bad} against {yard}'
        if k <= 1024:
            assert bad[1] >= 15 * yard[1]                 # the separation the cap of 8 is half of (it narrows above: 11 x at K = 4096, 6 x at 16 384)


def test_gate_metric_is_invariant_under_power_of_two_row_scaling():
    """Rows of A and of B scaled by 2^-20 .. 2^20: the envelope-relative error of fp32 arithmetic is bit-identical, so the graded-rows GPU
    cases ask nothing of a correct kernel beyond fp32's exponent range."""
    a, bt = G.logical_operands(96, 64, 256, seed=2, device='cpu')
    gen = torch.Generator().manual_seed(3)
    sa, sb = G.pow2_scales(96, gen, 'cpu'), G.pow2_scales(64, gen, 'cpu')
    a2, bt2 = a * sa[:, None], bt * sb[:, None]
    e1 = G.rel_errors(G.yardstick(a, bt), G.reference(a, bt), G.envelope(a, bt))
    e2 = G.rel_errors(G.yardstick(a2, bt2), G.reference(a2, bt2), G.envelope(a2, bt2))
    assert e1 == e2
    p1 = G.rel_errors(G.planes_product(a, bt, 6), G.reference(a, bt), G.envelope(a, bt))
    p2 = G.rel_errors(G.planes_product(a2, bt2, 6), G.reference(a2, bt2), G.envelope(a2, bt2))
    assert p1 == p2
