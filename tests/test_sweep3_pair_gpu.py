"""The paired S sub-steps of the three-plane sweeps (csrc/sweep3.hip, S3_PAIR): the 2 M similarity sub-steps of a tile run in pairs whose MFMAs
alternate between the two sub-steps, each sub-step accumulating its 20 products in ONE chain.  What can go wrong is bookkeeping -- an operand
requested into a register that a later MFMA of the pair still reads, a wait that retires too little, a chain read before it is complete, a
similarity filed under the wrong (table, half) -- so the shapes are the smallest that meet every form of it:

  M = 2, 3, 4       M = 3: the half-major order's pair (2, 3) straddles the two halves of the tile; M = 4: the one-launch gradient sweep with shared
                    small-product accumulators (table-major pairs) and the one-wave-per-SIMD forward sums;
  small             A = 40 anchors, J1 = 70, J2 = 33: partial owner blocks, segments whose first and last tiles are partial, and -- through the
                    anchor shard [7, 29), off the tile grid -- a one-tile anchor segment for the negative-owner groups;
  split             A = 300 against 2 x 5 500 negatives: nsplit = 3 work units per owner block (as test_sweep3_units_gpu.py forces it), the
                    two-buffer ring wraps, every pair of a tile carries its share of the next tile's copies;
  lite on / off     the forward sums from the h and m planes alone (11 of 20 products per sub-step) by lowering ops.BF16X6_SUMS_LITE_MIN_TERMS;
  lite_edge         A = 72, J1 = 2 070, J2 = 2 033: the small shape's partial tiles and owner blocks with enough terms per sum for the LITE form
                    (see _results: the bars are those of the fp32 comparison, so LITE's own rounding must fit inside them).

Everything is compared with the exact-fp32 MFMA sweeps (ops.set_mfma_mode('f32')) at the tolerances of
test_bf16x6_gpu.py::test_sweeps_vs_fp32_sweeps_and_anchor_shards (sums rtol 2e-6, table gradients 5e-6 of their maximum, dL/dbeta -- which
Gamma feeds -- 5e-5), LITE on and off alike.

Which kernels these tests run: the library's default build pairs the M = 3 and M = 4 gradient sweeps, the LITE forward sums of M = 2, 3, 4 and the
full forward sums of M = 2.  The M = 2 gradient sweep, the full M = 4 forward sums (paired only by -DS3_PAIR=2: measured no faster) and the full
M = 3 forward sums (no room for a second operand set) run the two-chain code here -- their cases check that the switch leaves them intact.

The lattice case needs no tolerance: rows whose entries are sums of at most three powers of two, built so that every similarity is the
integer -1, 0 or 1 and every partial sum of its products is exact in fp32 IN ANY ORDER, temperatures that make the exp2 arguments integers
-- every term is a power of two, every fp32 partial sum of terms exact -- so the paired kernels' sums equal the fp32 MFMA's bit for bit, and
both equal the integers' sum formed on the host."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = (40, 70, 33)
SPLIT = (300, 5500, 5500)
LITE_EDGE = (72, 2070, 2033)
SHARD = (7, 29)
_cache = {}


def _case(M, A, J1, J2, seed):
    """Index sets that name every object at most once, in scattered order, some rows named by nobody (as test_sweep3_units_gpu._case)."""
    rng = np.random.RandomState(seed)
    T = 2 * A + J1 + J2 + 17
    perm = rng.permutation(T).astype(np.int32)
    dd = {'e1i': perm[:A], 'e2i': perm[A:2 * A], 'e1j': perm[2 * A:2 * A + J1], 'e2j': perm[2 * A + J1:2 * A + J1 + J2]}
    g = torch.Generator(device='cuda').manual_seed(seed)
    base = [torch.randn(T, 100, device='cuda', generator=g) for _ in range(M)]
    w0 = torch.tensor([[0.3], [1.1], [-0.4], [0.6]], device='cuda')[:M].contiguous()
    cot = torch.randn(M + 1 + 2 * M, device='cuda', generator=g)
    return dd, base, w0, cot


def _run(mode, case, lite):
    """One forward + backward in `mode`; lite: the smallest global sum counts as large enough for the LITE forward sums (bf16x6 only)."""
    from sgaligner_amd import ops
    from test_sweep3_units_gpu import _run as run
    keep_terms, keep_ev = ops.BF16X6_SUMS_LITE_MIN_TERMS, ops.KERNEL_EVENTS
    assert ops.BF16X6_SUMS_LITE is None
    try:
        ops.BF16X6_SUMS_LITE_MIN_TERMS = 1 if lite else 1 << 62
        ops.KERNEL_EVENTS = {}
        out = run(mode, *case)
        if mode == 'bf16x6':
            assert ops.KERNEL_EVENTS['loss_multi_sums_bf16x6'][0][2][5] is bool(lite)      # (the form asked for is the one that ran)
        return out
    finally:
        ops.BF16X6_SUMS_LITE_MIN_TERMS, ops.KERNEL_EVENTS = keep_terms, keep_ev


def _results(M, shape):
    """(case, three-plane full, three-plane lite -- not at the small shape, whose sums have too few terms for that form --, fp32 MFMA) of a shape:
    computed once and shared, never modified"""
    key = (M, shape)
    if key not in _cache:
        case = _case(M, *shape, seed=300 + 11 * M + shape[0])
        _cache[key] = (case, _run('bf16x6', case, False), _run('bf16x6', case, True) if shape != SMALL else None, _run('f32', case, False))
    return _cache[key]


@pytest.mark.parametrize('M', [3, 2, 4])
@pytest.mark.parametrize('shape', [SMALL, SPLIT], ids=['small', 'split'])
def test_paired_sweeps_equal_the_fp32_sweeps(M, shape):
    """Sums, dZ of every table and dL/dbeta of the full-plane forward + the gradient sweep."""
    from test_sweep3_units_gpu import _check
    _, full, _, f32 = _results(M, shape)
    _check(full, f32, M)


@pytest.mark.parametrize('M', [3, 2, 4])
def test_paired_lite_sums_at_the_split_shape_equal_the_fp32_sweeps(M):
    """LITE forward sums (+ the same gradient sweep, fed by them) at the split shape.  LITE's own rounding there: every term exp(S / tau0) carries
    an unbiased relative eps <= 1e-4 (sweep3.hip, LITE), a sum of n terms moves by eps sqrt(sum t^2) / sum t = eps sqrt(e / n) for S / tau0 ~
    N(0, 1) (unit rows of 100 random columns): 1.3e-7 at n = 300 x 5 500 -- inside the 2e-6 of the comparison with the fp32 sweeps."""
    from test_sweep3_units_gpu import _check
    _, _, lite, f32 = _results(M, SPLIT)
    _check(lite, f32, M)


@pytest.mark.parametrize('M', [3, 2, 4])
def test_paired_lite_sums_at_an_edge_shape_equal_the_fp32_sweeps(M):
    """The LITE forward on partial tiles and partial owner blocks (no count a multiple of 32, 64 or 128), sums, every dZ and dL/dbeta against
    the fp32 sweeps at the same bars.  The shape is the small one grown until LITE's own rounding fits the sums' 2e-6: a term exp(S / tau0)
    carries an unbiased relative eps <= 1e-4 (sweep3.hip, LITE), a sum of n terms moves by eps sqrt(e / n) (see the split-shape case); at the
    small shape's n = 40 x 33 that bound is 4.5e-6 -- above the bar whatever the kernel -- at n = 72 x 2 033 it is 4.3e-7."""
    from test_sweep3_units_gpu import _check
    A, J1, J2 = LITE_EDGE
    assert 4.5 * 1e-4 * math.sqrt(math.e / (A * min(J1, J2))) < 2e-6
    _, _, lite, f32 = _results(M, LITE_EDGE)
    _check(lite, f32, M)


@pytest.mark.parametrize('M', [3, 2, 4])
def test_paired_sweeps_anchor_shard_off_the_tile_grid(M):
    """Anchor shards [0, 7), [7, 29), [29, 40): no cut on the tile grid; for [7, 29) the negative-owner groups meet ONE anchor tile per segment,
    partial at both ends.  Per shard sums and the summed gradients against the fp32 sweeps' with the same replayed all-reduces."""
    from sgaligner_amd import ops
    from test_c3_gpu import _replay_sharded
    from test_sweep3_units_gpu import _check
    (dd, base, w0, cot), _, _, _ = _results(M, SMALL)
    cuts = [0, SHARD[0], SHARD[1], SMALL[0]]
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


# ------------------------------------------------------------------------------------------------ the lattice case
# Row classes as in the census (tests/loss_gate.py): a row's entries sit in ONE block of seven columns (block b: columns 7 b + 1 .. 7 b + 6;
# block 13 = columns 92 .. 97 straddles the K tail at 96), anchors and negatives of the same block meet, all others are orthogonal.
# Inside a block (anchor x | negative y), a = 2^-10, b = 2^-19; planes of a value: h | m | l of the exact bf16 split:
#   three-plane rows                                                        products of the six that the column exercises
#     x1 = 1 + a + b   y1 = 1/2                  -> 1/2 + a/2 + b/2         h h, h m, h l      (other plane x owner plane; owner = anchor)
#     x2 = 1           y2 = -(a + b)/2           -> -(a + b)/2              h h, m h
#     x3 = 1 + a       y3 = (1 + a)/4            -> 1/4 + a/2 + a^2/4       h h, h m, m h, m m
#     x4 = 1           y4 = -(a/2 + a^2/4)       -> -(a/2 + a^2/4)          h h, m h
#     x5 = 1           y5 = (1 + a + b)/4        -> 1/4 + (a + b)/4         h h, m h, l h
#     x6 = -(a + b)    y6 = 1/4                  -> -(a + b)/4              h h, h m
#   sum = 1; no column pairs an m with an l or two l planes (the three products the kernels drop are zero); every product and every partial
#   sum lies on the lattice 2^-22 Z below 2: exact in fp32 whatever the order, and within the 16-bit MFMA's alignment window.
#   two-plane rows (LITE multiplies h h + h m + m h only: no l plane, no m m product)
#     x1 = 1 + a  y1 = 1/2 | x2 = 1  y2 = -a/2 | x3 = 1  y3 = (1 + a)/2 | x4 = -a  y4 = 1/2 | x5 = x6 = y5 = y6 = 0:   sum = 1.
# Row i carries a sign: S_m(i, j) = s_i t_j or 0.  With beta = +-1 the joint S_J is an integer in [-M, M]; temperatures tau1 = log2(e),
# tau0 = log2(e) / 2 (as floats) make the kernels' scales k1 = 1, k0 = 2 exactly: the terms are 2^S and 2^(2 S), powers of two between 2^-8
# and 2^8, and a lane's fp32 partial sum of <= 32 of them (LITE: four tiles) needs <= 22 bits.
_A, _B = 2.0 ** -10, 2.0 ** -19


def _lattice_tables(M, A, J1, J2, planes, seed):
    g = torch.Generator().manual_seed(seed)
    R = 2 * A + J1 + J2
    if planes == 3:
        xs = [1 + _A + _B, 1.0, 1 + _A, 1.0, 1.0, -(_A + _B)]
        ys = [0.5, -(_A + _B) / 2, (1 + _A) / 4, -(_A / 2 + _A * _A / 4), (1 + _A + _B) / 4, 0.25]
    else:
        xs = [1 + _A, 1.0, 1.0, -_A, 0.0, 0.0]
        ys = [0.5, -_A / 2, (1 + _A) / 2, 0.5, 0.0, 0.0]
    xs, ys = torch.tensor(xs, dtype=torch.float64), torch.tensor(ys, dtype=torch.float64)
    assert float((xs * ys).sum()) == 1.0
    tabs = []
    for m in range(M):
        z = torch.zeros(R, 100, dtype=torch.float64)
        for s0, n, vals in ((0, A, xs), (A, A, xs), (2 * A, J1, ys), (2 * A + J1, J2, ys)):
            off = int(torch.randint(0, 14, (1,), generator=g))
            blk = (torch.arange(n) + off) % 14
            sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
            for c in range(6):
                z[s0 + torch.arange(n), 7 * blk + 1 + c] = sign * vals[c]
        assert torch.equal(z.float().double(), z)                                   # every entry is an fp32 value
        assert float(z.mean(0).pow(2).sum()) < 0.25                                 # (the tables are not centred)
        tabs.append(z)
    return tabs


def _lattice_sums_host(tabs, beta, A, J1, J2, lo, hi):
    """The 8 (M + 1) sums in fp64 from integer similarities: exact."""
    M = len(tabs)
    segs = lambda z: (z[lo:hi], z[A + lo:A + hi], z[2 * A:2 * A + J1], z[2 * A + J1:])
    fams = ((0, 2), (0, 3), (1, 3), (1, 2))                                         # X1 N1 | X1 N2 | X2 N2 | X2 N1
    out = torch.zeros(M + 1, 8, dtype=torch.float64)
    SJ = [torch.zeros(1)] * 4
    for m in range(M + 1):
        for f, (o, t) in enumerate(fams):
            if m < M:
                sg = segs(tabs[m])
                S = sg[o] @ sg[t].t()
                assert torch.equal(S, S.round()) and float(S.abs().max()) <= 1.0
                SJ[f] = SJ[f] + float(beta[m]) * S
            else:
                S = SJ[f]
            out[m, 2 * f] = torch.ldexp(torch.ones_like(S), (2 * S).int()).sum()
            out[m, 2 * f + 1] = torch.ldexp(torch.ones_like(S), S.int()).sum()
    return out


@pytest.mark.parametrize('M', [3, 2, 4])
@pytest.mark.parametrize('lite', [0, 1], ids=['full', 'lite'])
def test_lattice_sums_equal_the_fp32_sweeps_bit_for_bit(M, lite):
    import loss_gate as LG
    lib, L, p, pa, st = LG._abi()
    A, J1, J2 = SMALL
    tabs = _lattice_tables(M, A, J1, J2, 2 if lite else 3, seed=70 + M)
    beta = torch.tensor([1.0, -1.0, 1.0, 1.0])[:M].contiguous()
    tau1 = float(np.float32(1.4426950408889634))
    tau0 = tau1 / 2
    zs = [LG.packed(z, 100).cuda() for z in tabs]
    nb = int(L.sga_loss_split3_bytes(A, J1, J2))
    zbs = []
    for z in zs:
        zb = torch.zeros(nb, device='cuda', dtype=torch.uint8)
        zc = torch.zeros(2 * A + 32, LG.DP, device='cuda')
        lib.check(L.sga_loss_split3_tables(p(z), A, J1, J2, p(zb), p(zc), st), 'sga_loss_split3_tables')
        zbs.append(zb)
    b = beta.cuda()
    for lo, hi in ((0, A), SHARD):
        want = _lattice_sums_host(tabs, beta, A, J1, J2, lo, hi)
        bufs = []
        for planes in (False, True):
            buf = torch.full((LG._slots(), M + 1, 8), float('nan'), device='cuda', dtype=torch.float64)
            if planes:
                lib.check(L.sga_loss_multi_sums_bf16x6(pa(zbs), M, p(b), A, J1, J2, tau0, tau1, p(buf), lo, hi, lite, st), 'sga_loss_multi_sums_bf16x6')
            else:
                lib.check(L.sga_loss_multi_sums(pa(zs), M, 100, p(b), A, J1, J2, tau0, tau1, p(buf), lo, hi, st), 'sga_loss_multi_sums')
            bufs.append(buf[0].cpu())
        assert torch.equal(bufs[0], want), ('fp32 MFMA', lo, hi, bufs[0], want)
        assert torch.equal(bufs[1], bufs[0]), ('planes', lo, hi, bufs[1], bufs[0])
