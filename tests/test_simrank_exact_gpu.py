"""csrc/simrank.hip on data where its arithmetic is exact (tests/simrank_cases.py): rank, top-K, Hits@K, MRR, SGAR and the node
correspondences are integers, ties are dense, and every route -- staged KQ = 7 / 13 / 20 / 26 in fp32 and fp16, the fp32 stream
kernel, the fp16-table stream kernel -- has to return the reference's integers with no tolerance and no agreement threshold.
tests/test_simrank_cases_cpu.py shows that a reversed tie-break would change these integers on every case used here.

Route of each width (ceil(D/16) <= 7 / 13 / 20 / 26 staged, wider streamed):
  D = 7, 16, 112 -> staged<7>;  113, 208 -> staged<13>;  209, 320 -> staged<20>;  321, 416 -> staged<26>;
  417, 419, 430, 1000, 1024 -> simrank_stream_kernel (f16=False) / simrank_stream16_kernel (f16=True; Dp = 448, 448, 448, 1024,
  1024: odd and even counts of 32-wide K steps, zero-filled padding for all but 1024).
  D % 4 != 0 (scalar tail of a K group): 7, 113, 209, 321, 417, 419, 430."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simrank_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

_dev = {}


def _emb(case):
    if id(case) not in _dev:
        _dev[id(case)] = torch.from_numpy(case['emb']).float().cuda()
    return _dev[id(case)]


def _all_queries(case):
    """Every object as a query.  Target: the object before it in its pair (cyclic); anchors ask for their matches and the
    matches for their anchors; the object of a 1-object pair asks for the object before it, which is in another pair."""
    offs, counts = case['offs'], case['counts']
    T = int(offs[-1])
    tgt = np.concatenate([np.roll(np.arange(o, o + n), 1) for o, n in zip(offs[:-1], counts)])
    for b in np.flatnonzero(counts == 1):
        tgt[offs[b]] = offs[b] - 1 if offs[b] else 1
    dd = case['data_dict']
    inside = np.asarray([np.searchsorted(offs, a, side='right') == np.searchsorted(offs, t, side='right')
                         for a, t in zip(dd['e1i'], dd['e2i'])], dtype=bool)
    tgt[dd['e1i'][inside]] = dd['e2i'][inside]
    tgt[dd['e2i'][inside]] = dd['e1i'][inside]
    return np.arange(T, dtype=np.int32), tgt.astype(np.int32)


def _simrank(case, qi, tgt, k, f16):
    from sgaligner_amd import ops
    rank, tki, tks, _ = ops.simrank(_emb(case), case['counts'], qi, tgt, k, f16=f16)
    return rank.cpu().numpy(), tki.cpu().numpy(), tks.cpu().numpy()


def _check_simrank(case, qi, tgt, k, f16, what):
    """rank and topk_idx equal the reference exactly; topk_sim within 2e-6 (inf where the reference has inf).  Returns the
    largest distance difference (0.0: bit-equal)."""
    rank, tki, tks = _simrank(case, qi, tgt, k, f16)
    r_rank, r_idx, r_dist = C.ref_simrank(case, qi, tgt, k)
    assert rank.shape == (len(qi),) and tki.shape == (len(qi), k) and tks.shape == (len(qi), k)
    assert np.array_equal(rank, r_rank), (what, np.flatnonzero(rank != r_rank)[:8])
    assert np.array_equal(tki, r_idx), (what, np.argwhere(tki != r_idx)[:8])
    fin = np.isfinite(r_dist)
    assert np.array_equal(np.isposinf(tks), ~fin), what
    err = float(np.abs(tks[fin].astype(np.float64) - r_dist[fin]).max()) if fin.any() else 0.0
    print(f'[simrank exact] {what}: max |topk_sim - fp64| = {err:.3e}' + (' (bit-equal)' if err == 0.0 else ''))
    assert err <= 2e-6, what
    return rank, tki, tks


def _check_evaluate(case, got, ref):
    for k in (1, 2, 3, 4, 5):
        assert got[k] == ref[k], k
    # evaluate_batch reports 1/rank from fp32 ranks: exactly the fp32 reciprocal of the reference's integer rank (0 for no rank)
    want = np.asarray([np.float32(1) / np.float32(r) if r >= 1 else np.float32(0) for r in ref['ranks']], dtype=np.float32)
    assert np.isfinite(got['mrr']).all()
    assert np.array_equal(np.asarray(got['mrr'], dtype=np.float32), want) and len(got['mrr']) == len(want)
    for mode in ('2', '50', '100'):
        assert got['sgar'][mode] == ref['sgar'][mode], mode
    assert got['node_corrs'] == ref['node_corrs']


# ---- every route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', C.ROUTE_DIMS)
@pytest.mark.parametrize('f16', [False, True])
def test_every_route_returns_the_reference_integers(f16, D):
    """Ragged pairs of 130 / 8 / 37 / 11 objects, every object a query, K = 5; then the whole evaluate_batch (reg_k = 3).
    topk_sim was bit-equal to fp64 on the MI355X for every width and both modes (the printed maximum difference is 0)."""
    from sgaligner_amd import ops
    from sgaligner_amd.utils import alignment
    case = C.route_case(D)
    qi, tgt = _all_queries(case)
    _check_simrank(case, qi, tgt, 5, f16, f'D={D} f16={f16}')
    old = ops.SIMRANK_F16
    ops.SIMRANK_F16 = f16
    try:
        got = alignment.evaluate_batch(_emb(case), case['data_dict'], reg_k=3)
    finally:
        ops.SIMRANK_F16 = old
    _check_evaluate(case, got, C.ref_evaluate(case, reg_k=3))


@pytest.mark.parametrize('D', C.ROUTE_DIMS)
def test_f16_and_f32_routes_agree_on_every_rank(D):
    """On data where both arithmetics are exact the fp16 routes return ALL of the fp32 routes' ranks and neighbours."""
    case = C.route_case(D)
    qi, tgt = _all_queries(case)
    r32, k32, s32 = _simrank(case, qi, tgt, 5, False)
    r16, k16, s16 = _simrank(case, qi, tgt, 5, True)
    assert np.array_equal(r32, r16) and np.array_equal(k32, k16)
    assert np.abs(s32 - s16).max() <= 2e-6


# ---- pair sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,f16', [(416, False), (416, True), (417, False), (1000, True)])
def test_pair_size_edges(D, f16):
    """Pairs of 512, 1, 2, 15, 16, 17, 63, 64, 65, 129 and 511 objects in one batch (the small pairs' strips are sized for the
    512-object pair; at D = 416 the strip and the KQ = 26 tile take 158 208 B of the 160 KB of LDS), every object a query, K = 3."""
    from sgaligner_amd import ops
    from sgaligner_amd.utils import alignment
    case = C.edge_case(D)
    qi, tgt = _all_queries(case)
    rank, tki, tks = _check_simrank(case, qi, tgt, 3, f16, f'edges D={D} f16={f16}')
    one, two = int(case['offs'][1]), int(case['offs'][2])
    assert case['counts'][1] == 1 and case['counts'][2] == 2
    assert rank[one] == -1 and (tki[one] == -1).all() and np.isposinf(tks[one]).all()          # nobody else in the pair
    for q in (two, two + 1):
        assert rank[q] == 1 and tki[q].tolist() == [1 - (q - two), -1, -1] and np.isposinf(tks[q, 1:]).all()
    # the 1-object pair has an anchor (its target is the last object of the 512-object pair): finite, and a miss
    old = ops.SIMRANK_F16
    ops.SIMRANK_F16 = f16
    try:
        got = alignment.evaluate_batch(_emb(case), case['data_dict'], reg_k=3)
    finally:
        ops.SIMRANK_F16 = old
    ref = C.ref_evaluate(case, reg_k=3)
    _check_evaluate(case, got, ref)
    lone = int(case['na'][0])                                                                    # its place in the anchor list
    assert case['data_dict']['e1i'][lone] == one and got['mrr'][lone] == 0.0
    assert [got['sgar'][m][1] for m in ('2', '50', '100')] == [0.0, 1.0, 0.0]                    # '50' of one anchor looks at none


@pytest.mark.parametrize('f16', [False, True])
def test_513_objects_are_refused(f16):
    """Rejected by the argument check of sga_simrank, before any kernel is launched."""
    from sgaligner_amd import ops
    emb = torch.ones(513, 16, device='cuda')
    with pytest.raises(RuntimeError, match='at most 512'):
        ops.simrank(emb, [513], np.arange(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32), 1, f16=f16)


# ---- K and targets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,f16', [(209, False), (1000, True)])
def test_k_and_target_edges(D, f16):
    from sgaligner_amd import ops
    case = C.route_case(D)
    qi, tgt = _all_queries(case)
    _check_simrank(case, qi, tgt, 8, f16, f'K=8 D={D} f16={f16}')                               # SR_MAXK; > n - 1 in the 8-object pair: -1 / inf at the end
    with pytest.raises(RuntimeError, match=r'K=9 outside \[0,8\]'):                              # argument check, nothing launched
        ops.simrank(_emb(case), case['counts'], qi, tgt, 9, f16=f16)
    rank, tki, tks = _simrank(case, qi, tgt, 0, f16)                                             # ranks only
    assert tki.shape == (len(qi), 0) and tks.shape == (len(qi), 0)
    assert np.array_equal(rank, C.ref_simrank(case, qi, tgt, 0)[0])
    # targets in ANOTHER pair: the next pair's first object (cyclic), for every second query
    offs = case['offs']
    pair = np.searchsorted(offs, qi, side='right') - 1
    far = tgt.copy()
    far[::2] = offs[(pair[::2] + 1) % len(case['counts'])]
    rank, _, _ = _check_simrank(case, qi, far, 2, f16, f'foreign targets D={D} f16={f16}')
    assert (rank[::2] == -1).all() and (rank[1::2] >= 1).all()
    rank, tki, _ = _simrank(case, qi, None, 5, f16)                                              # no targets at all
    assert (rank == -1).all() and np.array_equal(tki, C.ref_simrank(case, qi, None, 5)[1])


def test_repeated_queries_come_back_in_caller_order():
    """Objects listed once, twice and three times with another target per occurrence (rank_ops.simrank serves them in rounds of
    distinct objects): row i of the result belongs to entry i of q_idx."""
    case = C.route_case(321)
    offs, counts = case['offs'], case['counts']
    rng = np.random.default_rng(11)
    objs = rng.permutation(int(offs[-1]))[:90]
    qi = np.concatenate([objs[:30], np.repeat(objs[30:60], 2), np.repeat(objs[60:], 3)])
    qi = qi[rng.permutation(len(qi))].astype(np.int32)
    pair = np.searchsorted(offs, qi, side='right') - 1
    tgt = (offs[pair] + (qi - offs[pair] + 1 + rng.integers(0, counts[pair] - 1)) % counts[pair]).astype(np.int32)
    assert (tgt != qi).all() and len({(int(a), int(t)) for a, t in zip(qi, tgt)}) > len(set(qi.tolist()))
    for f16 in (False, True):
        _check_simrank(case, qi, tgt, 4, f16, f'repeated queries f16={f16}')


# ---- pair_metrics_kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 3])
def test_pair_metrics_columns(k):
    """0, 1, 2, 3, 64, 65 and 200 anchors per pair (the lane loop past 64; the 200 in a 512-object pair), top-1 distances that tie
    between right and wrong predictions; all twelve columns.  Column 6 is an fp32 tree sum of at most 200 reciprocals
    (<= 4 per lane, then 6 shuffle levels): within 12 * 2^-24 of the fp64 sum relative to it."""
    from sgaligner_amd import ops
    from sgaligner_amd.utils import alignment
    case = C.metric_case()
    dd = case['data_dict']
    assert case['na'].tolist() == [0, 1, 2, 3, 64, 65, 200] and case['counts'][-1] == 512
    rank, tki, tks, lay = ops.simrank(_emb(case), case['counts'], dd['e1i'], dd['e2i'], k)
    got = ops.pair_metrics(rank, tki, tks, dd['e2i'], lay, dd['e1i_count']).cpu().numpy().astype(np.float64)
    ref, _ = C.ref_pair_metrics(case)
    assert got.shape == ref.shape == (7, 12)
    cols = [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]
    assert np.array_equal(got[:, cols], ref[:, cols]), (got[:, cols], ref[:, cols])
    assert (np.abs(got[:, 6] - ref[:, 6]) <= 12 * 2.0 ** -24 * np.maximum(ref[:, 6], 1.0)).all()
    assert got[0].tolist() == [0.0] * 7 + [1.0, 1.0, 1.0, 0.0, 0.0]                              # no anchors: nothing to get wrong
    res = alignment.evaluate_batch(_emb(case), dd, reg_k=3)
    _check_evaluate(case, res, C.ref_evaluate(case, reg_k=3))
    assert all(len(res['sgar'][m]) == 6 for m in ('2', '50', '100'))                             # the anchor-less pair: dropped here only
    assert res[1]['total'] == 335 and len(res['mrr']) == 335 and len(res['node_corrs']) == 7


# ---- real-valued operands at the dispatch boundaries ---------------------------------------------------------------------
@pytest.mark.parametrize('D', [113, 209, 321, 417, 419, 1024])
def test_fp32_route_accuracy_at_the_boundaries(D):
    """Exact data cannot see a precision regression.  Gaussian rows (as in test_simrank_gpu._setup), fp32 route, the first width
    of every route: |topk_sim - fp64| <= (D + 8) 2^-24, the forward bound of a length-D fp32 dot of unit vectors plus the
    scalings (under 6.2e-5 at D = 1024, an order of magnitude below the fp16 routes' ~1e-3).  Indices are held to the margin:
    the k-th returned object is at most twice that bound farther (in fp64) than the k-th nearest."""
    from sgaligner_amd import ops
    K = 5
    counts = np.asarray([100, 67, 103])
    g = torch.Generator().manual_seed(D)
    emb = torch.randn(int(counts.sum()), D, generator=g, dtype=torch.float64)
    half = np.concatenate([np.arange(o, o + n // 2) for o, n in zip(np.cumsum(counts) - counts, counts)])
    emb[half + 33] = emb[half] + 0.8 * torch.randn(len(half), D, generator=g, dtype=torch.float64)     # noisy copies, as _setup
    emb *= 0.5 + torch.rand(len(emb), 1, generator=g, dtype=torch.float64)
    emb32 = emb.float()
    qi = np.arange(len(emb), dtype=np.int32)
    _, tki, tks, _ = ops.simrank(emb32.cuda(), counts, qi, None, K, f16=False)
    tki, tks = tki.cpu().numpy(), tks.cpu().numpy().astype(np.float64)
    bound = (D + 8) * 2.0 ** -24
    worst = 0.0
    o = 0
    for n in counts:
        sim = C.pair_sim(emb32[o:o + n].double().numpy())                                       # fp64 on the kernel's own inputs
        for i in range(n):
            got = tki[o + i]
            assert len(set(got.tolist())) == K and i not in got and (got >= 0).all() and (got < n).all()
            true = np.sort(np.delete(sim[i], i))[:K]
            worst = max(worst, np.abs(tks[o + i] - sim[i][got]).max())
            assert (np.abs(tks[o + i] - sim[i][got]) <= bound).all(), (o, i)
            assert (sim[i][got] - true <= 2 * bound).all(), (o, i)
        o += n
    print(f'[simrank fp32] D={D}: max |topk_sim - fp64| = {worst:.3e}, bound {bound:.3e}')
