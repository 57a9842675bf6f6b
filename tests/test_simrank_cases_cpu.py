"""The fixtures of tests/simrank_cases.py discriminate: on every case that tests/test_simrank_exact_gpu.py runs, the similarity is
exact in every arithmetic the kernels use, ties are dense, and the stable tie-break decides Hits@1 and SGAR -- shown with the
reference alone, by recomputing it with the tie-break reversed.  These are conditions on the inputs (the seeds in
simrank_cases.py were picked so that they hold), not measurements of the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simrank_cases as C  # noqa: E402

K = 5


@pytest.fixture(params=C.ALL_CASES, ids=lambda p: f'{p[0]}-{p[1]}')
def case(request):
    return C.get_case(*request.param)


def test_layout_and_forced_columns(case):
    dd, D = case['data_dict'], case['D']
    assert case['emb'].shape == (int(case['counts'].sum()), D)
    assert ((case['emb'] != 0).sum(axis=1) == case['nnz']).all()
    for b, n in enumerate(case['counts']):
        E = case['emb'][int(case['offs'][b]):int(case['offs'][b + 1])]
        assert (E[0::2, D - 1] != 0).all() and (E[0::2, D - 2] != 0).all()      # even rows: the last two columns
        assert (E[1::2, 0] != 0).all()                                           # odd rows: the first column
    assert int(dd['e1i_count'].sum()) == len(dd['e1i']) == len(dd['e2i'])


def test_every_arithmetic_is_exact(case):
    for b in range(len(case['counts'])):
        E = case['emb'][int(case['offs'][b]):int(case['offs'][b + 1])]
        s64 = C.pair_sim(E)
        s32 = C.pair_sim_f32_emulation(E)
        s16 = C.pair_sim_f16_emulation(E)
        assert s32.dtype == np.float32 and s16.dtype == np.float32
        assert np.array_equal(s64, s32.astype(np.float64)), b
        assert np.array_equal(s64, s16.astype(np.float64)), b
        assert np.array_equal(s64, s64.T)


def test_ties_are_dense_and_fall_on_both_sides(case):
    c = C.tie_census(case, K)
    assert c['tied'] >= 3 and c['tied'] >= 0.10 * c['anchors'], c
    assert c['tied_lower'] >= 1 and c['tied_higher'] >= 1, c
    assert c['near_tie'] >= 0.25 * c['queries'], c
    assert c['mixed_top1_tie'], c


def test_reversed_tie_break_changes_the_metrics(case):
    """A kernel whose tie comparison is inverted (larger index first) would give other Hits@1 and other SGAR flags."""
    fwd, rev = C.ref_evaluate(case), C.ref_evaluate(case, reverse_ties=True)
    assert 0 < fwd[1]['correct'] < fwd[1]['total']
    assert fwd[1]['correct'] != rev[1]['correct']
    assert any(fwd['sgar'][m] != rev['sgar'][m] for m in ('2', '50', '100'))
    assert not np.array_equal(fwd['ranks'], rev['ranks'])


def test_reversed_sgar_order_alone_changes_a_flag(case):
    """The order of equal top-1 distances among a pair's anchors is a tie-break of its own (pair_metrics_kernel's `pos`): with
    every rank and prediction as they are, reversing it alone changes an SGAR flag."""
    fwd, rev = C.ref_pair_metrics(case)[0], C.ref_pair_metrics(case, reverse_sgar_order=True)[0]
    assert np.array_equal(fwd[:, :7], rev[:, :7])
    assert not np.array_equal(fwd[:, 7:10], rev[:, 7:10])


def test_reference_agrees_with_the_oracle():
    """The helper's reference and oracle/sga_oracle.py are written independently; where the oracle is defined (every target in
    its pair) they give the same metrics."""
    from oracle import sga_oracle as O
    case = C.route_case(113)
    ref = C.ref_evaluate(case, reg_k=3)
    orc = O.evaluate_batch(torch.from_numpy(case['emb']), case['data_dict'])
    assert [ref[k]['correct'] for k in (1, 2, 3, 4, 5)] == [orc['hits'][k][0] for k in (1, 2, 3, 4, 5)]
    assert ref['mrr'] == orc['mrr'] and ref['sgar'] == orc['sgar']
    for b in range(len(case['counts'])):
        sim, _ = O.pair_similarity(torch.from_numpy(case['emb'][int(case['offs'][b]):int(case['offs'][b + 1])]))
        assert ref['node_corrs'][b] == O.node_corrs(sim, int(case['ns'][b]), 3)
