"""GPU tier of the pair-job contract (csrc/pair_jobs.h): the two nearest-neighbour searches, given the same job list over the same
points, answer alike -- same output layout, same index for every query, same squared distance -- in the one-pass and in the split form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1025, 0, 129, 300]                               # two nn_kernel query tiles; nine featnn tiles, the last holding one query
PAIRS = [(0, 3), (0, 1), (1, 0), (2, 2), (3, 0)]          # an empty support, an empty query set, a self-match


def test_the_two_searches_honour_one_contract():
    """Integer lattice points in [0, 8)^3: every fp32 score |b|^2 - 2 a.b and every fp64 d2 is an exact integer, the score's arg-min IS
    the distance's, and ties are dense (512 distinct points), so both lowest-index-among-minima rules must pick the same row and no
    tolerance is needed.  Once with the default chunks, once with chunk = 128 (featnn) / 100 (nn): supports of 300 and 1025 rows split into
    3 / 9 and 3 / 11 chunks with a ragged last one."""
    from sgaligner_amd.utils import point_cloud as PC, registration as RG
    rng = np.random.default_rng(5)
    pts = rng.integers(0, 8, size=(sum(SIZES), 3)).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    d_pts = torch.from_numpy(pts).cuda()
    d_feats = torch.from_numpy(np.concatenate([pts, np.zeros((len(pts), 1))], axis=1).astype(np.float32)).cuda()
    want_off = np.concatenate([[0], np.cumsum([SIZES[a] for a, _ in PAIRS])])
    ties = 0
    for nn_chunk, fn_chunk in ((None, None), (100, 128)):
        dist, n_idx, n_off = PC.nearest_neighbor_batch(d_pts, off, PAIRS, chunk=nn_chunk, squared=True)
        f_idx, f_d2, f_off = RG.feature_nn_batch(d_feats, off, PAIRS, chunk=fn_chunk)
        assert np.array_equal(n_off, f_off) and np.array_equal(n_off, want_off) and n_off.dtype == f_off.dtype == np.int64
        dist, n_idx, f_idx, f_d2 = dist.cpu().numpy(), n_idx.cpu().numpy(), f_idx.cpu().numpy(), f_d2.cpu().numpy()
        assert n_idx.dtype == f_idx.dtype == np.int32 and dist.dtype == f_d2.dtype == np.float64
        assert np.array_equal(n_idx, f_idx), (nn_chunk, int((n_idx != f_idx).sum()))
        assert np.array_equal(dist.view(np.int64), f_d2.view(np.int64)), (nn_chunk, int((dist != f_d2).sum()))
        for p, (a, b) in enumerate(PAIRS):
            got_i, got_d = n_idx[n_off[p]:n_off[p + 1]], dist[n_off[p]:n_off[p + 1]]
            assert len(got_i) == SIZES[a]
            if SIZES[b] == 0:
                assert (got_i == -1).all() and np.isposinf(got_d).all() and len(got_i) == 1025          # the empty support: (-1, +inf)
                continue
            q, s = pts[off[a]:off[a + 1]], pts[off[b]:off[b + 1]]
            d = ((q[:, None, :] - s[None, :, :]) ** 2).sum(2)                                           # exact integers in fp64
            assert np.array_equal(got_i, d.argmin(1)) and np.array_equal(got_d, d.min(1))               # numpy.argmin: the lowest index
            ties += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
        assert (dist[n_off[3]:n_off[4]] == 0.0).all()                                                   # the self-match finds itself (or an earlier twin)
    assert ties > 1000                                                                                  # the data exists for its ties
