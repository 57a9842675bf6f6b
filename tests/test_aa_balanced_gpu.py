"""GPU: the launch plan of the anchors x anchors backward (csrc/aa_launch.h: two runs of row blocks, each with its own split count) on
the three-plane kernels, at sizes where it matters: A = 2080 (65 row blocks x 33 steps: more row blocks than a whole number of rounds
takes, so both runs are there and the second is cut finer) and A = 2085 (both ends ragged: a last row block of 5 rows, a last column
tile of 5 columns).  The reference is the fp32 entry through test_anchor3_gpu._against_fp32, as it is and at its tolerances; the stashes
start as NaN, so a tile nobody visits stays NaN and fails the comparison of the masks, and a tile visited twice doubles the terms, gs
and gamma.

What this reference does and does not share with the code under test: the fp32 kernels take their launch from the SAME host plan
(aa_plan) and decode their workgroup with the same aa_unit, so it is not independent of the plan.  It runs it with another geometry (two
J shares against four, a 16-column tile against 32, 512 slots against 256), so the two entries cut every job differently, and a tile that
one of them loses or doubles shows unless the other loses or doubles the very same one; the owned masks of the single jobs and the fp64
gate of test_loss_gate_gpu do not go through the fp32 entry at all.  _against_fp32 fixes the padding segments of the image at
J1 = 33 and J2 = 17 rows (its _edge), not 64 and 64: it is reused unchanged.  The walks cover the whole matrix, so "no NaN" is their
owned mask; the single jobs compare the mask itself."""
import pytest
import torch

import loss_gate as LG
from test_anchor3_gpu import _against_fp32

pytestmark = pytest.mark.gpu


def _owned(A, job):
    lo, hi, jl, jh, mir = job
    own = torch.zeros(A, A, dtype=torch.bool)
    own[lo:hi, jl:jh] = True
    if mir < jh:
        own[mir:jh, lo:hi] = True
    return own


@pytest.mark.parametrize('M', [2, 3])
@pytest.mark.parametrize('A', [2080, 2085])
def test_walks_and_single_jobs_against_the_fp32_entry(A, M):
    bound = 4 * M * 2 * A * 416                      # first block 416 rows: four blocks, the last one all own square
    sym = LG.sym_jobs(A, M, bound)
    c1 = (A // 3 + 31) // 32 * 32
    sym3 = LG.sym_jobs(A, M, bound, [0, c1, 2 * c1, A])
    assert len(sym) >= 4 and sym[-1][1] == A and sym[-1][4] >= A and any(j[2] == 0 and j[4] == 0 for j in sym3)
    for label, jobs, symmetric in (('ordered', LG.ordered_jobs(A, 544), False), ('sym', sym, True), ('sym3', sym3, True)):
        got, _ = _against_fp32(A, M, jobs, symmetric)
        assert not any(torch.isnan(d).any() for d in got[0]), label
    for job in ((0, 32, 0, A, 32),                   # one row block: every workgroup a split of the same rows
                (0, 64, 1024, A, 1024),              # all mirrored, far from the diagonal
                (1024, 1088, 0, 512, 0)):            # the wrap-around form
        got, _ = _against_fp32(A, M, [job], True)
        own = _owned(A, job)
        for d in got[0]:
            assert torch.equal(~torch.isnan(d), own), job
