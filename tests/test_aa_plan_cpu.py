"""CPU: the launch plan of the anchors x anchors backward (csrc/aa_launch.h: aa_plan, queried through sga_loss_anchor_plan; nothing is
launched).  A job is two runs of row blocks, each cut into `n` interleaved splits; split s of n walks the steps s, s + n, ... of its row
block, a step being H 16-column halves side by side.  For every job:

  cover    every (row block, 16-column half) of the job belongs to exactly one workgroup;
  balance  NOT the per-workgroup bound ("no workgroup above the mean modelled cost by more than 3 %"): one equal-cost contiguous range per
           workgroup, the partition that bound describes, was built and timed, and lost (the walk of configs[2] 497.6 ms against 425.6 ms,
           profiles/aa_fill_contiguous_ranges.txt), so the workgroups come in two sizes by design -- 1217 steps against 145 in
           the first launch of that walk -- and the 3 % is asked of what runs side by side instead: of the workgroups of a run (equal to
           within one step), and of the SLOTS.  With the workgroups handed out in launch order to min(slots, workgroups) slots, each slot
           taking the next one when it is free, no slot's modelled cost (steps + 1 per workgroup, aa_plan's model) is above the mean by
           more than 3 %, or by more than 2 units where 3 % of the mean is less than that: costs are whole numbers, so a slot's total
           is up to 1 above a fractional mean before anything is uneven, and one step, the least that can be moved, is 1 more.  Every job
           is held to this, the small ones too; nothing wider.
  fill     mean / largest slot total of the same hand-out >= 0.97 -- or >= mean / (mean + 2) where the mean is below 2 / 0.03 = 67 units,
           the same two units.  Every job.  A job with fewer workgroups than slots is measured on the slots it uses: no plan fills the rest.

Because the interleaving gives every split of a row block the same mix of own-square and mirrored tiles (to within one step of either
class: checked), steps stand for cost and the two classes need no weights.

The plan this replaces -- one n = ceil(3 CUs / nib) for the whole job, ceil(nib n / 256) rounds, the last part-filled -- is recomputed for
the configs[2] walk from its formula: 0.850 of the slots filled, work-weighted."""
import ctypes
import heapq

import numpy as np
import pytest

A2 = 155648                    # configs[2]: 4096 pairs x 38 anchors


def _plan(planes, M, A, job, slots):
    from sgaligner_amd import _lib
    out = (ctypes.c_int32 * 8)()
    a_lo, a_hi, j_lo, j_hi = job[:4]
    _lib.check(_lib.lib().sga_loss_anchor_plan(planes, M, A, a_lo, a_hi, j_lo, j_hi, slots, out), 'plan')
    return dict(zip(('rows', 'shares', 'nib', 'nib1', 'n1', 'n2', 'wgs', 'steps'), out))


def _walk_jobs(A, n_tables, stash_bytes):
    """The jobs of the symmetric walk of one rank, from the code that sizes them (loss_ops._sym_jobs under that stash budget)."""
    import loss_gate as LG
    return [tuple(j) for j in LG.sym_jobs(A, n_tables, stash_bytes)]


def _workgroups(p):
    """[(row block, [steps])] in launch order, decoded the way the kernels do (aa_epilogue.h: aa_unit)."""
    wgs = []
    for w in range(p['wgs']):
        n_first = p['nib1'] * p['n1']
        if w < n_first:
            n, ib, s = p['n1'], w // p['n1'], w % p['n1']
        else:
            n, ib, s = p['n2'], p['nib1'] + (w - n_first) // p['n2'], (w - n_first) % p['n2']
        wgs.append((ib, list(range(s, p['steps'], n))))
    return wgs


def _check(planes, M, A, job, slots):
    a_lo, a_hi, j_lo, j_hi, mir = job
    p = _plan(planes, M, A, job, slots)
    ct = 32 if planes else 16
    halves = ((j_hi + ct - 1) // ct * ct - j_lo) // 16
    assert p['nib'] == -(-(a_hi - a_lo) // p['rows']) and p['steps'] == -(-halves // p['shares'])
    wgs = _workgroups(p)
    # cover: every (row block, half) once -- steps past the last half are no tiles (the kernels' loop bound)
    seen = np.zeros((p['nib'], p['steps']), dtype=np.int32)
    for ib, steps in wgs:
        assert 0 <= ib < p['nib']
        for t in steps:
            seen[ib, t] += 1
    assert (seen == 1).all(), (job, p)
    # the two tile classes, per workgroup of one row block: equal to within one step each
    own_steps = (min(max(mir, j_lo), j_lo + 16 * halves) - j_lo) // (16 * p['shares'])       # whole steps left of the mirror start
    for ib0 in {0, p['nib'] - 1}:
        own = [sum(t < own_steps for t in steps) for ib, steps in wgs if ib == ib0]
        n = len(own)
        assert max(own) - min(own) <= 1 and all(abs(o - own_steps / n) < 1 for o in own), (job, p)
    # balance: within a run, and over the slots after the greedy hand-out in launch order
    cost = np.array([len(steps) + 1 for _, steps in wgs], dtype=np.float64)
    for run in (cost[:p['nib1'] * p['n1']], cost[p['nib1'] * p['n1']:]):
        assert len(run) == 0 or run.max() <= max(1.03 * run.mean(), run.mean() + 1.0), (job, p)
    free = [0.0] * min(slots, len(cost))
    heapq.heapify(free)
    for c in cost:
        heapq.heappush(free, heapq.heappop(free) + c)
    mean = cost.sum() / len(free)
    fill = mean / max(free)
    print('%s slots %d: %d workgroups, slot mean %.2f, largest %.0f, fill %.4f' % (job, slots, len(cost), mean, max(free), fill))
    assert max(free) <= max(1.03 * mean, mean + 2.0), (job, p, max(free), mean)
    assert fill >= min(0.97, mean / (mean + 2.0)), (job, p, fill)
    return fill, cost.sum()


def test_configs2_walk_fills_the_slots():
    jobs = _walk_jobs(A2, 3, 16 << 30)
    assert len(jobs) == 19 and [hi - lo for lo, hi, *_ in jobs[:2]] == [4576, 4736]
    num = den = 0.0
    for job in jobs:
        fill, work = _check(1, 3, A2, job, 256)
        num += work
        den += work / fill
    print('configs[2] walk, three-plane kernel, 256 slots: work-weighted modelled fill %.4f' % (num / den))
    assert num / den >= 0.985


def test_the_plan_before_filled_085():
    """The single split count the launches used, by its formula: nsplit = ceil(3 x 256 / nib), capped by the steps; equal workgroups in
    ceil(nib nsplit / 256) rounds."""
    num = den = 0.0
    fills = {}
    for lo, hi, j_lo, j_hi, _ in _walk_jobs(A2, 3, 16 << 30):
        nib, steps = (hi - lo + 31) // 32, -(-((j_hi + 31) // 32 * 32 - j_lo) // 64)
        nsplit = max(1, min(-(-3 * 256 // nib), steps))
        wgs = nib * nsplit
        fills[hi - lo] = wgs / (-(-wgs // 256) * 256)
        num += nib * steps
        den += nib * steps / fills[hi - lo]
    assert abs(fills[8256] - 0.755) < 0.002 and abs(fills[10304] - 0.943) < 0.002 and abs(fills[4576] - 0.84) < 0.005
    assert abs(num / den - 0.850) <= 0.005, num / den


SMALL = [
    # (planes, M, A, (a_lo, a_hi, j_lo, j_hi, mir), slots)
    (1, 3, 2080, (0, 32, 0, 2080, 32), 256),               # one row block
    (1, 3, 97, (0, 97, 0, 97, 97), 256),                   # fewer steps than workgroup slots, ragged both ways
    (0, 3, 97, (0, 97, 0, 97, 97), 256),
    (0, 4, 97, (32, 97, 32, 97, 97), 512),
    (1, 3, 2085, (0, 2085, 0, 2085, 2085), 256),           # A = 2085: the ordered block
    (1, 2, 2085, (0, 512, 0, 2085, 512), 256),
    (1, 3, 2085, (1536, 2085, 1536, 2085, 2085), 256),     # all own-square
    (1, 3, 2085, (0, 64, 1024, 2085, 1024), 256),          # all mirrored
    (1, 3, 2085, (1024, 1088, 0, 512, 0), 256),            # the wrap-around form
    (0, 3, 2085, (0, 2085, 0, 2085, 2085), 512),
    (0, 4, 2085, (0, 1024, 0, 2085, 1024), 256),
    (1, 3, 2080, (0, 2080, 0, 2080, 2080), 1),             # one slot
    (0, 2, 2080, (0, 2080, 0, 2080, 2080), 1),
    (1, 3, 19456, (0, 2048, 0, 19456, 2048), 104),         # a smaller chip
    (1, 3, 19456, (2048, 4096, 2048, 19456, 4096), 104),
    (1, 3, 19456, (0, 2048, 0, 19456, 2048), 256),
    (1, 3, 19456, (0, 2048, 0, 19456, 2048), 512),
    (0, 4, 19456, (0, 2048, 0, 19456, 2048), 512),
    (1, 3, 19456, (18432, 19456, 18432, 19456, 19456), 256),
    (1, 3, A2, (0, 32, 0, A2, 32), 256),
    (1, 3, A2, (0, 8224, 0, A2, 8224), 256),               # 257 row blocks: one more than the slots
    (1, 2, A2, (A2 - 8928, A2, A2 - 8928, A2, A2), 256),
    (0, 3, A2, (0, 4576, 0, A2, 4576), 512),
    (1, 3, A2, (77824, 87552, 0, 38912, 0), 256),          # a rank's wrap-around rectangle
]


@pytest.mark.parametrize('planes,M,A,job,slots', SMALL)
def test_small_and_awkward_jobs(planes, M, A, job, slots):
    _check(planes, M, A, job, slots)


def test_an_empty_job_has_no_workgroups():
    assert _plan(1, 3, 2080, (64, 64, 0, 2080), 256)['wgs'] == 0
    assert _plan(1, 3, 2080, (0, 64, 64, 64), 256)['wgs'] == 0
