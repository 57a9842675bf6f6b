"""CPU: how sga_loss_stash_grad_symx_bf16x6 cuts a job into workgroups (csrc/sweep3.hip: stash_plan, queried through sga_loss_stash_plan;
nothing is launched).  A product is owner blocks of 128 rows x runs of 32-row tiles; workgroup blk0 + s * nob + ob takes owner block ob and
run s = tiles [t0 + s per, min(t1, t0 + (s + 1) per)), per = ceil((t1 - t0) / nsplit) -- decoded here the way stash3_kernel does.

  cover   every (owner block, tile) of every product belongs to exactly one workgroup; the products' workgroup ranges tile the grid;
  unit    no run is longer than the unit length asked for (default 128 tiles); a product has ~4 workgroups per CU or one-tile runs;
  fill    the workgroups handed out in launch order to 2 x CUs slots (two resident workgroups per CU), each slot taking the next one when
          it is free.  List scheduling leaves no slot above the mean by more than the largest workgroup, so with costs of tiles + 1
          fill = mean / largest slot >= mean / (mean + unit + 1): asserted per launch, from the decoded workgroups, for the 19 launches of
          the configs[2] walk; the work-weighted fill of the walk is printed and held to 0.95 (every launch's bound is above that: the
          smallest launch has a slot mean of ~1400 tiles)."""
import ctypes
import heapq

import numpy as np
import pytest

A2 = 155648                    # configs[2]: 4096 pairs x 38 anchors
CUS = 256
DEFAULT_UNIT = 128              # S3_STASH_UNIT_TILES


@pytest.fixture
def unit_tiles():
    from sgaligner_amd import _lib
    before = _lib.lib().sga_loss_stash_unit_tiles(0)
    yield _lib.lib().sga_loss_stash_unit_tiles
    _lib.lib().sga_loss_stash_unit_tiles(before)


def _plan(A, job, cus=CUS):
    from sgaligner_amd import _lib
    out = (ctypes.c_int32 * 25)()
    _lib.check(_lib.lib().sga_loss_stash_plan(A, *job, cus, out), 'plan')
    prods = [dict(zip(('nown', 't0', 't1', 'nsplit', 'blk0', 'tn'), out[1 + 6 * i:7 + 6 * i])) for i in range(4)]
    return out[0], [p for p in prods if p['nown'] > 0]


def _check(A, job, unit, cus=CUS, exact=False):
    lo, hi, jl, jh, mir = job
    wgs, prods = _plan(A, job, cus)
    ns, c1, c2 = hi - lo, jh - jl, max(0, jh - mir)
    want = [(ns, jl, c1, 1), (c1, lo, ns, 0)] + ([(c2, lo, ns, 0), (ns, mir, c2, 1)] if c2 else [])
    assert [(p['nown'], p['t0'], p['t1'], p['tn']) for p in prods] == [(n, o // 32, (o + m + 31) // 32, t) for n, o, m, t in want]
    cost, nxt = [], 0
    for p in prods:
        assert p['blk0'] == nxt
        nob, tiles = -(-p['nown'] // 128), p['t1'] - p['t0']
        per = -(-tiles // p['nsplit'])
        seen = np.zeros((nob, tiles), dtype=np.int32)
        for w in range(nob * p['nsplit']):
            s, ob = divmod(w, nob)
            a, b = p['t0'] + s * per, min(p['t1'], p['t0'] + (s + 1) * per)
            if a < b:
                seen[ob, a - p['t0']:b - p['t0']] += 1
                cost.append(b - a + 1)
        assert (seen == 1).all(), (job, p)
        assert per <= unit, (job, p, per)
        if exact:
            assert p['nsplit'] == -(-tiles // unit)
        else:
            assert nob * p['nsplit'] >= 4 * cus or p['nsplit'] == tiles, (job, p)
        nxt += nob * p['nsplit']
    assert nxt == wgs
    free = [0.0] * min(2 * cus, len(cost))
    heapq.heapify(free)
    for c in cost:
        heapq.heappush(free, heapq.heappop(free) + c)
    mean = sum(cost) / len(free)
    assert max(free) <= mean + unit + 1
    return mean / max(free), float(sum(cost))


def test_configs2_walk_covers_and_fills(unit_tiles):
    import loss_gate as LG
    jobs = [tuple(j) for j in LG.sym_jobs(A2, 3, 16 << 30)]
    assert len(jobs) == 19
    for unit in (0, 64, 256, 512):
        unit_tiles(unit)
        num = den = 0.0
        for job in jobs:
            fill, work = _check(A2, job, unit or DEFAULT_UNIT)
            num += work
            den += work / fill
        print('configs[2] walk, units of %d tiles, %d slots: work-weighted modelled fill %.4f' % (unit or DEFAULT_UNIT, 2 * CUS, num / den))
        if unit == 0:
            assert num / den >= 0.95


SMALL = [(200, (0, 200, 0, 200, 200)), (200, (0, 64, 0, 200, 64)), (200, (32, 96, 32, 200, 96)), (200, (7, 29, 0, 200, 29)),
         (320, (0, 128, 0, 320, 128)), (2085, (0, 512, 0, 2085, 512)), (2085, (1536, 2085, 1536, 2085, 2085)),
         (19456, (0, 2048, 0, 19456, 2048)), (A2, (0, 32, 0, A2, 32)), (A2, (77824, 87552, 0, 38912, 0))]


@pytest.mark.parametrize('A,job', SMALL)
def test_small_and_awkward_jobs(unit_tiles, A, job):
    for cus in (256, 104, 1):
        _check(A, job, DEFAULT_UNIT, cus)
    for n in (1, 2, 3, 4, 5, 64):
        unit_tiles(-n)
        _check(A, job, n, exact=True)


def test_an_empty_job_has_no_workgroups():
    assert _plan(2080, (64, 64, 0, 2080, 64))[0] == 0
    assert _plan(2080, (0, 64, 64, 64, 64))[0] == 0
