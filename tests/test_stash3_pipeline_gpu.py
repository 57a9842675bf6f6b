"""GPU: the multi-tile pipeline of stash3_kernel (csrc/sweep3.hip), called directly.

Through the training step a small problem never reaches it: with few owner blocks the launch plan cuts every product into as many runs as
it has tiles, and every work unit is ONE tile.  Here sga_loss_stash_unit_tiles(-n) asks for units of exactly n tiles, so that runs shorter
than the pipeline's depth (1, 2), odd and even runs against the two-step loop (3, 4, 5), both forms of the coefficient loads (whole 128-row
owner blocks of an untransposed, 32-aligned product take the dwordx4 form, everything else the element-wise one) and the ragged edges are
all met on tables of a few hundred rows.

Reference: the four products of sga_loss_stash_grad_symx_bf16x6 in fp64 on the host, from the centred rows Zc that
sga_loss_split3_tables writes beside the planes (columns 0..99 = z - zbar, column 101 = 1: the row-sum column).
Tolerance: from the project, not from the kernel under test -- the fp32-MFMA route the planes replaced (sga_loss_stash_grad_symx on Zc:
ops.BF16X6_STASH = False) runs on the same inputs in the same test, and per table and per part
    error(planes) <= 1.25 * error(fp32 route) + 5e-7,   error = max |got - fp64| / max |fp64|
(the form of test_bf16x6_gpu.py::test_nearly_identical_rows_vs_fp64_oracle).
The lattice case asks for equality: small integers times powers of two, every partial sum exact in fp32, so a stale LDS buffer, a dropped
tile or a tile used twice cannot hide inside a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

J = 32                                     # negatives per side: present in the layout, never touched by the stash products


def _p(t):
    return t.data_ptr() if t is not None else None


def _call(name, *args):
    from sgaligner_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


class Tables:
    """The tables of one anchor count, their planes and centred rows (device) and the centred rows in fp64 (host): built once per A."""

    def __init__(self, A, lattice=False):
        from sgaligner_amd import _lib
        self.A, R = A, 2 * A + 2 * J
        g = torch.Generator().manual_seed(100 + A)
        if lattice:
            # integer rows in {-2 .. 2}, in +/- pairs: every column sums to zero exactly, so the table is not centred and the planes hold the
            # integers themselves (h plane; m = l = 0)
            half = torch.randint(-2, 3, (R // 2, 100), generator=g).float()
            zs = [torch.stack([half, -half], 1).reshape(R, 100)]
        else:
            spread = torch.randn(R, 100, generator=g)
            par = torch.randn(1, 100, generator=g) + 1e-2 * torch.randn(R, 100, generator=g)        # nearly parallel rows: centred planes
            zs = [torch.nn.functional.normalize(z, dim=1) for z in (spread, par)]
        nb = _lib.lib().sga_loss_split3_bytes(A, J, J)
        self.planes, self.zc, self.zc64 = [], [], []
        for z in zs:
            packed = torch.zeros(R + 32, 104)
            packed[:R, :100] = z
            packed = packed.cuda()
            planes = torch.empty(nb, device='cuda', dtype=torch.uint8)
            zc = torch.zeros(2 * A + 32, 104, device='cuda')
            _call('sga_loss_split3_tables', _p(packed), A, J, J, _p(planes), _p(zc))
            self.planes.append(planes)
            self.zc.append(zc)
            self.zc64.append(zc[:2 * A].cpu().double())
        torch.cuda.synchronize()
        if lattice:
            assert torch.equal(self.zc64[0][:, :100], zs[0][:2 * A].double()) and bool((self.zc64[0][:, 101] == 1).all())
        else:
            assert float(self.zc64[0][:, :100].sub(zs[0][:2 * A].double()).abs().max()) == 0.0          # the spread table: zbar = 0
            assert float(self.zc64[1][:, :100].abs().max()) < 0.1 * float(zs[1].abs().max())            # the parallel one: centred


_TABLES = {}


def tables(A, lattice=False):
    if (A, lattice) not in _TABLES:
        _TABLES[A, lattice] = Tables(A, lattice)
    return _TABLES[A, lattice]


def host_products(zc64, A, m1, m2, job):
    """dZ [2A, 104] in fp64: the four products of sga_loss_stash_grad_symx_bf16x6 (its own comment), from the centred rows."""
    lo, hi, jl, jh, mir = job
    x1, x2 = zc64[:A], zc64[A:2 * A]
    d = torch.zeros(2 * A, 104, dtype=torch.float64)
    m1 = m1.double()
    d[lo:hi] += m1.t() @ x2[jl:jh]
    d[A + jl:A + jh] += m1 @ x1[lo:hi]
    if m2 is not None:
        m2 = m2.double()
        d[mir:jh] += m2 @ x2[lo:hi]
        d[A + lo:A + hi] += m2.t() @ x1[mir:jh]
    return d


def stashes(job, seed, lattice=False):
    lo, hi, jl, jh, mir = job
    ns, c1, c2 = hi - lo, jh - jl, max(0, jh - mir)
    g = torch.Generator().manual_seed(seed)
    out = []
    for rows in (c1, c2):
        if rows == 0:
            out.append(None)
        elif lattice:
            # integers below 2^8 (the h plane alone), and at most 8 per row and per column of up to 320 with 20 significant bits (all three
            # planes): |any partial sum| <= 8 * 2^19 * 2 + 320 * 2^8 * 2 < 2^24, exact in fp32 in any order
            m = torch.randint(-255, 256, (rows, ns), generator=g)
            big = torch.randint(-(1 << 19) + 1, 1 << 19, (rows, ns), generator=g) | 1
            jj, ii = torch.meshgrid(torch.arange(rows), torch.arange(ns), indexing='ij')
            out.append(torch.where((ii + 3 * jj) % 41 == 0, big, m).float())
        else:
            out.append(torch.randn(rows, ns, generator=g) * torch.rand(rows, 1, generator=g))
    return out


def run_planes(T, k, m1, m2, job, unit):
    from sgaligner_amd import _lib
    dz = torch.zeros(2 * T.A + 32, 104, device='cuda')
    before = _lib.lib().sga_loss_stash_unit_tiles(unit)
    try:
        _call('sga_loss_stash_grad_symx_bf16x6', _p(m1), _p(m2), _p(T.planes[k]), T.A, J, J, _p(dz), *job)
        torch.cuda.synchronize()
    finally:
        _lib.lib().sga_loss_stash_unit_tiles(before)
    return dz[:2 * T.A].cpu()


def run_fp32(T, k, m1, m2, job):
    dz = torch.zeros(2 * T.A + 32, 104, device='cuda')
    _call('sga_loss_stash_grad_symx', _p(m1), _p(m2), _p(T.zc[k]), T.A, 104, _p(dz), *job)
    torch.cuda.synchronize()
    return dz[:2 * T.A].cpu()


def _errors(got, ref):
    got = got.double()
    return tuple(float((got[:, c] - ref[:, c]).abs().max() / ref[:, c].abs().max()) for c in (slice(0, 100), slice(101, 102)))


def check_job(A, job, units, seed):
    """Both tables, every unit length: the planes kernel within 1.25 x the fp32 route's error + 5e-7 of fp64, columns 0..99 and column 101."""
    T = tables(A)
    m1, m2 = stashes(job, seed)
    d1, d2 = m1.cuda(), (m2.cuda() if m2 is not None else None)
    for k in range(2):
        ref = host_products(T.zc64[k], A, m1, m2, job)
        e32 = _errors(run_fp32(T, k, d1, d2, job), ref)
        for unit in units:
            got = run_planes(T, k, d1, d2, job, unit)
            e = _errors(got, ref)
            print('A %d job %s table %d unit %d: error planes (%.3g, %.3g), fp32 route (%.3g, %.3g)' % (A, job, k, unit, *e, *e32))
            assert e[0] <= 1.25 * e32[0] + 5e-7 and e[1] <= 1.25 * e32[1] + 5e-7, (job, k, unit, e, e32)
            # nothing outside the parts: columns 100, 102, 103 and rows the job does not own stay zero
            assert float(got[:, 100].abs().max()) == 0.0 and float(got[:, 102:].abs().max()) == 0.0
            assert not bool(((got != 0).any(1) & ~(ref != 0).any(1)).any())


@pytest.mark.parametrize('unit', [1, 2, 3, 4, 5])
def test_units_of_one_to_five_tiles(unit):
    """A = 320, ten tiles: runs of (1 x 10) | (2 x 5) | (3, 3, 3, 1) | (4, 4, 2) | (5, 5) -- shorter than the pipeline's depth, odd and even
    against the two-step loop; the ordered block and a symmetric one (all four products, whole owner blocks on the dwordx4 form)."""
    check_job(320, (0, 320, 0, 320, 320), [-unit], seed=1)
    check_job(320, (0, 128, 0, 320, 128), [-unit], seed=2)


@pytest.mark.parametrize('nown', [1, 31, 33, 127, 129, 160])
def test_owner_counts(nown):
    """ns owner rows of the transposed products (and ns 'other' rows of the untransposed ones): a part-filled second row set, more than one
    owner block, a part-filled last block; units as the plan cuts them (one tile) and of two and three tiles."""
    check_job(200, (0, nown, 0, 200, nown), [0, -2, -3], seed=10 + nown)


JOBS = [(0, 200, 0, 200, 200),                                                      # ordered, no M2
        (0, 64, 0, 200, 64), (32, 96, 32, 200, 96), (64, 200, 64, 200, 200),        # the blocks of a symmetric walk
        (7, 29, 0, 200, 29)]                                                        # an anchor shard: ld = 22, others off the tile grid


@pytest.mark.parametrize('job', JOBS)
def test_jobs(job):
    check_job(200, job, [0, -2, -3], seed=sum(job))


@pytest.mark.parametrize('unit', [1, 3, 4])
def test_lattice_is_exact(unit):
    """Integer rows and integer coefficients (up to 20 significant bits: all three coefficient planes), every partial sum below 2^24: dZ
    equals the host's integer result bit for bit, whatever the order of the additions."""
    A = 320
    T = tables(A, lattice=True)
    for job, seed in (((0, 128, 0, 320, 128), 5), ((128, 320, 128, 320, 320), 6)):
        m1, m2 = stashes(job, seed, lattice=True)
        ref = host_products(T.zc64[0], A, m1, m2, job)
        assert 2 ** 19 < float(ref.abs().max()) < 2 ** 24
        got = run_planes(T, 0, m1.cuda(), m2.cuda() if m2 is not None else None, job, -unit)
        want = ref.float()
        want[:, 100] = 0
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, (job, unit, bad[:8].tolist(), [(float(got[i, j]), float(want[i, j])) for i, j in bad[:8].tolist()])
