"""The exact (lattice) and fp32-faithful (gate) checks of the PointNet kernels, and the plumbing they share (no tests in this module).

Reference.  y[t,c] = max_p relu(W3 relu(W2 relu(W1 x[t,p] + b1) + b2) + b3)[c] literally, in fp64 torch on the CPU, with the FIRST maximiser as
arg-max; the backward over the C3 "winner rows" of an object (row (t,c) = point argmax[t,c]) as autograd defines it (ReLU' = 0 at 0):
    g = gy [y > 0]    gb3 = sum g    gW3[c,:] = sum_t g relu(Z2)    dZ2 = g W3[c,:] [Z2 > 0]    gW2 = dZ2^T H1    gb2 = colsum dZ2
    dZ1 = (dZ2 W2) [Z1 > 0]    gW1 = dZ1^T x    gb1 = colsum dZ1

Metric.  gemm_gate.rel_errors: |out - ref| / envelope in u = 2^-24, the envelope PROPAGATED through the chain (running-error kind):
    e1 = |W1||x| + |b1|     e2 = |W2|(e1 [Z1 > 0]) + |b2|     e3 = |W3|(e2 [Z2 > 0]) + |b3|
    env gb3 = sum |g|       env gW3 = sum |g| (e2 [Z2 > 0])   env gW2 = sum |dZ2|^T (e1 [Z1 > 0])   env gb2 = sum |dZ2|
    env gW1 = sum ((|dZ2||W2|) [Z1 > 0])^T |x|                env gb1 = sum (|dZ2||W2|) [Z1 > 0]
(the envelope of H1, not H1: where Z1 cancels to nearly zero, H1's own rounding error is many u of H1 but a fraction of a u of e1).  y is judged
against e3 at the reference's arg-max point (max and relu are 1-Lipschitz).

Yardstick.  The same forward and backward in plain float32 torch on the CPU with the reference's masks and arg-max -- never the library.  The
two reductions over all winner rows (gW1, gW2) are written out, 32 rows per product and the partial results added in order (rows_tn).

Guard.  The true gradient jumps where a pre-activation crosses zero; any fp32 evaluation may flip such a mask against fp64 and one flipped row
costs a whole term.  A winner row is GUARDED when any of its fp64 Z1 / Z2 values lies within DELTA = 2^-16 of its envelope (|z| <= DELTA e); its
gy is set to 0 before kernel and reference see it, so it contributes nothing under either mask.  At most GUARD_MAX of the rows may be guarded.

Lattice.  Integer-valued x, parameters and gy for which every output's envelope -- a bound of every partial sum in any order, and of the sums
of the bf16 planes' products up to the factor PLANE_SLACK -- stays below 2^24: every correct evaluation, in fp32 or on three planes, with the
atomics in any order, gives the reference bit for bit.  The builder asserts that condition; it is what makes torch.equal legitimate.

Gate.  gate_ok below -- gemm_gate.gate_ok with its floor of FLOOR_U on the max, and the rms within r x the yardstick's with no floor -- at r per
(output, mode) from profiles/pointnet_accuracy_vs_fp32.json (tools/pointnet_accuracy.py writes it): "worst measured kernel / yardstick ratio
x 2, rounded up".  tests/test_pointnet_gate_cpu.py keeps table and profile together and asserts that the emulated three-plane arithmetic
passes with six products and FAILS with five or four."""
import functools
import json
import math
import os

import torch

import gemm_gate as G

ROOT = G.ROOT
PROFILE = os.path.join(ROOT, 'profiles', 'pointnet_accuracy_vs_fp32.json')
DELTA = 2.0 ** -16
GUARD_MAX = 0.05
LIMIT = 2.0 ** 24
# |h| + |m| + |l| <= (1 + 2^-8 + 2^-16) |v| for the round-to-nearest planes of v: the sum of the absolute plane products of a term is within
# (1 + 2^-8 + 2^-16)^2 of the term's own absolute value
PLANE_SLACK = (1 + 2.0 ** -8 + 2.0 ** -16) ** 2
CUS_MI355X = 256                         # the CPU self-tests build the inputs the GPU tests build on a 256-CU card
GRADS = ('gw1', 'gb1', 'gw2', 'gb2', 'gw3', 'gb3')
MODES = {0: 'f32', 4: 'bf16x6'}

# r per output and kernel mode (0: fp32 MFMA, 4: three bf16 planes): ceil(2 x the worst ratio measured, rms or max) over the gate cases of
# profiles/pointnet_accuracy_vs_fp32.json.  test_pointnet_gate_cpu.py::test_gate_ratios_are_the_measured_ones keeps them together.
R = {
    0: {'gw1': 3, 'gb1': 6, 'gw2': 2, 'gb2': 11, 'gw3': 3, 'gb3': 6, 'y': 3},
    4: {'gw1': 3, 'gb1': 10, 'gw2': 2, 'gb2': 6, 'gw3': 2, 'gb3': 5, 'y': 1},
}

# The three-plane kernels' partial products per GEMM, as gemm_gate.PRODUCTS counts them (6 = the kernel's).  Set one short and
# test_pointnet_gate_cpu.py says which output the gate no longer sees.
PRODUCTS = {'z2': 6, 'dh1': 6, 'gw2': 6, 'l2': 6, 'l3': 6}


def ratios_from_profile(path=PROFILE):
    """mode -> output -> ceil(2 x worst measured kernel / yardstick ratio), the derivation R states."""
    worst = {}
    for c in json.load(open(path))['cases']:
        w = worst.setdefault(int(c['mode']), {})
        w[c['output']] = max(w.get(c['output'], 0.0), c['ratio_rms'], c['ratio_max'])
    return {m: {k: int(math.ceil(2.0 * v - 1e-9)) for k, v in w.items()} for m, w in worst.items()}


# ------------------------------------------------------------------------------------------------ reference, envelopes, yardstick
def forward_full(x, ws, dtype=torch.float64):
    """Every point through the chain: (Z3 with the bias [T,P,C3], Z2 [T,P,128], Z3 without the bias)."""
    w1, b1, w2, b2, w3, b3 = [w.to(dtype) for w in ws]
    z1 = x.to(dtype) @ w1.t() + b1
    z2 = z1.clamp_min(0) @ w2.t() + b2
    u3 = z2.clamp_min(0) @ w3.t()
    return u3 + b3, z2, u3


def first_argmax(z3):
    """(max over points, FIRST maximiser) of z3 [T,P,C]."""
    mx = z3.amax(dim=1)
    p = torch.arange(z3.shape[1]).view(1, -1, 1).expand_as(z3)
    am = torch.where(z3 == mx[:, None, :], p, torch.full_like(p, z3.shape[1])).amin(dim=1)
    return mx, am


def winner_rows(x, am):
    """x [T,P,3], am [T,C] -> the winners' points [T,C,3]."""
    return torch.gather(x, 1, am.long()[:, :, None].expand(-1, -1, 3))


def winner_chain(xr, ws, dtype=torch.float64):
    """Z1 [T,C,64], Z2 [T,C,128] of the winner rows and the propagated envelopes e1, e2, e3 (e3 [T,C]: row (t,c) feeds channel c alone)."""
    w1, b1, w2, b2, w3, b3 = [w.to(dtype) for w in ws]
    xr = xr.to(dtype)
    z1 = xr @ w1.t() + b1
    z2 = z1.clamp_min(0) @ w2.t() + b2
    e1 = xr.abs() @ w1.abs().t() + b1.abs()
    e2 = (e1 * (z1 > 0)) @ w2.abs().t() + b2.abs()
    e3 = ((e2 * (z2 > 0)) * w3.abs()[None]).sum(-1) + b3.abs()
    return z1, z2, e1, e2, e3


def rows_tn(a, b):
    """a^T b over the rows [R,M] x [R,N] in a STATED order: the products of 32 rows (a tile of the kernels) at a time, the partial results added
    one after the other in a's dtype.  (One big matmul leaves the order to the BLAS at hand: the float32 error of gW1 differs four-fold
    between two machines' torch builds.)"""
    R = a.shape[0]
    pad = (-R) % 32
    if pad:
        a = torch.cat([a, a.new_zeros(pad, a.shape[1])])
        b = torch.cat([b, b.new_zeros(pad, b.shape[1])])
    parts = torch.bmm(a.reshape(-1, 32, a.shape[1]).transpose(1, 2), b.reshape(-1, 32, b.shape[1]))
    acc = torch.zeros_like(parts[0])
    for part in parts:                                     # (not cumsum: torch accumulates float32 scans in double on the CPU)
        acc = acc + part
    return acc


def backward_rows(xr, g, ws, m1, m2, dtype, products=None):
    """The six gradients from winner rows xr [T,C,3], g = gy [y > 0] [T,C] and the ReLU masks m1 [T,C,64], m2 [T,C,128], in `dtype` arithmetic.
    products: None = plain matmuls; a dict like PRODUCTS = the three GEMMs of the three-plane kernel by gemm_gate.planes_product (float32)."""
    w1, b1, w2, b2, w3, b3 = [w.to(dtype) for w in ws]
    xr, g = xr.to(dtype), g.to(dtype)
    m1, m2 = m1.to(dtype), m2.to(dtype)
    T, C, _ = xr.shape
    h1 = (xr @ w1.t() + b1) * m1
    if products is None:
        z2 = h1 @ w2.t() + b2
    else:
        z2 = G.planes_product(h1.reshape(T * C, 64), w2, products['z2']).reshape(T, C, 128) + b2
    gw3 = (g[:, :, None] * (z2 * m2)).sum(0)
    dz2 = g[:, :, None] * w3[None] * m2
    if products is None:
        dh1 = dz2 @ w2
        gw2 = rows_tn(dz2.reshape(T * C, 128), h1.reshape(T * C, 64))
    else:
        dh1 = G.planes_product(dz2.reshape(T * C, 128), w2.t().contiguous(), products['dh1']).reshape(T, C, 64)
        gw2 = G.planes_product(dz2.reshape(T * C, 128).t().contiguous(), h1.reshape(T * C, 64).t().contiguous(), products['gw2'])
    dz1 = dh1 * m1
    return dict(gw1=rows_tn(dz1.reshape(T * C, 64), xr.reshape(T * C, 3)), gb1=dz1.sum((0, 1)), gw2=gw2, gb2=dz2.sum((0, 1)), gw3=gw3, gb3=g.sum(0))


def backward_envelopes(xr, g, ws, m1, m2, e1, e2):
    w1, b1, w2, b2, w3, b3 = [w.double() for w in ws]
    T, C, _ = xr.shape
    ag = g.double().abs()
    adz2 = ag[:, :, None] * w3.abs()[None] * m2
    adh1 = (adz2 @ w2.abs()) * m1
    return dict(gw1=adh1.reshape(T * C, 64).t() @ xr.double().abs().reshape(T * C, 3), gb1=adh1.sum((0, 1)),
                gw2=adz2.reshape(T * C, 128).t() @ (e1 * m1).reshape(T * C, 64), gb2=adz2.sum((0, 1)),
                gw3=(ag[:, :, None] * (e2 * m2)).sum(0), gb3=ag.sum(0))


def reference(x, ws, gy, guard=False, keep_z3=False, backward=True):
    """Everything the tests compare against, from float32 inputs, in fp64.  guard: zero gy on the guarded rows first (see the module text).
    Returns a dict: y, am (int32), gy (as the kernel must be given it), the six gradients, env (per gradient and 'y'), guarded (share of rows),
    m1, m2, xr, g (for yardstick and emulation) and, on request, z3 [T,P,C3] (float64) and the BatchNorm sums."""
    z3, z2f, u3 = forward_full(x, ws)
    mx, am = first_argmax(z3)
    y = mx.clamp_min(0)
    out = dict(y=y, am=am.int(), gy=gy, guarded=0.0)
    xd = x.double().reshape(-1, 3)
    out['bn'] = torch.cat([xd.sum(0), (xd[:, [0, 0, 0, 1, 1, 2]] * xd[:, [0, 1, 2, 1, 2, 2]]).sum(0), z2f.sum((0, 1)), (z2f * z2f).sum((0, 1)),
                           u3.sum((0, 1)), (u3 * u3).sum((0, 1))])
    out['bn_object_sq'] = max((z2f * z2f).sum(1).max().item(), (u3 * u3).sum(1).max().item(), z2f.abs().max().item() * 2.0 ** 8)
    if keep_z3:
        out['z3'] = z3
    xr = winner_rows(x, am)
    z1, z2, e1, e2, e3 = winner_chain(xr, ws)
    out['env'] = dict(y=e3)
    if not backward:
        return out
    if guard:
        near = ((z1.abs() <= DELTA * e1).any(-1) | (z2.abs() <= DELTA * e2).any(-1))
        out['guarded'] = near.float().mean().item()
        gy = torch.where(near, torch.zeros_like(gy), gy)
        out['gy'] = gy
    m1, m2 = z1 > 0, z2 > 0
    g = gy.double() * (y > 0)
    out.update(backward_rows(xr, g, ws, m1, m2, torch.float64))
    out['env'].update(backward_envelopes(xr, g, ws, m1, m2, e1, e2))
    out.update(m1=m1, m2=m2, xr=xr, g=g)
    return out


def yardstick_backward(ref, ws):
    """Plain float32 torch on the CPU with the reference's arg-max (its winner rows) and masks."""
    return backward_rows(ref['xr'], ref['g'], ws, ref['m1'], ref['m2'], torch.float32)


def yardstick_forward(x, ws):
    """y in plain float32 torch on the CPU."""
    z3, _, _ = forward_full(x, ws, torch.float32)
    return z3.amax(dim=1).clamp_min(0)


def emulate_backward(ref, ws, **short):
    """The three-plane backward's arithmetic on the CPU (float32 VALU parts, the three GEMMs by planes_product) with PRODUCTS, `short`
    overriding single entries (z2=5 forgets a product of the Z2 recomputation, ...)."""
    return backward_rows(ref['xr'], ref['g'], ws, ref['m1'], ref['m2'], torch.float32, products=dict(PRODUCTS, **short))


def emulate_forward(x, ws, **short):
    """y of the three-plane forward emulated: layer 1 in float32, layers 2 and 3 by planes_product."""
    p = dict(PRODUCTS, **short)
    w1, b1, w2, b2, w3, b3 = [w.float() for w in ws]
    T, P, _ = x.shape
    h1 = (x.float().reshape(T * P, 3) @ w1.t() + b1).clamp_min(0)
    h2 = (G.planes_product(h1, w2, p['l2']) + b2).clamp_min(0)
    z3 = G.planes_product(h2, w3, p['l3']).reshape(T, P, -1)
    return (z3.amax(dim=1) + b3).clamp_min(0)


def errors(out, ref, name):
    return G.rel_errors(out.cpu(), ref[name], ref['env'][name])


# ------------------------------------------------------------------------------------------------ inputs
def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


@functools.lru_cache(maxsize=16)
def gate_input(T, P, C3=256, seed=0, backward=True):
    """Random inputs at the weight scales of test_pointnet_fwd_out_sizes_and_modes_vs_oracle, guarded.  Returns (x, ws, ref)."""
    gen = torch.Generator().manual_seed(1000 * T + 10 * P + C3 + seed)
    ws = (_randn(gen, 64, 3) * 0.3, _randn(gen, 64) * 0.1, _randn(gen, 128, 64) * 0.15, _randn(gen, 128) * 0.1,
          _randn(gen, C3, 128) * 0.1, _randn(gen, C3) * 0.1)
    x = _randn(gen, T, P, 3) + torch.tensor([0.5, -1.0, 0.25])
    gy = _randn(gen, T, C3)
    ref = reference(x, ws, gy, guard=True, backward=backward)
    assert ref['guarded'] <= GUARD_MAX, f'{ref["guarded"]:.3%} of the winner rows sit within 2^-16 of a ReLU edge'
    return x, ws, ref


def gate_shapes(cus=CUS_MI355X):
    """(T, P) of the backward gate: one more object than the three-plane kernel has workgroup quadruples, and several objects per workgroup."""
    return [(cus // 4 + 1, 40), (300, 40)]


def _sparse_pm1(gen, rows, cols, nnz):
    """rows x cols of {-1, 0, 1} with exactly nnz non-zeros per row."""
    w = torch.zeros(rows, cols)
    idx = torch.rand(rows, cols, generator=gen).argsort(dim=1)[:, :nnz]
    w.scatter_(1, idx, (torch.randint(0, 2, (rows, nnz), generator=gen) * 2 - 1).float())
    return w


def _ri(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _sparse_rows(gen, v, keep):
    """Keep `keep` random entries of every row of v."""
    idx = torch.rand(v.shape, generator=gen).argsort(dim=1)[:, :keep]
    return torch.zeros_like(v).scatter_(1, idx, v.gather(1, idx))


LATTICES = ('narrow', 'wide', 'mirror', 'mirror_g')


@functools.lru_cache(maxsize=32)
def lattice(kind, T, P, C3=256, seed=0, backward=True, keep_z3=False):
    """Integer inputs whose every output is exact in any correct evaluation (module text).  Returns (x, ws, ref).
    narrow    x in [-4,4], parameters in {-1,0,1} (W2: 8, W3: 8 non-zeros per row), gy in [-2,2]: exact zeros in Z1, Z2, y; dense arg-max ties.
    wide      x of 19 bits, W1 in {-1,0,1}, W2 4 and W3 2 non-zeros per row, sparse gy: H1 fills all three bf16 planes, each of its planes meets
              the one plane of W2 (Z2 recomputation) and of dZ2 (gW2).
    mirror    W2 of 19 bits (4 per row) against H1 in {0,1} and dZ2 in {-1,0,1}: W2's three planes in the Z2 recomputation and in dH1 = dZ2 W2.
    mirror_g  gy of 19 bits, everything else small: the three planes of dZ2 in dH1 = dZ2 W2 and in gW2 += dZ2^T H1.
    (Round-to-nearest planes hold 8 + 1 + 8 + 1 bits in h and m: an integer needs more than 18 significant bits to have an l plane at all.)"""
    gen = torch.Generator().manual_seed(7919 * LATTICES.index(kind) + 1000 * T + 10 * P + C3 + seed)
    if kind == 'narrow':
        x = _ri(gen, -4, 4, T, P, 3)
        ws = (_ri(gen, -1, 1, 64, 3), _ri(gen, -1, 1, 64), _sparse_pm1(gen, 128, 64, 8), _ri(gen, -1, 1, 128),
              _sparse_pm1(gen, C3, 128, 8), _ri(gen, -1, 1, C3))
        gy = _ri(gen, -2, 2, T, C3)
    elif kind == 'wide':
        x = _ri(gen, -(2 ** 18), 2 ** 18, T, P, 3)
        ws = (_ri(gen, -1, 1, 64, 3), _ri(gen, -1, 1, 64), _sparse_pm1(gen, 128, 64, 4), _ri(gen, -1, 1, 128),
              _sparse_pm1(gen, C3, 128, 2), _ri(gen, -1, 1, C3))
        gy = _sparse_rows(gen, _ri(gen, 1, 2, T, C3) * (_ri(gen, 0, 1, T, C3) * 2 - 1), 3)
    elif kind == 'mirror':
        x = _ri(gen, -1, 1, T, P, 3)
        ws = (_sparse_pm1(gen, 64, 3, 1), torch.zeros(64), _sparse_pm1(gen, 128, 64, 4) * _ri(gen, 2 ** 18, 2 ** 19 - 1, 128, 64), _ri(gen, -1, 1, 128),
              _sparse_pm1(gen, C3, 128, 2), _ri(gen, -1, 1, C3))
        gy = _sparse_rows(gen, _ri(gen, 0, 1, T, C3) * 2 - 1, 2)
    elif kind == 'mirror_g':
        x = _ri(gen, -1, 1, T, P, 3)
        ws = (_ri(gen, -1, 1, 64, 3), _ri(gen, -1, 1, 64), _sparse_pm1(gen, 128, 64, 4), _ri(gen, -1, 1, 128),
              _sparse_pm1(gen, C3, 128, 4), _ri(gen, -1, 1, C3))
        gy = _sparse_rows(gen, _ri(gen, 2 ** 18, 2 ** 19 - 1, T, C3) * (_ri(gen, 0, 1, T, C3) * 2 - 1), 2)
    else:
        raise ValueError(kind)
    ref = reference(x, ws, gy, backward=backward, keep_z3=keep_z3)
    ref['limits'] = lattice_limits(x, ws, ref, backward, bn=kind == 'narrow')
    worst = max(ref['limits'].values())
    assert worst * PLANE_SLACK < LIMIT, f'lattice {kind} T={T} P={P} C3={C3}: {ref["limits"]} reaches 2^24, the outputs are not exact'
    return x, ws, ref


def lattice_limits(x, ws, ref, backward=True, bn=True):
    """The largest envelope per quantity: every pre-activation of every point, the fp32 per-object partial sums of the BatchNorm statistics
    (and 2^8 |z2|: the three-plane kernel passes z2 to its sums on two planes, 16 bits) and every gradient."""
    w1, b1, w2, b2, w3, b3 = [w.double() for w in ws]
    e1 = x.double().abs() @ w1.abs().t() + b1.abs()
    e2 = e1 @ w2.abs().t() + b2.abs()                      # no masks: a bound of the masked envelope at every point
    e3 = e2 @ w3.abs().t() + b3.abs()
    lim = dict(z1=e1.max().item(), z2=e2.max().item(), z3=e3.max().item())
    if bn:                                                 # only the narrow lattice goes through the forward with statistics
        lim['bn'] = ref['bn_object_sq']
    if backward:
        for k in GRADS:
            lim[k] = ref['env'][k].max().item()
        # the intermediate dH1 = dZ2 W2 of one row
        lim['dh1'] = ((ref['g'].abs()[:, :, None] * w3.abs()[None]) @ w2.abs()).max().item()
    return lim


# ------------------------------------------------------------------------------------------------ launches (GPU)
def run_backward(x, ws, ref, mode, separate=False):
    """sga_pointnet_bwd through the C ABI as pointnet_ops.PointNetFn.backward calls it, with the REFERENCE's arg-max and y (a tie resolved
    differently cannot enter the comparison).  separate: six gradient buffers that are not adjacent (the library then zeroes each).
    Returns name -> gradient on the device; buffers are pre-filled with NaN: the library owes the zeroing."""
    from sgaligner_amd import _lib
    from sgaligner_amd.ops import _p, _stream
    T, P, _ = x.shape
    C3 = ws[4].shape[0]
    xd = x.float().contiguous().cuda()
    wd = [w.float().contiguous().cuda() for w in ws]
    am, y, gy = ref['am'].int().cuda(), ref['y'].float().cuda(), ref['gy'].float().contiguous().cuda()
    sizes = [w.numel() for w in ws]
    if separate:
        bufs = [torch.full((n + 64,), float('nan'), device='cuda') for n in sizes]
        g = [b[32:32 + n] for b, n in zip(bufs, sizes)]
    else:
        flat = torch.full((sum(sizes),), float('nan'), device='cuda')
        g, o = [], 0
        for n in sizes:
            g.append(flat[o:o + n])
            o += n
    rc = _lib.lib().sga_pointnet_bwd(_p(xd), _p(am), _p(y), _p(gy), _p(wd[0]), _p(wd[1]), _p(wd[2]), _p(wd[3]), _p(wd[4]),
                                     _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), _p(g[4]), _p(g[5]), T, P, C3, mode, _stream())
    _lib.check(rc, 'sga_pointnet_bwd')
    torch.cuda.synchronize()
    if separate:
        for b, n in zip(bufs, sizes):
            assert torch.isnan(b[:32]).all() and torch.isnan(b[32 + n:]).all(), 'the backward wrote outside a gradient buffer'
    return {k: t.view(w.shape) for k, t, w in zip(GRADS, g, ws)}


def run_forward(x, ws, mode, want_argmax=True, bn=False):
    """ops.pointnet_forward in kernel mode 0 / 4.  Returns (y, arg-max or None, BatchNorm sums or None)."""
    from sgaligner_amd import ops
    C3 = ws[4].shape[0]
    sums = torch.full((265 + 2 * C3,), float('nan'), device='cuda', dtype=torch.float64) if bn else None
    old = ops.set_mfma_mode(MODES[mode])
    try:
        assert ops._POINTNET_MODE[ops.get_mfma_mode()] == mode
        y, am = ops.pointnet_forward(x.float().contiguous().cuda(), *[w.float().contiguous().cuda() for w in ws], want_argmax=want_argmax, bn_sums=sums)
        torch.cuda.synchronize()
    finally:
        ops.set_mfma_mode(old)
    return y, am, sums


# ------------------------------------------------------------------------------------------------ the gate, and the cases tests and profile share
def gate_ok(kernel, yard, r):
    """gemm_gate.gate_ok (its max floor FLOOR_U kept) and, on top of it, the rms within r x the yardstick's WITHOUT gemm_gate's rms floor of
    FLOOR_U / sqrt(n): that floor is for outputs of a few entries whose rms is a single draw; here it would be 0.125 u for the 64 entries of
    gb1, above the 0.10 u that a forgotten product of dH1 = dZ2 W2 leaves there."""
    return G.gate_ok(kernel, yard, r) and kernel[1] <= r * yard[1]


def forward_shapes(split_max):
    """(case, T, P): objects split over a workgroup's waves; one wave per object (the Python layer's threshold + 77 objects); few objects of one
    32-point tile, which are not split -- three of them (their partials buffer is too small to serve as LG scratch: at C3 = 256 two half-workgroups
    share an object), and nine (at C3 = 256 in mode 4 the partials buffer becomes the LG scratch)."""
    return [('split', 9, 33), ('wave', split_max + 77, 33), ('halves', 3, 31), ('lg', 9, 32)]


# What each case of forward_shapes is there for: (case, kernel mode) -> (launch form, what the workspace holds) at C3 = 64, 128, 256, as
# sga_pointnet_plan names them.  The GPU tests assert this of every call before they compare numbers: a moved threshold fails here, not silently.
_ALL = lambda form, use='NONE': {c3: (form, use) for c3 in (64, 128, 256)}
FORWARD_FORMS = {
    ('split', 0): _ALL('F32_SPLIT', 'PARTIALS'), ('split', 4): _ALL('P3_SPLIT', 'PARTIALS'),
    ('wave', 0): _ALL('F32_WAVE'), ('wave', 4): {**_ALL('P3'), 256: ('P3_LG', 'LG')},
    ('halves', 0): _ALL('F32_WAVE'), ('halves', 4): _ALL('P3'),
    ('lg', 0): _ALL('F32_WAVE'), ('lg', 4): {**_ALL('P3'), 256: ('P3_LG', 'LG')},
}
BACKWARD_FORMS = {0: 'BWD_F32', 4: 'BWD_P3'}


def planned_forward(C3, T, P, mode, bn=False):
    """The plan of the call ops.pointnet_forward makes for this shape on this card (the workspace it would offer included)."""
    from sgaligner_amd import ops
    return ops.pointnet_plan('FWD_BN' if bn else 'FWD', T, P, C3, mode, ws_bytes=ops.pointnet_workspace_bytes(T, C3, mode))


def measure_backward(T, P, mode):
    """name -> (kernel errors, yardstick errors) of the six gradients of the guarded random input (T, P) on the card."""
    x, ws, ref = gate_input(T, P)
    got = run_backward(x, ws, ref, mode)
    yard = yardstick_backward(ref, ws)
    return {k: (errors(got[k], ref, k), errors(yard[k], ref, k)) for k in GRADS}


def measure_forward(C3, T, P, mode, want_argmax=True, bn=False):
    """(kernel errors, yardstick errors) of y on the card, against e3 at the reference's arg-max point."""
    x, ws, ref = gate_input(T, P, C3, backward=False)
    y, _, _ = run_forward(x, ws, mode, want_argmax, bn)
    return errors(y, ref, 'y'), errors(yardstick_forward(x, ws), ref, 'y')
