"""Self-tests of tests/pointnet_gate.py (no card): the gate ratios are the measured ones, the guard and the lattice conditions hold for every
input the GPU tests build, and the gate has teeth -- the emulated three-plane arithmetic passes with its six partial products and fails, in
rms, with five or four, for every output the shortened product feeds."""
import pytest
import torch

import gemm_gate as G
import pointnet_gate as PG

CUS = PG.CUS_MI355X
EMU_T, EMU_P = 96, 40                    # the emulation's shape: the gate shapes' P, T kept to what a CPU test affords


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' of profiles/pointnet_accuracy_vs_fp32.json, per mode and output."""
    assert PG.ratios_from_profile() == PG.R
    for mode in (0, 4):
        assert set(PG.R[mode]) == set(PG.GRADS) | {'y'}


@pytest.mark.parametrize('T,P', PG.gate_shapes(CUS) + [(EMU_T, EMU_P)])
def test_guarded_share_of_gate_inputs(T, P):
    """At most 5 % of the winner rows sit within 2^-16 of a ReLU edge (their gy is zeroed); the guard does zero some, and leaves the rest."""
    x, ws, ref = PG.gate_input(T, P)
    assert 0 < ref['guarded'] <= PG.GUARD_MAX
    assert (ref['gy'] == 0).float().mean() <= PG.GUARD_MAX
    assert (ref['g'] != 0).float().mean() > 0.8           # y <= 0 entries carry no gradient by definition; most rows do


def _lattice_cases():
    q, h = CUS // 4, CUS // 2
    cases = [('narrow', T, P, 256, True) for T in (1, q - 1, q, q + 1, h - 1, h, h + 1, 300) for P in (1, 33)]
    cases += [('narrow', 5, 33, 256, True)] + [(k, 66, 5, 256, True) for k in ('wide', 'mirror', 'mirror_g')]
    cases += [('narrow', T, P, C3, False) for C3 in (64, 128, 256) for (_, T, P) in PG.forward_shapes(1023)]
    return cases


@pytest.mark.parametrize('kind,T,P,C3,backward', _lattice_cases())
def test_lattices_satisfy_their_envelope_condition(kind, T, P, C3, backward):
    """Every envelope below 2^24 (with the planes' slack), every reference output an integer that float32 holds."""
    x, ws, ref = PG.lattice(kind, T, P, C3, backward=backward)
    assert max(ref['limits'].values()) * PG.PLANE_SLACK < PG.LIMIT
    for k in ('y',) + (PG.GRADS if backward else ()):
        assert torch.equal(ref[k], ref[k].round()) and torch.equal(ref[k].float().double(), ref[k]), k
    assert torch.equal(ref['bn'], ref['bn'].round())
    if kind == 'narrow' and T > 1:                         # the discontinuities are hit exactly
        assert (ref['y'] == 0).any()
        if backward:
            z1, z2, _, _, _ = PG.winner_chain(ref['xr'], ws)
            assert (z1 == 0).float().mean() > 0.01 and (z2 == 0).float().mean() > 0.01


@pytest.mark.parametrize('kind', ['narrow', 'wide', 'mirror', 'mirror_g'])
def test_lattices_are_exact_in_float32_and_on_three_planes(kind):
    """What makes torch.equal legitimate: the float32 yardstick and the six-product emulation give the fp64 reference bit for bit."""
    x, ws, ref = PG.lattice(kind, 66, 5)
    yard, emu = PG.yardstick_backward(ref, ws), PG.emulate_backward(ref, ws)
    for k in PG.GRADS:
        assert torch.equal(yard[k].double(), ref[k]), k
        assert torch.equal(emu[k].double(), ref[k]), k
    assert torch.equal(PG.yardstick_forward(x, ws).double(), ref['y'])
    assert torch.equal(PG.emulate_forward(x, ws).double(), ref['y'])


@pytest.mark.parametrize('kind,short,output', [
    ('wide', dict(z2=5), 'gw3'), ('mirror', dict(z2=4), 'gw3'),            # H1's l plane, W2's l plane in the Z2 recomputation
    ('mirror_g', dict(dh1=5), 'gw1'), ('mirror', dict(dh1=4), 'gw1'),      # dZ2's l plane, W2's l plane in dH1 = dZ2 W2
    ('mirror_g', dict(gw2=5), 'gw2'), ('wide', dict(gw2=4), 'gw2'),        # dZ2's l plane, H1's l plane in gW2 += dZ2^T H1
])
def test_many_bit_lattices_need_every_plane(kind, short, output):
    """A forgotten partial product breaks bit-exactness on the lattice built to carry bits in that plane."""
    x, ws, ref = PG.lattice(kind, 66, 5)
    assert not torch.equal(PG.emulate_backward(ref, ws, **short)[output].double(), ref[output])


def test_backward_gate_would_catch_a_dropped_product():
    """Six partial products pass the gate at the three-plane kernel's r; five (l h' forgotten) and four (no l plane) fail it IN RMS for every
    output the product feeds: Z2 recomputation -> gW3, dH1 = dZ2 W2 -> gW1 and gb1, gW2 += dZ2^T H1 -> gW2.  Set a PRODUCTS entry of
    pointnet_gate.py short, or raise an r, and this test names the output that went blind."""
    x, ws, ref = PG.gate_input(EMU_T, EMU_P)
    yd = PG.yardstick_backward(ref, ws)
    yard = {k: PG.errors(yd[k], ref, k) for k in PG.GRADS}
    six = PG.emulate_backward(ref, ws)
    for k in PG.GRADS:
        e = PG.errors(six[k], ref, k)
        assert PG.gate_ok(e, yard[k], PG.R[4][k]), f'the six-product emulation misses the gate at {k}: {e} against {yard[k]}, r = {PG.R[4][k]}'
    for stage, outputs in (('z2', ('gw3',)), ('dh1', ('gw1', 'gb1')), ('gw2', ('gw2',))):
        for nprod in (5, 4):
            bad = PG.emulate_backward(ref, ws, **{stage: nprod})
            for k in outputs:
                e = PG.errors(bad[k], ref, k)
                r = PG.R[4][k]
                assert not PG.gate_ok(e, yard[k], r), f'{nprod} products in {stage} pass the gate at {k}: {e} against {yard[k]}, r = {r}'
                assert e[1] > r * yard[k][1], f'{nprod} products in {stage} are not caught by the rms of {k}: {e} against {yard[k]}, r = {r}'


@pytest.mark.parametrize('C3', [64, 256])
def test_forward_gate_would_catch_a_dropped_product(C3):
    """The same for y: layers 2 and 3 of the forward with six products pass, with five or four they fail in rms."""
    x, ws, ref = PG.gate_input(9, 33, C3, backward=False)
    yard = PG.errors(PG.yardstick_forward(x, ws), ref, 'y')
    r = PG.R[4]['y']
    six = PG.errors(PG.emulate_forward(x, ws), ref, 'y')
    assert PG.gate_ok(six, yard, r), (six, yard, r)
    for stage in ('l2', 'l3'):
        for nprod in (5, 4):
            e = PG.errors(PG.emulate_forward(x, ws, **{stage: nprod}), ref, 'y')
            assert not PG.gate_ok(e, yard, r) and e[1] > r * yard[1], f'{nprod} products in {stage} pass the gate at y: {e} against {yard}, r = {r}'


def test_gate_asks_more_than_gemm_gate_of_short_outputs():
    """gb1 has 64 entries: gemm_gate's rms floor of FLOOR_U / sqrt(n) = 0.125 u would admit the 0.10 u of a forgotten product; this gate has none."""
    e, yard = (0.3, 0.10, 64), (0.03, 0.009, 64)
    assert G.gate_ok(e, yard, 3) and not PG.gate_ok(e, yard, 3)
