"""The fusion kernels on the card: bit-equal to fp64 on the lattice of tests/fusion_gate.py at the widths and row counts where the row kernels
go wrong (below one wave, 64, 65, a ragged last trip; one pass of the row loop -1, +0, +1 and two passes and a bit), and fp32-faithful under
the gate on Gaussian inputs built to cancel."""
import functools

import pytest
import torch

import fusion_gate as FG

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def P():
    return FG.device_rows_per_pass()


SMALL_T = ('1', '5')
BIG_T = ('P-1', 'P', 'P+1', '2P+7')


def rows(t):
    return {'1': 1, '5': 5, 'P-1': P() - 1, 'P': P(), 'P+1': P() + 1, '2P+7': 2 * P() + 7}[t]


EQUAL = [(M, D, t) for M in FG.LATTICE_MS for D in FG.LATTICE_DS for t in SMALL_T] + \
        [(M, D, t) for M in FG.LATTICE_MS for D in FG.LATTICE_BIG_DS for t in BIG_T]


@pytest.mark.parametrize('M,D,t', EQUAL)
def test_lattice_equal_widths(M, D, t):
    lat = FG.lattice(rows(t), (D,) * M)
    FG.assert_lattice_equal(FG.run(lat['weight'], lat['tabs'], lat['gj'], 'equal'), lat, f'M {M} D {D} T {rows(t)}')


@pytest.mark.parametrize('widths', FG.LATTICE_VAR_WIDTHS)
@pytest.mark.parametrize('t', ['1', 'P+1', '2P+7'])
def test_lattice_differing_widths(widths, t):
    lat = FG.lattice(rows(t), widths)
    FG.assert_lattice_equal(FG.run(lat['weight'], lat['tabs'], lat['gj'], 'var'), lat, f'widths {widths} T {rows(t)}')


@pytest.mark.parametrize('M,D', [(3, 100), (8, 65)])
def test_equal_widths_through_both_routes(M, D):
    """test_eva_gpu.py::test_fusion_equal_widths_keep_the_old_entry_point at two passes of the row loop and a bit: equal bits for the output
    and the table gradients (the weight gradient folds fp64 atomics in no fixed order: the gate judges it)."""
    T = 2 * P() + 7
    gen = torch.Generator().manual_seed(M * 1000 + D)
    tabs = [torch.randn(T, D, generator=gen) for _ in range(M)]
    w, gj = torch.randn(M, 1, generator=gen), torch.randn(T, M * D, generator=gen)
    old, var = FG.run(w, tabs, gj, 'equal'), FG.run(w, tabs, gj, 'var')
    assert FG.same_bits(old[0], var[0]) and FG.same_bits(old[1], var[1])
    assert torch.allclose(old[2], var[2], rtol=1e-5, atol=1e-7)
    FG.assert_gate(FG.measure(var, w, tabs, gj), f'var route M {M} D {D} T {T}')


@pytest.mark.parametrize('M', FG.GATE_MS)
@pytest.mark.parametrize('kind', ['equal', 'ragged'])
@pytest.mark.parametrize('t', ['33', 'P+1'])
def test_gate(M, kind, t):
    T = 33 if t == '33' else P() + 1
    case = FG.gate_case(T, FG.gate_widths(M, kind))
    w, tabs, gj = case['weight'], case['tabs'], case['gj']
    got = FG.run(w, tabs, gj)
    FG.assert_gate(FG.measure(got, w, tabs, gj, case['judged']), f'M {M} {kind} T {T}')
    assert FG.zero_rows_ok(got, case['judged'], gj)


@pytest.mark.parametrize('route,widths', [('equal', (65,) * 4), ('equal', (3,) * 8), ('var', (1, 64, 65, 257))])
def test_weight_shift_changes_no_bit(route, widths):
    """softmax subtracts the maximum: adding 3.0 to every weight leaves the output (and, on the lattice, every gradient) as it was."""
    lat = FG.lattice(P() + 1, widths)
    plain = FG.run(lat['weight'], lat['tabs'], lat['gj'], route)
    shifted = FG.run(lat['weight'] + 3.0, lat['tabs'], lat['gj'], route)
    assert FG.same_bits(plain[0], shifted[0])
    FG.assert_lattice_equal(shifted, lat, f'weights + 3, {route} {widths}')
