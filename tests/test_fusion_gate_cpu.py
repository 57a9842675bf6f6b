"""No card needed: the fusion gate's table against its profile, the lattice's exactness claim, the sensitivity of both checks to four emulated
defects (and of the ELU bound to an expf(x) - 1), and the argument contract of the four fusion entries."""
import ctypes
import math

import pytest
import torch

import eva_gate as EG
import fusion_gate as FG

P_MI355X = FG.rows_per_pass()
GATE_CASES = FG.gate_cases(P_MI355X)


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' of profiles/fusion_accuracy_vs_fp32.json per output, the ELU bounds
    are 'the worst measured error x 2, rounded up' of its element-wise rows, and neither exceeds its cap."""
    assert FG.ratios_from_profile() == FG.R
    assert FG.ulps_from_profile() == FG.ULP
    assert set(FG.R) == set(FG.OUTPUTS) and all(1 <= r <= FG.R_CAP for r in FG.R.values())
    assert set(FG.ULP) == {'elu_fwd', 'elu_bwd'} and all(1 <= b <= FG.ULP_CAP for b in FG.ULP.values())


def test_gate_cases_are_the_issues():
    assert P_MI355X == 8192
    assert len(GATE_CASES) == 24 and {len(w) for _, _, w in GATE_CASES} == {1, 2, 3, 5, 7, 8} and {t for _, t, _ in GATE_CASES} == {33, 8193}
    for _, _, w in GATE_CASES:
        assert w == (100,) * len(w) or (len(set(w)) == len(w) and w[0] > 64 and w[0] % 64)      # the ragged mix starts with a ragged last trip


# ------------------------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize('M', FG.LATTICE_MS)
@pytest.mark.parametrize('D', FG.LATTICE_DS)
def test_lattice_float32_equals_fp64(M, D):
    """The exactness claim: the float32 yardstick (autograd) and the kernels' formulas in float32 both equal the fp64 reference bit for bit."""
    lat = FG.lattice(300, (D,) * M)
    for j, x in enumerate(lat['tabs']):
        nz = (x != 0).sum(1)
        assert (x.abs().sum(1) > 0).all() and ((nz == 1) | (nz == 4) | (nz == 16) | (nz == 64)).all() and (nz <= D).all()
    FG.assert_lattice_equal(FG.evaluate(lat['weight'], lat['tabs'], lat['gj'], torch.float32), lat, 'float32 autograd')
    FG.assert_lattice_equal(FG.emulate(lat['weight'], lat['tabs'], lat['gj']), lat, 'float32 formulas')
    shifted = FG.evaluate(lat['weight'] + 3.0, lat['tabs'], lat['gj'], torch.float32)
    FG.assert_lattice_equal(shifted, lat, 'weights + 3')


@pytest.mark.parametrize('widths', FG.LATTICE_VAR_WIDTHS)
@pytest.mark.parametrize('T', [1, 2 * 64 + 7])
def test_lattice_of_differing_widths_is_exact(widths, T):
    lat = FG.lattice(T, widths)
    FG.assert_lattice_equal(FG.evaluate(lat['weight'], lat['tabs'], lat['gj'], torch.float32), lat)
    FG.assert_lattice_equal(FG.emulate(lat['weight'], lat['tabs'], lat['gj']), lat)


def test_lattice_at_the_largest_row_count_round_trips():
    """2 P + 7 rows of 8 tables: the builder's assertion (every reference value a float32 number) holds where the sums a_m are longest."""
    lat = FG.lattice(2 * P_MI355X + 7, (65,) * 8)
    assert lat['gw'].abs().max() > 0


@pytest.mark.parametrize('defect', FG.DEFECTS)
@pytest.mark.parametrize('widths', [(100,), (100,) * 4, (65, 257, 130, 100), (400, 200, 100, 100)])
def test_lattice_catches_the_defect(defect, widths):
    """Each emulated defect differs from the lattice's reference: 'tail' on widths with D > 64 and D % 64 != 0, 'rows' at T > P (P = 64 here)."""
    P = 64
    lat = FG.lattice(2 * P + 7, widths)
    got = FG.emulate(lat['weight'], lat['tabs'], lat['gj'], defect, P)
    assert not FG.lattice_equal(got, lat)
    hit = {k for k, g in zip(FG.OUTPUTS, got) if not torch.equal(g, lat[k])}
    want = {'tail': {'out', 'gx', 'gw'}, 'c2': {'gx'}, 'jacobian': {'gw'}, 'rows': {'out', 'gx', 'gw'}}[defect]
    if len(widths) == 1 and defect != 'jacobian':
        want = want - {'gw'}                              # one table: a - w a is 0 whatever a is
    assert hit == want


def test_rows_defect_needs_more_rows_than_a_pass():
    lat = FG.lattice(64, (65,) * 2)
    assert FG.lattice_equal(FG.emulate(lat['weight'], lat['tabs'], lat['gj'], 'rows', 64), lat)
    lat = FG.lattice(65, (65,) * 2)
    assert not FG.lattice_equal(FG.emulate(lat['weight'], lat['tabs'], lat['gj'], 'rows', 64), lat)


# ------------------------------------------------------------------------------------------------ the gate
# (defect, output) pairs the gate does NOT see at a case, with the reason -- none: every arithmetic defect fails at every gate case.
UNSEEN = {}
SEEN_IN = {'tail': ('out', 'gx'), 'c2': ('gx',), 'jacobian': ('gw',)}


@pytest.mark.parametrize('name,T,widths', GATE_CASES, ids=[c[0] for c in GATE_CASES])
def test_gate_passes_the_formulas_and_catches_the_defects(name, T, widths):
    """At the r in use the kernels' formulas in float32 pass, and each arithmetic defect fails on the outputs it touches."""
    case = FG.gate_case(T, widths)
    w, tabs, gj, judged = case['weight'], case['tabs'], case['gj'], case['judged']
    assert int((~judged['keep']).sum()) <= FG.ZERO_ROWS_MAX and len(judged['zero']) == 2
    yard = FG.errors(FG.evaluate(w, tabs, gj, torch.float32), judged)
    good = FG.emulate(w, tabs, gj)
    FG.assert_gate({k: (v, yard[k]) for k, v in FG.errors(good, judged).items()}, name)
    assert FG.zero_rows_ok(good, judged, gj)
    for defect, outputs in SEEN_IN.items():
        if defect == 'tail' and not any(d > 64 and d % 64 for d in widths):
            continue
        ke = FG.errors(FG.emulate(w, tabs, gj, defect), judged)
        for k in outputs:
            print(f'{name} {defect} {k}: max {ke[k][0]:.3g} u rms {ke[k][1]:.3g} u | yardstick max {yard[k][0]:.3f} u rms {yard[k][1]:.4f} u')
            assert EG.gate_ok(ke[k], yard[k], FG.R[k]) == ((name, defect, k) in UNSEEN), (name, defect, k, ke[k], yard[k])


def test_every_gate_case_has_a_ragged_tail():
    assert all(any(d > 64 and d % 64 for d in w) for _, _, w in GATE_CASES)


# ------------------------------------------------------------------------------------------------ ELU
def test_elu_bound_catches_expf_minus_one():
    """An ELU written expf(x) - 1 (float32 exp, then the subtraction) sits thousands of ulps out at small |x|; torch's own float32 F.elu is
    inside the bound, and so is its backward."""
    x = FG.elu_strata()
    gy = torch.tensor(FG.ELU_GY)[torch.arange(x.numel()) % 3]
    assert x.numel() == 3011
    ry, rg = FG.elu_reference(x, gy)
    bad = FG.ulp_errors(torch.exp(x) - 1.0, ry)
    at, nxt = torch.nonzero(x == -2.0 ** -20).item(), torch.nonzero(x == -2.0 ** -20 * (1 + 1 / 64)).item()
    print(f'expf(x) - 1: {bad[at].item():.0f} ulp at x = -2^-20, {bad[nxt].item():.0f} ulp at -2^-20 (1 + 1/64), worst {bad.max().item():.3g} ulp')
    # at the power of two itself exp(x) is nearly a float32 number (1 - 2^-20 + 2^-41), so the emulation is only 8 ulp out there; one stratum on, thousands
    assert bad[at] > FG.ULP_CAP and bad[nxt] > 1000 and bad.max() > 1e6
    y, gx = FG.elu_yardstick(x, gy)
    fy, fg = FG.ulp_errors(y, ry).max().item(), FG.ulp_errors(gx, rg).max().item()
    print(f'torch float32 F.elu: forward {fy:.3f} ulp, backward {fg:.3f} ulp')
    assert fy <= FG.ULP_CAP and fg <= FG.ULP_CAP
    assert y[-1] == -1.0 and gx[-1] == 0.0 and math.isinf(x[-1].item())


def test_elementwise_inputs_cover_both_trips():
    x, gy = FG.ew_inputs(FG.EW_SIZES[-1])
    assert FG.EW_SIZES[4] == FG.EW_STRIDE and FG.EW_SIZES[5] == FG.EW_STRIDE + 1
    for part in (x[:FG.EW_STRIDE], x[FG.EW_STRIDE:]):
        assert (part > 0).any() and (part < 0).any() and torch.isinf(part).any()
        zeros = part[part == 0]
        assert torch.signbit(zeros).any() and (~torch.signbit(zeros)).any()
    strata = FG.elu_strata()
    for g in FG.ELU_GY:                                            # every stratum meets every gy in the second trip too
        sel = x[FG.EW_STRIDE:][gy[FG.EW_STRIDE:] == g]
        assert set(strata.tolist()) <= set(sel.tolist())


# ------------------------------------------------------------------------------------------------ argument contract (no launch)
def _buf(nbytes=256):
    b = ctypes.create_string_buffer(nbytes)
    return b, ctypes.cast(b, ctypes.c_void_p)


def _call(l, name, M, T=4, D=4, widths=None, tables='ok', gtables='ok', ws_bytes=None):
    """One call of a fusion entry with host dummies for every pointer: each refusal under test comes before anything touches them."""
    keep = [_buf() for _ in range(6)]
    dummy = [p for _, p in keep]
    n = max(M, 1)
    arr = lambda kind: (ctypes.c_void_p * n)(*[(dummy[0].value if kind == 'ok' else None)] * n)
    embs, gembs = arr(tables), arr(gtables)
    wd = (ctypes.c_int32 * n)(*(widths if widths is not None else [D] * n))
    nb = l.sga_fusion_bwd_workspace_bytes(M) if ws_bytes is None else ws_bytes
    if name == 'sga_fusion_fwd':
        rc = l.sga_fusion_fwd(embs, M, dummy[1], dummy[2], T, D, None)
    elif name == 'sga_fusion_bwd':
        rc = l.sga_fusion_bwd(embs, M, dummy[1], dummy[2], gembs, dummy[3], T, D, dummy[4], nb, None)
    elif name == 'sga_fusion_var_fwd':
        rc = l.sga_fusion_var_fwd(embs, M, wd, dummy[1], dummy[2], T, None)
    else:
        rc = l.sga_fusion_var_bwd(embs, M, wd, dummy[1], dummy[2], gembs, dummy[3], T, dummy[4], nb, None)
    return rc, l.sga_last_error()


ENTRIES = ('sga_fusion_fwd', 'sga_fusion_bwd', 'sga_fusion_var_fwd', 'sga_fusion_var_bwd')


@pytest.mark.parametrize('name', ENTRIES)
def test_fusion_entries_refuse_bad_arguments(name):
    """M = 0, M = 9, a width < 1, a null table with T > 0 and a short workspace are refused under the entry's own name, before any launch."""
    from sgaligner_amd import _lib
    l = _lib.lib()
    own = name.encode() + b':'
    for M in (0, FG.FU_MAXM + 1):
        rc, err = _call(l, name, M)
        assert rc != 0 and err.startswith(own) and b'modal_num' in err, (M, rc, err)
    for M in (1, 3, FG.FU_MAXM):
        if 'var' in name:
            rc, err = _call(l, name, M, widths=[4] * (M - 1) + [0])
            assert rc != 0 and err.startswith(own) and b'width 0 < 1' in err, (rc, err)
            rc, err = _call(l, name, M, widths=[-1] + [4] * (M - 1))
            assert rc != 0 and err.startswith(own) and b'width -1 < 1' in err, (rc, err)
        else:
            for D in (0, -1):
                rc, err = _call(l, name, M, D=D)
                assert rc != 0 and err.startswith(own) and b'bad argument' in err, (D, rc, err)
        rc, err = _call(l, name, M, tables='null')
        assert rc != 0 and err.startswith(own) and b'null table 0' in err, (rc, err)
        if name.endswith('bwd'):
            rc, err = _call(l, name, M, gtables='null')
            assert rc != 0 and err.startswith(own) and b'null table 0' in err, (rc, err)
            for nb in (0, 8 * M - 1):
                rc, err = _call(l, name, M, ws_bytes=nb)
                assert rc != 0 and err.startswith(own) and b'workspace too small' in err, (nb, rc, err)
