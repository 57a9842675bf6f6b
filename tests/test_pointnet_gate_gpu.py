"""PointNet kernels on the card against the fp64 winner-row reference of tests/pointnet_gate.py: bit for bit on integer lattices (both forward
families in every launch form, both backward kernels across the sizes at which their launch geometry changes), and within the measured
multiple of plain fp32's own error on guarded random inputs.  Every forward call and the backward gate first assert, through
sga_pointnet_plan on this card, the launch form they reach (pointnet_gate.FORWARD_FORMS / BACKWARD_FORMS)."""
import pytest
import torch

import pointnet_gate as PG

pytestmark = pytest.mark.gpu


def _cus():
    from sgaligner_amd import _lib
    return int(_lib.lib().sga_device_cus())


# Objects at which the backward launches change: mode 4 runs quadruples of workgroups (one per object up to q = CUs / 4 objects), mode 0 pairs
# (h = CUs / 2); 300: several objects per workgroup on a 256-CU card.
BWD_T = {'1': lambda q, h: 1, 'q-1': lambda q, h: q - 1, 'q': lambda q, h: q, 'q+1': lambda q, h: q + 1,
         'h-1': lambda q, h: h - 1, 'h': lambda q, h: h, 'h+1': lambda q, h: h + 1, '300': lambda q, h: 300}


def _assert_grads_equal(got, ref, what):
    for k in PG.GRADS:
        g = got[k].cpu().double()
        if not torch.equal(g, ref[k]):
            bad = (g != ref[k]).nonzero()
            i = tuple(bad[0].tolist())
            raise AssertionError(f'{what}: {k} differs from the exact reference at {len(bad)} of {g.numel()} entries; first {i}: '
                                 f'got {g[i].item()!r}, want {ref[k][i].item()!r}')


# ------------------------------------------------------------------------------------------------ backward, exact
@pytest.mark.parametrize('mode', [0, 4])
@pytest.mark.parametrize('P', [1, 33])
@pytest.mark.parametrize('objects', list(BWD_T))
def test_pointnet_bwd_exact_narrow_lattice(objects, P, mode):
    """Small integers everywhere (exact zeros of Z1, Z2 and y; the reference's arg-max among dense ties): all six gradients of
    pointnet_bwd_fused_kernel (mode 0) and pointnet_bwd_p3_kernel (mode 4) equal the fp64 reference bit for bit."""
    cus = _cus()
    T = max(1, BWD_T[objects](cus // 4, cus // 2))
    x, ws, ref = PG.lattice('narrow', T, P)
    _assert_grads_equal(PG.run_backward(x, ws, ref, mode), ref, f'narrow T={T} P={P} mode={mode}')


@pytest.mark.parametrize('mode', [0, 4])
@pytest.mark.parametrize('kind', ['wide', 'mirror', 'mirror_g'])
def test_pointnet_bwd_exact_many_bit_lattices(kind, mode):
    """19-bit integers in H1 (wide), in W2 (mirror) or in gy (mirror_g), everything else small: each operand's three bf16 planes carry bits
    that the exact result needs, in the Z2 recomputation, dH1 = dZ2 W2 and gW2 += dZ2^T H1.  T = 66 is what the 2^24 envelope condition
    allows with a second object for the first workgroups of a 256-CU card."""
    x, ws, ref = PG.lattice(kind, 66, 5)
    _assert_grads_equal(PG.run_backward(x, ws, ref, mode), ref, f'{kind} mode={mode}')


@pytest.mark.parametrize('mode', [0, 4])
def test_pointnet_bwd_exact_separate_gradient_buffers(mode):
    """Six gradient buffers that are not adjacent: the library zeroes each on its own, and writes nothing around them."""
    x, ws, ref = PG.lattice('narrow', 5, 33)
    _assert_grads_equal(PG.run_backward(x, ws, ref, mode, separate=True), ref, f'separate buffers mode={mode}')


# ------------------------------------------------------------------------------------------------ backward, gate
@pytest.mark.parametrize('mode', [0, 4])
@pytest.mark.parametrize('big', [False, True])
def test_pointnet_bwd_gate(big, mode):
    """Guarded random inputs: every gradient's envelope-relative error (max and rms, in u) within r x the float32 CPU yardstick's, r per
    output and mode from profiles/pointnet_accuracy_vs_fp32.json."""
    from sgaligner_amd import ops
    T, P = PG.gate_shapes(_cus())[int(big)]
    plan = ops.pointnet_plan('BWD', T, P, 256, mode)
    assert plan.form == PG.BACKWARD_FORMS[mode], plan
    # gate_shapes' first case: one more object than the three-plane kernel has workgroup quadruples, as the plan reports them
    assert PG.gate_shapes(_cus())[0][0] == ops.pointnet_plan('BWD', PG.gate_shapes(_cus())[0][0], P, 256, 4).workgroups // 4 + 1
    res = PG.measure_backward(T, P, mode)
    bad = []
    for k, (ke, ye) in res.items():
        r = PG.R[mode][k]
        print(f'[gate] bwd T={T} P={P} mode={mode} {k}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
        if not PG.gate_ok(ke, ye, r):
            bad.append((k, ke[:2], ye[:2], r))
    assert not bad, f'(output, kernel (max, rms), yardstick (max, rms), r) beyond the gate: {bad}'


# ------------------------------------------------------------------------------------------------ forward
def _forward_cases():
    from sgaligner_amd import ops
    return PG.forward_shapes(ops.POINTNET_SPLIT_MAX_OBJECTS)


def _assert_form(case, C3, T, P, mode, bn):
    """The call ops.pointnet_forward is about to make reaches, on this card, the launch form the case is named for."""
    plan = PG.planned_forward(C3, T, P, mode, bn)
    assert (plan.form, plan.ws_use) == PG.FORWARD_FORMS[case, mode][C3], f'{case} C3={C3} T={T} P={P} mode={mode} bn={bn}: {plan}'
    assert (plan.bn_bytes > 0) == bn


@pytest.mark.parametrize('form', [0, 1, 2, 3])
@pytest.mark.parametrize('C3', [64, 128, 256])
def test_pointnet_fwd_exact_narrow_lattice(C3, form):
    """Both forward families (mode 0, mode 4), with and without arg-max, with and without the fused BatchNorm sums, in every launch form (the
    cases of pointnet_gate.forward_shapes; each call is first asserted to reach the form its case is named for): y equals the fp64 reference
    bit for bit, EVERY returned index is a maximiser of the reference's Z3 (ties are dense here), and the BatchNorm sums are the reference's
    integers."""
    case, T, P = _forward_cases()[form]
    x, ws, ref = PG.lattice('narrow', T, P, C3, backward=False, keep_z3=True)
    z3 = ref['z3']
    assert ((z3 == z3.amax(1, keepdim=True)).sum(1) > 1).float().mean() > 0.1 and (ref['y'] == 0).any()        # ties and exact zeros are there
    for mode in (0, 4):
        for want_am in (True, False):
            for bn in (False, True):
                what = f'C3={C3} T={T} mode={mode} argmax={want_am} bn={bn}'
                _assert_form(case, C3, T, P, mode, bn)
                y, am, sums = PG.run_forward(x, ws, mode, want_am, bn)
                assert torch.equal(y.cpu().double(), ref['y']), what
                if want_am:
                    am = am.cpu().long()
                    assert am.min() >= 0 and am.max() < P, what
                    at = torch.gather(z3, 1, am[:, None, :])[:, 0, :].clamp_min(0)
                    wrong = (at != ref['y']).nonzero()
                    assert len(wrong) == 0, f'{what}: {len(wrong)} indices are no maximisers, first (t, c) = {wrong[0].tolist()}'
                if bn:
                    s = sums.cpu()
                    wrong = (s != ref['bn']).nonzero()
                    assert len(wrong) == 0, f'{what}: BatchNorm sums differ at {wrong[:8].flatten().tolist()}'


@pytest.mark.parametrize('form', [0, 1, 2, 3])
@pytest.mark.parametrize('C3', [64, 128, 256])
def test_pointnet_fwd_gate(C3, form):
    """Random inputs: y against e3 at the reference's arg-max point, within r x the float32 CPU yardstick's error, both modes, every launch form."""
    case, T, P = _forward_cases()[form]
    for mode in (0, 4):
        for want_am, bn in ((True, False), (False, True)):
            _assert_form(case, C3, T, P, mode, bn)
            ke, ye = PG.measure_forward(C3, T, P, mode, want_am, bn)
            r = PG.R[mode]['y']
            print(f'[gate] fwd C3={C3} T={T} P={P} mode={mode}: kernel max {ke[0]:.3f} u rms {ke[1]:.4f} u | yardstick max {ye[0]:.3f} u rms {ye[1]:.4f} u | r = {r}')
            assert PG.gate_ok(ke, ye, r), f'C3={C3} T={T} mode={mode}: kernel (max, rms) = {ke[:2]} u against yardstick {ye[:2]} u exceeds r = {r}'
