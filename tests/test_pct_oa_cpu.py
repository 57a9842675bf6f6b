"""What offset attention can be held to without a card: the fp64 restatement (tests/pct_oa_ref.py) against the reference's recorded run
(tests/golden/pct_oa.npz), the state_dict keys of OA, SPCT and NaivePCT(attention='oa'), the C ABI's new symbols, the register budget of the
new kernels, and the self-tests of tests/pct_oa_gate.py: the lattice builders' conditions, the gate's reference against the restatement, the
table of ratios against the committed profile, the yardstick's own standing, and emulated defects that must FAIL at the ratios in use."""
import os
import sys

import numpy as np
import pytest
import torch

import gemm_gate as G
import pct_gate as PG
import pct_oa_gate as OG
import pct_oa_ref as REF
from conftest import load_golden

sys.path.insert(0, os.path.join(G.ROOT, 'tools'))


def _close(got, ref, tol=2e-6):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), (np.abs(got - ref).max(), np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ golden and restatement
def test_golden_inputs_are_the_seeded_ones():
    g = load_golden('pct_oa')
    x, cot = REF.oa_inputs()
    assert np.array_equal(g['oa_pin'], torch.stack([x[:, ::16], cot[:, ::16]]).numpy())
    x, cx, cmax, cmean = REF.spct_inputs()
    assert np.array_equal(g['spct_x_pin'], x.numpy()) and np.array_equal(g['spct_cx_pin'], cx[:, ::64].numpy())
    assert np.array_equal(g['spct_cpool_pin'], torch.stack([cmax[:, ::16], cmean[:, ::16]]).numpy())
    assert all(v.dtype.kind in 'fiU' for v in g.values()), 'the golden holds numbers and key names only'


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_restatement_of_oa_equals_the_golden(mode):
    """Output, input gradient, every parameter gradient and the updated running statistics (the golden stores float32: 2e-6 of the maximum)."""
    g = load_golden('pct_oa')
    sd, leaves = REF.leaves64(REF.golden_state_dict('oa'))
    x, cot = REF.oa_inputs()
    xi = x.double().transpose(1, 2).clone().requires_grad_()
    up = {}
    y = REF.oa_layer(xi, sd, '', mode == 'train', up)
    (y * cot.double().transpose(1, 2)).sum().backward()
    _close(y.detach().transpose(1, 2).numpy(), g[f'oa_{mode}__y'])
    _close(xi.grad.transpose(1, 2).numpy(), g[f'oa_{mode}__dx'])
    recorded = {k.split('__g__')[1] for k in g if k.startswith(f'oa_{mode}__g__')}
    assert recorded == set(leaves)
    for k, leaf in leaves.items():
        _close(leaf.grad.numpy(), g[f'oa_{mode}__g__{k}'])
    if mode == 'train':
        for k, v in up.items():
            _close(v.numpy(), g['oa_train__after__' + k], 1e-12)


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_restatement_of_spct_equals_the_golden(mode):
    g = load_golden('pct_oa')
    sd, leaves = REF.leaves64(REF.golden_state_dict('spct'))
    x, cx, cmax, cmean = REF.spct_inputs()
    y, ymax, ymean, up = REF.spct(x.double(), sd, mode == 'train')
    ((y * cx.double()).sum() + (ymax * cmax.double()).sum() + (ymean * cmean.double()).sum()).backward()
    _close(y.detach()[:, ::REF.SUB].numpy(), g[f'spct_{mode}__x'])
    _close(ymax.detach().numpy(), g[f'spct_{mode}__max'])
    _close(ymean.detach().numpy(), g[f'spct_{mode}__mean'])
    assert {k.split('__g__')[1] for k in g if k.startswith(f'spct_{mode}__g__')} == set(leaves)
    for k, leaf in leaves.items():
        _close(REF.sub_rows(leaf.grad).numpy(), g[f'spct_{mode}__g__{k}'])
    if mode == 'train':
        assert {k[len('spct_train__after__'):] for k in g if k.startswith('spct_train__after__')} == set(up)
        for k, v in up.items():
            _close(v.numpy(), g['spct_train__after__' + k], 1e-12)


def test_state_dict_keys_match_the_reference():
    from sgaligner_amd.aligner.networks.pct import OA, SPCT, NaivePCT
    g = load_golden('pct_oa')
    assert list(OA(128).state_dict()) == list(g['oa_keys'])
    assert list(SPCT().state_dict()) == list(g['spct_keys'])
    naive = [k[4:] for k in load_golden('pct_eval') if k.startswith('sd__')]
    assert list(NaivePCT(attention='oa').state_dict()) == list(NaivePCT().state_dict()) and set(NaivePCT('oa').state_dict()) == set(naive)
    for cls, kind in ((OA, 'oa'), (SPCT, 'spct'), (NaivePCT, 'naive')):
        m = cls(128) if cls is OA else (cls('oa') if cls is NaivePCT else cls())
        m.load_state_dict(REF.golden_state_dict(kind), strict=True)
    oa = OA(128)
    assert oa.q_conv.weight is oa.k_conv.weight
    with pytest.raises(ValueError):
        NaivePCT(attention='other')


def test_encoder_passes_the_attention_switch_through():
    from sgaligner_amd.aligner.networks.pct import OA, SA
    from sgaligner_amd.aligner.sg_aligner import MultiModalEncoder
    assert isinstance(MultiModalEncoder(['pct', 'rel'], 41, 164).object_encoder.sa1, SA)
    enc = MultiModalEncoder(['pct', 'rel'], 41, 164, pct_attention='oa')
    assert all(isinstance(getattr(enc.object_encoder, n), OA) for n in REF.LAYERS)
    assert list(enc.state_dict()) == list(MultiModalEncoder(['pct', 'rel'], 41, 164).state_dict())


def test_new_symbols_are_exported():
    from sgaligner_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        pytest.skip('library not built')
    L = _lib.lib()
    for name in ('sga_pct_offset_attention', 'sga_pct_offset_attention_bwd', 'sga_segment_mean', 'sga_segment_mean_bwd'):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None


def test_new_kernels_use_no_scratch():
    """tools/kernel_resources.py on csrc/pct.hip: the OA instantiations of the attention kernels, the prep kernel and the point mean compile
    for gfx950 without scratch or spills; the backward's tile loop has no scratch traffic."""
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    _, res = kr.analyse(os.path.join(_build.CSRC, 'pct.hip'))
    want = ('attn_apply_kernelILb0ELb1E', 'attn_apply_kernelILb1ELb1E', 'attn_bwd_dq_kernelILb1E', 'rowdot_kernelILb1E', 'oa_prep_kernel',
            'segment_mean_kernel', 'segment_mean_bwd_kernel')
    for w in want:
        ks = {k: v for k, v in res.items() if w in k}
        assert len(ks) == 1, (w, sorted(res))
        (k, v), = ks.items()
        print(k, v)
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
        assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
        assert v['vgpr'] + v['agpr'] <= 512 and v['lds'] <= 160 * 1024, (k, v)


# ------------------------------------------------------------------------------------------------ the gate's own standing
@pytest.mark.parametrize('N', OG.N_EXACT)
def test_lattice_conditions(N):
    """The builders' assertions (exp(-4096) = 0, column sums exactly 1, 1 + eps = 1 in float32) hold at every listed shape, and the literal fp64
    evaluation gives the group means."""
    q, v, g, x, exact = OG.lattice('groups', 3, N)
    ref = OG.reference(q, v, g, 3, N)
    assert (ref['xr'] - exact['xr']).abs().max() < 1e-8 and (ref['dv'] - exact['dv']).abs().max() < 1e-8      # fp64 keeps the eps float32 drops
    assert torch.equal(x, x.round()) and torch.equal(exact['diff'], exact['diff'].float().double())
    if N & (N - 1) == 0:
        OG.lattice('uniform', 3, N)


def test_gate_reference_is_the_restatement():
    """pct_oa_gate.reference (the formulas with eps = 1e-9f) against pct_oa_ref.offset_attention and its autograd."""
    q, v, g, ref = OG.gate_input('a', 2, 33)
    q64 = q.double().view(2, 33, 32).clone().requires_grad_()
    v64 = v.double().view(2, 33, 128).clone().requires_grad_()
    xr = REF.offset_attention(q64, v64, eps=OG.EPS32)
    (xr * g.double().view(2, 33, 128)).sum().backward()
    for got, want in ((ref['xr'], xr.detach()), (ref['dv'], v64.grad), (ref['dq'], q64.grad)):
        assert torch.allclose(got, want.reshape(got.shape), rtol=1e-13, atol=1e-13)


def test_shadowed_family_sits_below_eps():
    """Family d at every gate N: the shadowed columns' sums lie in [7.5e-10, 3.1e-9] (the builder asserts it), d_j there is between eps and
    4.1 eps, and leaving eps out moves the output by more than 1 on values of size 3."""
    for N in OG.N_GATE:
        q, v, g, ref = OG.gate_input('d', 2, N)
        d = ref['d'].view(2, N)[:, (N + 1) // 2:]
        assert d.min().item() > 1.7e-9 and d.max().item() < 4.2e-9
        moved = (OG.yardstick(q, v, g, 2, N)['xr'] - OG.yardstick(q, v, g, 2, N, defect='no_eps')['xr']).abs().max().item()
        assert moved > 1.0 and ref['xr'].abs().max().item() < 6.0, (N, moved)


def test_gate_ratios_are_the_measured_ones():
    assert OG.R == OG.ratios_from_profile()
    assert set(OG.R) == {c[0] for c in OG.cases()}


def test_yardstick_passes_its_own_gate_in_every_case():
    for family, T, N, layout, outputs in OG.cases():
        if layout != 'plain':
            continue
        q, v, g, ref = OG.gate_input(family[3:], T, N)
        yard = OG.yardstick(q, v, g, T, N)
        for k in outputs:
            e = PG.errors(yard[k], ref[k], ref['env'][k])
            assert G.gate_ok(e, e, OG.R[family][k])


# defect -> (family, outputs that must fail).  eps matters where a column sum is of its size (d); the others show wherever attention is spread (a).
CAUGHT = {'no_eps': ('d', ('xr', 'dv', 'dq')), 'eps_rowsum': ('d', ('xr', 'dv', 'dq')), 'scaled': ('a', ('xr', 'dv', 'dq')),
          'no_kappa': ('a', ('dq',)), 'no_pkappa': ('a', ('dq',)), 'rows_only': ('a', ('xr', 'dv', 'dq'))}


@pytest.mark.parametrize('N', OG.N_GATE)
@pytest.mark.parametrize('defect', OG.DEFECTS)
def test_gate_catches_emulated_defects(defect, N):
    """eps omitted; eps added to the row sum (where float32 cannot see it); SA's 1/sqrt(32) applied; kappa dropped from dP; sum P kappa dropped
    from delta; normalising over rows only -- each FAILS the gate at the r in use, at every gate N."""
    assert set(CAUGHT) == set(OG.DEFECTS)
    family, outs = CAUGHT[defect]
    q, v, g, ref = OG.gate_input(family, 2, N)
    bad, yard = OG.yardstick(q, v, g, 2, N, defect=defect), OG.yardstick(q, v, g, 2, N)
    for k in outs:
        ke, ye = PG.errors(bad[k], ref[k], ref['env'][k]), PG.errors(yard[k], ref[k], ref['env'][k])
        print(f'{defect} {family} N={N} {k}: {ke[:2]} u against the yardstick {ye[:2]} u, r = {OG.R["oa_" + family][k]}')
        assert not G.gate_ok(ke, ye, OG.R['oa_' + family][k]), (k, ke, ye)
