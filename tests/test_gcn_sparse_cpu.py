"""CPU: the sparse GCN route's switches and defaults (MultiGCN, EVA, EVASteps, ops.multi_gcn_layers), MultiGCN's depth and dropout rules, the new C
entry points' argument checks, the new kernels' resource use, and the gate's bookkeeping -- r against the committed profile and against the
dense route's, the ReLU guard at the committed seeds (no GPU launches)."""
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import eva_gate as EG  # noqa: E402
import gcn_sparse_gate as CG  # noqa: E402

BAD_ROUTES = ('csr', '', None, 'Dense')
MODS = ['gcn', 'point', 'rel', 'attr']


def test_route_values():
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.eva import EVA
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    for bad in BAD_ROUTES:
        with pytest.raises(ValueError, match='route'):
            MultiGCN([3, 200, 400], route=bad)
        with pytest.raises(ValueError, match='route'):
            EVA(MODS, 41, 164, gcn_route=bad)
        with pytest.raises(ValueError, match='route'):
            ops.multi_gcn_layers(None, torch.zeros(1, 3), [], route=bad)
        with pytest.raises(ValueError, match='route'):
            ops.gcn_aggregate(torch.zeros(1, 3), None, route=bad)


def test_defaults_are_dense_and_state_dicts_unchanged():
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.eva import EVA
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    from sgaligner_amd.trainer import EVASteps
    for fn, name in ((MultiGCN.__init__, 'route'), (EVA.__init__, 'gcn_route'), (EVASteps.__init__, 'gcn_route'), (ops.multi_gcn_layers, 'route'),
                     (ops.gcn_aggregate, 'route')):
        assert inspect.signature(fn).parameters[name].default == 'dense', fn
    assert list(inspect.signature(EVA.__init__).parameters)[-1] == 'gcn_route'            # last: the reference's positional order stands
    assert MultiGCN().route == 'dense'
    base = EVA(MODS, 41, 164)
    assert base.gcn_route == 'dense' and base.structure_encoder.route == 'dense'
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    for route in ('sparse', 'auto'):
        assert shapes(MultiGCN([3, 200, 400], route=route)) == shapes(MultiGCN([3, 200, 400]))
        other = EVA(MODS, 41, 164, gcn_route=route)
        assert other.gcn_route == route and other.structure_encoder.route == route and shapes(other) == shapes(base)
    gcn_keys = [k for k in base.state_dict() if k.startswith('structure_encoder.')]
    assert gcn_keys == ['structure_encoder.layer_stack.0.bias', 'structure_encoder.layer_stack.0.lin.weight',
                        'structure_encoder.layer_stack.1.bias', 'structure_encoder.layer_stack.1.lin.weight']
    import test_eva_cpu as TE
    assert all({k: tuple(v.shape) for k, v in EVA(MODS, 41, 164, gcn_route=r).state_dict().items()} == TE.EVA_STATE for r in ('dense', 'sparse', 'auto'))


def test_depth_and_dropout():
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    for route in ('dense', 'sparse', 'auto'):
        deep = MultiGCN([3, 64, 64, 32], route=route)
        assert deep.num_layers == 3 and [tuple(l.lin.weight.shape) for l in deep.layer_stack] == [(64, 3), (64, 64), (32, 64)]
        assert [tuple(l.bias.shape) for l in deep.layer_stack] == [(64,), (64,), (32,)]
        assert list(deep.state_dict()) == [f'layer_stack.{i}.{n}' for i in range(3) for n in ('bias', 'lin.weight')]
        one = MultiGCN([17, 300], route=route)
        assert one.num_layers == 1 and tuple(one.layer_stack[0].lin.weight.shape) == (300, 17) and tuple(one.layer_stack[0].bias.shape) == (300,)
    with pytest.raises(ValueError, match='two entries'):
        MultiGCN([3])
    for route in ('dense', 'sparse'):
        with pytest.raises(NotImplementedError, match='dropout'):
            MultiGCN([3, 200, 400], dropout=0.1, route=route)


def test_sparse_entry_points_reject_bad_arguments_without_gpu():
    from sgaligner_amd import _lib
    l = _lib.lib()
    err = lambda: l.sga_last_error()
    one, two = 16, 32                                                    # any non-null addresses: an argument error comes before any device call
    assert l.sga_version() >= 105
    agg = lambda H=one, C=3, bias=None, ptr=one, nbr=one, mult=one, perm=None, dinv=one, T=4, cap=8, relu=0, out=two: \
        l.sga_gcn_sp_aggregate(H, C, bias, ptr, nbr, mult, perm, dinv, T, cap, relu, out, None)
    assert agg(C=0) == 1 and err() == b'sga_gcn_sp_aggregate: width 0 < 1'
    assert agg(C=-5) == 1 and b'width -5 < 1' in err()
    assert agg(T=-1) == 1 and err().startswith(b'sga_gcn_sp_aggregate') and b'negative' in err()
    assert agg(cap=-1) == 1 and b'negative' in err()
    assert agg(cap=2 ** 31 - 64) == 1 and err().startswith(b'sga_gcn_sp_aggregate') and b'2^31 - 64' in err()
    assert agg(T=9, cap=8) == 1 and b'self loops' in err()
    for name in ('H', 'ptr', 'nbr', 'mult', 'dinv', 'out'):
        assert agg(**{name: None}) == 1 and err().startswith(b'sga_gcn_sp_aggregate: null pointer'), name
    assert agg(out=one) == 1 and b'out aliases H' in err()
    assert agg(perm=one, bias=one) == 1 and b'transposed' in err()
    assert agg(perm=one, relu=1) == 1 and b'transposed' in err()
    assert agg(H=None, ptr=None, nbr=None, mult=None, dinv=None, out=None, T=0, cap=0) == 0                 # an empty batch is a no-op
    assert agg(T=0, cap=2 ** 31 - 65) == 0
    dinv = lambda row_ptr=one, mult=one, T=4, cap=8, out=two: l.sga_gcn_sp_dinv(row_ptr, mult, T, cap, out, None)
    assert dinv(T=-1) == 1 and err().startswith(b'sga_gcn_sp_dinv') and b'negative' in err()
    assert dinv(cap=2 ** 31 - 64) == 1 and err().startswith(b'sga_gcn_sp_dinv') and b'2^31 - 64' in err()
    assert dinv(T=9) == 1 and b'self loops' in err()
    for name in ('row_ptr', 'mult', 'out'):
        assert dinv(**{name: None}) == 1 and err() == b'sga_gcn_sp_dinv: null pointer', name
    assert dinv(row_ptr=None, mult=None, out=None, T=0, cap=0) == 0


def test_sparse_gcn_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    base, res = kr.analyse(os.path.join(_build.CSRC, 'gcn_sparse.hip'))
    assert len(res) == 5, sorted(res)
    for tag, count in (('gcn_sp_aggregate_kernel', 4), ('gcn_sp_dinv_kernel', 1)):
        ks = [k for k in res if tag in k]
        assert len(ks) == count, (tag, sorted(res))                       # the aggregation: 1 .. 4 channel slots per lane
        for k in ks:
            v = res[k]
            # (v_readlane inside the entry loop is the broadcast of the coefficient and the neighbour id, not a spilled scalar)
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0 and not v.get('loop_scratch'), (k, v)


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' per output over profiles/gcn_sparse_accuracy_vs_fp32.json, and no
    output is gated looser than twice the dense route's bound for the same output (a condition, not a measurement)."""
    profile = json.load(open(CG.PROFILE))['cases']
    assert CG.ratios_from_profile() == CG.R
    want = set(CG.EVA_OUTPUTS)
    for units in CG.CASES:
        want |= set(CG.outputs_of(units))
    assert set(CG.R) == want == set(CG.DENSE_OUTPUT) == {c['output'] for c in profile}
    assert sum(c['output'] == 'gcn_out' for c in profile) == len(CG.CASES) and sum(c['output'] == 'gcn_gw2' for c in profile) == 1
    assert all(CG.R[k] <= 2 * EG.R[CG.DENSE_OUTPUT[k]] for k in CG.R), (CG.R, EG.R)


@pytest.mark.parametrize('which', range(len(CG.CASES)))
def test_guard_holds_at_the_committed_seeds(which):
    """eva_gate's guard (DELTA = 2^-16; a guarded hidden channel is left out of its own layer's dW / db; at most 5 % of a layer's channels) at
    the committed seed of every case, and that seed is the first from 0 at which it holds.  The deep case cannot meet the 5 % at any seed
    (gcn_sparse_gate's text: 22 of its second hidden layer's 100 channels are guarded at seed 0, 29, 36 at the next two); it leaves out the 5 %
    closest to their edge and compares the rest, so the 5 % holds for what is left out in every case."""
    assert CG.DELTA == 2.0 ** -16 and CG.GUARD_MAX == 0.05 and set(CG.SEEDS) == set(range(len(CG.CASES)))
    ref = CG.case(which)['ref']
    hidden = len(CG.CASES[which]) - 2
    assert len(ref['guarded']) == len(ref['excluded']) == len(ref['masks']) == hidden
    for gd, ex, width in zip(ref['guarded'], ref['excluded'], CG.CASES[which][1:-1]):
        print(f'case {which}: {int(gd.sum())} of {width} channels guarded, {int(ex.sum())} left out')
        assert gd.numel() == width and int(ex.sum()) <= 0.05 * width and not (ex & ~gd).any()
    if which in CG.GUARD_CAPPED:
        assert CG.SEEDS[which] == 0 and not CG.guard_holds(ref['guarded'])
        for seed in (1, 2):
            assert not CG.guard_holds(CG._reference(*CG._inputs(which, seed))['guarded']), seed
    else:
        assert all(torch.equal(gd, ex) for gd, ex in zip(ref['guarded'], ref['excluded']))
        assert CG.find_seed(which) == CG.SEEDS[which]


def test_vectorised_adjacency_is_eva_refs():
    """gcn_sparse_gate.adjacency (np.add.at) against eva_ref.gcn_adjacency's per-edge loop on small graphs, in both dtypes."""
    import eva_ref as ER
    import gat_general_gate as GG
    for n, e in GG.dup_graphs(3, [1, 2, 9, 40]):
        for dtype in (torch.float64, torch.float32):
            assert torch.equal(CG.adjacency(n, e, dtype), ER.gcn_adjacency(n, e, dtype)), (n, dtype)
