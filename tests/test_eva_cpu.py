"""CPU: the EVA baseline's reference restatement against the reference's recorded results and a hand-evaluated case, the module / state-dict /
drop-in contract, the new C entry points' argument checks, the new kernels' resource use, and the gate's bookkeeping (no GPU launches)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import eva_gate as EG  # noqa: E402
import eva_ref as ER  # noqa: E402
import gcn_handcase as HC  # noqa: E402

EVA_STATE = {
    'meta_embedding_rel.weight': (100, 41), 'meta_embedding_rel.bias': (100,),
    'meta_embedding_attr.weight': (100, 164), 'meta_embedding_attr.bias': (100,),
    'object_encoder.conv1.weight': (64, 3, 1), 'object_encoder.conv1.bias': (64,),
    'object_encoder.conv2.weight': (128, 64, 1), 'object_encoder.conv2.bias': (128,),
    'object_encoder.conv3.weight': (200, 128, 1), 'object_encoder.conv3.bias': (200,),
    'object_encoder.bn1.weight': (64,), 'object_encoder.bn1.bias': (64,), 'object_encoder.bn1.running_mean': (64,),
    'object_encoder.bn1.running_var': (64,), 'object_encoder.bn1.num_batches_tracked': (),
    'object_encoder.bn2.weight': (128,), 'object_encoder.bn2.bias': (128,), 'object_encoder.bn2.running_mean': (128,),
    'object_encoder.bn2.running_var': (128,), 'object_encoder.bn2.num_batches_tracked': (),
    'object_encoder.bn3.weight': (200,), 'object_encoder.bn3.bias': (200,), 'object_encoder.bn3.running_mean': (200,),
    'object_encoder.bn3.running_var': (200,), 'object_encoder.bn3.num_batches_tracked': (),
    'structure_encoder.layer_stack.0.lin.weight': (200, 3), 'structure_encoder.layer_stack.0.bias': (200,),
    'structure_encoder.layer_stack.1.lin.weight': (400, 200), 'structure_encoder.layer_stack.1.bias': (400,),
    'fusion.weight': (4, 1),
}


def test_reference_nca_equals_the_recorded_reference():
    """eva_ref's NCALoss / OverallNCALoss against the reference's own fp64 results (tools/make_eva_golden.py): values and gradients to 1e-12."""
    g = load_golden('nca_cases')
    for name in g['names']:
        z1 = torch.from_numpy(g[f'{name}__z1']).requires_grad_(True)
        z2 = torch.from_numpy(g[f'{name}__z2']).requires_grad_(True)
        a, b, ep = [float(v) for v in g[f'{name}__abe']]
        loss = ER.nca_loss(z1, z2, a, b, ep)
        loss.backward()
        assert abs(float(loss.detach()) - float(g[f'{name}__loss'])) <= 1e-12 * max(1.0, abs(float(g[f'{name}__loss']))), name
        for got, key in ((z1.grad, 'g1'), (z2.grad, 'g2')):
            assert (got - torch.from_numpy(g[f'{name}__{key}'])).abs().max().item() <= 1e-12, (name, key)
    tabs = {str(k): torch.from_numpy(g[f'ov__tab__{k}']).requires_grad_(True) for k in g['ov__keys']}
    losses = ER.overall_nca(tabs, {'e1i': g['ov__e1i'], 'e2i': g['ov__e2i']})
    losses['loss'].backward()
    for k in list(tabs) + ['loss']:
        assert abs(float(losses[k].detach()) - float(g[f'ov__loss__{k}'])) <= 1e-12 * abs(float(g[f'ov__loss__{k}'])), k
    for k, t in tabs.items():
        assert (t.grad - torch.from_numpy(g[f'ov__grad__{k}'])).abs().max().item() <= 1e-12, k


def test_reference_gcn_equals_the_hand_case():
    adj = ER.gcn_adjacency(HC.N, HC.EDGES)
    assert torch.equal(adj, torch.from_numpy(HC.ADJ))
    h = torch.from_numpy(HC.H)
    # gcn_conv with the identity as weight: the aggregation itself
    assert torch.equal(ER.gcn_conv(h, torch.eye(2, dtype=torch.float64), torch.from_numpy(HC.BIAS), adj), torch.from_numpy(HC.OUT))
    assert torch.equal(adj.t() @ torch.from_numpy(HC.G), torch.from_numpy(HC.DH))
    assert torch.equal(ER.gcn_adjacency(HC.N, HC.EDGES, torch.float32).double(), adj)         # powers of two: exact in float32 too


def test_eva_state_dict_contract():
    from sgaligner_amd.aligner.eva import EVA
    model = EVA(modules=['gcn', 'point', 'rel', 'attr'], rel_dim=41, attr_dim=164)
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == EVA_STATE
    gen = torch.Generator().manual_seed(3)
    new = {k: (torch.randn(s, generator=gen) if s else torch.tensor(7)) for k, s in EVA_STATE.items()}
    model.load_state_dict(new, strict=True)
    assert torch.equal(model.structure_encoder.layer_stack[1].lin.weight, new['structure_encoder.layer_stack.1.lin.weight'])
    # PyG's init: glorot weights, zero bias
    fresh = EVA(modules=['gcn'], rel_dim=41, attr_dim=164).structure_encoder.layer_stack[1]
    assert float(fresh.bias.detach().abs().max()) == 0.0 and float(fresh.lin.weight.detach().abs().max()) <= (6.0 / 600) ** 0.5
    assert abs(float(fresh.lin.weight.detach().std()) - (2.0 / 600) ** 0.5) < 0.002
    from sgaligner_amd.aligner.networks.gat import MultiGCN
    with pytest.raises(NotImplementedError, match='dropout'):
        MultiGCN(n_units=[3, 200, 400], dropout=0.1)


SCRIPT = r'''
import sys
sys.path.append('.')                                      # trainval_eva.py:6-7 (cwd = <ref>/src)
sys.path.insert(0, SGA_DIR)                               # INTEGRATION.md 1: the one edit a maintainer makes
from aligner.eva import *                                 # trainval_eva.py:11
from aligner.losses import OverallNCALoss                 # :12
import aligner.eva, aligner.losses
import sgaligner_amd.aligner.eva as canon
import sgaligner_amd.aligner.losses as canon_l
assert aligner.eva is canon and aligner.losses is canon_l
assert EVA is canon.EVA and OverallNCALoss is canon_l.OverallNCALoss and MultiGCN is canon.MultiGCN
assert F is torch.nn.functional and nn is torch.nn
# ---- trainval_eva.py:36-45 -------------------------------------------------------------------------------------
modules = ['gcn', 'point', 'rel', 'attr']
device = torch.device('cpu')                              # construction only: forward needs the MI355X
model = EVA(modules=modules, rel_dim=41, attr_dim=164).to(device)
loss_func = OverallNCALoss(modules=modules, device=device)
params = [{'params': list(model.parameters())}]
opt = torch.optim.Adam(params, lr=1e-3, weight_decay=0.0)
assert 'structure_encoder.layer_stack.0.lin.weight' in model.state_dict()
try:
    model({'tot_obj_pts': torch.zeros(2, 8, 3)})
    raise SystemExit('CPU tensors must raise')
except RuntimeError as e:
    assert 'no CPU path' in str(e)
try:
    loss_func({'gcn': torch.zeros(4, 8)}, {'e1i': [0], 'e2i': [1]})
    raise SystemExit('CPU tables must raise')
except RuntimeError as e:
    assert 'no CPU path' in str(e)
print('EVA-DROPIN-OK')
'''


def test_eva_dropin_in_a_fresh_interpreter(tmp_path):
    ref = tmp_path / 'ref'
    (ref / 'src').mkdir(parents=True)
    script = tmp_path / 'run.py'
    script.write_text(f'SGA_DIR = {os.path.join(ROOT, "sgaligner_amd")!r}\n' + textwrap.dedent(SCRIPT))
    env = dict(os.environ)
    env['PYTHONPATH'] = str(ref)
    r = subprocess.run([sys.executable, str(script)], cwd=str(ref / 'src'), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'EVA-DROPIN-OK' in r.stdout, r.stdout + r.stderr


def test_sharded_data_dict_raises():
    from sgaligner_amd.aligner.losses import OverallNCALoss
    with pytest.raises(RuntimeError, match='_sga_shard'):
        OverallNCALoss(['gcn'], 'cpu')({'gcn': torch.zeros(4, 8)}, {'e1i': [0], 'e2i': [1], '_sga_shard': (0, 1)})


def test_new_entry_points_reject_bad_arguments_without_gpu():
    import ctypes
    from sgaligner_amd import _lib
    l = _lib.lib()
    assert l.sga_version() >= 101
    w4 = (ctypes.c_int32 * 4)(400, 200, 100, 100)
    w0 = (ctypes.c_int32 * 4)(400, 0, 100, 100)
    for m in (0, 9):
        assert l.sga_fusion_var_fwd(None, m, w4, None, None, 4, None) != 0 and b'modal_num' in l.sga_last_error()
        assert l.sga_fusion_var_bwd(None, m, w4, None, None, None, None, 4, None, 0, None) != 0 and b'modal_num' in l.sga_last_error()
    assert l.sga_fusion_var_fwd(None, 4, w0, None, None, 4, None) != 0 and b'width 0 < 1' in l.sga_last_error()
    assert l.sga_fusion_var_bwd(None, 4, w0, None, None, None, None, 4, None, 0, None) != 0 and b'width 0 < 1' in l.sga_last_error()
    assert l.sga_gcn_aggregate(None, 200, None, None, None, None, 1, 257, 0, 0, None, None, None) != 0
    assert b'at most 256 per graph' in l.sga_last_error()
    assert l.sga_gcn_aggregate(None, 0, None, None, None, None, 1, 8, 0, 0, None, None, None) != 0 and b'width 0 < 1' in l.sga_last_error()
    # the NCA path pads its rows through sga_loss_gather's Dp, which must be a multiple of 8
    assert l.sga_loss_gather(None, 1, 100, None, 2, None, 100, None, None) != 0 and b'multiple of 8' in l.sga_last_error()
    # a row block outside the anchors, a leading dimension shorter than a row
    assert l.sga_nca_block_sums(None, 8, 4, 8, 6, 1.0, 0.0, None, None, None, None) != 0 and b'outside the 8 anchors' in l.sga_last_error()
    assert l.sga_nca_coef(None, 4, None, 4, None, 4, 4, 8, 0, 1.0, 1.0, 0.0, None, None, None, None) != 0 and b'leading dimension' in l.sga_last_error()
    assert l.sga_nca_loss(None, None, 0, None, 8, 1.0, 1.0, None, None, None, None, None) != 0 and b'row groups' in l.sga_last_error()


def test_new_kernels_use_no_scratch():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    want = {'gcn.hip': ['gcn_aggregate_kernel', 'relu_bwd_kernel'],
            'nca.hip': ['nca_row_kernel', 'nca_col_kernel', 'nca_fold_kernel', 'nca_loss_kernel', 'nca_coef_kernel']}
    for f, names in want.items():
        base, res = kr.analyse(os.path.join(_build.CSRC, f))
        for n in names:
            assert any(n in k for k in res), (f, n, sorted(res))
        for k, v in res.items():
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' of profiles/eva_accuracy_vs_fp32.json, per output."""
    assert EG.ratios_from_profile() == EG.R
    assert set(EG.R) == set(EG.GCN_OUTPUTS) | set(EG.NCA_OUTPUTS) | set(EG.TABLE_OUTPUTS)


@pytest.mark.parametrize('seed', [0, 1])
def test_gcn_guard_condition_holds_for_the_gate_inputs(seed):
    """At most 5 % of the 200 hidden channels have a layer-0 pre-activation within 2^-16 of its envelope (computed from eva_ref alone)."""
    x, graphs, ws, g, ref = EG.gcn_input(seed)
    assert [n for n, _ in graphs] == list(EG.GCN_SIZES) and all(len(e) == (4 * n if n > 1 else 0) for n, e in graphs)
    e = np.concatenate([e for _, e in graphs])
    assert (e[:, 0] == e[:, 1]).any()                                         # self loops are in
    big = graphs[2][1]
    assert len(np.unique(big, axis=0)) < len(big)                             # and duplicates
    assert ref['guarded'].shape == (200,)
    assert ref['guarded'].float().mean().item() <= EG.GUARD_MAX, int(ref['guarded'].sum())
    # the float32 yardstick passes its own gate trivially and is not exact: the metric measures something
    ye = EG.gcn_errors(EG.gcn_yardstick(x, graphs, ws, g, ref), ref)
    assert all(0 < ye[k][1] < 1 for k in EG.GCN_OUTPUTS), ye


def test_small_stash_cuts_three_ragged_blocks():
    from sgaligner_amd import nca_ops, ops
    keep = ops.STASH_BYTES
    try:
        for A, _ in EG.NCA_SHAPES:
            if A < 3:
                continue
            ops.STASH_BYTES = EG.small_stash(A)
            b = nca_ops._row_blocks(A)
            assert len(b) >= 3 and b[0][0] == 0 and b[-1][1] == A and all(x[1] == y[0] for x, y in zip(b, b[1:])), (A, b)
            assert b[-1][1] - b[-1][0] < b[0][1] - b[0][0], (A, b)
        ops.STASH_BYTES = 1 << 30
        assert nca_ops._row_blocks(257) == [(0, 257)]
    finally:
        ops.STASH_BYTES = keep
