"""CPU: MultiGAT of any shape -- construction, PyG's state-dict names and shapes, strict loading of the oracle's parameters --, the new C
entry points' argument checks, the new kernels' resource use, and the gate's bookkeeping (no GPU launches)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gat_general_gate as GG  # noqa: E402


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_default_multigat_constructs_with_pyg_shapes():
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    m = MultiGAT()
    s = _shapes(m)
    assert s['layer_stack.0.lin_src.weight'] == (256, 17) and s['layer_stack.0.att_src'] == (1, 2, 128)
    assert s['layer_stack.1.lin_src.weight'] == (200, 256) and s['layer_stack.1.att_src'] == (1, 2, 100) and s['layer_stack.1.bias'] == (200,)
    assert set(s) == {f'layer_stack.{i}.{k}' for i in (0, 1) for k in ('lin_src.weight', 'lin_dst.weight', 'att_src', 'att_dst', 'bias')}
    for l in m.layer_stack:
        assert l.lin_src is l.lin_dst and l.lin_src.weight is l.lin_dst.weight


def test_deep_stack_with_dropout_loads_the_oracle_parameters():
    from oracle import sga_oracle as O
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    units, heads = [3, 48, 100, 32], [3, 1, 8]
    m = MultiGAT(units, heads, dropout=0.3)
    assert m.dropout == 0.3 and m.num_layers == 3
    pre = 'structure_encoder.'
    p = {k[len(pre):]: v for k, v in O.init_params(['point', 'gat'], hidden_units=units, heads=heads).items() if k.startswith(pre)}
    assert _shapes(m) == {k: tuple(v.shape) for k, v in p.items()}
    m.load_state_dict(p, strict=True)
    assert torch.equal(m.layer_stack[2].att_dst, p['layer_stack.2.att_dst']) and tuple(m.layer_stack[2].lin_src.weight.shape) == (256, 100)
    with pytest.raises(NotImplementedError, match='256'):
        MultiGAT([3, 300, 128], [1, 2])
    with pytest.raises(ValueError, match='n_heads'):
        MultiGAT([3, 128, 128], [2])


def test_canonical_state_dict_is_unchanged():
    from oracle import sga_oracle as O
    from sgaligner_amd.aligner.sg_aligner import MultiModalEncoder
    enc = MultiModalEncoder(['point', 'gat', 'rel'], rel_dim=41, attr_dim=164)
    want = {k: tuple(v.shape) for k, v in O.init_params(['point', 'gat', 'rel']).items()}
    got = {k: s for k, s in _shapes(enc).items() if 'num_batches_tracked' not in k}
    assert got == want
    assert got['structure_encoder.layer_stack.0.lin_src.weight'] == (256, 3) and got['structure_encoder.layer_stack.1.att_dst'] == (1, 2, 128)
    # hidden_units / heads / dropout reach the structure encoder; structure_embedding stays the reference's Linear(256, emb_dim)
    enc = MultiModalEncoder(['point', 'gat'], 41, 164, hidden_units=[3, 64, 96, 64], heads=[4, 2, 4], dropout=0.25)
    assert enc.structure_encoder.dropout == 0.25
    assert tuple(enc.structure_encoder.layer_stack[2].lin_src.weight.shape) == (256, 192) and enc.structure_embedding.in_features == 256


def test_general_entry_points_reject_bad_arguments_without_gpu():
    from sgaligner_amd import _lib
    l = _lib.lib()
    for heads, channels, word in ((2, 257, b'channels'), (2, 0, b'channels'), (0, 128, b'heads')):
        assert l.sga_gat_attn_fwd_hc(None, heads, channels, None, None, None, None, None, None, 1, 8, None, None, None, None) != 0
        assert word in l.sga_last_error()
        assert l.sga_gat_attn_bwd_hc(None, None, heads, channels, None, None, None, None, None, 1, 8, None, None, None, None, None) != 0
        assert word in l.sga_last_error()
    assert l.sga_gat_attn_fwd_hc(None, 2, 100, None, None, None, None, None, None, 1, 257, None, None, None, None) != 0
    assert b'at most 256' in l.sga_last_error()
    assert l.sga_gat_lds_nodes(257, 0) < 0 and b'channels' in l.sga_last_error()
    # the residency boundary: never above the node limit, never larger backward (two copies) than forward, and no larger for wider heads
    prev = (256, 256)
    for c in (1, 32, 64, 65, 100, 128, 129, 192, 200, 256):
        f, b = l.sga_gat_lds_nodes(c, 0), l.sga_gat_lds_nodes(c, 1)
        assert 1 <= b <= f <= 256 and f <= prev[0] and b <= prev[1], (c, f, b)
        prev = (f, b)
    assert l.sga_gat_lds_nodes(1, 1) == 256 and l.sga_gat_lds_nodes(256, 1) < 128 < l.sga_gat_lds_nodes(256, 0) < 256


def test_general_gat_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    base, res = kr.analyse(os.path.join(_build.CSRC, 'gat.hip'))
    names = kr.demangle(list(res))
    # general kernels: NJ in {2, 4} x CJ in 1 .. 4 x LDSF; the kernels the entry points launch at 2 x 128: <NJ, LDSF> = <2, true> and <4, false>
    for tag, count in (('gat_attn_fwd_hc_kernel', 16), ('gat_attn_bwd_hc_kernel', 16), ('gat_attn_fwd_kernel', 2), ('gat_attn_bwd_kernel', 2)):
        ks = [k for k in res if tag in k]
        assert len(ks) == count, (tag, sorted(res))
        if count == 2:
            assert sorted(names[k] for k in ks) == [tag + '<2, true>', tag + '<4, false>'], sorted(names.values())
        for k in ks:
            v = res[k]
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
            assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' of profiles/gat_general_accuracy_vs_fp32.json, per output kind."""
    assert GG.ratios_from_profile() == GG.R
    assert set(GG.R) == set(GG.OUTPUTS)


def test_guard_holds_at_the_frozen_seeds():
    """Every pre-activation on a counted edge is clear of LeakyReLU's kink at the committed seed, and that seed is the first that is."""
    for heads, channels in ((1, 1), (3, 100)):
        assert GG.find_kernel_seed(heads, channels) == GG.SEEDS[('kernel', heads, channels)]
    assert GG.find_canon_seed(4) == GG.SEEDS[('canon', 4)]
    assert GG.find_stack_seed(1, False) == GG.SEEDS[('stack', 1, False)] and GG.find_stack_seed(GG.MASKED_STACK, True) == GG.SEEDS[('stack', 0, True)]
