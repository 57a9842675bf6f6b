"""CPU: the sparse GAT route's structure restatement against the oracle's edge rules, the new C entry points' argument checks, the route
switch of the Python layer and its defaults, the new kernels' resource use, and the gate's bookkeeping (no GPU launches)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gat_csr_ref as CSR  # noqa: E402
import gat_general_gate as GG  # noqa: E402
import gat_handcase as HC  # noqa: E402
import gat_sparse_gate as SG  # noqa: E402
from oracle import sga_oracle as O  # noqa: E402


def _all_graphs():
    gen = torch.Generator().manual_seed(0)
    return [(3, HC.EDGES, False)] + SG.mix_graphs('dense', gen)          # dense = light + two graphs


def test_restatement_is_the_oracles_edge_multiset():
    graphs = _all_graphs()
    assert [g[0] for g in graphs[1:14]] == [1, 2, 3, 64, 65, 0, 7, 40, 257, 700, 1025, 601, 130] and [g[0] for g in graphs[14:]] == [257, 300]
    for n, e, _ in graphs:
        c = CSR.csr([(n, e)])
        ok = (e >= 0).all(1) & (e < n).all(1)
        src, dst = O._canon_edges(GG._ei(e[ok]), n) if n else (torch.zeros(0, dtype=torch.int64),) * 2
        want = np.stack([src.numpy(), dst.numpy()], 1).reshape(-1, 2)
        want = want[np.lexsort((want[:, 0], want[:, 1]))]
        assert np.array_equal(CSR.expand(c), want), n
        assert c['U'] <= len(e) + n and (c['mult'] >= 1).all()
    # the hand case: node 1 hears 0 twice, 2 once and itself; node 0 hears 1 and itself; node 2 only itself
    c = CSR.csr([(3, HC.EDGES)])
    assert c['row_ptr'].tolist() == [0, 2, 5, 6] and c['src'].tolist() == [0, 1, 0, 1, 2, 2] and c['mult'].tolist() == [1, 1, 2, 1, 1, 1]
    # the 300-fold pair keeps its count, the double star its two long segments
    mix = graphs[1:14]
    c = CSR.csr([mix[SG.FOLD_AT]])
    j, i = SG.FOLD_PAIR
    seg = slice(c['row_ptr'][i], c['row_ptr'][i + 1])
    assert c['mult'][seg][c['src'][seg] == j][0] >= SG.FOLD_COPIES
    c = CSR.csr([mix[SG.STAR_AT]])
    assert np.diff(c['row_ptr'])[0] == SG.STAR == np.diff(c['col_ptr'])[0] and (np.diff(c['row_ptr'])[1:] == 2).all()


def test_transpose_restatement_is_a_sorted_permutation():
    graphs = _all_graphs()
    c = CSR.csr(graphs)                                                   # one batch: global ids
    U, T = c['U'], c['T']
    assert T == sum(g[0] for g in graphs) and c['row_ptr'][-1] == U == c['col_ptr'][-1]
    assert np.array_equal(np.sort(c['perm']), np.arange(U))
    tgt_of_entry = np.repeat(np.arange(T), np.diff(c['row_ptr']))
    src_t = np.repeat(np.arange(T), np.diff(c['col_ptr']))
    assert np.array_equal(tgt_of_entry[c['perm']], c['tgt']) and np.array_equal(c['src'][c['perm']], src_t)
    key_r, key_c = tgt_of_entry * (T + 1) + c['src'], src_t * (T + 1) + c['tgt']
    assert (np.diff(key_r) > 0).all() and (np.diff(key_c) > 0).all()      # strictly ascending: sorted, no pair twice


def test_sparse_entry_points_reject_bad_arguments_without_gpu():
    from sgaligner_amd import _lib
    l = _lib.lib()
    err = lambda: l.sga_last_error()
    one = 16                                                             # any non-null address: an argument error comes before any device call
    assert l.sga_gat_sp_capacity(-1, 0) < 0 and b'sga_gat_sp_capacity' in err()
    assert l.sga_gat_sp_capacity(2 ** 30, 2 ** 30) < 0 and b'2^31' in err()
    assert l.sga_gat_sp_capacity(5, 7) == 12 and l.sga_gat_sp_capacity(0, 0) == 0
    assert l.sga_gat_sp_capacity(2 ** 31 - 65, 0) == 2 ** 31 - 65 and l.sga_gat_sp_capacity(2 ** 31 - 65, 1) < 0      # chunks of 64 stay inside int
    assert l.sga_gat_sp_heads(one, 2 ** 31 - 64, one, None) == 1 and b'2^31 - 64' in err()
    assert l.sga_gat_sp_bwd(one, one, 2, 100, one, one, one, one, one, one, one, one, 4, 2 ** 31 - 64, one, one, one, one, 1 << 20, None) == 1
    assert b'capacity' in err()
    assert l.sga_gat_sp_fwd(one, 65537, 1, one, one, one, one, one, one, 4, one, one, 1 << 30, None) == 1 and b'heads' in err()
    assert l.sga_gat_sp_bwd(None, None, 65537, 256, None, None, None, None, None, None, None, None, 0, 0, one, one, one, None, 0, None) == 1
    assert b'heads' in err()                                             # heads * channels stays inside int, also for the empty batch's zeroing
    assert l.sga_gat_sp_build_workspace_bytes(12) == 13 * 4
    for heads, channels, word in ((2, 257, b'channels'), (2, 0, b'channels'), (0, 128, b'heads')):
        assert l.sga_gat_sp_workspace_bytes(4, 8, heads, channels, 1) == 0 and word in err() and b'sga_gat_sp_workspace_bytes' in err()
        assert l.sga_gat_sp_fwd(one, heads, channels, one, one, one, one, one, one, 4, one, one, 1 << 20, None) == 1
        assert word in err() and err().startswith(b'sga_gat_sp_fwd')
        assert l.sga_gat_sp_bwd(one, one, heads, channels, one, one, one, one, one, one, one, one, 4, 8, one, one, one, one, 1 << 20, None) == 1
        assert word in err() and err().startswith(b'sga_gat_sp_bwd')
    assert l.sga_gat_sp_workspace_bytes(4, 9, 2, 100, 0) == 2 * 4 * 2 * 4
    assert l.sga_gat_sp_workspace_bytes(4, 9, 2, 100, 1) == (4 * 4 * 2 + 2 * 2 * 9 + 1 * 2 * 200) * 4
    assert l.sga_gat_sp_workspace_bytes(0, 0, 2, 100, 1) == 0
    # the d att fold tree: 256 nodes per partial, 64 partials per group and level -- 20000 nodes: 79 + 2 + 1 partial slots
    assert l.sga_gat_sp_workspace_bytes(20000, 20000, 1, 3, 1) == (4 * 20000 + 2 * 20000 + 82 * 2 * 3) * 4
    # negative sizes
    assert l.sga_gat_sp_keys(one, one, one, 1, -1, 0, one, None) == 1 and err().startswith(b'sga_gat_sp_keys') and b'negative' in err()
    assert l.sga_gat_sp_heads(one, -1, one, None) == 1 and err().startswith(b'sga_gat_sp_heads')
    assert l.sga_gat_sp_rows(one, one, -1, 0, one, one, one, one, one, 64, None) == 1 and err().startswith(b'sga_gat_sp_rows')
    assert l.sga_gat_sp_cols(one, one, 4, -1, one, one, one, None) == 1 and err().startswith(b'sga_gat_sp_cols')
    assert l.sga_gat_sp_fwd(one, 2, 100, one, one, one, one, one, one, -1, one, one, 1 << 20, None) == 1 and b'negative' in err()
    assert l.sga_gat_sp_bwd(one, one, 2, 100, one, one, one, one, one, one, one, one, 4, -1, one, one, one, one, 1 << 20, None) == 1 and b'negative' in err()
    assert l.sga_gat_sp_rows(one, one, 3, 4, one, one, one, one, one, 64, None) == 1 and b'self loops' in err()
    # null pointers
    assert l.sga_gat_sp_keys(None, one, one, 1, 2, 3, one, None) == 1 and b'sga_gat_sp_keys: null' in err()
    assert l.sga_gat_sp_keys(one, one, one, 1, 2, 3, None, None) == 1 and b'null' in err()
    assert l.sga_gat_sp_heads(None, 4, one, None) == 1 and b'sga_gat_sp_heads: null' in err()
    assert l.sga_gat_sp_rows(one, one, 4, 2, None, one, one, one, one, 64, None) == 1 and b'sga_gat_sp_rows: null' in err()
    assert l.sga_gat_sp_rows(one, one, 4, 2, one, one, None, one, one, 64, None) == 1 and b'null' in err()
    assert l.sga_gat_sp_cols(one, None, 4, 2, one, one, one, None) == 1 and b'sga_gat_sp_cols: null' in err()
    assert l.sga_gat_sp_fwd(None, 2, 100, one, one, one, one, one, one, 4, one, one, 1 << 20, None) == 1 and b'sga_gat_sp_fwd: null' in err()
    assert l.sga_gat_sp_bwd(one, one, 2, 100, one, one, one, one, one, one, one, None, 4, 8, one, one, one, one, 1 << 20, None) == 1
    assert b'sga_gat_sp_bwd: null' in err()
    assert l.sga_gat_sp_bwd(None, None, 2, 100, None, None, None, None, None, None, None, None, 0, 0, None, None, one, None, 0, None) == 1
    assert b'null' in err()                                              # d att_* are written (zeroed) even for an empty batch
    # a workspace that is too small
    assert l.sga_gat_sp_rows(one, one, 4, 2, one, one, one, one, one, 19, None) == 3 and b'sga_gat_sp_rows: workspace' in err()
    need = l.sga_gat_sp_workspace_bytes(4, 9, 2, 100, 0)
    assert l.sga_gat_sp_fwd(one, 2, 100, one, one, one, one, one, one, 4, one, one, need - 1, None) == 3 and b'sga_gat_sp_fwd: workspace' in err()
    need = l.sga_gat_sp_workspace_bytes(4, 9, 2, 100, 1)
    assert l.sga_gat_sp_bwd(one, one, 2, 100, one, one, one, one, one, one, one, one, 4, 9, one, one, one, one, need - 1, None) == 3
    assert b'sga_gat_sp_bwd: workspace' in err()
    # empty batches are no-ops
    assert l.sga_gat_sp_keys(None, None, None, 0, 0, 0, None, None) == 0 and l.sga_gat_sp_heads(None, 0, None, None) == 0
    assert l.sga_gat_sp_fwd(None, 2, 100, None, None, None, None, None, None, 0, None, None, 0, None) == 0


def test_route_values():
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    from sgaligner_amd.aligner.sg_aligner import MultiModalEncoder
    for bad in ('csr', '', None, 'Dense'):
        with pytest.raises(ValueError, match='route'):
            ops.resolve_route(bad)
        with pytest.raises(ValueError, match='route'):
            MultiGAT(route=bad)
        with pytest.raises(ValueError, match='route'):
            MultiModalEncoder(['point', 'gat'], 41, 164, gat_route=bad)
        with pytest.raises(ValueError, match='route'):
            ops.multi_gat_layers(None, torch.zeros(1, 3), [], route=bad)
    assert [ops.resolve_route(r) for r in ('dense', 'sparse', 'auto')] == ['dense', 'sparse', 'dense']

    class _GB:
        nmax = 256
    assert ops.resolve_route('auto', _GB) == 'dense'
    _GB.nmax = 257
    assert ops.resolve_route('auto', _GB) == 'sparse' and ops.resolve_route('dense', _GB) == 'dense'


def test_defaults_are_dense_and_state_dicts_unchanged():
    from sgaligner_amd import ops
    from sgaligner_amd.aligner.networks.gat import MultiGAT
    from sgaligner_amd.aligner.sg_aligner import MultiModalEncoder
    assert MultiGAT().route == 'dense' and inspect.signature(MultiGAT.__init__).parameters['route'].default == 'dense'
    assert inspect.signature(MultiModalEncoder.__init__).parameters['gat_route'].default == 'dense'
    assert inspect.signature(ops.multi_gat_layers).parameters['route'].default == 'dense'
    enc = MultiModalEncoder(['point', 'gat', 'rel'], rel_dim=41, attr_dim=164)
    assert enc.gat_route == 'dense' and enc.structure_encoder.route == 'dense'
    for route in ('sparse', 'auto'):
        assert list(MultiGAT(route=route).state_dict()) == list(MultiGAT().state_dict())
        other = MultiModalEncoder(['point', 'gat', 'rel'], rel_dim=41, attr_dim=164, gat_route=route)
        assert other.structure_encoder.route == route
        assert {k: tuple(v.shape) for k, v in other.state_dict().items()} == {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in O.init_params(['point', 'gat', 'rel']).items()}
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items() if 'num_batches_tracked' not in k} == want


def test_sparse_gat_kernels_do_not_spill():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    base, res = kr.analyse(os.path.join(_build.CSRC, 'gat_sparse.hip'))
    for tag, count in (('sp_logits_kernel', 4), ('sp_fwd_kernel', 4), ('sp_bwd_t_kernel', 4), ('sp_bwd_s_kernel', 4), ('sp_keys_kernel', 1),
                       ('sp_heads_kernel', 1), ('sp_rows_kernel', 1), ('sp_mult_kernel', 1), ('sp_cols_kernel', 1), ('sp_datt_part_kernel', 1),
                       ('sp_datt_fold_kernel', 1)):
        ks = [k for k in res if tag in k]
        assert len(ks) == count, (tag, sorted(res))                       # the attention kernels: CJ in 1 .. 4
        for k in ks:
            v = res[k]
            # (v_readlane inside the entry loops is the broadcast of alpha and the source id, not a spilled scalar)
            assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0 and not v.get('loop_scratch'), (k, v)


def test_gate_ratios_are_the_measured_ones():
    """R is 'the worst measured kernel / yardstick ratio x 2, rounded up' over the many-entry rows of profiles/gat_sparse_accuracy_vs_fp32.json
    per output kind; R1 the same over the single-entry rows, never below R.  The many-entry gate is not set by a single-entry draw."""
    profile = json.load(open(SG.PROFILE))['cases']
    assert SG.ratios_from_profile() == (SG.R, SG.R1)
    assert set(SG.R) == set(SG.OUTPUTS) and set(SG.R1) == {c['output'] for c in profile if c['n'] <= 1} == {'das', 'dad'}
    assert all(SG.R1[k] >= SG.R[k] for k in SG.R1)
    assert sum(c['output'] == 'dad' and c['n'] > 1 for c in profile) == 14 and sum(c['output'] == 'dad' and c['n'] <= 1 for c in profile) == 1
    assert SG.r_of('dad1', 200) == SG.R['dad'] and SG.r_of('dad', 1) == SG.R1['dad']
    # no kind of many entries is gated looser than twice the dense route's bound for it
    assert all(SG.R[k] <= 2 * GG.R[k] for k in SG.R), (SG.R, GG.R)


def test_guard_holds_at_the_frozen_seeds():
    """Every pre-activation on a counted edge is clear of LeakyReLU's kink at the committed seed, and that seed is the first that is."""
    assert set(SG.SEEDS) == {('kernel',) + c for c in SG.KERNEL_CASES} | {('stack', w) for w in range(len(SG.STACKS))}
    for c in SG.KERNEL_CASES:
        assert SG.find_kernel_seed(*c) == SG.SEEDS[('kernel',) + c], c
    for w in range(len(SG.STACKS)):
        assert SG.find_stack_seed(w) == SG.SEEDS[('stack', w)], w
