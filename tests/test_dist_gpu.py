"""The REAL one-process-per-GPU path under the driver's GPU test tier: 2 ranks (torch.multiprocessing spawn, gloo backend,
both on cuda:0 -- the box has one GPU; on a multi-GPU node the same code runs over RCCL) each take a contiguous block of the
pairs of ONE global batch and run AlignerSteps.forward_backward: layout + index-set all-gathers, table all-gather,
anchor-sharded global loss with its three scalar all-reduces, reduce of dL/dE to the owning rank, flat parameter-gradient
all-reduce.  Loss and EVERY parameter gradient must equal the single-process result on the full batch (M = 3 and M = 1,
even and uneven pair splits incl. a rank with zero pairs), and two accumulated micro-steps must equal their single-process
sum (EpochBasedTrainer with grad_acc_steps = 2)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, mods, n_pairs, cuts, out, nobj=14, ragged=True, emb_dim=100):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from sgaligner_amd import dist as sdist
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    backend = os.environ.get('SGA_TEST_DIST_BACKEND', 'gloo')       # 'nccl' (= RCCL): one GPU per rank, the *_rccl tests below
    di = rank if backend == 'nccl' else 0
    torch.cuda.set_device(di)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        dev = torch.device('cuda', di)
        full = to_device(make_batch(n_pairs, nobj, 48, seed=21, ragged=ragged), dev)
        lo, hi = cuts[rank], cuts[rank + 1]
        mine = sdist.shard_data_dict(full, lo, hi)
        from sgaligner_amd import loss_ops as ops_mod          # (where FusedContrastiveFn looks _sym_jobs up)
        orig_jobs, ops_mod._sym_calls = ops_mod._sym_jobs, []
        ops_mod._sym_jobs = lambda c, r, nt: (ops_mod._sym_calls.append((len(c) - 1, r)), orig_jobs(c, r, nt))[1]
        from sgaligner_amd import ops, trainer as trainer_mod
        if os.environ.get('SGA_TEST_MFMA_MODE'):
            ops.set_mfma_mode(os.environ['SGA_TEST_MFMA_MODE'])
        if os.environ.get('SGA_TEST_WIDE_REPLICA') == '1':
            trainer_mod.WIDE_SHARDED = False
        shards = []
        orig_terms = ops_mod.ContrastiveTermsFn.forward
        steps = AlignerSteps(mods, device=dev, seed=42, emb_dim=emb_dim)
        orig_loss = steps.loss_func.forward
        def spy(output_dict, data_dict):                        # (what anchor range the general path was handed)
            shards.append(tuple(data_dict['_sga_shard'][:2]) if data_dict.get('_sga_shard') is not None else None)
            return orig_loss(output_dict, data_dict)
        steps.loss_func.forward = spy
        _, loss = steps.forward_backward(mine)
        torch.cuda.synchronize()
        res = {'loss': float(loss['loss'].item()), 'sym_jobs': list(getattr(ops_mod, '_sym_calls', [])), 'shards': shards}
        for n, p in steps.model.named_parameters():
            if p.grad is not None:
                res['g:' + n] = p.grad.detach().cpu()
        for tag, layer in (('ial', steps.multi_loss_layer_ial), ('icl', steps.multi_loss_layer_icl)):
            for p in layer.parameters():
                if p.grad is not None:
                    res['lv:' + tag] = p.grad.detach().cpu()
        out[rank] = res
    finally:
        dist.destroy_process_group()


def _single(mods, n_pairs, nobj=14, ragged=True, emb_dim=100):
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    full = to_device(make_batch(n_pairs, nobj, 48, seed=21, ragged=ragged), 'cuda')
    ref = AlignerSteps(mods, device='cuda', seed=42, emb_dim=emb_dim)
    _, loss = ref.forward_backward(full)
    torch.cuda.synchronize()
    return ref, loss


@pytest.mark.parametrize('mods,n_pairs,cuts', [(['point', 'gat', 'rel'], 6, [0, 3, 6]), (['point', 'gat', 'rel'], 5, [0, 4, 5]),
                                               (['point'], 6, [0, 3, 6]), (['point', 'gat', 'rel'], 4, [0, 4, 4])])
def test_two_ranks_equal_single_process(mods, n_pairs, cuts):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), mods, n_pairs, cuts, out), nprocs=world, join=True)
    ref, loss = _single(mods, n_pairs)
    for rank in range(world):
        r = out[rank]
        assert abs(r['loss'] - loss['loss'].item()) <= 1e-5 * max(1.0, abs(loss['loss'].item())), (rank, r['loss'], loss['loss'].item())
        seen = 0
        for n, p in ref.model.named_parameters():
            if p.grad is None:
                continue
            g = r['g:' + n]
            sc = p.grad.abs().max().item()
            assert (g - p.grad.cpu()).abs().max().item() <= 1e-4 * max(1.0, sc), (rank, n)
            seen += 1
        assert seen >= 8
        if len(mods) > 1:
            for tag, layer in (('ial', ref.multi_loss_layer_ial), ('icl', ref.multi_loss_layer_icl)):
                a = next(layer.parameters()).grad.cpu()
                assert (r['lv:' + tag] - a).abs().max().item() <= 1e-4 * max(1.0, a.abs().max().item()), (rank, tag)

@pytest.mark.parametrize('how', ['sharded', 'f16', 'replica'])
@pytest.mark.parametrize('mods', [['point', 'gat', 'rel'], ['point']])
def test_two_ranks_wide_tables_equal_single_process(mods, how, monkeypatch):
    """Tables the fused kernels do not take (emb_dim 160: wider than the fused path's 104 columns and the per-table path's 128 -- BASELINE
    configs[4]'s 1024-d tables on 8 GPUs take this branch) under N > 1.  Round 6: the general per-table kernels SHARDED BY ANCHORS (balanced
    cuts on 32-anchor boundaries; the wide-table kernels take an anchor range), in exact fp32 and in mode 'f16'; and the round-5 form -- a
    REPLICA of the whole loss on every rank -- as a cross-check.  Same loss and parameter gradients as one process on the whole batch."""
    if how == 'f16':
        monkeypatch.setenv('SGA_TEST_MFMA_MODE', 'f16')
    if how == 'replica':
        monkeypatch.setenv('SGA_TEST_WIDE_REPLICA', '1')
    world, n_pairs, cuts = 2, 6, [0, 3, 6]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), mods, n_pairs, cuts, out, 40, True, 160), nprocs=world, join=True)     # (40 objects per scene: > 32 anchors)
    from sgaligner_amd import ops
    old_mode = ops.set_mfma_mode('f16') if how == 'f16' else None
    try:
        ref, loss = _single(mods, n_pairs, 40, emb_dim=160)
    finally:
        if old_mode is not None:
            ops.set_mfma_mode(old_mode)
    for rank in range(world):
        r = out[rank]
        if how == 'replica':
            assert r['shards'] == [None], r['shards']
        else:                                                   # a proper anchor range on a 32-anchor boundary, the two ranks' ranges adjacent
            assert len(r['shards']) == 1 and r['shards'][0] is not None and r['shards'][0][0] % 32 == 0, r['shards']
            assert out[0]['shards'][0][1] == out[1]['shards'][0][0] and out[0]['shards'][0][0] == 0
            assert out[1]['shards'][0][1] > out[1]['shards'][0][0] > 0                  # both ranks own anchors
        assert abs(r['loss'] - loss['loss'].item()) <= 1e-5 * max(1.0, abs(loss['loss'].item())), (rank, r['loss'], loss['loss'].item())
        seen = 0
        for n, p in ref.model.named_parameters():
            if p.grad is None:
                continue
            sc = p.grad.abs().max().item()
            assert (r['g:' + n] - p.grad.cpu()).abs().max().item() <= 1e-4 * max(1.0, sc), (rank, n)
            seen += 1
        assert seen >= 8
        if len(mods) > 1:
            for tag, layer in (('ial', ref.multi_loss_layer_ial), ('icl', ref.multi_loss_layer_icl)):
                a = next(layer.parameters()).grad.cpu()
                assert (r['lv:' + tag] - a).abs().max().item() <= 1e-4 * max(1.0, a.abs().max().item()), (rank, tag)


def test_two_ranks_walk_the_anchor_pairs_symmetrically():
    """Both ranks' anchor cuts on 32-row boundaries (32 anchors per pair): the one-pass anchors x anchors walk is SYMMETRIC across the ranks
    (ops._sym_jobs with R = 2: rank 0 its square + the rectangle against rank 1's rows, rank 1 its square) -- loss and every parameter
    gradient still equal the single process."""
    mods, n_pairs, cuts, world = ['point', 'gat', 'rel'], 8, [0, 4, 8], 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), mods, n_pairs, cuts, out, 107, False), nprocs=world, join=True)
    ref, loss = _single(mods, n_pairs, 107, False)
    for rank in range(world):
        r = out[rank]
        assert (2, rank) in [tuple(x) for x in r['sym_jobs']], r['sym_jobs']          # the cross-rank symmetric plan ran on this rank
        assert abs(r['loss'] - loss['loss'].item()) <= 1e-5 * max(1.0, abs(loss['loss'].item())), (rank, r['loss'], loss['loss'].item())
        for n, p in ref.model.named_parameters():
            if p.grad is None:
                continue
            sc = p.grad.abs().max().item()
            assert (r['g:' + n] - p.grad.cpu()).abs().max().item() <= 1e-4 * max(1.0, sc), (rank, n)


def _overlap_worker(rank, world, port, out):
    import sys
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch.distributed as dist
    from sgaligner_amd import dist as sdist
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    backend = os.environ.get('SGA_TEST_DIST_BACKEND', 'gloo')       # 'nccl' (= RCCL): one GPU per rank, the *_rccl tests below
    di = rank if backend == 'nccl' else 0
    torch.cuda.set_device(di)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        dev = torch.device('cuda', di)
        full = to_device(make_batch(6, 12, 48, seed=33), dev)             # uniform scenes: equal shards -> the asynchronous gathers
        mine = sdist.shard_data_dict(full, 3 * rank, 3 * rank + 3)
        res = {}
        for tag, overlap, known in (('overlap', True, True), ('blocking', False, False)):
            steps = AlignerSteps(['point', 'gat', 'rel'], device=dev, seed=42)
            steps.overlap_gather = overlap
            dd = dict(mine)
            if known:                                                     # no layout all-gather, no host read-back
                dd['_sga_layout'] = sdist.known_layout(mine['tot_obj_pts'].shape[0], len(mine['e1i']), len(mine['e1j']), len(mine['e2j']), world)
            sdist.COLLECTIVE_EVENTS = []
            _, loss = steps.forward_backward(dd)
            torch.cuda.synchronize()
            ev, sdist.COLLECTIVE_EVENTS = sdist.COLLECTIVE_EVENTS, None
            r = {'loss': float(loss['loss'].item()), 'kinds': sorted(set(e[0] for e in ev)),
                 'n_gather': sum(1 for e in ev if e[0] == 'all_gather')}
            for n, p in steps.model.named_parameters():
                if p.grad is not None:
                    r['g:' + n] = p.grad.detach().cpu()
            if overlap:
                r['summary'] = sdist.collective_summary(ev, 1, dev, repeats=1)
            res[tag] = r
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_overlapped_gathers_equal_blocking_and_single_process():
    """The table all-gathers launched from inside the encoder (dist.EarlyGather: cheap modalities first, asynchronous) + a known
    batch layout (no host sync) give the loss and gradients of the blocking path and of the single-process run; the step's
    collectives are logged for bench.py's `collectives` object."""
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_overlap_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    ref = AlignerSteps(['point', 'gat', 'rel'], device='cuda', seed=42)
    _, loss = ref.forward_backward(to_device(make_batch(6, 12, 48, seed=33), 'cuda'))
    torch.cuda.synchronize()
    for rank in range(world):
        a, b = out[rank]['overlap'], out[rank]['blocking']
        assert abs(a['loss'] - b['loss']) <= 1e-6 * max(1.0, abs(b['loss']))
        assert abs(a['loss'] - loss['loss'].item()) <= 1e-5 * max(1.0, abs(loss['loss'].item()))
        # 3 table gathers + the packed index sets (+ the layout gather on the blocking path only)
        assert a['n_gather'] == 4 and b['n_gather'] == 5, (a['n_gather'], b['n_gather'])
        for n, p in ref.model.named_parameters():
            if p.grad is None:
                continue
            sc = max(1.0, p.grad.abs().max().item())
            assert (a['g:' + n] - b['g:' + n]).abs().max().item() <= 1e-5 * sc, (rank, n)
            assert (a['g:' + n] - p.grad.cpu()).abs().max().item() <= 1e-4 * sc, (rank, n)
        summ = a['summary']
        assert summ['world_size'] == 2 and len(summ['ranks_seen']) == 2 and summ['all_gather_bytes'] > 0
        assert all(t['ms_each'] > 0 for t in summ['timed_alone'])


def _acc_worker(rank, world, port, out):
    import sys
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch.distributed as dist
    from sgaligner_amd.epoch_trainer import EpochBasedTrainer
    from sgaligner_amd.synthetic import make_batch
    from sgaligner_amd.trainer import AlignerSteps
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    backend = os.environ.get('SGA_TEST_DIST_BACKEND', 'gloo')       # 'nccl' (= RCCL): one GPU per rank, the *_rccl tests below
    di = rank if backend == 'nccl' else 0
    torch.cuda.set_device(di)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        steps = AlignerSteps(['point', 'gat', 'rel'], device='cuda', seed=42)
        tr = EpochBasedTrainer(steps, output_dir=f'/tmp/sga_acc_{port}', max_epoch=1, lr=0.0, grad_acc_steps=2, log_steps=100)
        batches = [make_batch(4, 10, 32, seed=50 + i) for i in range(2)]
        grads = {}
        tr._optimizer_step = lambda it: grads.update({n: p.grad.detach().cpu().clone() for n, p in steps.model.named_parameters()
                                                      if p.grad is not None}) if it % 2 == 0 else None
        tr.register_loader(batches, batches)
        tr.train_epoch()
        out[rank] = grads
    finally:
        dist.destroy_process_group()


def test_grad_accumulation_two_ranks_equals_single_process_sum():
    """with grad_acc_steps = 2 under two ranks the gradient the optimiser sees must be G1 + G2 of the global
    batches (one reduce per optimiser step), not world*G1 + G2."""
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_acc_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    ref = AlignerSteps(['point', 'gat', 'rel'], device='cuda', seed=42)
    ref.zero_grad()
    for i in range(2):
        dd = to_device(make_batch(4, 10, 32, seed=50 + i), 'cuda')
        o, l = ref.train_step(0, 0, dd)
        l['loss'].backward()
    torch.cuda.synchronize()
    for rank in range(world):
        g = out[rank]
        assert g, 'optimizer step never reached'
        for n, p in ref.model.named_parameters():
            if p.grad is not None:
                sc = p.grad.abs().max().item()
                assert (g[n] - p.grad.cpu()).abs().max().item() <= 1e-4 * max(1.0, sc), (rank, n)


def _rccl_worker(rank, world, port, mods, ragged_pad, out):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from sgaligner_amd import dist as sdist
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        assert sdist._has_reduce_scatter()
        dev = torch.device('cuda', 0)
        dd = to_device(make_batch(5, 14, 48, seed=23, ragged=True), dev)
        steps = AlignerSteps(mods, device=dev, seed=42)
        steps.zero_grad()
        sdist.COLLECTIVE_EVENTS = []
        early = None
        if len(mods) > 1:                                   # as AlignerSteps.train_step does for N > 1: asynchronous RCCL gathers
            early = sdist.EarlyGather([int(dd['tot_obj_pts'].shape[0])])
            steps.model._on_table = early
        output_dict = steps.model(dd)
        steps.model._on_table = None
        loss = steps._global_loss(output_dict, dd, None, early)   # the N > 1 code path, over RCCL, with a world of one
        loss['loss'].backward()
        steps.reduce_grads()
        torch.cuda.synchronize()
        ev, sdist.COLLECTIVE_EVENTS = sdist.COLLECTIVE_EVENTS, None
        res = {'loss': float(loss['loss'].item()), 'summary': sdist.collective_summary(ev, 1, dev, repeats=2)}
        for n, p in steps.model.named_parameters():
            if p.grad is not None:
                res['g:' + n] = p.grad.detach().cpu()
        # the ragged reduce-scatter branch (blocks padded to the largest shard) cannot arise with one rank through the trainer:
        # drive AllGatherRows.backward's padded path directly with a row count below the padded block size
        x = torch.randn(7, 5, device=dev, requires_grad=True)
        y = sdist.AllGatherRows.apply(x, [7], True)
        (y * torch.arange(35, device=dev, dtype=torch.float32).view(7, 5)).sum().backward()
        res['ag_grad'] = x.grad.cpu()
        lay = sdist.gather_batch_layout(dd, dev)
        res['layout'] = lay.tolist()
        out[0] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('mods', [['point', 'gat', 'rel'], ['point']])
def test_rccl_collectives_world_of_one(mods):
    """The box has one GPU and RCCL refuses two ranks on one device, so the 2-rank tests above run over gloo.  This one
    initialises the nccl (= RCCL) backend with a world of ONE and drives the multi-GPU code path (AlignerSteps._global_loss +
    reduce_grads) through it: all_gather_into_tensor of int64 / int32 / fp32 device tensors, reduce_scatter_tensor of the table
    gradients, the fp64 scalar all-reduces and the flat fp32 gradient all-reduce are real RCCL calls here.  Results must equal
    the plain single-process path."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_rccl_worker, args=(1, _free_port(), mods, False, out), nprocs=1, join=True)
    from sgaligner_amd.synthetic import make_batch, to_device
    from sgaligner_amd.trainer import AlignerSteps
    dd = to_device(make_batch(5, 14, 48, seed=23, ragged=True), 'cuda')
    ref = AlignerSteps(mods, device='cuda', seed=42)
    _, loss = ref.forward_backward(dd)
    torch.cuda.synchronize()
    r = out[0]
    assert abs(r['loss'] - loss['loss'].item()) <= 1e-5 * max(1.0, abs(loss['loss'].item()))
    seen = 0
    for n, p in ref.model.named_parameters():
        if p.grad is None:
            continue
        sc = p.grad.abs().max().item()
        assert (r['g:' + n] - p.grad.cpu()).abs().max().item() <= 1e-4 * max(1.0, sc), n
        seen += 1
    assert seen >= (8 if len(mods) > 1 else 4)
    assert torch.equal(r['ag_grad'], torch.arange(35, dtype=torch.float32).view(7, 5))
    assert r['layout'][0][0] == int(dd['tot_obj_pts'].shape[0])
    summ = r['summary']                                       # bench.py's `collectives` object, from real RCCL calls
    assert summ['backend'] == 'nccl' and summ['ranks_seen'][0]['rank'] == 0
    kinds = set(summ['per_step_this_rank'])
    assert 'all_gather' in kinds and 'reduce_scatter' in kinds and 'all_reduce' in kinds      # (M = 1 too since round 5: its loss is sharded by anchors as well)
    assert all(t['ms_each'] > 0 for t in summ['timed_alone'])


def test_bench_gpus2_creates_its_two_ranks():
    """`python bench.py --gpus 2` launched bare (no torchrun, the way the driver launches N = 1) must create its two ranks itself
    and say so in the line: n_gpus == 2 and two distinct ranks in the self-certifying `collectives` object (round-3 review: it ran ONE
    process and only warned).  One GPU on the box: the ranks share it and talk over gloo."""
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '1', '--config', 'c2',
                        '--full', '--no-cpu-baseline', '--no-hits', '--no-scale-ref'], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2
    seen = line['collectives']['ranks_seen']
    assert sorted(x['rank'] for x in seen) == [0, 1]
    assert line['collectives']['world_size'] == 2
    assert line['config']['global_pairs'] == 1024 and line['config']['pairs_per_gpu'] == 512


def test_bench_refuses_a_world_that_is_not_gpus():
    """WORLD_SIZE (set by a launcher) != --gpus is an error, not a warning."""
    import subprocess
    import sys
    env = dict(os.environ)
    env.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--config', 'c2'],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert 'WORLD_SIZE=1' in (r.stderr + r.stdout)


# ---- the same two-rank checks over RCCL, one GPU per rank: they run on the first box that has two GPUs (the builder's and the driver's test
# boxes have one: RCCL refuses two ranks on one device, so there the gloo variants above carry the path)
needs2 = pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs (RCCL: one rank per device)')


@pytest.fixture
def rccl_backend():
    os.environ['SGA_TEST_DIST_BACKEND'] = 'nccl'
    yield
    os.environ.pop('SGA_TEST_DIST_BACKEND', None)


@needs2
def test_two_ranks_equal_single_process_rccl(rccl_backend):
    test_two_ranks_equal_single_process(['point', 'gat', 'rel'], 6, [0, 3, 6])
    test_two_ranks_equal_single_process(['point', 'gat', 'rel'], 5, [0, 4, 5])


@needs2
def test_two_ranks_walk_the_anchor_pairs_symmetrically_rccl(rccl_backend):
    test_two_ranks_walk_the_anchor_pairs_symmetrically()


@needs2
def test_overlapped_gathers_equal_blocking_and_single_process_rccl(rccl_backend):
    """asynchronous all_gather_into_tensor from the table hook + reduce_scatter_tensor of the table gradients with TWO real RCCL ranks"""
    test_overlapped_gathers_equal_blocking_and_single_process()


@needs2
def test_grad_accumulation_two_ranks_equals_single_process_sum_rccl(rccl_backend):
    test_grad_accumulation_two_ranks_equals_single_process_sum()
