"""MultiGCN / GCNConv message passing of the EVA baseline (reference src/aligner/networks/gat.py:6-25) on csrc/gcn.hip (the dense route) and
csrc/gcn_sparse.hip (the sparse route over GraphBatch.sparse(): graphs of any size).

Part of the autograd layer over the C-ABI HIP kernels (see ops.py, which re-exports everything here: `sgaligner_amd.ops.<name>` keeps
working).  The run-time switches live in ops.py and are read through the module at call time (`_o.FLAG`)."""
from __future__ import annotations

import torch

from . import _lib
from . import ops as _o
from .gat_ops import resolve_route
from .ops import _ev_start, _ev_stop, _p, _req, _stream, DEFERRED_CHECKS, cast_f32, colsum, gemm


def _gcn_status_verdict(v):
    if v[0] == 0:
        return None
    return ('sgaligner_amd: a (source, target) edge occurs more than 255 times in one graph of the PREVIOUS batch; the GCN kernels count '
            'duplicate edges in 8 bits (PyG would count them all), so that step\'s structure embeddings were not PyG-equivalent -- '
            'deduplicate the edge list')


def gcn_aggregate(h, gb, bias=None, transpose=False, relu=False, check_status=False, route='dense'):
    """out = A^ h + bias (relu: max(., 0) on top), or A^T h with transpose=True, for all graphs of `gb` in one launch.
    route: 'dense' (csrc/gcn.hip: at most 256 nodes per graph, 255 copies of a pair), 'sparse' (csrc/gcn_sparse.hip over gb.sparse(): graphs
    of any size, 32-bit multiplicities, hence no status word) or 'auto' (sparse exactly when gb.nmax > 256).  Where the dense route can run,
    both return the same bits."""
    if resolve_route(route, gb) == 'sparse':
        return _gcn_aggregate_sp(h, gb, bias, transpose, relu)
    out = torch.empty_like(h)
    st = None
    if check_status and _o.VALIDATE:
        st = torch.zeros((1,), device=h.device, dtype=torch.int32)      # a fresh status word per batch, as the GAT path does
    ev = _ev_start()
    _lib.check(_lib.lib().sga_gcn_aggregate(_p(h), int(h.shape[1]), _p(bias), _p(gb.edges), _p(gb.node_off), _p(gb.edge_off), gb.G, gb.nmax,
                                            int(transpose), int(relu), _p(out), _p(st), _stream()), 'sga_gcn_aggregate')
    _ev_stop(ev, 'gcn_aggregate', (int(h.shape[0]), int(h.shape[1]), int(gb.edges.shape[0]), bool(transpose)))
    if st is not None:
        DEFERRED_CHECKS.submit_fn(st, _gcn_status_verdict)
    return out


def _gcn_aggregate_sp(h, gb, bias, transpose, relu):
    if transpose and (bias is not None or relu):
        raise RuntimeError('sgaligner_amd.gcn_aggregate: the transposed aggregation takes no bias and no ReLU')
    sp = gb.sparse()
    if int(h.shape[0]) != sp.T:
        raise RuntimeError(f'sgaligner_amd.gcn_aggregate: the features have {int(h.shape[0])} rows but the graphs hold {sp.T} nodes')
    dinv = sp.dinv()
    out = torch.empty_like(h)
    ptr, nbr, perm = (sp.col_ptr, sp.tgt, sp.perm) if transpose else (sp.row_ptr, sp.src, None)
    ev = _ev_start()
    _lib.check(_lib.lib().sga_gcn_sp_aggregate(_p(h), int(h.shape[1]), _p(bias), _p(ptr), _p(nbr), _p(sp.mult), _p(perm), _p(dinv), sp.T, sp.cap,
                                               int(relu), _p(out), _stream()), 'sga_gcn_sp_aggregate')
    _ev_stop(ev, 'gcn_sp_aggregate', (int(h.shape[0]), int(h.shape[1]), sp.cap, bool(transpose)))
    return out


# ------------------------------------------------------------------------------------------ GCN, any stack, both routes
def _relu_bwd(y, gy):
    y, gy = y.contiguous(), gy.contiguous()               # the kernel walks memory: a strided view would be read as if it were dense
    gx = torch.empty_like(y)
    _lib.check(_lib.lib().sga_relu_bwd(_p(y), _p(gy), _p(gx), y.numel(), _stream()), 'sga_relu_bwd')
    return gx


class GCNLayerFn(torch.autograd.Function):
    """One GCNConv(in, out) over ALL graphs of a batch, with the ReLU that follows it where relu is set: the projection on the GEMM, then the
    aggregation with bias (and ReLU) on the route given ('dense' | 'sparse', already resolved).  Backward: relu_bwd, colsum, the transposed
    aggregation and the two GEMMs.  The input gets a gradient only where it asks for one (not the first layer's)."""

    @staticmethod
    def forward(ctx, gb, x, w, bias, relu, route, check_status):
        x = _req(x.contiguous(), 'gcn.x')
        w, bias = _req(w.contiguous(), 'gcn.lin.weight'), _req(bias.contiguous(), 'gcn.bias')
        t, f = int(x.shape[0]), int(x.shape[1])
        c = int(w.shape[0])
        if t != gb.T:
            raise RuntimeError(f'sgaligner_amd: the GCN input has {t} rows but the graphs hold {gb.T} nodes')
        if w.dim() != 2 or int(w.shape[1]) != f or tuple(bias.shape) != (c,):
            raise RuntimeError(f'sgaligner_amd: GCNConv({f}, {c}) needs lin.weight [{c}, {f}] and bias [{c}], got {tuple(w.shape)} and '
                               f'{tuple(bias.shape)}')
        h = gemm(x, w, False, True, t, c, f)
        y = gcn_aggregate(h, gb, bias, relu=relu, check_status=check_status, route=route)
        ctx.gb, ctx.relu, ctx.route = gb, relu, route
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        t, f = x.shape
        c = w.shape[0]
        gy = gy.contiguous()
        d_pre = _relu_bwd(y, gy) if ctx.relu else gy
        db = colsum(d_pre)
        dh = gcn_aggregate(d_pre, ctx.gb, transpose=True, route=ctx.route)
        dw = gemm(dh, x, True, False, c, f, t)
        dx = gemm(dh, w, False, False, t, f, c) if ctx.needs_input_grad[1] else None
        return None, dx, dw, db, None, None, None


def multi_gcn_layers(gb, x, layers, route='dense'):
    """MultiGCN.forward (gat.py:17-25) for a stack of any depth >= 1: GCNConv per layer, ReLU between layers and none after the last.
    layers: (lin_weight [out, in], bias [out]) per layer.  route: 'dense' (at most 256 nodes per graph), 'sparse' (the CSR kernels: graphs of
    any size, no status word) or 'auto' (sparse exactly when gb.nmax > 256).  Dropout is not implemented (the reference's default is 0)."""
    route = resolve_route(route, gb)
    if len(layers) < 1:
        raise ValueError('sgaligner_amd.multi_gcn_layers: at least one layer')
    if not x.is_cuda:
        raise RuntimeError('sgaligner_amd.multi_gcn_layers: HIP device tensor required; there is no CPU path')
    if x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f'sgaligner_amd.multi_gcn_layers: tot_rel_pose must be float32 or float64, got {x.dtype}')
    x = cast_f32(x.contiguous())
    for i, (w, b) in enumerate(layers):
        x = GCNLayerFn.apply(gb, x, w, b, i + 1 < len(layers), route, i == 0)      # every layer sees the same edge list: one multiplicity check per batch
    return x
