"""MultiGCN / GCNConv message passing of the EVA baseline (reference src/aligner/networks/gat.py:6-25) on csrc/gcn.hip.

Part of the autograd layer over the C-ABI HIP kernels (see ops.py, which re-exports everything here: `sgaligner_amd.ops.<name>` keeps
working).  The run-time switches live in ops.py and are read through the module at call time (`_o.FLAG`)."""
from __future__ import annotations

import torch

from . import _lib
from . import ops as _o
from .ops import _ev_start, _ev_stop, _p, _req, _stream, DEFERRED_CHECKS, cast_f32, colsum, gemm


def _gcn_status_verdict(v):
    if v[0] == 0:
        return None
    return ('sgaligner_amd: a (source, target) edge occurs more than 255 times in one graph of the PREVIOUS batch; the GCN kernels count '
            'duplicate edges in 8 bits (PyG would count them all), so that step\'s structure embeddings were not PyG-equivalent -- '
            'deduplicate the edge list')


def gcn_aggregate(h, gb, bias=None, transpose=False, relu=False, check_status=False):
    """out = A^ h + bias (relu: max(., 0) on top), or A^T h with transpose=True, for all graphs of `gb` in one launch (csrc/gcn.hip)."""
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


class MultiGCNFn(torch.autograd.Function):
    """MultiGCN.forward over ALL graphs of a batch (reference gat.py:17-25 x eva.py:44-72): GCNConv, ReLU, GCNConv."""

    @staticmethod
    def forward(ctx, gb, x, w0, b0, w1, b1):
        if not x.is_cuda:
            raise RuntimeError('sgaligner_amd.MultiGCNFn: HIP device tensor required; there is no CPU path')
        if x.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f'sgaligner_amd.MultiGCNFn: tot_rel_pose must be float32 or float64, got {x.dtype}')
        x32 = cast_f32(x.contiguous())
        w0, b0, w1, b1 = [_req(t.contiguous(), n) for t, n in ((w0, 'gcn0.lin.weight'), (b0, 'gcn0.bias'), (w1, 'gcn1.lin.weight'), (b1, 'gcn1.bias'))]
        t, f = x32.shape
        c0, c1 = w0.shape[0], w1.shape[0]
        if t != gb.T:
            raise RuntimeError(f'sgaligner_amd: tot_rel_pose has {t} rows but the graphs hold {gb.T} nodes')
        if w0.shape[1] != f or w1.shape[1] != c0 or b0.shape != (c0,) or b1.shape != (c1,):
            raise RuntimeError('sgaligner_amd.MultiGCNFn: layer shapes do not chain')
        h0 = gemm(x32, w0, False, True, t, c0, f)
        x1 = gcn_aggregate(h0, gb, b0, relu=True, check_status=True)     # both layers see the same edge list: one check per batch
        h1 = gemm(x1, w1, False, True, t, c1, c0)
        o1 = gcn_aggregate(h1, gb, b1)
        ctx.gb = gb
        ctx.save_for_backward(x32, x1, w1)
        return o1

    @staticmethod
    def backward(ctx, d_o1):
        x32, x1, w1 = ctx.saved_tensors
        gb = ctx.gb
        t, f = x32.shape
        c1, c0 = w1.shape
        d_o1 = d_o1.contiguous()
        db1 = colsum(d_o1)
        dh1 = gcn_aggregate(d_o1, gb, transpose=True)
        dw1 = gemm(dh1, x1, True, False, c1, c0, t)
        dx1 = gemm(dh1, w1, False, False, t, c0, c1)
        d_p0 = torch.empty_like(dx1)
        _lib.check(_lib.lib().sga_relu_bwd(_p(x1), _p(dx1), _p(d_p0), x1.numel(), _stream()), 'sga_relu_bwd')
        db0 = colsum(d_p0)
        dh0 = gcn_aggregate(d_p0, gb, transpose=True)
        dw0 = gemm(dh0, x32, True, False, c0, f, t)
        return None, None, dw0, db0, dw1, db1


def multi_gcn(gb, x, layer0, layer1):
    """layer = (lin_weight [out, in], bias [out])."""
    return MultiGCNFn.apply(gb, x, *layer0, *layer1)
