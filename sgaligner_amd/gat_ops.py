"""MultiGAT / GATConv message passing (reference src/aligner/networks/gat.py:27-48) on csrc/gat.hip.

Part of the autograd layer over the C-ABI HIP kernels (see ops.py, which re-exports everything here: `sgaligner_amd.ops.<name>` keeps
working).  The run-time switches live in ops.py and are read through the module at call time (`_o.FLAG`), so `ops.FLAG = value` set by a
caller or a test takes effect here."""
from __future__ import annotations

import ctypes as _ct

import numpy as _np
import torch

from . import _lib
from . import ops as _o
from .ops import (_SmallCache, _ev_start, _ev_stop, _fingerprint, _h2d, _p, _ptr_array, _req, _stream, get_mfma_mode, DEFERRED_CHECKS, IndexSets,
                  _POINTNET_MODE, _stash_bytes, cast_f32, colsum, gemm)

# ------------------------------------------------------------------------------------------ GAT
class GraphBatch:
    """Device-side CSR-style description of the 2B scene graphs of a batch: node/edge offsets in the
    src,ref,src,ref... order of reference sg_aligner.py:86-110, plus the int64 [sum E, 2] edge list
    (graph-local node ids, column 0 = source j, column 1 = target i) exactly as collated."""

    def __init__(self, node_counts, edge_counts, edges, keep_edges=True):
        nc = _np.asarray(node_counts, dtype=_np.int64).reshape(-1)
        ec = _np.asarray(edge_counts, dtype=_np.int64).reshape(-1)
        if nc.shape != ec.shape:
            raise RuntimeError('sgaligner_amd: graph_per_obj_count and graph_per_edge_count disagree')
        self.G = int(nc.shape[0])
        self.nmax = int(nc.max()) if self.G else 0
        self.T = int(nc.sum())
        self.E = int(ec.sum())
        dev = edges.device
        if edges.dtype != torch.int64:
            edges = edges.to(torch.int64)
        edges = edges.contiguous()
        if edges.shape[0] < self.E:
            raise RuntimeError('sgaligner_amd: edge list shorter than graph_per_edge_count says')
        if _o.VALIDATE and self.E and edges.is_cuda:
            # Node ids are graph-LOCAL (scan3r.py:99): anything outside [0, largest graph) can not be a node of any graph.
            # The kernels drop out-of-range endpoints (PyG would raise an index error); catch the gross case here, once per batch.
            DEFERRED_CHECKS.poll()                                   # earlier batches' answers (no waiting)
            DEFERRED_CHECKS.submit(torch.stack(torch.aminmax(edges[:self.E])), self.nmax,
                                   'sgaligner_amd: edge endpoints span [%d, %d] but the largest graph has %d nodes '
                                   '(edges must hold graph-local node ids)')
        self.edges = edges if keep_edges else None
        offs = _h2d(_np.concatenate([[0], _np.cumsum(nc), [0], _np.cumsum(ec)]).astype(_np.int32), dev)     # one upload
        self.node_off, self.edge_off = offs[:self.G + 1], offs[self.G + 1:]
        self.complete = self._complete_flags() if keep_edges else None

    def _complete_flags(self):
        """uint8 [G]: 1 = the graph is COMPLETE (every ordered pair once, nothing else); the attention kernels then never read its edge list.
        Recomputed from the edge tensor's CONTENT on every call (one streaming pass; a caller may refill the same device buffer)."""
        if not _o.GAT_COMPLETE_FAST_PATH or self.G == 0 or self.edges is None or not self.edges.is_cuda:
            return None
        flags = torch.empty((self.G,), device=self.edges.device, dtype=torch.uint8)
        _lib.check(_lib.lib().sga_gat_complete_flags(_p(self.edges), _p(self.node_off), _p(self.edge_off), self.G, _p(flags), _stream()),
                   'sga_gat_complete_flags')
        return flags

    def sparse(self):
        """The canonical CSR structure of the batch for the sparse route (csrc/gat_sparse.hip), built on the device without a host read and
        kept on THIS object: every layer, head and pass of a step shares it."""
        sp = self.__dict__.get('_sparse')
        if sp is None:
            sp = self._sparse = SparseGraph(self)
        return sp

    _cache = _SmallCache(2)

    @staticmethod
    def of(data_dict):
        """Offsets are cached by the CONTENT of the two host count arrays + the identity of the device edge list (nothing is
        stored in the caller's dict).  The cached object keeps only the small offset arrays, never the edge tensor."""
        edges = data_dict['edges']
        if _o.VALIDATE:
            DEFERRED_CHECKS.poll()                                   # earlier batches' answers (no waiting): a bad batch raises here
        key = _fingerprint([_np.asarray(data_dict['graph_per_obj_count']), _np.asarray(data_dict['graph_per_edge_count'])],
                           (str(edges.device), edges.data_ptr(), tuple(edges.shape), str(edges.dtype)))
        proto = GraphBatch._cache.get(key, lambda: GraphBatch(data_dict['graph_per_obj_count'], data_dict['graph_per_edge_count'],
                                                              edges, keep_edges=False))
        gb = GraphBatch.__new__(GraphBatch)
        gb.__dict__.update(proto.__dict__)
        gb.edges = edges if edges.dtype == torch.int64 and edges.is_contiguous() else edges.to(torch.int64).contiguous()
        gb.complete = gb._complete_flags()
        return gb


def _gat_status_verdict(v):
    if v[0] == 0:
        return None
    return ('sgaligner_amd: a (source, target) edge occurs more than 255 times in one graph of the PREVIOUS batch; the GAT kernels count '
            'duplicate edges in 8 bits (PyG would count them all), so that step\'s structure embeddings were not PyG-equivalent -- '
            'deduplicate the edge list')


def _elu(x):
    y = torch.empty_like(x)
    _lib.check(_lib.lib().sga_elu_fwd(_p(x), _p(y), x.numel(), _stream()), 'sga_elu_fwd')
    return y


def gat_lds_nodes(channels, bwd=False):
    """Largest nodes-per-graph for which a head's [N, channels] features stay LDS-resident in the general attention kernels.  Not the answer
    for 2 heads x 128 channels: that shape launches kernels of its own, resident up to 128 nodes in both directions."""
    n = _lib.lib().sga_gat_lds_nodes(int(channels), int(bool(bwd)))
    if n < 0:
        _lib.check(1, 'sga_gat_lds_nodes')
    return n


def _ev_stop_attn(ev, which, h, heads, channels, gb, complete):
    # the benchmark's roofline rows read 2 x 128 launches under 'gat_attn_fwd' / 'gat_attn_bwd' with (T, E, complete)
    t, e = int(h.shape[0]), int(gb.edges.shape[0])
    if (heads, channels) == (2, 128):
        _ev_stop(ev, which, (t, e, complete is not None))
    else:
        _ev_stop(ev, which + '_hc', (t, e, heads, channels, complete is not None))


def _attn_fwd_hc(h, heads, channels, att_s, att_d, bias, gb, check_status=False):
    """The attention of `heads` heads of `channels` channels (h [T, heads * channels], head-major) over all graphs of gb in one launch."""
    out = torch.empty_like(h)
    st = None
    if check_status and _o.VALIDATE:
        # a FRESH status word per batch: a sticky shared one re-raised for clean batches whose read-back was enqueued before its reset
        st = torch.zeros((1,), device=h.device, dtype=torch.int32)
    complete = getattr(gb, 'complete', None)
    ev = _ev_start()
    _lib.check(_lib.lib().sga_gat_attn_fwd_hc(_p(h), heads, channels, _p(att_s), _p(att_d), _p(bias), _p(gb.edges), _p(gb.node_off),
                                              _p(gb.edge_off), gb.G, gb.nmax, _p(out), _p(st), _p(complete), _stream()), 'sga_gat_attn_fwd_hc')
    _ev_stop_attn(ev, 'gat_attn_fwd', h, heads, channels, gb, complete)
    if st is not None:            # read back without blocking; raises at the next batch's poll (or DEFERRED_CHECKS.flush())
        DEFERRED_CHECKS.submit_fn(st, _gat_status_verdict)
    return out


def _attn_bwd_hc(h, d_o, heads, channels, att_s, att_d, gb):
    dh = torch.empty_like(h)
    dboth = torch.empty((2,) + tuple(att_s.shape), device=att_s.device, dtype=att_s.dtype)      # adjacent: zeroed in one launch
    das, dad = dboth[0], dboth[1]
    complete = getattr(gb, 'complete', None)
    ev = _ev_start()
    _lib.check(_lib.lib().sga_gat_attn_bwd_hc(_p(h), _p(d_o), heads, channels, _p(att_s), _p(att_d), _p(gb.edges), _p(gb.node_off),
                                              _p(gb.edge_off), gb.G, gb.nmax, _p(dh), _p(das), _p(dad), _p(complete), _stream()),
               'sga_gat_attn_bwd_hc')
    _ev_stop_attn(ev, 'gat_attn_bwd', h, heads, channels, gb, complete)
    return dh, das, dad


def _gat_layer_forward(ctx, who, gb, x, w, att_s, att_d, bias, attn_fwd):
    """The part of a GATConv layer both routes share: checks, the projection on the GEMM, attn_fwd(h, heads, channels, att_s, att_d, bias, gb)."""
    if not x.is_cuda:
        raise RuntimeError(f'sgaligner_amd.{who}: HIP device tensor required; there is no CPU path')
    if att_s.dim() != 3 or att_s.shape != att_d.shape:
        raise RuntimeError(f'sgaligner_amd: att_src / att_dst must be [1, heads, channels], got {tuple(att_s.shape)} / {tuple(att_d.shape)}')
    heads, channels = int(att_s.shape[1]), int(att_s.shape[2])
    hc = heads * channels
    x = _req(x.contiguous(), 'gat.x')
    w, asf, adf, bias = [_req(t.contiguous(), n) for t, n in ((w, 'gat.lin'), (att_s.reshape(-1), 'gat.att_src'),
                                                              (att_d.reshape(-1), 'gat.att_dst'), (bias, 'gat.bias'))]
    t, f = int(x.shape[0]), int(x.shape[1])
    if t != gb.T:
        raise RuntimeError(f'sgaligner_amd: the GAT input has {t} rows but the graphs hold {gb.T} nodes')
    if tuple(w.shape) != (hc, f) or bias.numel() != hc:
        raise RuntimeError(f'sgaligner_amd: GATConv({f}, {channels}, heads={heads}) needs lin [{hc}, {f}] and bias [{hc}], '
                           f'got {tuple(w.shape)} and {tuple(bias.shape)}')
    h = gemm(x, w, False, True, t, hc, f)
    out = attn_fwd(h, heads, channels, asf, adf, bias, gb)
    ctx.gb, ctx.hc, ctx.att_shape = gb, (heads, channels), tuple(att_s.shape)
    ctx.save_for_backward(x, h, w, asf, adf)
    return out


def _gat_layer_backward(ctx, d_o, attn_bwd):
    """(dx or None, dW, d att_src, d att_dst, d bias) of a layer, attn_bwd(h, dO, heads, channels, att_s, att_d, gb) being its route's backward."""
    x, h, w, asf, adf = ctx.saved_tensors
    heads, channels = ctx.hc
    hc, (t, f) = heads * channels, x.shape
    d_o = d_o.contiguous()
    dh, das, dad = attn_bwd(h, d_o, heads, channels, asf, adf, ctx.gb)
    db = colsum(d_o)
    dw = gemm(dh, x, True, False, hc, f, t)
    dx = gemm(dh, w, False, False, t, f, hc) if ctx.needs_input_grad[1] else None
    return dx, dw, das.reshape(ctx.att_shape), dad.reshape(ctx.att_shape), db


class GATLayerFn(torch.autograd.Function):
    """One GATConv(in, channels, heads) over ALL graphs of a batch: the projection on the GEMM, then the general attention kernels.
    att_src / att_dst are PyG's [1, heads, channels].  The input gets a gradient only where it asks for one (not the first layer's)."""

    @staticmethod
    def forward(ctx, gb, x, w, att_s, att_d, bias, check_status):
        return _gat_layer_forward(ctx, 'GATLayerFn', gb, x, w, att_s, att_d, bias,
                                  lambda *a: _attn_fwd_hc(*a, check_status=check_status))

    @staticmethod
    def backward(ctx, d_o):
        return (None,) + _gat_layer_backward(ctx, d_o, _attn_bwd_hc) + (None,)


# ------------------------------------------------------------------------------------------ GAT, sparse route
ROUTES = ('dense', 'sparse', 'auto')
DENSE_MAX_NODES = 256          # nodes per graph the dense kernels take (their N x N multiplicity matrix lives in LDS)


class SparseGraph:
    """Canonical structure of a GraphBatch over batch-global node ids (rules of the dense kernels' prologue: input self loops and out-of-range
    endpoints dropped, one self loop per node, duplicates counted in 32 bits), all int32 HIP tensors of capacity cap = E + T:
      row_ptr [T+1], src, mult      target-major, the sources of a target ascending
      col_ptr [T+1], tgt, perm      the transpose, the targets of a source ascending; perm indexes the target-major entry
    U = row_ptr[T] entries are used; U stays on the device.  Keys from a kernel, torch.sort, kernels for the run-length compaction behind a
    torch.cumsum (the form of utils/voxel.py); nothing is read back."""

    def __init__(self, gb):
        L = _lib.lib()
        if gb.edges is None:
            raise RuntimeError('sgaligner_amd: this GraphBatch holds no edge list')
        dev, T, E = gb.edges.device, gb.T, gb.E
        cap = L.sga_gat_sp_capacity(T, E)
        if cap < 0:
            _lib.check(1, 'sga_gat_sp_capacity')
        self.T, self.cap = T, cap
        i32 = lambda n: torch.empty((n,), device=dev, dtype=torch.int32)
        self.row_ptr, self.src, self.mult = i32(T + 1), i32(cap), i32(cap)
        self.col_ptr, self.tgt, self.perm = i32(T + 1), i32(cap), i32(cap)
        s = _stream()
        ev = _ev_start()
        keys = torch.empty((cap,), device=dev, dtype=torch.int64)
        _lib.check(L.sga_gat_sp_keys(_p(gb.edges), _p(gb.node_off), _p(gb.edge_off), gb.G, T, E, _p(keys), s), 'sga_gat_sp_keys')
        skeys = torch.sort(keys)[0]
        head = i32(cap)
        _lib.check(L.sga_gat_sp_heads(_p(skeys), cap, _p(head), s), 'sga_gat_sp_heads')
        incl = torch.cumsum(head, 0, dtype=torch.int32)
        keys_t = torch.empty((cap,), device=dev, dtype=torch.int64)
        ws = torch.empty((L.sga_gat_sp_build_workspace_bytes(cap),), device=dev, dtype=torch.uint8)
        _lib.check(L.sga_gat_sp_rows(_p(skeys), _p(incl), cap, T, _p(self.row_ptr), _p(self.src), _p(self.mult), _p(keys_t), _p(ws), ws.numel(), s),
                   'sga_gat_sp_rows')
        skeys_t, order_t = torch.sort(keys_t)
        _lib.check(L.sga_gat_sp_cols(_p(skeys_t), _p(order_t), cap, T, _p(self.col_ptr), _p(self.tgt), _p(self.perm), s), 'sga_gat_sp_cols')
        _ev_stop(ev, 'gat_sp_build', (T, E))

    def dinv(self):
        """deg^-1/2 per node [T] for the GCN over this structure (csrc/gcn_sparse.hip: deg = the row's multiplicities summed, the self loop
        counting 1; correctly rounded).  Computed at the first call and kept: a GAT batch never pays for it."""
        d = self.__dict__.get('_dinv')
        if d is None:
            d = torch.empty((self.T,), device=self.row_ptr.device, dtype=torch.float32)
            _lib.check(_lib.lib().sga_gcn_sp_dinv(_p(self.row_ptr), _p(self.mult), self.T, self.cap, _p(d), _stream()), 'sga_gcn_sp_dinv')
            self._dinv = d
        return d


def _sp_workspace(sp, heads, channels, bwd, dev):
    n = _lib.lib().sga_gat_sp_workspace_bytes(sp.T, sp.cap, heads, channels, int(bwd))
    if n == 0 and sp.T:
        _lib.check(1, 'sga_gat_sp_workspace_bytes')
    return torch.empty((n,), device=dev, dtype=torch.uint8)


def _attn_fwd_sp(h, heads, channels, att_s, att_d, bias, gb):
    """_attn_fwd_hc on the sparse route: no limit on the nodes of a graph, no status word (32-bit multiplicities)."""
    sp = gb.sparse()
    out = torch.empty_like(h)
    ws = _sp_workspace(sp, heads, channels, False, h.device)
    ev = _ev_start()
    _lib.check(_lib.lib().sga_gat_sp_fwd(_p(h), heads, channels, _p(att_s), _p(att_d), _p(bias), _p(sp.row_ptr), _p(sp.src), _p(sp.mult), sp.T,
                                         _p(out), _p(ws), ws.numel(), _stream()), 'sga_gat_sp_fwd')
    _ev_stop(ev, 'gat_sp_fwd', (int(h.shape[0]), sp.cap, heads, channels))
    return out


def _attn_bwd_sp(h, d_o, heads, channels, att_s, att_d, gb):
    sp = gb.sparse()
    dh = torch.empty_like(h)
    dboth = torch.empty((2,) + tuple(att_s.shape), device=att_s.device, dtype=att_s.dtype)
    das, dad = dboth[0], dboth[1]
    ws = _sp_workspace(sp, heads, channels, True, h.device)
    ev = _ev_start()
    _lib.check(_lib.lib().sga_gat_sp_bwd(_p(h), _p(d_o), heads, channels, _p(att_s), _p(att_d), _p(sp.row_ptr), _p(sp.src), _p(sp.mult),
                                         _p(sp.col_ptr), _p(sp.tgt), _p(sp.perm), sp.T, sp.cap, _p(dh), _p(das), _p(dad), _p(ws), ws.numel(),
                                         _stream()), 'sga_gat_sp_bwd')
    _ev_stop(ev, 'gat_sp_bwd', (int(h.shape[0]), sp.cap, heads, channels))
    return dh, das, dad


class GATLayerSparseFn(torch.autograd.Function):
    """GATLayerFn on the sparse route: the projection on the GEMM, then the CSR attention kernels."""

    @staticmethod
    def forward(ctx, gb, x, w, att_s, att_d, bias):
        return _gat_layer_forward(ctx, 'GATLayerSparseFn', gb, x, w, att_s, att_d, bias, _attn_fwd_sp)

    @staticmethod
    def backward(ctx, d_o):
        return (None,) + _gat_layer_backward(ctx, d_o, _attn_bwd_sp)


def resolve_route(route, gb=None):
    """'dense' | 'sparse' | 'auto' -> 'dense' | 'sparse'.  'auto' is sparse exactly when a graph of the batch has more nodes than the dense
    kernels take -- decided from gb.nmax, a host number."""
    if route not in ROUTES:
        raise ValueError(f"sgaligner_amd: route must be one of {ROUTES}, got {route!r}")
    if route == 'auto':
        return 'sparse' if gb is not None and gb.nmax > DENSE_MAX_NODES else 'dense'
    return route


class EluFn(torch.autograd.Function):
    """F.elu between the layers (gat.py:45-46) on sga_elu_fwd / sga_elu_bwd."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return _elu(x)

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().sga_elu_bwd(_p(x), _p(gy), _p(gx), x.numel(), _stream()), 'sga_elu_bwd')
        return gx


def multi_gat_layers(gb, x, layers, p=0.0, training=False, masks=None, route='dense'):
    """MultiGAT.forward (gat.py:40-48) for a stack of any depth: dropout on the input of every layer, GATConv, ELU between layers.
    layers: (lin_weight, att_src [1, H, C], att_dst, bias) per layer.  masks: one [T, in_width] tensor per layer, already scaled by
    1 / (1 - p) -- it replaces the draw; otherwise, training with p > 0, torch.nn.functional.dropout draws once per layer in layer order.
    route: 'dense' (at most 256 nodes per graph), 'sparse' (the CSR kernels: graphs of any size, no atomics) or 'auto' (sparse exactly when
    gb.nmax > 256)."""
    sparse = resolve_route(route, gb) == 'sparse'
    if not x.is_cuda:
        raise RuntimeError('sgaligner_amd.multi_gat_layers: HIP device tensor required; there is no CPU path')
    if x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f'sgaligner_amd.multi_gat_layers: tot_rel_pose must be float32 or float64, got {x.dtype}')
    if masks is not None and len(masks) != len(layers):
        raise RuntimeError(f'sgaligner_amd.multi_gat_layers: {len(masks)} dropout masks for {len(layers)} layers')
    x = cast_f32(x.contiguous())
    for i, layer in enumerate(layers):
        if masks is not None:
            x = x * masks[i]
        elif training and p > 0.0:
            x = torch.nn.functional.dropout(x, p, True)
        if sparse:
            x = GATLayerSparseFn.apply(gb, x, *layer)
        else:
            x = GATLayerFn.apply(gb, x, *layer, i == 0)      # every layer sees the same edge list: one multiplicity check per batch
        if i + 1 < len(layers):
            x = EluFn.apply(x)
    return x
