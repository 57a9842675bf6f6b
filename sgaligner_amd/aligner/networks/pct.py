"""Point-Cloud-Transformer object encoder -- drop-in for the reference's `NaivePCT` (src/aligner/networks/pct.py:
275-317, with `Embedding` :101-125 and `SA` :187-232; selected by `modules: ['pct', ...]`,
configs/scan3r/scan3r_ground_truth.yaml:5), its offset attention `OA` (:234-273) and the encoder built on it, `SPCT`
(:319-351).  Same class names, constructor signatures, sub-module names and state_dict keys, so reference checkpoints
load with strict=True.  `NaivePCT(attention='oa')` puts SPCT's trunk (four OA layers) under NaivePCT's head; the keys
are the same either way, and the default 'sa' is the reference's NaivePCT.

Eval mode (inference): per-point convolutions as exact-fp32 MFMA GEMMs with the eval-mode BatchNorm folded into
weight/bias (sga_gemm_ex), the self-attention flash style (sga_pct_attention), the point max (sga_segment_max);
Dropout is the identity; no autograd graph.
Train mode: the same computation as differentiable HIP ops (sgaligner_amd.pct_ops): GEMM forward/backward, BatchNorm
with BATCH statistics over all objects x points (running statistics updated as nn.BatchNorm1d does) fused with the
activation / SA residual, attention forward + backward, arg-max routed point max; the two Dropout(0.5) of the head
draw their masks from torch's device RNG (F.dropout on the [T, 512] / [T, 256] tensors -- the reference's CPU/CUDA
streams cannot be reproduced anyway, parity is tested with p = 0).  Activations are materialised point-major
([T*N, C] fp32, the widest is [T*N, 1024]): sized for the reference's batch sizes, not for configs[1]'s 65 536 objects.
"""
import torch
import torch.nn as nn

from ... import _lib
from ...ops import _p, _stream


def _gemm_ex(a, w, bias, act=0, resid=None, out=None):
    """out[m, n] = act(a[m, k] @ w[n, k]^T + bias) (+ resid);  a / out / resid may be column slices of wider buffers."""
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    rc = _lib.lib().sga_gemm_ex(0, 1, m, n, k, _p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), _p(bias),
                                act, _p(resid), resid.stride(0) if resid is not None else 0, _stream())
    _lib.check(rc, 'sga_gemm_ex')
    return out


def _fold(conv_w, conv_b, bn):
    """conv1d(k=1) / linear followed by an eval-mode BatchNorm1d -> one affine map: W' = s W, b' = s (b - mean) + beta,
    s = gamma / sqrt(running_var + eps).  Tiny tensors; done on the device with torch ops once per forward."""
    w = conv_w.reshape(conv_w.shape[0], -1).float()
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    b = -bn.running_mean if conv_b is None else conv_b - bn.running_mean
    return (w * s[:, None]).contiguous(), (b * s + bn.bias).contiguous()


class Embedding(nn.Module):
    """pct.py:101-125: two Conv1d(k=1, bias=False) + BatchNorm + ReLU layers."""

    def __init__(self, in_channels=3, out_channels=128):
        super().__init__()
        self.conv1 = nn.Conv1d(in_channels, out_channels, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(out_channels, out_channels, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(out_channels)
        self.bn2 = nn.BatchNorm1d(out_channels)

    def forward_rows(self, x_rows):
        """x_rows [T*N, in] point-major -> [T*N, out]."""
        w1, b1 = _fold(self.conv1.weight, None, self.bn1)
        w2, b2 = _fold(self.conv2.weight, None, self.bn2)
        h = _gemm_ex(x_rows, w1, b1, act=1)
        return _gemm_ex(h, w2, b2, act=1)


class SA(nn.Module):
    """pct.py:187-232.  q_conv and k_conv share one weight tensor (:199) -- both keys appear in the state_dict."""

    def __init__(self, channels):
        super().__init__()
        self.da = channels // 4
        self.q_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv = nn.Conv1d(channels, channels, 1)
        self.trans_conv = nn.Conv1d(channels, channels, 1)
        self.after_norm = nn.BatchNorm1d(channels)
        self.act = nn.ReLU()
        self.softmax = nn.Softmax(dim=-1)

    def forward_rows(self, x_rows, n_obj, n_pts, out):
        """x_rows [T*N, 128] (may be a column slice) -> out (column slice) = x + relu(bn(trans_conv(x_v @ attention)))."""
        if self.q_conv.weight.data_ptr() != self.k_conv.weight.data_ptr() and not torch.equal(self.q_conv.weight, self.k_conv.weight):
            raise RuntimeError('sgaligner_amd SA: q_conv / k_conv weights differ; the HIP attention relies on the shared '
                               'weight of the reference (pct.py:199) for a symmetric energy matrix')
        if self.da != 32 or x_rows.shape[1] != 128:
            raise NotImplementedError('sgaligner_amd SA: channels must be 128 (NaivePCT)')
        dev = x_rows.device
        q = _gemm_ex(x_rows, self.k_conv.weight.reshape(self.da, -1), None)
        v = _gemm_ex(x_rows, self.v_conv.weight.reshape(128, -1), self.v_conv.bias)
        stats = torch.empty((2 * n_obj * n_pts,), device=dev, dtype=torch.float32)
        xs = torch.empty((n_obj * n_pts, 128), device=dev, dtype=torch.float32)
        rc = _lib.lib().sga_pct_attention(_p(q), q.stride(0), _p(v), v.stride(0), n_obj, n_pts, _p(stats), _p(xs), xs.stride(0), _stream())
        _lib.check(rc, 'sga_pct_attention')
        wt, bt = _fold(self.trans_conv.weight, self.trans_conv.bias, self.after_norm)
        return _gemm_ex(xs, wt, bt, act=1, resid=x_rows, out=out)

    def forward_autograd(self, h, t, n):
        """The differentiable form of forward_rows (pct_ops): h [T*N, 128] -> [T*N, 128]."""
        import torch.nn.functional as F
        from ... import pct_ops as P
        if self.q_conv.weight is not self.k_conv.weight and not torch.equal(self.q_conv.weight, self.k_conv.weight):
            raise RuntimeError('sgaligner_amd SA: q_conv / k_conv weights differ (pct.py:199 ties them)')
        # q (= q_conv(x) = k_conv(x): one shared weight, no bias) and v as ONE N = 160 GEMM over x
        wqv = torch.cat([self.k_conv.weight.reshape(self.k_conv.weight.shape[0], -1), self.v_conv.weight.reshape(128, -1)])
        bqv = F.pad(self.v_conv.bias, (wqv.shape[0] - 128, 0))
        a = P.pct_attention_qv(P.rows_linear(h, wqv, bqv), t, n) if wqv.shape[0] == 160 else \
            P.pct_attention(P.rows_linear(h, self.k_conv.weight), P.rows_linear(h, self.v_conv.weight, self.v_conv.bias), t, n)
        return P.batch_norm_act(P.rows_linear(a, self.trans_conv.weight, self.trans_conv.bias, bn_stats=True), self.after_norm, act=1, resid=h)


class OA(nn.Module):
    """pct.py:234-273, offset attention: the row softmax of q k^T (no 1/sqrt(da)) L1-normalised over its columns, and trans_conv applied
    to x - x_r.  q_conv and k_conv share one weight tensor (:244) -- both keys appear in the state_dict."""

    def __init__(self, channels):
        super().__init__()
        self.q_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv = nn.Conv1d(channels, channels, 1)
        self.trans_conv = nn.Conv1d(channels, channels, 1)
        self.after_norm = nn.BatchNorm1d(channels)
        self.act = nn.ReLU()
        self.softmax = nn.Softmax(dim=-1)

    def _check(self, width):
        if self.q_conv.weight is not self.k_conv.weight and not torch.equal(self.q_conv.weight, self.k_conv.weight):
            raise RuntimeError('sgaligner_amd OA: q_conv / k_conv weights differ; the HIP attention relies on the shared '
                               'weight of the reference (pct.py:244) for a symmetric energy matrix')
        if self.k_conv.weight.shape[0] != 32 or width != 128:
            raise NotImplementedError('sgaligner_amd OA: channels must be 128 (SPCT / NaivePCT)')

    def forward_rows(self, x_rows, n_obj, n_pts, out):
        """x_rows [T*N, 128] (may be a column slice) -> out (column slice) = x + relu(bn(trans_conv(x - x_r)))."""
        self._check(x_rows.shape[1])
        dev = x_rows.device
        q = _gemm_ex(x_rows, self.k_conv.weight.reshape(32, -1), None)
        v = _gemm_ex(x_rows, self.v_conv.weight.reshape(128, -1), self.v_conv.bias)
        stats = torch.empty((3 * n_obj * n_pts,), device=dev, dtype=torch.float32)
        xr = torch.empty((n_obj * n_pts, 128), device=dev, dtype=torch.float32)
        diff = torch.empty((n_obj * n_pts, 128), device=dev, dtype=torch.float32)
        rc = _lib.lib().sga_pct_offset_attention(_p(q), q.stride(0), _p(v), v.stride(0), _p(x_rows), x_rows.stride(0), n_obj, n_pts, _p(stats),
                                                 _p(xr), xr.stride(0), _p(diff), diff.stride(0), _stream())
        _lib.check(rc, 'sga_pct_offset_attention')
        wt, bt = _fold(self.trans_conv.weight, self.trans_conv.bias, self.after_norm)
        return _gemm_ex(diff, wt, bt, act=1, resid=x_rows, out=out)

    def forward_autograd(self, h, t, n):
        import torch.nn.functional as F
        from ... import pct_ops as P
        self._check(h.shape[1])
        wqv = torch.cat([self.k_conv.weight.reshape(32, -1), self.v_conv.weight.reshape(128, -1)])
        bqv = F.pad(self.v_conv.bias, (32, 0))
        d = P.pct_offset_attention_qv(P.rows_linear(h, wqv, bqv), t, n, x=h)                 # x - x_r, from the attention kernel itself
        return P.batch_norm_act(P.rows_linear(d, self.trans_conv.weight, self.trans_conv.bias, bn_stats=True), self.after_norm, act=1, resid=h)

    def forward(self, x):
        """x [T, 128, N] as in the reference -> [T, 128, N] (a permuted view of the point-major result)."""
        if not x.is_cuda:
            raise RuntimeError('sgaligner_amd OA: input must be on the HIP device (no CPU path)')
        t, c, n = x.shape
        rows = x.permute(0, 2, 1).reshape(t * n, c).float()
        if self.training or torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            y = self.forward_autograd(rows, t, n)
        else:
            with torch.no_grad():
                y = self.forward_rows(rows, t, n, None)
        return y.view(t, n, c).permute(0, 2, 1)


def _rows_of(x):
    """x [T, 3, N] as in the reference (a permuted view of data_dict['tot_obj_pts'] [T,N,3]) -> (point-major rows [T*N, 3], T, N)."""
    xt = x.permute(0, 2, 1)
    if not xt.is_contiguous():
        xt = xt.contiguous()
    t, n, _ = xt.shape
    return xt.reshape(t * n, 3).float(), t, n


def _trunk_eval(m, rows, t, n):
    """Embedding and the four attention layers sa1..sa4 (SA or OA) of `m`, eval mode: cat = x1 | x2 | x3 | x4 [T*N, 512] (pct.py:302, :343)."""
    h = m.embedding.forward_rows(rows)
    cat = torch.empty((t * n, 512), device=rows.device, dtype=torch.float32)
    src = h
    for k, sa in enumerate((m.sa1, m.sa2, m.sa3, m.sa4)):
        dst = cat[:, 128 * k:128 * (k + 1)]
        sa.forward_rows(src, t, n, dst)
        src = dst
    return cat


def _trunk_autograd(m, rows, t, n):
    """The same through the differentiable ops (pct_ops)."""
    from ... import pct_ops as P
    e = m.embedding
    h = P.batch_norm_act(P.rows_linear(rows, e.conv1.weight, bn_stats=True), e.bn1, act=1)
    h = P.batch_norm_act(P.rows_linear(h, e.conv2.weight, bn_stats=True), e.bn2, act=1)
    xs = []
    for sa in (m.sa1, m.sa2, m.sa3, m.sa4):
        h = sa.forward_autograd(h, t, n)
        xs.append(h)
    return torch.cat(xs, dim=1)


class SPCT(nn.Module):
    """pct.py:319-351: Embedding, four OA layers named sa1..sa4, the 512 -> 1024 stage; forward returns (x [T,1024,N], x_max, x_mean).
    x is a permuted view of the point-major activation [T*N, 1024]; x_max is sga_segment_max, x_mean sga_segment_mean (fixed order)."""

    def __init__(self):
        super().__init__()
        self.embedding = Embedding(3, 128)
        self.sa1 = OA(128)
        self.sa2 = OA(128)
        self.sa3 = OA(128)
        self.sa4 = OA(128)
        self.linear = nn.Sequential(nn.Conv1d(512, 1024, kernel_size=1, bias=False), nn.BatchNorm1d(1024),
                                    nn.LeakyReLU(negative_slope=0.2))

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('sgaligner_amd SPCT: input must be on the HIP device (no CPU path)')
        rows, t, n = _rows_of(x)
        if self.training or torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from ... import pct_ops as P
            cat = _trunk_autograd(self, rows, t, n)
            y = P.batch_norm_act(P.rows_linear(cat, self.linear[0].weight, bn_stats=True), self.linear[1], act=2)
            x_max, x_mean = P.segment_max(y, t, n), P.segment_mean(y, t, n)
        else:
            with torch.no_grad():
                cat = _trunk_eval(self, rows, t, n)
                w5, b5 = _fold(self.linear[0].weight, None, self.linear[1])
                y = _gemm_ex(cat, w5, b5, act=2)
                x_max = torch.empty((t, 1024), device=y.device, dtype=torch.float32)
                x_mean = torch.empty((t, 1024), device=y.device, dtype=torch.float32)
                _lib.check(_lib.lib().sga_segment_max(_p(y), y.stride(0), t, n, 1024, _p(x_max), None, _stream()), 'sga_segment_max')
                _lib.check(_lib.lib().sga_segment_mean(_p(y), y.stride(0), t, n, 1024, _p(x_mean), _stream()), 'sga_segment_mean')
        return y.view(t, n, 1024).permute(0, 2, 1), x_max, x_mean


class NaivePCT(nn.Module):
    """pct.py:275-317.  attention: 'sa' (the reference's NaivePCT) or 'oa' (SPCT's trunk, pct.py:323-328, under the same head)."""

    def __init__(self, attention='sa'):
        super().__init__()
        if attention not in ('sa', 'oa'):
            raise ValueError(f"sgaligner_amd NaivePCT: attention must be 'sa' or 'oa', not {attention!r}")
        self.attention = attention
        layer = SA if attention == 'sa' else OA
        self.embedding = Embedding(3, 128)
        self.sa1 = layer(128)
        self.sa2 = layer(128)
        self.sa3 = layer(128)
        self.sa4 = layer(128)
        self.linear = nn.Sequential(nn.Conv1d(512, 1024, kernel_size=1, bias=False), nn.BatchNorm1d(1024),
                                    nn.LeakyReLU(negative_slope=0.2))
        self.linear1 = nn.Linear(1024, 512, bias=False)
        self.linear2 = nn.Linear(512, 256)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.dp1 = nn.Dropout(p=0.5)
        self.dp2 = nn.Dropout(p=0.5)
        self.fused_head = True               # tests flip it to cross-check the two backward formulations of the widest stage
        self._check_gamma = False            # True: test |gamma| > 1e-3 before every fused training step (one host read-back per step)
        self.eval_chunk_rows = 1 << 19       # inference: points per chunk (x 1024 channels x 4 B = 2 GiB for the widest activation)

    def forward(self, x):
        """x [T, 3, N] as in the reference (a permuted view of data_dict['tot_obj_pts'] [T,N,3]) -> [T, 256]."""
        if not x.is_cuda:
            raise RuntimeError('sgaligner_amd NaivePCT: input must be on the HIP device (no CPU path)')
        rows, t, n = _rows_of(x)
        if self.training or torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_autograd(rows, t, n)
        with torch.no_grad():
            # objects are independent in eval mode (running-statistic BatchNorm), so the batch is walked in chunks that
            # keep the widest activation ([chunk*N, 1024] fp32) around 2 GiB -- configs[1]'s 65 536 objects x 512 points
            # would otherwise need 137 GB for that tensor alone
            chunk = max(1, self.eval_chunk_rows // max(n, 1))
            if t > chunk:
                outs = [self._forward_eval_rows(rows[c * n:min(t, c + chunk) * n], min(t, c + chunk) - c, n) for c in range(0, t, chunk)]
                return torch.cat(outs)
            return self._forward_eval_rows(rows, t, n)

    def _forward_eval_rows(self, rows, t, n):
        with torch.no_grad():
            x = rows
            cat = _trunk_eval(self, rows, t, n)                                        # x1 | x2 | x3 | x4 (pct.py:302)
            w5, b5 = _fold(self.linear[0].weight, None, self.linear[1])
            y = _gemm_ex(cat, w5, b5, act=2)                                           # LeakyReLU(0.2)
            g = torch.empty((t, 1024), device=x.device, dtype=torch.float32)
            _lib.check(_lib.lib().sga_segment_max(_p(y), y.stride(0), t, n, 1024, _p(g), None, _stream()), 'sga_segment_max')
            w6, b6 = _fold(self.linear1.weight, None, self.bn1)
            w7, b7 = _fold(self.linear2.weight, self.linear2.bias, self.bn2)
            f = _gemm_ex(g, w6, b6, act=1)
            return _gemm_ex(f, w7, b7, act=1)

    # ---- differentiable path (train mode, or eval mode with gradients enabled) -------------------------------------
    def _forward_autograd(self, rows, t, n):
        import torch.nn.functional as F
        from ... import pct_ops as P
        cat = _trunk_autograd(self, rows, t, n)
        # The fused node's sparse backward pass (sga_pct_head_scatter) is built for <= 1024 points per object and <= 1024 channels, and it
        # recovers x_hat from the pooled output as (z - beta) / gamma: objects with more points and a BatchNorm whose |gamma| has collapsed
        # take the chain of separate nodes (same numbers, more memory) instead of failing or dividing by ~0 in backward.
        fused_ok = self.fused_head and n <= 1024 and self.linear[0].weight.shape[0] <= 1024
        if fused_ok and torch.is_grad_enabled() and self.linear[1].weight.requires_grad:
            fused_ok = bool((self.linear[1].weight.detach().abs().min() > 1e-3).item()) if self._check_gamma else True
        if fused_ok:      # conv + BatchNorm + LeakyReLU + point max as one node with the algebraic backward (pct_ops.LinearBNActMaxFn)
            g = P.linear_bn_lrelu_max(cat, self.linear[0].weight, self.linear[1], t, n)
        else:
            y = P.batch_norm_act(P.rows_linear(cat, self.linear[0].weight, bn_stats=True), self.linear[1], act=2)
            g = P.segment_max(y, t, n)
        f = P.batch_norm_act(P.rows_linear(g, self.linear1.weight, bn_stats=True), self.bn1, act=1)
        f = F.dropout(f, self.dp1.p, self.training)
        f = P.batch_norm_act(P.rows_linear(f, self.linear2.weight, self.linear2.bias, bn_stats=True), self.bn2, act=1)
        return F.dropout(f, self.dp2.p, self.training)
