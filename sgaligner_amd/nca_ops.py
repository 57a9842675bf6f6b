"""NCA loss of the EVA baseline (reference src/aligner/losses.py:154-205) on csrc/nca.hip and the library's GEMMs.

Per table: the anchor rows are gathered and L2-normalised once (sga_loss_gather: Z [2A, Dp], Dp = D padded to 8), then the A x A score
matrix s = Z1 Z2^T is walked in row blocks of [h, A] sized by the stash budget (ops._stash_bytes()):
  forward    per block: GEMM, row sums / diagonal / column partials (sga_nca_block_sums); then sga_nca_loss folds them into the loss
  backward   per block: the coefficient block g and its transpose (sga_nca_coef), dZ1[block] = g Z2 and dZ2 += g^T Z1[block] (two GEMMs),
             then sga_loss_scatter takes dZ back to the table through the normalisation's Jacobian
When all A rows fit one block the forward's scores are kept for the backward; otherwise the backward forms each block again.
Every reduction has a fixed order (the GEMM calls are kept below the K at which the library splits K with atomics): loss, dZ1 and dZ2 are
bitwise repeatable.  Single device: a data_dict that carries `_sga_shard` raises."""
from __future__ import annotations

import numpy as _np
import torch

from . import _lib
from .ops import _SmallCache, _fingerprint, _h2d, _p, _req, _stash_bytes, _stream, gemm
from . import ops as _o

_K_NOSPLIT = 4064          # sga_gemm splits K (atomic partial sums) from K = 4096 on when its output grid is small: stay below, in whole 32-chunks


def _gemm_fixed(a, b, m, n, k, out, accumulate=False):
    """out (+)= a [m,k] @ b [k,n] with K walked in chunks the library never splits: a fixed order of additions."""
    for k0 in range(0, k, _K_NOSPLIT):
        k1 = min(k, k0 + _K_NOSPLIT)
        gemm(a[:, k0:k1], b[k0:k1], False, False, m, n, k1 - k0, out=out, accumulate=accumulate or k0 > 0)
    return out


def _row_blocks(A):
    """Row blocks [lo, hi) of the A x A scores: the block [h, A] and its transposed coefficient copy inside the stash budget."""
    h = max(1, min(A, _stash_bytes() // (8 * max(A, 1))))           # (a kept single block has a third copy beside it: the coefficients)
    if h < A and h >= 32:
        h -= h % 32
    return [(lo, min(A, lo + h)) for lo in range(0, A, h)]


_idx_cache = _SmallCache()


def _anchor_index(data_dict, device, n_rows):
    arrs = [_np.ascontiguousarray(_np.asarray(data_dict[k]).astype(_np.int32)).reshape(-1) for k in ('e1i', 'e2i')]
    if arrs[0].shape != arrs[1].shape:
        raise RuntimeError('sgaligner_amd: e1i and e2i must have the same length')

    def make():
        host = _np.concatenate(arrs)
        if _o.VALIDATE and host.size:
            lo, hi = int(host.min()), int(host.max())
            if lo < 0 or hi >= n_rows:
                raise RuntimeError(f'sgaligner_amd: e1i/e2i hold object indices in [{lo}, {hi}] but the embedding tables have {n_rows} rows')
        return _h2d(host, device)
    return _idx_cache.get(_fingerprint(arrs, (str(device), n_rows)), make), int(arrs[0].shape[0])


def _r4(n):
    return (n + 3) // 4 * 4


def _nca_forward(e, idx, A, alpha, beta, ep, keep):
    """(loss [1] float64, state for _nca_backward or None).  The anchor rows sit in z [2 Ap, Dp] as Z1 | Z2 with A padded to Ap, a
    multiple of 4, by zero rows: every GEMM below then has aligned operands and a K that is a multiple of 4."""
    T, D = e.shape
    dev = e.device
    L, st = _lib.lib(), _stream()
    dp = (D + 7) // 8 * 8
    ap = _r4(A)
    z = torch.zeros((2 * ap, dp), device=dev, dtype=torch.float32)
    nrm = torch.empty((2 * ap,), device=dev, dtype=torch.float32)
    for half in (0, 1):
        _lib.check(L.sga_loss_gather(_p(e), T, D, _p(idx[half * A:]), A, _p(z[half * ap:]), dp, _p(nrm[half * ap:]), st), 'sga_loss_gather')
    blocks = _row_blocks(A)
    rg = L.sga_nca_row_group()
    ngroups = sum((hi - lo + rg - 1) // rg for lo, hi in blocks)
    hmax = max(hi - lo for lo, hi in blocks)
    s = torch.empty((hmax, ap), device=dev, dtype=torch.float32)
    rsum = torch.empty((A,), device=dev, dtype=torch.float64)
    csum = torch.empty((A,), device=dev, dtype=torch.float64)
    cpart = torch.empty((ngroups, A), device=dev, dtype=torch.float64)
    diag = torch.empty((A,), device=dev, dtype=torch.float32)
    inv = torch.empty((2, A), device=dev, dtype=torch.float32)
    loss = torch.empty((1,), device=dev, dtype=torch.float64)
    g0 = 0
    for lo, hi in blocks:
        h = hi - lo
        gemm(z[lo:hi], z[ap:], False, True, h, ap, dp, out=s)
        _lib.check(L.sga_nca_block_sums(_p(s), ap, h, A, lo, alpha, ep, _p(rsum), _p(diag), _p(cpart[g0]), st), 'sga_nca_block_sums')
        g0 += (h + rg - 1) // rg
    _lib.check(L.sga_nca_loss(_p(rsum), _p(cpart), ngroups, _p(diag), A, alpha, beta, _p(csum), _p(inv[0]), _p(inv[1]), _p(loss), st),
               'sga_nca_loss')
    state = None
    if keep:
        state = dict(z=z, nrm=nrm, idx=idx, inv=inv, s=s if len(blocks) == 1 else None, cfg=(A, T, D, dp, alpha, beta, ep, blocks))
    return loss, state


def _nca_backward(state, gout):
    """dz [2 Ap, Dp] = dloss/dZ1 | dloss/dZ2 (rows A .. Ap of each half stay zero) times gout (a 1-element float64 device tensor)."""
    z, inv, s = state['z'], state['inv'], state['s']
    A, T, D, dp, alpha, beta, ep, blocks = state['cfg']
    dev = z.device
    L, st = _lib.lib(), _stream()
    ap = _r4(A)
    hmax = max(hi - lo for lo, hi in blocks)
    ldt = _r4(hmax)
    kept = s is not None
    # the coefficient block: beside the kept scores (they stay as they are: a second backward over a retained graph finds them), or in
    # place in a block formed again here; columns A .. ap must be zero for the K = ap product
    g = (torch.zeros if kept else torch.empty)((hmax, ap), device=dev, dtype=torch.float32)       # (formed again: the GEMM writes those columns)
    if not kept:
        s = g
    gt = torch.empty((A, ldt), device=dev, dtype=torch.float32)
    dz = torch.zeros((2 * ap, dp), device=dev, dtype=torch.float32)
    for n, (lo, hi) in enumerate(blocks):
        h = hi - lo
        if not kept:
            gemm(z[lo:hi], z[ap:], False, True, h, ap, dp, out=s)
        _lib.check(L.sga_nca_coef(_p(s), ap, _p(g), ap, _p(gt), ldt, h, A, lo, alpha, beta, ep, _p(inv[0]), _p(inv[1]), _p(gout), st),
                   'sga_nca_coef')
        _gemm_fixed(g[:h], z[ap:], h, dp, ap, dz[lo:hi])                                       # dZ1[block] = g Z2
        # dZ2 (+)= g^T Z1[block]; K = h rounded up to 4: gt's extra columns are zero, the rows of z they meet are finite
        _gemm_fixed(gt[:, :_r4(h)], z[lo:lo + _r4(h)], A, dp, _r4(h), dz[ap:ap + A], accumulate=n > 0)
    return dz


class NCAFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, idx, A, alpha, beta, ep):
        e = _req(emb.contiguous(), 'embedding table')
        loss, ctx.state = _nca_forward(e, idx, A, alpha, beta, ep, keep=ctx.needs_input_grad[0])
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        state = ctx.state
        A, T, D, dp = state['cfg'][:4]
        z, nrm, idx = state['z'], state['nrm'], state['idx']
        ap = _r4(A)
        L, st = _lib.lib(), _stream()
        dz = _nca_backward(state, gout.to(torch.float64).reshape(1).contiguous())
        de = torch.zeros((T, D), device=z.device, dtype=torch.float32)
        for half in (0, 1):
            o = half * ap
            _lib.check(L.sga_loss_scatter(_p(dz[o:]), _p(z[o:]), _p(nrm[o:]), _p(idx[half * A:]), A, D, dp, _p(de), st), 'sga_loss_scatter')
        return de, None, None, None, None, None


def nca_loss(emb, data_dict, alpha=1.0, beta=1.0, ep=0.0):
    """NCALoss(alpha, beta, ep) of F.normalize(emb)[e1i] against F.normalize(emb)[e2i] (losses.py:161-173,189-198): a 0-d float64 tensor."""
    if not isinstance(emb, torch.Tensor) or not emb.is_cuda:
        raise RuntimeError('sgaligner_amd.nca_loss: HIP device tensor required; there is no CPU path')
    if isinstance(data_dict, dict) and data_dict.get('_sga_shard') is not None:
        raise RuntimeError('sgaligner_amd.nca_loss: the NCA loss is single-device; a data_dict that carries `_sga_shard` is not supported')
    if emb.dim() != 2 or emb.shape[1] < 1:
        raise RuntimeError(f'sgaligner_amd.nca_loss: the embedding table must be [T, D], got {tuple(emb.shape)}')
    if not alpha > 0:
        raise RuntimeError('sgaligner_amd.nca_loss: alpha must be positive')
    idx, A = _anchor_index(data_dict, emb.device, int(emb.shape[0]))
    if A == 0:                       # the reference's three means over nothing
        return emb.sum() * float('nan')
    return NCAFn.apply(emb, idx, A, float(alpha), float(beta), float(ep))
