"""Plain-torch fp64 restatement of offset attention (OA), the encoder SPCT and NaivePCT with the OA trunk, written from the formulas
(no tests in this module); tests/test_pct_oa_cpu.py pins it on tests/golden/pct_oa.npz, which tools/make_pct_oa_golden.py records from the
reference modules.

Point-major throughout: an activation is [T, N, C].  Per object, with one shared weight W_qk (32 x 128, no bias):
    Q = x W_qk^T,   V = x W_v^T + b_v
    E = Q Q^T                                   (no 1/sqrt(32))
    P[i,j] = exp(E[i,j] - m_i) / l_i            softmax over j
    d_j = 1e-9 + sum_i P[i,j]
    Xr[j] = sum_i P[i,j] V[i] / d_j
    out = x + relu(BatchNorm((x - Xr) W_t^T + b_t))
BatchNorm1d over all T*N rows: train mode with the biased batch variance, the running statistics updated with momentum 0.1 and the unbiased
variance; eval mode with the running statistics.  SPCT: Embedding (two conv + BatchNorm + ReLU), four OA layers, cat of their outputs,
conv(512 -> 1024) + BatchNorm + LeakyReLU(0.2), then the max and the mean over the points.  NaivePCT with OA: the same trunk, the max, then
linear1 + bn1 + ReLU and linear2 + bn2 + ReLU (Dropout p = 0).

eps: the golden is a float64 run, which adds the literal 1e-9 -- the default here.  A float32 run adds the float32 nearest 1e-9 (the reference
adds the Python float to a float32 tensor), 2.8e-8 smaller in relative terms; tests/pct_oa_gate.py passes that value, because its shadowed
family has column sums of eps' own size and is judged to a few 2^-24."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
QK_GAIN = {'oa': 1.0, 'spct': 2.0, 'naive': 2.0}      # logits of a few units in each case (tools/make_pct_oa_golden.py)
SUB = 8                      # the golden keeps every SUB-th channel of SPCT's x ...


def sub_rows(t):
    """... and 16 evenly spaced rows of each of SPCT's matrix gradients (a vector whole)."""
    return t[::max(1, t.shape[0] // 16)] if t.dim() > 1 else t
OA_T, OA_N = 2, 37
SP_T, SP_N = 2, 24
BN_EPS, BN_MOM = 1e-5, 0.1
LAYERS = ('sa1', 'sa2', 'sa3', 'sa4')


def golden_state_dict(kind):
    """The float32 parameters the golden was recorded with: those of tests/golden/pct_eval.npz, every shared q/k weight times QK_GAIN[kind].
    kind 'naive': all of NaivePCT's keys; 'spct': SPCT's subset; 'oa': those of sa1, without the prefix."""
    g = np.load(os.path.join(GOLDEN, 'pct_eval.npz'), allow_pickle=False)
    sd = {k[4:]: torch.from_numpy(g[k]).clone() for k in g.files if k.startswith('sd__')}
    for k in sd:
        if k.endswith('q_conv.weight') or k.endswith('k_conv.weight'):
            sd[k] = sd[k] * QK_GAIN[kind]
    if kind == 'naive':
        return sd
    if kind == 'spct':
        return {k: v for k, v in sd.items() if k.split('.')[0] in ('embedding', 'linear') + LAYERS}
    if kind == 'oa':
        return {k[4:]: v for k, v in sd.items() if k.startswith('sa1.')}
    raise ValueError(kind)


def oa_inputs():
    """(x, cot) [T, 128, N] float32 for OA(128)."""
    gen = torch.Generator().manual_seed(2341)
    return torch.randn(OA_T, 128, OA_N, generator=gen), torch.randn(OA_T, 128, OA_N, generator=gen)


def spct_inputs():
    """(x [T,3,N], c_x [T,1024,N], c_max [T,1024], c_mean [T,1024]) float32 for SPCT: input and the linear functional's coefficients."""
    gen = torch.Generator().manual_seed(2342)
    x = torch.randn(SP_T, 3, SP_N, generator=gen) * 0.6
    return x, torch.randn(SP_T, 1024, SP_N, generator=gen) / SP_N, torch.randn(SP_T, 1024, generator=gen), torch.randn(SP_T, 1024, generator=gen)


def offset_attention(q, v, eps=1e-9):
    """q [T,N,32], v [T,N,128] -> Xr [T,N,128], in the dtype of q."""
    e = q @ q.transpose(1, 2)
    p = torch.softmax(e, dim=-1)
    d = eps + p.sum(1)                                            # [T, j]
    return (p.transpose(1, 2) @ v) / d[:, :, None]


def batch_norm(y, sd, pre, training, updates):
    """BatchNorm1d over the rows of y [R, C] with the parameters sd[pre + ...]; train mode records the updated statistics in `updates`."""
    w, b = sd[pre + '.weight'], sd[pre + '.bias']
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        R = y.shape[0]
        with torch.no_grad():
            updates[pre + '.running_mean'] = (1 - BN_MOM) * sd[pre + '.running_mean'] + BN_MOM * mean
            updates[pre + '.running_var'] = (1 - BN_MOM) * sd[pre + '.running_var'] + BN_MOM * var * R / (R - 1)
            updates[pre + '.num_batches_tracked'] = sd[pre + '.num_batches_tracked'] + 1
    else:
        mean, var = sd[pre + '.running_mean'], sd[pre + '.running_var']
    return (y - mean) / torch.sqrt(var + BN_EPS) * w + b


def _mat(w):
    return w.reshape(w.shape[0], -1)


def oa_layer(x, sd, pre, training, updates):
    """x [T,N,128] -> [T,N,128]; sd keys pre + 'k_conv.weight' etc. (pre '' or 'sa1.')."""
    T, N, C = x.shape
    q = x @ _mat(sd[pre + 'k_conv.weight']).t()
    v = x @ _mat(sd[pre + 'v_conv.weight']).t() + sd[pre + 'v_conv.bias']
    xr = offset_attention(q, v)
    z = (x - xr) @ _mat(sd[pre + 'trans_conv.weight']).t() + sd[pre + 'trans_conv.bias']
    z = batch_norm(z.reshape(T * N, C), sd, pre + 'after_norm', training, updates).reshape(T, N, C)
    return x + torch.relu(z)


def trunk(x, sd, training, updates):
    """x [T,3,N] -> the widest activation [T,N,1024] (after BatchNorm and LeakyReLU)."""
    h = x.transpose(1, 2)
    T, N, _ = h.shape
    for conv, bn in (('embedding.conv1', 'embedding.bn1'), ('embedding.conv2', 'embedding.bn2')):
        z = h @ _mat(sd[conv + '.weight']).t()
        h = torch.relu(batch_norm(z.reshape(T * N, -1), sd, bn, training, updates)).reshape(T, N, -1)
    outs = []
    for layer in LAYERS:
        h = oa_layer(h, sd, layer + '.', training, updates)
        outs.append(h)
    z = torch.cat(outs, -1) @ _mat(sd['linear.0.weight']).t()
    z = batch_norm(z.reshape(T * N, -1), sd, 'linear.1', training, updates).reshape(T, N, -1)
    return torch.where(z > 0, z, 0.2 * z)


def spct(x, sd, training):
    """(x [T,1024,N], x_max, x_mean, updates)."""
    updates = {}
    y = trunk(x, sd, training, updates)
    return y.transpose(1, 2), y.max(1)[0], y.mean(1), updates


def naive_pct_oa(x, sd, training):
    """NaivePCT(attention='oa'), Dropout p = 0: ([T,256], updates)."""
    updates = {}
    g = trunk(x, sd, training, updates).max(1)[0]
    f = torch.relu(batch_norm(g @ sd['linear1.weight'].t(), sd, 'bn1', training, updates))
    f = torch.relu(batch_norm(f @ sd['linear2.weight'].t() + sd['linear2.bias'], sd, 'bn2', training, updates))
    return f, updates


def leaves64(sd):
    """(sd in fp64 whose parameters require grad, k_conv.weight the same tensor as q_conv.weight; name -> leaf) for autograd through the restatement."""
    out, leaves = {}, {}
    for k, v in sd.items():
        if not v.dtype.is_floating_point or 'running' in k:
            out[k] = v.double() if v.dtype.is_floating_point else v
            continue
        if k.endswith('k_conv.weight'):
            continue
        out[k] = leaves[k] = v.double().clone().requires_grad_()
    for k in sd:
        if k.endswith('k_conv.weight'):
            out[k] = out[k.replace('k_conv', 'q_conv')]           # one tensor, named as nn.Module.named_parameters names it
    return out, leaves
