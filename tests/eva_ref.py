"""fp64 torch restatement, on the CPU, of the EVA baseline (no tests in this module): GCNConv as PyG 2.2.0 defines it with default arguments,
MultiGCN (reference src/aligner/networks/gat.py:6-25), EVA.forward (src/aligner/eva.py:33-96), NCALoss and OverallNCALoss
(src/aligner/losses.py:154-205).  Written from the definitions; it never calls the library.

GCNConv(in, out, cached=False):  h = x W^T (no bias in the linear, W [out, in]); every explicit self loop is removed, then every node gets
exactly one self loop of weight 1; deg_i = 1 + #{listed edges j -> i, j != i} (duplicates counted);
out_i = sum_{j -> i} deg_j^-1/2 deg_i^-1/2 h_j + bias over the remaining listed edges (duplicates as separate terms) and the self loop.
Edge columns are (source j, target i).  Every function takes a dtype, so the same text is the float32 yardstick of tests/eva_gate.py."""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ GCN
def gcn_adjacency(n, edges, dtype=torch.float64):
    """A^ [n, n] (row = target i, column = source j) of one graph from its [E, 2] (source, target) list."""
    cnt = torch.zeros((n, n), dtype=torch.float64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    for sj, di in e:
        if sj != di:
            cnt[di, sj] += 1.0
    cnt += torch.eye(n, dtype=torch.float64)
    deg = cnt.sum(1)                                     # 1 + listed edges into i
    dinv = (deg ** -0.5).to(dtype)                       # the correctly rounded value of deg^-1/2 in `dtype`
    return dinv[:, None] * cnt.to(dtype) * dinv[None, :]


def graphs_of(data_dict):
    """[(n, edges [E, 2])] in the src, ref, src, ref ... order of eva.py:47-70."""
    nc = np.asarray(data_dict['graph_per_obj_count']).reshape(-1)
    ec = np.asarray(data_dict['graph_per_edge_count']).reshape(-1)
    edges = data_dict['edges'].cpu().numpy() if isinstance(data_dict['edges'], torch.Tensor) else np.asarray(data_dict['edges'])
    out, o = [], 0
    for n, e in zip(nc, ec):
        out.append((int(n), edges[o:o + int(e)]))
        o += int(e)
    return out


def block_adjacency(graphs, dtype=torch.float64):
    return torch.block_diag(*[gcn_adjacency(n, e, dtype) for n, e in graphs]) if graphs else torch.zeros((0, 0), dtype=dtype)


def gcn_conv(x, w, b, adj):
    return adj @ (x @ w.t()) + b


def multi_gcn(x, adj, w0, b0, w1, b1):
    """gat.py:17-25 with dropout 0: layer, ReLU, layer."""
    return gcn_conv(F.relu(gcn_conv(x, w0, b0, adj)), w1, b1, adj)


# ------------------------------------------------------------------------------------------------ the other encoders
def pointnet_feat(pts, sd, prefix='object_encoder.'):
    """PointNetfeat(global_feat, no transforms): max over points of relu(conv3(relu(conv2(relu(conv1 x))))) -- the BatchNorm outputs are discarded
    by the reference (pointnet.py:141-159)."""
    h = pts
    for k in (1, 2, 3):
        w = sd[f'{prefix}conv{k}.weight']
        h = F.relu(h @ w.reshape(w.shape[0], -1).t() + sd[f'{prefix}conv{k}.bias'])
    return h.amax(dim=1)


def fusion(weight, tabs):
    """sg_aligner.py:30-35."""
    w = F.softmax(weight, dim=0)
    return torch.cat([w[m] * F.normalize(t) for m, t in enumerate(tabs)], dim=1)


def eva_forward(sd, data_dict, modules, dtype=torch.float64):
    """EVA.forward from a state dict (tensors of `dtype`, possibly requiring grad) and a host data_dict."""
    c = lambda t: t.detach().cpu().to(dtype)
    embs = {}
    for m in modules:
        if m == 'gcn':
            adj = block_adjacency(graphs_of(data_dict), dtype)
            embs[m] = multi_gcn(c(data_dict['tot_rel_pose']), adj, sd['structure_encoder.layer_stack.0.lin.weight'],
                                sd['structure_encoder.layer_stack.0.bias'], sd['structure_encoder.layer_stack.1.lin.weight'],
                                sd['structure_encoder.layer_stack.1.bias'])
        elif m == 'point':
            embs[m] = pointnet_feat(c(data_dict['tot_obj_pts']), sd)
        elif m == 'rel':
            embs[m] = c(data_dict['tot_bow_vec_object_edge_feats']) @ sd['meta_embedding_rel.weight'].t() + sd['meta_embedding_rel.bias']
        elif m == 'attr':
            embs[m] = c(data_dict['tot_bow_vec_object_attr_feats']) @ sd['meta_embedding_attr.weight'].t() + sd['meta_embedding_attr.bias']
        else:
            raise NotImplementedError(m)
    if len(modules) > 1:
        embs['joint'] = fusion(sd['fusion.weight'], [embs[m] for m in modules])
    return embs


# ------------------------------------------------------------------------------------------------ NCA
def nca_loss(z1, z2, alpha=1.0, beta=1.0, ep=0.0):
    """NCALoss.forward from its definition: S off the diagonal, row and column sums, the three means."""
    s = z1 @ z2.t()
    off = 1.0 - torch.eye(s.shape[0], dtype=s.dtype)
    S = torch.exp(alpha * (s - ep)) * off
    return (torch.log1p(S.sum(0)) / alpha).mean() + (torch.log1p(S.sum(1)) / alpha).mean() - beta * torch.log1p(F.relu(torch.diagonal(s))).mean()


def nca_table(emb, e1i, e2i, alpha=1.0, beta=1.0, ep=0.0):
    """OverallNCALoss's per-table step: normalise (eps 1e-12), gather the anchor rows, NCALoss."""
    x = F.normalize(emb)
    return nca_loss(x[torch.as_tensor(np.asarray(e1i), dtype=torch.long)], x[torch.as_tensor(np.asarray(e2i), dtype=torch.long)], alpha, beta, ep)


def overall_nca(output_dict, data_dict):
    out = {k: nca_table(v, data_dict['e1i'], data_dict['e2i'], 1.0, 1.0, 0.0) for k, v in output_dict.items()}
    out['loss'] = sum(out.values())
    return out
