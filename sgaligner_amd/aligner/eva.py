"""EVA baseline encoder -- drop-in for reference src/aligner/eva.py (same class name, constructor signature, attributes, state_dict
keys and data_dict contract), computing on the HIP kernels through sgaligner_amd.ops.  There is no CPU path."""
import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: F401  (re-exported by `from aligner.eva import *`, as the reference does)

from .. import ops
from .networks.gat import MultiGAT, MultiGCN  # noqa: F401  (MultiGAT: importers of the reference's module find the name here)
from .networks.pointnet import PointNetfeat
from .sg_aligner import MultiModalFusion, _Linear


class EVA(nn.Module):
    """eva.py:9-96.  `modules` (list of 'gcn' | 'point' | 'rel' | 'attr') is kept as an attribute with the reference's name -- it
    shadows nn.Module.modules(), exactly as in the reference (:12).  The tables keep their own widths (gcn n_units[-1] = 400, point 200,
    rel / attr emb_dim = 100): the reference has no projection to emb_dim for the first two (:72,:75).
    gcn_route (last, so the reference's positional order stands): MultiGCN's route -- 'dense' (default; scenes of at most 256 objects), 'sparse'
    or 'auto' (scenes of any size)."""

    def __init__(self, modules, rel_dim, attr_dim, n_units=[3, 200, 400], emb_dim=100, pt_out_dim=256, dropout=0.0, attn_dropout=0.0,
                 instance_norm=False, gcn_route='dense'):
        super().__init__()
        self.modules = modules
        self.pt_out_dim = pt_out_dim
        self.rel_dim = rel_dim
        self.emb_dim = emb_dim
        self.attr_dim = attr_dim
        self.n_units = n_units
        self.dropout = dropout
        self.attn_dropout = attn_dropout
        self.instance_norm = instance_norm
        self.inner_view_num = len(self.modules)

        self.meta_embedding_rel = _Linear(self.rel_dim, self.emb_dim)
        self.meta_embedding_attr = _Linear(self.attr_dim, self.emb_dim)
        self.object_encoder = PointNetfeat(global_feat=True, batch_norm=True, point_size=3, input_transform=False,
                                           feature_transform=False, out_size=200)                     # eva.py:27
        self.gcn_route = gcn_route
        self.structure_encoder = MultiGCN(n_units=self.n_units, dropout=self.dropout, route=gcn_route)
        self.fusion = MultiModalFusion(modal_num=self.inner_view_num, with_weight=1)

    def forward(self, data_dict):
        pts = data_dict['tot_obj_pts']
        if not pts.is_cuda:
            raise RuntimeError('sgaligner_amd.EVA: data_dict tensors must be on the HIP device '
                               '(utils/torch_util.to_cuda in the reference); there is no CPU path')
        embs = {}
        for module in self.modules:
            if module == 'gcn':
                # all 2B graphs in one launch per layer (reference: 2B sequential MultiGCN calls, :47-70)
                gb = ops.GraphBatch.of(data_dict)
                emb = self.structure_encoder.forward_batched(data_dict['tot_rel_pose'], gb)
            elif module == 'point':
                emb = self.object_encoder(pts.permute(0, 2, 1))                                       # :34,:75
            elif module == 'rel':
                emb = self.meta_embedding_rel(data_dict['tot_bow_vec_object_edge_feats'])
            elif module == 'attr':
                emb = self.meta_embedding_attr(data_dict['tot_bow_vec_object_attr_feats'])
            else:
                raise NotImplementedError                                                             # :83-84
            embs[module] = emb
        if len(self.modules) > 1:
            embs['joint'] = self.fusion([embs[m] for m in self.modules])
        return embs
