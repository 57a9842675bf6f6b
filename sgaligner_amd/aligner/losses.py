"""Contrastive (ICL) + alignment (IAL) losses -- drop-in for reference src/aligner/losses.py
(CustomMultiLossLayer :17-34, ICLLoss :36-58, IALLoss :60-97, OverallLoss :99-152, NCALoss :154-173, OverallNCALoss :175-205) on the tiled HIP
loss kernels (csrc/contrastive.hip, loss_anchor.hip, loss_pertable.hip).  The heavy op is ops.contrastive_terms, which returns the raw
double-summed terms; what remains here is the reference's scalar arithmetic on 1-element tensors."""
import torch
from torch import nn
import torch.nn.functional as F  # noqa: F401  (re-exported by `from aligner.losses import *`, as the reference does)

from .. import ops


FUSED_JOINT = True     # tests flip this to cross-check the fused path against the independent-table path
FUSED_HEAD = True      # the scalar loss head as one launch (ops.LossHeadFn); False: the same arithmetic as torch ops


class CustomMultiLossLayer(nn.Module):
    def __init__(self, loss_num, device=None):
        super().__init__()
        self.loss_num = loss_num
        self.log_vars = nn.Parameter(torch.zeros(self.loss_num, ), requires_grad=True)

    def forward(self, loss_list):
        """sum_i exp(-log_vars[i]) * L_i + log_vars[i]  (reference losses.py:28-34), as four tensor ops instead of 3 per term:
        at the reference's own batch sizes the step is bound by the number of launches, not by their size.  `loss_list` may be
        a list of 0-d tensors or one [loss_num] tensor."""
        terms = loss_list if isinstance(loss_list, torch.Tensor) else torch.stack([t.reshape(()) for t in loss_list])
        assert terms.shape[0] == self.loss_num
        lv = self.log_vars.to(terms.dtype)
        return (torch.exp(-lv) * terms + lv).sum()


class ICLLoss(nn.Module):
    def __init__(self, device, temperature=0.05, alpha=0.5):
        super().__init__()
        self.temp = 0.1                 # the reference ignores the ctor argument (losses.py:39)
        self.alpha = alpha
        self.device = device

    def forward(self, emb, data_dict):
        sums, s = ops.contrastive_terms([emb], data_dict, alpha=self.alpha, shard=data_dict.get('_sga_shard'), reduce=data_dict.get('_sga_reduce'))
        return sums[0] / float(s.A * s.A)                         # .mean() over the A x A matrix (:57)


class IALLoss(nn.Module):
    def __init__(self, device, temperature=0.05, alpha=0.5):
        super().__init__()
        self.temp = 1.0                 # losses.py:63
        self.alpha = alpha
        self.device = device
        self.zoom = 0.1

    def forward(self, src_emb, ref_emb, data_dict):
        """src_emb: modality table (gives qo), ref_emb: joint table (gives qm) -- call order of losses.py:122."""
        sums, _ = ops.contrastive_terms([src_emb, ref_emb], data_dict)
        return self.zoom * (self.alpha * sums[2] + (1 - self.alpha) * sums[3])


class OverallLoss(nn.Module):
    """losses.py:99-152.  `loss_group` (metadata['loss_group'] or the attribute; default 'global') selects what "the batch"
    of the loss is:
      'global' -- one loss over all pairs of the batch (the reference's semantics applied to the whole device batch);
      b (int)  -- the batch is cut into groups of b consecutive pairs and the reference's loss is evaluated on every group
                  independently (its anchors against ITS negatives only); every returned value is the SUM over groups, i.e.
                  exactly what the reference accumulates when it is fed b pairs per iteration (scan3r_ground_truth.yaml:27)."""

    def __init__(self, ial_loss_layer, icl_loss_layer, device, metadata):
        super().__init__()
        self.zoom = metadata['zoom']
        self.device = device
        self.modules = metadata['modules']
        self.weight_align_loss = metadata['wt_align_loss']            # stored, unused (as in the reference)
        self.weight_contrastive_loss = metadata['wt_contrastive_loss']
        self.loss_group = metadata.get('loss_group', 'global')
        self.align_loss = IALLoss(device)
        self.contrastive_loss = ICLLoss(self.device)
        self.align_multi_loss_layer = ial_loss_layer
        self.contrastive_multi_loss_layer = icl_loss_layer

    def forward(self, output_dict, data_dict):
        if self.loss_group not in (None, 'global'):
            return self._forward_groups(output_dict, data_dict, int(self.loss_group))
        return self._forward_global(output_dict, data_dict)

    _warned_untagged = False

    def _fusion_source(self, output_dict, mods):
        m = len(mods)
        tabs = [output_dict[k] for k in mods]
        src = getattr(output_dict['joint'], '_sga_fusion', None)
        fused = (src is not None and FUSED_JOINT and 2 <= m <= 4 and len(src[1]) == m
                 and all(a is b for a, b in zip(src[1], tabs)) and all(t.shape[1] <= 104 for t in tabs))
        tag_ok = src is not None and len(src[1]) == m and all(a is b for a, b in zip(src[1], tabs))
        if not fused and not tag_ok and FUSED_JOINT and 2 <= m <= 4 and not OverallLoss._warned_untagged and tabs[0].is_cuda:
            # the provenance tag is a tensor ATTRIBUTE: any .clone() / .to() / arithmetic on `joint` between the encoder and the loss drops
            # it, and the loss then (correctly, but ~2x slower) treats `joint` as an independent table -- say so once instead of silently
            OverallLoss._warned_untagged = True
            import warnings
            warnings.warn("sgaligner_amd: output_dict['joint'] reached OverallLoss without the fusion provenance tag (it was copied or "
                          "modified after MultiModalFusion, or is not a fusion of output_dict's modality tables): the loss takes the general "
                          "per-table path -- correct, but the 100*M-wide joint table is swept explicitly (about twice the loss time).",
                          RuntimeWarning, stacklevel=3)
        return tabs, (src if fused else None)

    def _forward_global(self, output_dict, data_dict):
        mods = list(self.modules)
        m = len(mods)
        if m > 1:
            # one fused pass over all M+1 tables: every similarity tile is computed once and shared by
            # ICL_m, ICL_joint and IAL_m (the reference recomputes the joint table's q's M times)
            tabs, src = self._fusion_source(output_dict, mods)
            al = self.align_loss
            ml_a, ml_c = self.align_multi_loss_layer, self.contrastive_multi_loss_layer
            head_fused = FUSED_HEAD and tabs[0].is_cuda and type(ml_a) is CustomMultiLossLayer and type(ml_c) is CustomMultiLossLayer
            if src is not None:      # the joint table IS the fusion of these tables: never multiply the 100*M-d table
                hint = None
                if head_fused and torch.is_grad_enabled() and ops.FUSED_AA_ONEPASS:
                    # dL/d(terms) of the standard head depends on the log_vars and constants only: announce it, and the anchors x
                    # anchors similarities are computed once (terms + gradients together) instead of once per direction
                    n_anc = len(data_dict['e1i']) if data_dict.get('_sga_index_sets') is None else data_dict['_sga_index_sets'].A
                    hint = ops.LossHeadFn.coef_hint(ml_a.log_vars, ml_c.log_vars, n_anc, al.zoom, al.alpha, self.zoom)
                sums, s = ops.fused_contrastive_terms(tabs, src[0], data_dict, alpha=self.contrastive_loss.alpha,
                                                      shard=data_dict.get('_sga_shard'), reduce=data_dict.get('_sga_reduce'), coef_hint=hint)
            else:          # arbitrary joint table: treat it as an independent (M+1)-th table
                if output_dict['joint'].numel() == 0 and tabs[0].numel() > 0:
                    raise RuntimeError("sgaligner_amd.OverallLoss: output_dict['joint'] is the empty placeholder of the anchor-sharded fused path, but the fused "
                                       "path cannot be taken here (tables wider than 104 columns, more than 4 modules, or FUSED_JOINT off): pass the real joint table")
                sums, s = ops.contrastive_terms(tabs + [output_dict['joint']], data_dict, alpha=self.contrastive_loss.alpha,
                                                shard=data_dict.get('_sga_shard'), reduce=data_dict.get('_sga_reduce'))
            nt = m + 1
            if head_fused and sums.is_cuda:
                # losses.py:114-152 + the two multi-loss layers as one launch (ops.LossHeadFn)
                loss, icl_uni, icl_multi, total_align_loss = ops.LossHeadFn.apply(
                    sums, ml_a.log_vars, ml_c.log_vars, s.A, al.zoom, al.alpha, self.zoom).unbind(0)
            else:
                a2 = float(s.A * s.A)
                icl = sums[:nt] / a2
                ial = al.zoom * (al.alpha * sums[nt:nt + m] + (1 - al.alpha) * sums[nt + m:nt + 2 * m])
                total_align_loss = ml_a(ial) * self.zoom
                icl_uni = ml_c(icl[:m])
                icl_multi = icl[m]
                loss = total_align_loss + icl_uni + icl_multi
        else:
            total_align_loss = 0.0
            icl_multi = 0.0
            icl_uni = self.contrastive_loss(output_dict[mods[0]], data_dict)
            loss = icl_uni
        return {'loss': loss, 'icl_loss_unimodal': icl_uni, 'icl_loss_multimodal': icl_multi, 'ial_loss': total_align_loss}

    def _forward_groups(self, output_dict, data_dict, b):
        mods = list(self.modules)
        m = len(mods)
        if data_dict.get('_sga_shard') is not None:
            raise RuntimeError('sgaligner_amd: loss_group=b groups never cross ranks; evaluate it on the local batch')
        if m > 1:
            tabs, src = self._fusion_source(output_dict, mods)
            if src is None:
                # arbitrary joint tensor: the reference's loop, literally -- one global-loss evaluation per group
                tot = None
                for gd in ops.group_data_dicts(data_dict, b):
                    r = self._forward_global(output_dict, gd)
                    tot = r if tot is None else {k: tot[k] + r[k] for k in r}
                return tot
            out, gr = ops.grouped_contrastive_terms(tabs, src[0], data_dict, b, alpha=self.contrastive_loss.alpha)
            nt = m + 1
            a2 = (gr.na * gr.na).unsqueeze(1)                                  # .mean() over each group's A_g x A_g matrix
            icl = out[:, :nt] / a2
            al = self.align_loss
            ial = al.zoom * (al.alpha * out[:, nt:nt + m] + (1 - al.alpha) * out[:, nt + m:nt + 2 * m])
            ml_a, ml_c = self.align_multi_loss_layer, self.contrastive_multi_loss_layer
            # sum over groups of CustomMultiLossLayer: sum_m exp(-lv_m) * (sum_g x_gm) + G * lv_m
            total_align_loss = ((torch.exp(-ml_a.log_vars) * ial.sum(0)).sum() + gr.G * ml_a.log_vars.sum()) * self.zoom
            icl_uni = (torch.exp(-ml_c.log_vars) * icl[:, :m].sum(0)).sum() + gr.G * ml_c.log_vars.sum()
            icl_multi = icl[:, m].sum()
            loss = total_align_loss + icl_uni + icl_multi
        else:
            out, gr = ops.grouped_contrastive_terms([output_dict[mods[0]]], None, data_dict, b, alpha=self.contrastive_loss.alpha)
            total_align_loss = 0.0
            icl_multi = 0.0
            icl_uni = (out[:, 0] / (gr.na * gr.na)).sum()
            loss = icl_uni
        return {'loss': loss, 'icl_loss_unimodal': icl_uni, 'icl_loss_multimodal': icl_multi, 'ial_loss': total_align_loss}


class NCALoss(nn.Module):
    """losses.py:154-173 on csrc/nca.hip (ops.nca_loss).  The reference's forward takes the two gathered, normalised row sets; gathering
    and normalising are part of the kernels here, so `forward(emb, data_dict)` takes the raw table and the batch's e1i / e2i."""

    def __init__(self, alpha, beta, ep):
        super().__init__()
        self.alpha = alpha
        self.beta = beta
        self.ep = ep

    def forward(self, emb, data_dict):
        return ops.nca_loss(emb, data_dict, alpha=self.alpha, beta=self.beta, ep=self.ep)


class OverallNCALoss(nn.Module):
    """losses.py:175-205: NCALoss(1, 1, 0) on every table of output_dict ('joint' included), the per-key losses and their sum."""

    def __init__(self, modules, device):
        super().__init__()
        self.device = device
        self.criterion_dict = {}
        for module in modules:
            self.criterion_dict[module] = NCALoss(alpha=1, beta=1, ep=0.0)
        self.criterion_dict['joint'] = NCALoss(alpha=1, beta=1, ep=0.0)

    def forward(self, output_dict, data_dict):
        if isinstance(data_dict, dict) and data_dict.get('_sga_shard') is not None:
            raise RuntimeError('sgaligner_amd.OverallNCALoss: multi-GPU sharding of the NCA loss is not implemented (`_sga_shard` in data_dict)')
        loss_dict = {}
        for module in output_dict.keys():
            loss_dict[module] = self.criterion_dict[module](output_dict[module], data_dict)
        loss_sum = 0
        for module in loss_dict.keys():
            loss_sum = loss_sum + loss_dict[module]
        loss_dict['loss'] = loss_sum
        return loss_dict
