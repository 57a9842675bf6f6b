"""EVA baseline train step (forward, OverallNCALoss, backward, Adam) on the HIP path against the same step written in plain torch ops on
the same device: a dense A^ per graph (batched when the graphs have one size), PointNetfeat as 1x1 convolutions and a max, NCALoss as the
reference writes it (src/aligner/losses.py:161-173).  Two sizes: the reference's batch (4 pairs x ~40 objects x 512 points) and
BASELINE.json configs[1] (512 pairs x 64 objects x 512 points).  The ratio is REPORTED, not gated.

    python tools/bench_eva.py [out.json]        (default profiles/eva_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sgaligner_amd.synthetic import make_batch, make_batch_fast, to_device  # noqa: E402
from sgaligner_amd.trainer import EVASteps  # noqa: E402

MODULES = ['gcn', 'point', 'rel', 'attr']


class TorchEVA:
    """The same model on the same parameters' values, every operation a torch op."""

    def __init__(self, model):
        self.p = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and k in dict(model.named_parameters()))
                  for k, v in model.state_dict().items()}
        self.params = [v for v in self.p.values() if v.requires_grad]
        self.opt = torch.optim.Adam([{'params': self.params}], lr=1e-3)

    def adjacency(self, dd):
        nc = np.asarray(dd['graph_per_obj_count']).reshape(-1)
        ec = np.asarray(dd['graph_per_edge_count']).reshape(-1)
        edges, dev = dd['edges'], dd['edges'].device
        if len(set(nc.tolist())) == 1:                     # one size: all graphs as one [G, n, n] batch
            G, n = len(nc), int(nc[0])
            gid = torch.repeat_interleave(torch.arange(G, device=dev), torch.as_tensor(ec, device=dev))
            keep = edges[:, 0] != edges[:, 1]
            cnt = torch.zeros((G, n, n), device=dev)
            cnt.index_put_((gid[keep], edges[keep, 1], edges[keep, 0]), torch.ones(int(keep.sum()), device=dev), accumulate=True)
            cnt = cnt + torch.eye(n, device=dev)
            dinv = cnt.sum(2).pow(-0.5)
            return dinv[:, :, None] * cnt * dinv[:, None, :]
        out, o = [], 0
        for n, e in zip(nc, ec):                           # the reference's way: graph by graph
            ed = edges[o:o + int(e)]
            o += int(e)
            keep = ed[:, 0] != ed[:, 1]
            cnt = torch.zeros((int(n), int(n)), device=dev)
            cnt.index_put_((ed[keep, 1], ed[keep, 0]), torch.ones(int(keep.sum()), device=dev), accumulate=True)
            cnt = cnt + torch.eye(int(n), device=dev)
            dinv = cnt.sum(1).pow(-0.5)
            out.append(dinv[:, None] * cnt * dinv[None, :])
        return out

    def aggregate(self, adj, h):
        if isinstance(adj, torch.Tensor):
            return torch.bmm(adj, h.view(adj.shape[0], adj.shape[1], -1)).reshape(h.shape)
        parts, o = [], 0
        for a in adj:
            parts.append(a @ h[o:o + a.shape[0]])
            o += a.shape[0]
        return torch.cat(parts)

    def forward(self, dd):
        p = self.p
        adj = self.adjacency(dd)
        x = dd['tot_rel_pose'].float()
        x1 = F.relu(self.aggregate(adj, x @ p['structure_encoder.layer_stack.0.lin.weight'].t()) + p['structure_encoder.layer_stack.0.bias'])
        embs = {'gcn': self.aggregate(adj, x1 @ p['structure_encoder.layer_stack.1.lin.weight'].t()) + p['structure_encoder.layer_stack.1.bias']}
        h = dd['tot_obj_pts'].permute(0, 2, 1)
        for k in (1, 2, 3):
            h = F.relu(F.conv1d(h, p[f'object_encoder.conv{k}.weight'], p[f'object_encoder.conv{k}.bias']))
        embs['point'] = h.amax(dim=2)
        embs['rel'] = F.linear(dd['tot_bow_vec_object_edge_feats'].float(), p['meta_embedding_rel.weight'], p['meta_embedding_rel.bias'])
        embs['attr'] = F.linear(dd['tot_bow_vec_object_attr_feats'].float(), p['meta_embedding_attr.weight'], p['meta_embedding_attr.bias'])
        w = F.softmax(p['fusion.weight'], dim=0)
        embs['joint'] = torch.cat([w[i] * F.normalize(embs[m]) for i, m in enumerate(MODULES)], dim=1)
        return embs

    @staticmethod
    def nca(z1, z2, alpha=1.0, beta=1.0, ep=0.0):
        n = z1.shape[0]
        scores = z1.mm(z2.t())
        eye = torch.eye(n, device=z1.device)
        s_diag = eye * scores
        s_ = torch.exp(alpha * (scores - ep))
        s_ = s_ - s_ * eye
        loss_diag = -torch.log(1 + F.relu(s_diag.sum(0)))
        return (torch.log(1 + s_.sum(0)) / alpha).mean() + (torch.log(1 + s_.sum(1)) / alpha).mean() + (beta * loss_diag).mean()

    def step(self, dd):
        for q in self.params:
            q.grad = None
        embs = self.forward(dd)
        i1 = torch.as_tensor(np.asarray(dd['e1i']), device=embs['gcn'].device, dtype=torch.long)
        i2 = torch.as_tensor(np.asarray(dd['e2i']), device=embs['gcn'].device, dtype=torch.long)
        loss = 0
        for e in embs.values():
            z = F.normalize(e)
            loss = loss + self.nca(z[i1], z[i2])
        loss.backward()
        self.opt.step()
        return loss


def timed(fn, batches, warmup, n):
    for i in range(warmup):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'eva_bench.json')
    rows = []
    sizes = [('reference batch', 4, 40, 512, [to_device(make_batch(4, 40, 512, seed=7 + i, ragged=True), 'cuda') for i in range(4)], 10, 40),
             ('configs[1]', 512, 64, 512, [make_batch_fast(512, 64, 512, seed=7, device='cuda')], 2, 5)]
    for name, B, N, P, batches, warmup, n in sizes:
        steps = EVASteps(MODULES, device='cuda', seed=42)
        ref = TorchEVA(steps.model)

        def hip_step(dd):
            steps.forward_backward(dd)
            steps.optimizer_step()

        l_hip = float(steps.forward_backward(batches[0])[1]['loss'].detach())
        l_ref = float(ref.step(batches[0]).detach())
        ms_hip = timed(hip_step, batches, warmup, n)
        ms_ref = timed(ref.step, batches, warmup, n)
        rows.append(dict(size=name, pairs=B, objects=N, points=P, anchors=int(len(batches[0]['e1i'])), hip_ms_per_step=round(ms_hip, 3),
                         torch_ms_per_step=round(ms_ref, 3), torch_over_hip=round(ms_ref / ms_hip, 3), first_loss_hip=l_hip, first_loss_torch=l_ref))
        print(json.dumps(rows[-1]), flush=True)
        del steps, ref
        torch.cuda.empty_cache()
    doc = dict(what='EVA baseline train step (forward + OverallNCALoss + backward + Adam), ms per step wall clock, HIP path vs the same step in '
                    'plain torch ops on the same device (tools/bench_eva.py); reported, not gated',
               device=torch.cuda.get_device_name(0), modules=MODULES, cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
