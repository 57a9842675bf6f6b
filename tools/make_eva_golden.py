"""Record the reference's NCALoss / OverallNCALoss on fixed inputs: tests/golden/nca_cases.npz.

    python tools/make_eva_golden.py <reference root> [out.npz]

Imports `aligner.losses` from <reference root>/src (it needs nothing but torch), feeds it seeded fp64 inputs on the CPU and stores inputs,
losses and autograd gradients.  Nothing of the reference's text is in this file or in the output."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, A, D, alpha, beta, ep)
NCA_CASES = (('a1', 1, 100, 1.0, 1.0, 0.0), ('a2', 2, 100, 1.0, 1.0, 0.0), ('a9', 9, 24, 1.0, 1.0, 0.0), ('a33', 33, 200, 1.0, 1.0, 0.0),
             ('a40_ab', 40, 104, 2.0, 0.5, 0.25))
OVERALL = dict(T=30, A=11, widths=dict(gcn=40, point=24, joint=64))


def main():
    ref_root = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'nca_cases.npz')
    sys.path.insert(0, os.path.join(ref_root, 'src'))
    from aligner.losses import NCALoss, OverallNCALoss
    data = {'names': np.array([c[0] for c in NCA_CASES])}
    for name, A, D, alpha, beta, ep in NCA_CASES:
        gen = torch.Generator().manual_seed(7000 + A * 13 + D)
        z1 = F.normalize(torch.randn(A, D, generator=gen, dtype=torch.float64))
        z2 = F.normalize(z1 + 0.4 * torch.randn(A, D, generator=gen, dtype=torch.float64))
        if A > 1:
            z2[1::4] = -z2[1::4]                            # negative diagonal scores: the relu branch
        z1.requires_grad_(True)
        z2.requires_grad_(True)
        loss = NCALoss(alpha, beta, ep)(z1, z2)
        loss.backward()
        data.update({f'{name}__z1': z1.detach().numpy(), f'{name}__z2': z2.detach().numpy(), f'{name}__abe': np.array([alpha, beta, ep]),
                     f'{name}__loss': loss.detach().numpy(), f'{name}__g1': z1.grad.numpy(), f'{name}__g2': z2.grad.numpy()})
    gen = torch.Generator().manual_seed(4242)
    T, A = OVERALL['T'], OVERALL['A']
    perm = torch.randperm(T, generator=gen).numpy()
    dd = {'e1i': perm[:A].astype(np.int32), 'e2i': perm[A:2 * A].astype(np.int32)}
    tabs = {k: (torch.randn(T, d, generator=gen, dtype=torch.float64) * 3).requires_grad_(True) for k, d in OVERALL['widths'].items()}
    losses = OverallNCALoss(modules=[k for k in tabs if k != 'joint'], device='cpu')(tabs, dd)
    losses['loss'].backward()
    data.update({'ov__e1i': dd['e1i'], 'ov__e2i': dd['e2i'], 'ov__keys': np.array(list(tabs))})
    for k, t in tabs.items():
        data.update({f'ov__tab__{k}': t.detach().numpy(), f'ov__grad__{k}': t.grad.numpy(), f'ov__loss__{k}': losses[k].detach().numpy()})
    data['ov__loss__loss'] = losses['loss'].detach().numpy()
    np.savez_compressed(out, **data)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
