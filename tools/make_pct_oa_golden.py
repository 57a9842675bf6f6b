"""Record the reference's offset attention `OA` and the encoder built on it, `SPCT`, on fixed inputs: tests/golden/pct_oa.npz.

    python tools/make_pct_oa_golden.py <reference root> [out.npz]

Imports `aligner.networks.pct` from <reference root>/src.  That module imports `pointnet2_ops` (a CUDA farthest-point sampler that OA and
SPCT never call); the few-line stub below stands in for it.

Parameters.  No new ones are stored: they are the float32 parameters of tests/golden/pct_eval.npz (`sd__*`, the reference NaivePCT's, with
randomised BatchNorm affines and running statistics -- SPCT's keys are a subset of NaivePCT's, and OA(128) takes those of `sa1`), with
every shared q/k weight multiplied by pct_oa_ref.QK_GAIN (1 for OA alone, whose input is a unit normal; 2 for SPCT -- exact in float32):
inside SPCT the default initialisation gives logits within one unit of each other and an attention all but uniform, at 2 x they spread
over several units and the column sums over 0.35 .. 3.7.  tests/pct_oa_ref.golden_state_dict() rebuilds them the same way.  The modules run
in float64 on the CPU.

Recorded (float32 where the tolerance of the tests is 1e-3, to stay within the size a committed file may have):
  OA(128), T = 2, N = 37, train and eval mode: output, every parameter gradient, the input gradient, the updated running statistics (train);
  SPCT(), T = 2, N = 24, eval and train mode: the three outputs (of x every SUB-th channel) and, of the fixed linear functional
      <x, c_x> + <x_max, c_max> + <x_mean, c_mean>, the gradient of every parameter (of a matrix 16 evenly spaced rows);
      inputs and cotangents are drawn from the seeds of tests/pct_oa_ref.oa_inputs() / spct_inputs(); a slice of each is stored to pin that;
  the state_dict key lists of OA(128) and SPCT().
Numbers and key names only: nothing of the reference's text is in this file or in the output."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def stub_pointnet2_ops():
    mod, utils = types.ModuleType('pointnet2_ops'), types.ModuleType('pointnet2_ops.pointnet2_utils')
    mod.pointnet2_utils = utils
    sys.modules['pointnet2_ops'], sys.modules['pointnet2_ops.pointnet2_utils'] = mod, utils


def main():
    import pct_oa_ref as P
    ref_root = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'pct_oa.npz')
    sys.path.insert(0, os.path.join(ref_root, 'src'))
    stub_pointnet2_ops()
    from aligner.networks import pct as R
    f32 = lambda t: t.detach().numpy().astype(np.float32)
    data = {}

    # ---- OA(128)
    sd = P.golden_state_dict('oa')
    data['oa_keys'] = np.array(list(R.OA(128).state_dict()))
    x, cot = P.oa_inputs()
    data['oa_pin'] = torch.stack([x[:, ::16], cot[:, ::16]]).numpy()
    for mode in ('train', 'eval'):
        m = R.OA(128)
        m.load_state_dict(sd, strict=True)
        m = m.double().train(mode == 'train')
        xi = x.double().requires_grad_()
        y = m(xi)
        (y * cot.double()).sum().backward()
        data[f'oa_{mode}__y'] = f32(y)
        data[f'oa_{mode}__dx'] = f32(xi.grad)
        for name, p in m.named_parameters():
            data[f'oa_{mode}__g__{name}'] = f32(p.grad)
        if mode == 'train':
            for k, v in m.state_dict().items():
                if 'running' in k or 'num_batches' in k:
                    data[f'oa_train__after__{k}'] = v.numpy()

    # ---- SPCT()
    sd = P.golden_state_dict('spct')
    data['spct_keys'] = np.array(list(R.SPCT().state_dict()))
    x, cx, cmax, cmean = P.spct_inputs()
    data.update(spct_x_pin=x.numpy(), spct_cx_pin=cx[:, ::64].numpy(), spct_cpool_pin=torch.stack([cmax[:, ::16], cmean[:, ::16]]).numpy())
    for mode in ('eval', 'train'):
        m = R.SPCT()
        m.load_state_dict(sd, strict=True)
        m = m.double().train(mode == 'train')
        y, ymax, ymean = m(x.double())
        ((y * cx.double()).sum() + (ymax * cmax.double()).sum() + (ymean * cmean.double()).sum()).backward()
        data.update({f'spct_{mode}__x': f32(y[:, ::P.SUB]), f'spct_{mode}__max': f32(ymax), f'spct_{mode}__mean': f32(ymean)})
        for name, p in m.named_parameters():
            data[f'spct_{mode}__g__{name}'] = f32(P.sub_rows(p.grad))
        if mode == 'train':
            for k, v in m.state_dict().items():
                if 'running' in k or 'num_batches' in k:
                    data[f'spct_train__after__{k}'] = v.numpy()
    np.savez_compressed(out, **data)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
