"""Record the bits of NaivePCT()'s inference output (attention 'sa', the default) on the seeded inputs of tests/golden/pct_eval.npz:
tests/golden/pct_sa_bits.npz, which tests/test_pct_oa_gpu.py::test_sa_default_is_bit_for_bit_what_it_was compares with.  The committed file
was written by the commit before offset attention was added; run on any later tree it must reproduce that file.
Needs the card:  python tools/record_pct_sa_bits.py [out.npz]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sgaligner_amd.aligner.networks.pct import NaivePCT  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'pct_sa_bits.npz')
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'pct_eval.npz')))
    m = NaivePCT()
    m.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith('sd__')}, strict=True)
    m = m.cuda().eval()
    data = {}
    for tag in ('small', 'p512', 'ragged'):
        x = torch.from_numpy(g['x_' + tag]).cuda()
        with torch.no_grad():
            y1, y2 = m(x).cpu().numpy(), m(x).cpu().numpy()
        assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32)), 'two runs differ: nothing to record'
        data['y_' + tag] = y1
    np.savez_compressed(out, **data)
    print('wrote', out, {k: v.shape for k, v in data.items()})


if __name__ == '__main__':
    main()
