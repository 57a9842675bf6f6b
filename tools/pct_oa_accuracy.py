"""Measure the offset-attention kernels against plain fp32 arithmetic: the kernel's and the CPU yardstick's envelope-relative errors
(tests/pct_oa_gate.py) of every gate case -- Xr, dV, dQ; families a, b, c of the SA gate, the shadowed family d and the lattice (dQ); both
memory layouts -- written to profiles/pct_oa_accuracy_vs_fp32.json, the measurement the gate ratios R of the tests are derived from
("measured ratio x 2, rounded up").
Needs the card:  python tools/pct_oa_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import torch  # noqa: E402

import pct_oa_gate as OG  # noqa: E402
from pct_accuracy import rows_of  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OG.PROFILE
    rows = []
    for family, T, N, layout, outputs in OG.cases():
        rows += rows_of(family, f'T={T} N={N} {layout}', OG.measure(family[3:], T, N, layout, outputs))
    doc = dict(what='envelope-relative error |out - ref| / propagated envelope (tests/pct_oa_gate.py), units of u = 2^-24, fp64 reference; '
                    'yardstick = the same operation in float32 torch on the CPU in the stated order; ratio = kernel / max(yardstick, the floor of '
                    'gemm_gate.gate_ok: 1 u on the max, 1 u / sqrt(n) on the rms)',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per family and output:', json.dumps(OG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
