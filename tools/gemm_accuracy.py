"""Measure every GEMM route against plain fp32 arithmetic: the kernel's and the CPU yardstick's envelope-relative errors (tests/gemm_gate.py)
over the K sweep each route admits, written to profiles/gemm_accuracy_vs_fp32.json -- the measurement the gate ratios R of the tests
are derived from ("measured ratio x 2, rounded up").  Needs the card:  python tools/gemm_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import gemm_gate as G  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else G.PROFILE
    rows = []
    for case in G.accuracy_cases():
        r = G.run_accuracy_case(case)
        (km, kr), (ym, yr) = r['kernel'][:2], r['yard'][:2]
        rows.append(dict(route=case['route'], transA=case['ta'], transB=case['tb'], M=case['m'], N=case['n'], K=case['k'],
                         grade=case.get('grade'), splits=r['plan'][1],
                         kernel_max_u=round(km, 4), kernel_rms_u=round(kr, 4), yardstick_max_u=round(ym, 4), yardstick_rms_u=round(yr, 4),
                         ratio_max=round(km / ym, 4), ratio_rms=round(kr / yr, 4)))
    from sgaligner_amd import _lib
    doc = dict(what='envelope-relative error |C - ref| / (|A||B| + |bias|), units of u = 2^-24, fp64 reference; yardstick = fp32 on the CPU, '
                    'K in chunks of 32; ratio = kernel / yardstick.  The fp32 MFMA kernels (32x32x2: the running sum is rounded every two products) '
                    'sit at 0.47 u rms whatever K while the 32-wide yardstick falls like 1/sqrt(K), hence their ratios; split-K and the three-plane '
                    'kernels (one fp32 rounding per 16 products) follow the yardstick',
               device=torch.cuda.get_device_name(0), cus=_lib.lib().sga_device_cus(), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    worst = {}
    for c in rows:
        worst[c['route']] = max(worst.get(c['route'], 0.0), c['ratio_rms'], c['ratio_max'])
    print('worst ratio per route:', json.dumps(worst))


if __name__ == '__main__':
    main()
