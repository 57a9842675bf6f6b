"""Measure the sparse GCN route (csrc/gcn_sparse.hip) against plain fp32 arithmetic: the kernels' and the CPU yardstick's errors
(tests/gcn_sparse_gate.py: eva_gate's propagated envelopes, fp64 reference graph by graph) of every stack case over the light graph mix and of the
end-to-end EVA case on a 300-object scene, written to profiles/gcn_sparse_accuracy_vs_fp32.json in the row format of
tools/gat_sparse_accuracy.py -- the measurement the gate ratios R of the tests are derived from ("measured ratio x 2, rounded up").
Needs the card:  python tools/gcn_sparse_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import eva_gate as EG  # noqa: E402
import gcn_sparse_gate as CG  # noqa: E402


def row(output, case, ke, ye):
    rm, rr = EG.ratio(ke, ye)
    return dict(output=output, case=f'{case} {output}', n=ke[2], kernel_max_u=round(ke[0], 4), kernel_rms_u=round(ke[1], 5),
                yardstick_max_u=round(ye[0], 4), yardstick_rms_u=round(ye[1], 5), ratio_max=round(rm, 4), ratio_rms=round(rr, 4))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else CG.PROFILE
    rows = []
    for which, units in enumerate(CG.CASES):
        rows += [row(k, f'sparse GCN {list(units)} light mix', ke, ye) for k, (ke, ye) in CG.measure(which).items()]
        print(f'stack {list(units)} done', flush=True)
    rows += [row(k, "EVA gcn_route='auto' 300 + 40 objects", ke, ye) for k, (ke, ye) in CG.measure_eva().items()]
    doc = dict(what='error |out - ref| / envelope (eva_gate\'s propagated envelopes, any depth: tests/gcn_sparse_gate.py), units of u = 2^-24, fp64 '
                    'reference graph by graph; yardstick = the same chain in float32 torch on the CPU with the reference\'s ReLU masks; ratio = '
                    'kernel / yardstick; light graph mix of tests/gat_sparse_gate.py',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per output:', json.dumps(CG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
