"""Measure the sparse GAT route (csrc/gat_sparse.hip) against plain fp32 arithmetic: the kernels' and the CPU yardstick's errors
(tests/gat_sparse_gate.py: flat envelope, fp64 oracle reference) of every attention-kernel case over the light and the dense graph mix and of
every stack (the masked one included), written to profiles/gat_sparse_accuracy_vs_fp32.json in the format of the general profile -- the
measurement the gate ratios R of the tests are derived from ("measured ratio x 2, rounded up").
Needs the card:  python tools/gat_sparse_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import eva_gate as EG  # noqa: E402
import gat_general_gate as GG  # noqa: E402
import gat_sparse_gate as SG  # noqa: E402


def row(output, case, ke, ye):
    rm, rr = EG.ratio(ke, ye)
    return dict(output=GG.kind(output), case=f'{case} {output}', n=ke[2], kernel_max_u=round(ke[0], 4), kernel_rms_u=round(ke[1], 5),
                yardstick_max_u=round(ye[0], 4), yardstick_rms_u=round(ye[1], 5), ratio_max=round(rm, 4), ratio_rms=round(rr, 4))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else SG.PROFILE
    rows = []
    for mix, heads, channels in SG.KERNEL_CASES:
        rows += [row(k, f'sparse kernel {heads}x{channels} {mix} mix', ke, ye) for k, (ke, ye) in SG.measure_kernel(mix, heads, channels).items()]
        print(f'kernel {mix} {heads}x{channels} done', flush=True)
    for which, (units, heads, masked) in enumerate(SG.STACKS):
        rows += [row(k, f'sparse stack {list(units)}/{list(heads)} light mix' + (' masks p=0.5' if masked else ''), ke, ye)
                 for k, (ke, ye) in SG.measure_stack(which).items()]
        print(f'stack {which} done', flush=True)
    doc = dict(what='error |out - ref| / max |ref| of that output (flat envelope, tests/gat_general_gate.py), units of u = 2^-24, fp64 reference '
                    '(oracle.sga_oracle.gat_conv / multi_gat); yardstick = the same functions in float32 torch on the CPU; ratio = kernel / '
                    'yardstick (a single-entry output\'s yardstick floored at 1 u, as its gate is); graph mixes of tests/gat_sparse_gate.py',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per output:', json.dumps(SG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
