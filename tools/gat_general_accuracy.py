"""Measure the dense GAT path against plain fp32 arithmetic: the kernel's and the CPU yardstick's errors (tests/gat_general_gate.py: flat
envelope, fp64 oracle reference) of every attention-kernel case at every batch cut of it, of the kernels of 2 x 128 on the shapes
of test_multigat_fwd_bwd, and of every stack (the masked one included), written to
profiles/gat_general_accuracy_vs_fp32.json -- the measurement the gate ratios R of the tests are derived from ("measured ratio x 2,
rounded up").
Needs the card:  python tools/gat_general_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import eva_gate as EG  # noqa: E402
import gat_general_gate as GG  # noqa: E402


def row(output, case, ke, ye):
    rm, rr = EG.ratio(ke, ye)
    return dict(output=GG.kind(output), case=f'{case} {output}', n=ke[2], kernel_max_u=round(ke[0], 4), kernel_rms_u=round(ke[1], 5),
                yardstick_max_u=round(ye[0], 4), yardstick_rms_u=round(ye[1], 5), ratio_max=round(rm, 4), ratio_rms=round(rr, 4))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GG.PROFILE
    rows = []
    for heads, channels in GG.KERNEL_CASES:
        for cap, meas in GG.measure_kernel(heads, channels).items():
            rows += [row(k, f'kernel {heads}x{channels} nmax<={cap}', ke, ye) for k, (ke, ye) in meas.items()]
    for which in range(len(GG.CANON_SHAPES)):
        rows += [row(k, f'kernel 2x128 shapes[{which}]', ke, ye) for k, (ke, ye) in GG.measure_canon(which).items()]
    for which, (units, heads) in enumerate(GG.STACKS):
        rows += [row(k, f'stack {list(units)}/{list(heads)}', ke, ye) for k, (ke, ye) in GG.measure_stack(which).items()]
    units, heads = GG.STACKS[GG.MASKED_STACK]
    rows += [row(k, f'stack {list(units)}/{list(heads)} masks p=0.5', ke, ye) for k, (ke, ye) in GG.measure_stack(GG.MASKED_STACK, True).items()]
    doc = dict(what='error |out - ref| / max |ref| of that output (flat envelope, tests/gat_general_gate.py), units of u = 2^-24, fp64 reference '
                    '(oracle.sga_oracle.gat_conv / multi_gat); yardstick = the same functions in float32 torch on the CPU; ratio = kernel / '
                    'yardstick (a single-entry output\'s yardstick floored at 1 u, as its gate is)',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per output:', json.dumps(GG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
