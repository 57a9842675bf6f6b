"""Measure the EVA baseline's kernels against plain fp32 arithmetic: the kernel's and the CPU yardstick's envelope-relative errors
(tests/eva_gate.py) of the GCN gate case (forward and the four parameter gradients), of the NCA loss and its table gradient at every gate
shape with the default and a small row-block budget, and of the five tables and per-key losses of the end-to-end case, written to
profiles/eva_accuracy_vs_fp32.json -- the measurement the gate ratios R of the tests are derived from ("measured ratio x 2, rounded up").
Needs the card:  python tools/eva_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import eva_gate as EG  # noqa: E402


def row(output, case, ke, ye):
    rm, rr = EG.ratio(ke, ye)
    return dict(output=output, case=case, n=ke[2], kernel_max_u=round(ke[0], 4), kernel_rms_u=round(ke[1], 5), yardstick_max_u=round(ye[0], 4),
                yardstick_rms_u=round(ye[1], 5), ratio_max=round(rm, 4), ratio_rms=round(rr, 4))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else EG.PROFILE
    rows = []
    for seed in (0, 1):
        for k, (ke, ye) in EG.measure_gcn(seed).items():
            rows.append(row(k, f'gcn seed {seed}', ke, ye))
    for A, D in EG.NCA_SHAPES:
        for stash in (None, EG.small_stash(A)):
            for k, (ke, ye) in EG.measure_nca(A, D, stash).items():
                rows.append(row(k, f'nca A={A} D={D} stash={stash}', ke, ye))
    for k, (ke, ye) in EG.measure_eva().items():
        rows.append(row('nca_loss' if k.startswith('loss_') else k, f'eva {k}', ke, ye))
    doc = dict(what='envelope-relative error |out - ref| / propagated envelope (tests/eva_gate.py), units of u = 2^-24, fp64 reference '
                    '(tests/eva_ref.py); yardstick = the same computation in float32 torch on the CPU with the reference\'s ReLU masks; '
                    'ratio = kernel / yardstick (a scalar\'s yardstick floored at 1 u, as its gate is)',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per output:', json.dumps(EG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
