"""Measure the loss kernels against plain fp32 arithmetic: the kernel's and the CPU yardstick's envelope-relative errors (tests/loss_gate.py)
of every gated stage output -- gather, the global sums, the anchors x anchors terms and coefficients, the stash products, the negatives'
gradient, the scatter, the scalar head -- in every arithmetic tier over the gate cases, written to profiles/loss_accuracy_vs_fp32.json: the
measurement the gate ratios R of the tests are derived from ("measured ratio x 2, rounded up").  Needs the card:
python tools/loss_accuracy.py [out.json] [--tier f16]
--tier T: measure the rows of tier T alone and replace them in the profile, every other row kept as it is ('f16': the wide fp16 kernels of
csrc/wide16.hip and the Zh forms of the per-table anchors x anchors kernels, over loss_gate.f16_cases)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import loss_gate as LG  # noqa: E402


def row(output, tier, case, ke, ye):
    rm, rr = LG.ratio(ke, ye, LG.is_scalar(output))
    return dict(output=output, tier=tier, case=case, n=ke[2], kernel_max_u=round(ke[0], 4), kernel_rms_u=round(ke[1], 5), yardstick_max_u=round(ye[0], 4),
                yardstick_rms_u=round(ye[1], 5), ratio_max=round(rm, 4), ratio_rms=round(rr, 4))


def main():
    argv = list(sys.argv[1:])
    only = None
    if '--tier' in argv:
        i = argv.index('--tier')
        only = argv[i + 1]
        del argv[i:i + 2]
        if only != 'f16':
            sys.exit(f"--tier {only}: only the tier 'f16' can be measured on its own")
    out = argv[0] if argv else LG.PROFILE
    rows, failed = [], []

    def take(case, gen):
        try:                                               # a case that cannot be measured (a NaN left, a non-zero where every term is zero) is reported, the rest still is
            for output, t, ke, ye in gen:
                rows.append(row(output, t, case, ke, ye))
        except AssertionError as e:
            failed.append((case, repr(e)))
            print('NOT MEASURED', case, repr(e), flush=True)

    for c in ([] if only else LG.gate_cases() + LG.plain_cases()):
        for tier in LG.tier_for(c):
            take(c['name'], LG.measure_all(c['name'], tier))
            print(c['name'], tier, len(rows), flush=True)
    for name in ([] if only else LG.pertable_cases()):
        for nt in (1, 4):
            take(f'{name}-NT{nt}', LG.measure_pertable(name, nt))
        print(name, 'pertable', len(rows), flush=True)
    for M, b, valu in ([] if only else LG.GROUP_CASES):
        take(f'group-M{M}-b{b}-valu{valu}', LG.measure_group(M, b, valu))
    for name in ([] if only else LG.wide_cases()):
        take(f'{name}-wide', LG.measure_wide(name))
    for M, A, seed in ([] if only else LG.HEAD_CASES):
        for f64 in (1, 0):
            take(f'head-M{M}-A{A}-f64={f64}', LG.measure_head(M, A, seed, f64))
    for c in LG.f16_cases():
        take(c['name'], LG.measure_f16(c['name']))
        print(c['name'], 'f16', len(rows), flush=True)
    # one line per (output, tier, case): the worst of the case's launches (walks, shards, tables)
    worst = {}
    for r in rows:
        k = (r['output'], r['tier'], r['case'])
        if k not in worst or max(r['ratio_max'], r['ratio_rms']) > max(worst[k]['ratio_max'], worst[k]['ratio_rms']):
            worst[k] = r
    rows = list(worst.values())
    if only:                                               # the other tiers' rows stay as they were measured
        rows = [r for r in json.load(open(LG.PROFILE))['cases'] if r['tier'] != only] + rows
    doc = dict(what='envelope-relative error |out - ref| / running-error envelope (tests/loss_gate.py), units of u = 2^-24, fp64 stage reference on the '
                    'inputs the kernel gets; yardstick = the same stage in float32 torch on the CPU; ratio = kernel / yardstick (a scalar\'s '
                    'yardstick floored at 1 u; 0 where the gate\'s floor -- max 1 u, rms 1 u / sqrt(n) -- admits the kernel whatever r is); per (output, tier, case) the worst of the case\'s launches (walks, shards, tables)',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per output and tier:', json.dumps(LG.ratios_from_profile(out)))
    if failed:
        sys.exit(f'{len(failed)} case(s) could not be measured: {failed}')


if __name__ == '__main__':
    main()
