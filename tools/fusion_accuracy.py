"""Measure the fusion kernels and the element-wise kernels against plain fp32 arithmetic: the kernels' and the CPU yardstick's errors
(tests/fusion_gate.py: envelope-relative, fp64 autograd reference) of every gate case at this card's row-loop pass, of the equal-width tables
through the differing-width route and of the inputs of test_fusion_zero_row_and_large; and the worst error in ulps of sga_elu_fwd / sga_elu_bwd
over the stratified x <= 0 at every test size, next to torch's float32 F.elu.  Written to profiles/fusion_accuracy_vs_fp32.json -- the measurement the
gate ratios R and the ulp bounds ULP of the tests are derived from ("measured x 2, rounded up").
Needs the card:  python tools/fusion_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import fusion_gate as FG  # noqa: E402

SEEDS = (0, 1)


def rows_of(case, meas):
    out = []
    for k, (ke, ye) in meas.items():
        rm, rr = FG.ratio(ke, ye)
        out.append(dict(output=k, case=case, n=ke[2], kernel_max_u=round(ke[0], 4), kernel_rms_u=round(ke[1], 5),
                        yardstick_max_u=round(ye[0], 4), yardstick_rms_u=round(ye[1], 5), ratio_max=round(rm, 4), ratio_rms=round(rr, 4)))
        print(out[-1], flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else FG.PROFILE
    P = FG.device_rows_per_pass()
    rows = []
    for name, T, widths in FG.gate_cases(P):
        for seed in SEEDS:
            c = FG.gate_case(T, widths, seed)
            got = FG.run(c['weight'], c['tabs'], c['gj'])
            assert FG.zero_rows_ok(got, c['judged'], c['gj']), (name, seed)
            rows += rows_of(f'{name} seed {seed}', FG.measure(got, c['weight'], c['tabs'], c['gj'], c['judged']))
    for M, D in ((3, 100), (8, 65)):                             # test_equal_widths_through_both_routes
        T = 2 * P + 7
        gen = torch.Generator().manual_seed(M * 1000 + D)
        tabs = [torch.randn(T, D, generator=gen) for _ in range(M)]
        w, gj = torch.randn(M, 1, generator=gen), torch.randn(T, M * D, generator=gen)
        rows += rows_of(f'var route M{M} D{D} T{T}', FG.measure(FG.run(w, tabs, gj, 'var'), w, tabs, gj))
    w, tabs, gj = FG.large_inputs()
    rows += rows_of('test_fusion_zero_row_and_large', FG.measure(FG.run(w, tabs, gj), w, tabs, gj))
    ew = []
    for n in FG.EW_SIZES:
        x, gy = FG.ew_inputs(n)
        if not (x <= 0).any():
            continue
        kf, kb = FG.elu_worst_ulps(*FG.elu_run(x, gy), x, gy)
        yf, yb = FG.elu_worst_ulps(*FG.elu_yardstick(x, gy), x, gy)
        ew += [dict(kernel='elu_fwd', n=n, kernel_ulp=round(kf, 4), torch_f32_ulp=round(yf, 4)),
               dict(kernel='elu_bwd', n=n, kernel_ulp=round(kb, 4), torch_f32_ulp=round(yb, 4))]
        print(ew[-2], ew[-1], flush=True)
    doc = dict(what='fusion: error |out - ref| / envelope (tests/fusion_gate.py), units of u = 2^-24, fp64 autograd reference of the module text; '
                    'yardstick = the same text in float32 torch on the CPU; ratio = kernel / yardstick (a max up to 1 u counts as 0, a '
                    'single-entry output\'s yardstick is floored at 1 u, as the gate does).  elementwise: worst |out - ref| over the stratified '
                    'x <= 0 in float32 ulps of the fp64 result, expm1(x) forward and gy exp(x) backward',
               device=torch.cuda.get_device_name(0), cus=P // FG.WAVES_PER_CU, rows_per_pass=P, cases=rows, elementwise=ew)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k not in ('cases', 'elementwise')}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ],\n "elementwise": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in ew))
        f.write('\n ]\n}\n')
    print('r per output:', json.dumps(FG.ratios_from_profile(out)), 'ulps:', json.dumps(FG.ulps_from_profile(out)))


if __name__ == '__main__':
    main()
