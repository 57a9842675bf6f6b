"""Measure the PCT encoder kernels against plain fp32 arithmetic: the kernel's and the CPU yardstick's envelope-relative errors
(tests/pct_gate.py) of every gate case -- attention (Xs, dV, dQ; three logit regimes and the lattice, both memory layouts), BatchNorm (train
through sga_bn_stats and through the GEMM epilogue, eval) and the widest stage (fused node and the chain of separate nodes) -- written to
profiles/pct_accuracy_vs_fp32.json, the measurement the gate ratios R of the tests are derived from ("measured ratio x 2, rounded up").
Needs the card:  python tools/pct_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pct_gate as PG  # noqa: E402


def rows_of(family, case, results, guarded=0.0):
    out = []
    for k, (ke, ye) in results.items():
        (km, kr), (ym, yr) = ke[:2], ye[:2]
        rm, rr = PG.ratios(ke, ye)
        out.append(dict(family=family, output=k, case=case, guarded=round(guarded, 5), kernel_max_u=round(km, 4), kernel_rms_u=round(kr, 5),
                        yardstick_max_u=round(ym, 4), yardstick_rms_u=round(yr, 5), n=ke[2], ratio_max=round(rm, 4),
                        ratio_rms=round(rr, 4)))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else PG.PROFILE
    rows = []
    for family, T, N, layout, outputs in PG.attention_cases():
        rows += rows_of(family, f'T={T} N={N} {layout}', PG.measure_attention(family[5:], T, N, layout, outputs))
    for family, path, R_, C, training, act, resid in PG.bn_cases():
        res, guarded = PG.measure_bn(path, R_, C, training, act, resid)
        rows += rows_of(family, f'R={R_} C={C} act={act} resid={int(resid)}', res, guarded)
    for family, T, N, K, C, training, fused in PG.head_cases():
        res, guarded = PG.measure_head(T, N, K, C, training, fused)
        rows += rows_of(family, f'T={T} N={N} K={K} C={C} {"fused" if fused else "chain"}', res, guarded)
    doc = dict(what='envelope-relative error |out - ref| / propagated envelope (tests/pct_gate.py), units of u = 2^-24, fp64 reference; '
                    'yardstick = the same operation in float32 torch on the CPU with the reference\'s masks and arg-max; ratio = kernel / max(yardstick, the floor of gemm_gate.gate_ok: 1 u on the max, 1 u / sqrt(n) on the rms); '
                    'guarded = share of the case whose cotangent the guard zeroed',
               device=torch.cuda.get_device_name(0), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per family and output:', json.dumps(PG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
