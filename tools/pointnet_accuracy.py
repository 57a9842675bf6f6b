"""Measure the PointNet kernels against plain fp32 arithmetic: the kernel's and the CPU yardstick's envelope-relative errors
(tests/pointnet_gate.py) of y (every out_size, both launch forms) and of the six gradients (the gate shapes), in both kernel modes, written
to profiles/pointnet_accuracy_vs_fp32.json -- the measurement the gate ratios R of the tests are derived from ("measured ratio x 2, rounded
up").  Needs the card:  python tools/pointnet_accuracy.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pointnet_gate as PG  # noqa: E402


def row(output, mode, form, C3, T, P, ke, ye):
    (km, kr), (ym, yr) = ke[:2], ye[:2]
    return dict(output=output, mode=mode, form=form, C3=C3, T=T, P=P, kernel_max_u=round(km, 4), kernel_rms_u=round(kr, 5),
                yardstick_max_u=round(ym, 4), yardstick_rms_u=round(yr, 5), ratio_max=round(km / ym, 4), ratio_rms=round(kr / yr, 4))


def main():
    from sgaligner_amd import _lib, ops
    out = sys.argv[1] if len(sys.argv) > 1 else PG.PROFILE
    cus = int(_lib.lib().sga_device_cus())
    rows = []
    for mode in (0, 4):
        for (T, P) in PG.gate_shapes(cus):
            for k, (ke, ye) in PG.measure_backward(T, P, mode).items():
                rows.append(row(k, mode, 'bwd', 256, T, P, ke, ye))
        for C3 in (64, 128, 256):
            for form, T, P in PG.forward_shapes(ops.POINTNET_SPLIT_MAX_OBJECTS):
                ke, ye = PG.measure_forward(C3, T, P, mode)
                rows.append(row('y', mode, form, C3, T, P, ke, ye))
    doc = dict(what='envelope-relative error |out - ref| / propagated envelope (tests/pointnet_gate.py), units of u = 2^-24, fp64 reference; '
                    'yardstick = the same chain in float32 torch on the CPU with the reference\'s masks and arg-max; ratio = kernel / yardstick; '
                    'mode 0 = fp32 MFMA kernels, 4 = three bf16 planes',
               device=torch.cuda.get_device_name(0), cus=cus, cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:                            # one case per line
        head = {k: v for k, v in doc.items() if k != 'cases'}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(',\n'.join('  ' + json.dumps(c) for c in rows))
        f.write('\n ]\n}\n')
    print('r per mode and output:', json.dumps(PG.ratios_from_profile(out)))


if __name__ == '__main__':
    main()
