"""Subscan generation (csrc/visibility.hip, preprocessing/subscans.py) beside the host loop it replaces.
  python tools/bench_subscans.py [--quick] [--out FILE]     # one JSON object to stdout and to profiles/subscans_bench.json (or FILE)
Cases: one synthetic scan of 200 000 vertices x 300 frames (tests/subscan_ref.make_scan) and a batch of 16 such scans.  Per case:
`kernel_ms` = each of the three entry points alone on resident data (HIP events, after warm-up, median of the repeats; the walk runs in place, so
the visibility kernel refills the matrix before every timed walk, outside the timed window); `call_ms` = generate_subscan_masks, NumPy in ->
NumPy out, with the packing, the upload, the launches and the downloads (host clock, ends with the data on the host);
`host_ms` = the yardstick's restatement of the reference loop (visible_ref for every frame + walk_ref), one thread, same process -- measured on
ONE scan and, for the batch, multiplied by the number of scans (marked as such).  `visibility_gb_per_s` counts the bytes the kernel has to
move (12 B per vertex read once per frame group, F * N / 8 B written) over its kernel time; `visibility_gevals_per_s` the (frame, point)
tests.  No ratio is promised anywhere: the file records what was observed."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import subscan_ref as SR
from sgaligner_amd import _lib
from sgaligner_amd.preprocessing import subscans as SS
from sgaligner_amd.utils import point_cloud as PC

FRAME_GROUP = 16           # frames per workgroup of vis_kernel: the vertices are re-read once per group


def event_ms(fn, reps, before=None):
    times = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def kernels(scans, budgets, reps):
    """The three entry points alone: everything resident, buffers allocated once."""
    pts = torch.from_numpy(np.concatenate([s['pts'] for s in scans])).cuda()
    w2c = torch.from_numpy(np.concatenate([SR.w2c_rows(s['poses']) for s in scans])).cuda()
    intr = torch.from_numpy(np.stack([SR.intr_row(s['intrinsics']) for s in scans])).cuda()
    pt_off = np.concatenate([[0], np.cumsum([len(s['pts']) for s in scans])])
    fr_off = np.concatenate([[0], np.cumsum([len(s['poses']) for s in scans])])
    lay = PC.ScanLayout(pt_off, fr_off, int(pt_off[-1]), int(fr_off[-1]), device='cuda')
    vis = torch.empty((lay.total_words,), device='cuda', dtype=torch.int64)
    mp = torch.tensor(budgets, dtype=torch.int32).cuda()
    slot = torch.from_numpy(np.concatenate([np.unique(s['object_id'], return_inverse=True)[1].reshape(-1) for s in scans]).astype(np.int32)).cuda()
    n_slots = int(max(len(np.unique(s['object_id'])) for s in scans))
    fill = lambda: PC.visible_masks_batch(pts, None, w2c, None, intr, out=vis, layout=lay)
    fill()
    cum, walk = SS.subscan_walk_batch(vis, lay, mp, in_place=True)                       # warm-up of both, and the row list for the counts
    segs = SS.split_walk_output(walk.cpu().numpy(), lay)
    rows = [(s, int(f)) for s in range(lay.n_scans) for f in segs[s][0]]
    SS.object_counts_batch(cum, lay, rows, slot, n_slots)
    torch.cuda.synchronize()
    k_vis = event_ms(fill, reps)
    k_walk = event_ms(lambda: SS.subscan_walk_batch(vis, lay, mp, in_place=True), reps, before=fill)
    k_cnt = event_ms(lambda: SS.object_counts_batch(cum, lay, rows, slot, n_slots), reps)
    evals = float(sum(len(s['pts']) * len(s['poses']) for s in scans))
    moved = float(sum(len(s['pts']) * 12 * -(-len(s['poses']) // FRAME_GROUP) for s in scans)) + 8.0 * lay.total_words
    stat = lambda t: {'median': round(t[0], 4), 'min': round(t[1], 4), 'max': round(t[2], 4)}
    return {'kernel_ms': {'visibility': stat(k_vis), 'walk': stat(k_walk), 'object_counts': stat(k_cnt)},
            'bit_matrix_mib': round(8.0 * lay.total_words / 2 ** 20, 2), 'subscans': len(rows), 'object_slots': n_slots,
            'visibility_gevals_per_s': round(evals / (k_vis[0] * 1e-3) / 1e9, 2), 'visibility_gb_per_s': round(moved / (k_vis[0] * 1e-3) / 1e9, 2)}


def call_ms(scans, budgets, reps):
    args = [(s['pts'], s['poses'], s['intrinsics']) for s in scans]
    SS.generate_subscan_masks(args, budgets)                                             # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = SS.generate_subscan_masks(args, budgets)                                   # returns numpy arrays: the downloads have completed
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times)), out


def host_ms(scan, budget):
    t0 = time.perf_counter()
    masks = SR.visible_ref(scan['pts'], SR.w2c_rows(scan['poses']), SR.intr_row(scan['intrinsics']))
    t1 = time.perf_counter()
    ref = SR.walk_ref(masks, budget)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, ref


def main(argv):
    if not torch.cuda.is_available():
        raise RuntimeError('bench_subscans needs a HIP device; a timing without one says nothing')
    quick = '--quick' in argv
    torch.set_num_threads(1)
    n, f, batch = (20_000, 40, 4) if quick else (200_000, 300, 16)
    reps = 5 if quick else 11
    scans = [SR.make_scan(n, f, seed=100 + i) for i in range(batch)]
    budgets = [int(0.3 * n)] * batch
    out = {'device': torch.cuda.get_device_name(0), 'cus': int(_lib.lib().sga_device_cus()), 'vertices': n, 'frames': f,
           'host': 'tests/subscan_ref.py visible_ref + walk_ref (NumPy, one thread, same process); the reference additionally calls OpenCV and copies '
                   'the visible vertices every frame', 'cases': []}
    h_vis, h_walk, ref = host_ms(scans[0], budgets[0])
    for name, sub in (('1 scan', scans[:1]), (f'{batch} scans', scans)):
        case = {'case': f'{name} of {n} vertices x {f} frames', 'scans': len(sub)}
        case.update(kernels(sub, budgets[:len(sub)], reps))
        c = call_ms(sub, budgets[:len(sub)], max(3, reps // 2))
        case['call_ms'] = {'median': round(c[0], 2), 'min': round(c[1], 2), 'max': round(c[2], 2)}
        seg_end, seg_count, masks = c[3][0]
        case['equals_host'] = bool(np.array_equal(seg_end, ref['seg_end']) and np.array_equal(seg_count, ref['seg_count']) and
                                   np.array_equal(masks, ref['seg_masks']))
        case['host_ms'] = {'visibility': round(h_vis * len(sub), 1), 'walk': round(h_walk * len(sub), 1),
                           'measured_on': '1 scan' + ('' if len(sub) == 1 else f', multiplied by {len(sub)}')}
        out['cases'].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'subscans_bench.json')
    if not quick or '--out' in argv:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
