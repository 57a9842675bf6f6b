"""Time the anchors x anchors kernel (sga_loss_anchor_multi_bwd, TERMS build) and its stash GEMMs alone on random unit rows.
  python tools/bench_aa.py [anchors=19456] [rows_per_block=2048] [M=3] [reps=5]
  python tools/bench_aa.py 155648 2048 3 5 planes     # + the same symmetric block through sga_loss_anchor_multi_bwd_symx_bf16x6 (three-plane image)
  python tools/bench_aa.py 155648 0 3 5 walk          # every launch of the symmetric walk of that anchor set: launch plan, modelled fill, ms
  python tools/bench_aa.py 155648 0 3 5 classes       # an all-own-square job against an all-mirrored one, 8192 x 8192 each
  python tools/bench_aa.py 0 0 3 5 crossover         # symmetric 1024-row block, fp32 entry against the three-plane one, over a ladder of anchor counts"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as ct
import numpy as np, torch
from sgaligner_amd import _lib
from sgaligner_amd.ops import _p, _ptr_array, _stream
A = int(sys.argv[1]) if len(sys.argv) > 1 else 19456
NS = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
M = int(sys.argv[3]) if len(sys.argv) > 3 else 3
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
mode = sys.argv[5] if len(sys.argv) > 5 else ''
L = _lib.lib(); st = _stream(); dev = 'cuda'


def sym_block(A, NS, M, reps, planes):
    """Median ms of one symmetric block rows [0, NS) x columns [0, A) (mirrored from NS on): (fp32 entry, three-plane entry or None)."""
    g = torch.Generator(device=dev).manual_seed(0)
    zs = []
    for m in range(M):
        z = torch.zeros(2 * A + 32, 104, device=dev)
        z[:2 * A, :100] = torch.nn.functional.normalize(torch.randn(2 * A, 100, device=dev, generator=g), dim=1)
        zs.append(z)
    nt, slots = M + 1, 1 + L.sga_loss_slots()
    sums = torch.rand(nt, 8, device=dev, dtype=torch.float64, generator=g) * 1e5 + 1e5
    beta = torch.full((M,), 1.0 / M, device=dev)
    coef = (torch.rand(3 * M + 1, device=dev, generator=g) + 0.5) * 1e-4
    m1 = [torch.empty(A * NS, device=dev) for _ in range(M)]
    m2 = [torch.empty(max(1, (A - NS) * NS), device=dev) for _ in range(M)]
    gsc = torch.empty(slots + 1, nt, 8, device=dev, dtype=torch.float64)
    gam2 = torch.empty(slots, M, device=dev, dtype=torch.float64)
    out = torch.empty(slots * (nt + 2 * M), device=dev, dtype=torch.float64)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res, sums_out = [], []
    imgs = None
    if planes:
        imgs = [torch.empty((L.sga_loss_split3_bytes(A, 0, 0),), device=dev, dtype=torch.uint8) for _ in zs]
        for z, im in zip(zs, imgs):
            _lib.check(L.sga_loss_split3_tables(_p(z), A, 0, 0, _p(im), None, st), 'split3')
    for which in (0, 1) if planes else (0,):
        t = []
        for r in range(reps + 1):
            e[0].record()
            if which:
                _lib.check(L.sga_loss_anchor_multi_bwd_symx_bf16x6(_ptr_array(imgs), M, _p(beta), A, 0, 0, _p(sums), 0.5, 0.1, 1.0, _p(coef), _ptr_array(m1),
                                                                   _ptr_array(m2), _p(gsc), _p(gam2), 0, NS, 0, A, NS, _p(out), st), 'planes')
            else:
                _lib.check(L.sga_loss_anchor_multi_bwd_symx(_ptr_array(zs), M, _p(beta), A, _p(sums), 0.5, 0.1, 1.0, _p(coef), _ptr_array(m1), _ptr_array(m2),
                                                            _p(gsc), _p(gam2), 0, NS, 0, A, NS, _p(out), st), 'sym')
            e[1].record()
            torch.cuda.synchronize()
            if r:
                t.append(e[0].elapsed_time(e[1]))
        res.append(float(np.median(t)))
        sums_out.append((float(out[:nt + 2 * M].sum()), float(m1[0].abs().sum())))
    return res, sums_out


def walk(A, M, reps, stash_bytes=16 << 30, jobs=None):
    """Every launch of the symmetric walk (loss_ops._sym_jobs, one rank), or of the given jobs, through the three-plane entry: its launch plan
    (sga_loss_anchor_plan: workgroups, modelled fill of the slots) and the median ms.  The plan is asked for ONE slot per CU: the three-plane
    kernels' own rows (88 KiB of LDS for two tables, 132 KiB for three) leave room for one workgroup per CU.  The launch itself takes its
    slots from the occupancy query (aa_launch.h: aa_slots), so if that kernel's LDS ever shrinks, this line prints another plan than the
    one that ran: change the factor here with it."""
    from sgaligner_amd import loss_ops, ops
    ops.STASH_BYTES = stash_bytes
    jobs = jobs or loss_ops._sym_jobs([0, A], 0, M)
    g = torch.Generator(device=dev).manual_seed(0)
    imgs = []
    for m in range(M):
        z = torch.zeros(2 * A + 32, 104, device=dev)
        z[:2 * A, :100] = torch.nn.functional.normalize(torch.randn(2 * A, 100, device=dev, generator=g), dim=1)
        im = torch.empty((L.sga_loss_split3_bytes(A, 0, 0),), device=dev, dtype=torch.uint8)
        _lib.check(L.sga_loss_split3_tables(_p(z), A, 0, 0, _p(im), None, st), 'split3')
        imgs.append(im)
        del z
    nt, slots = M + 1, 1 + L.sga_loss_slots()
    sums = torch.rand(nt, 8, device=dev, dtype=torch.float64, generator=g) * 1e5 + 1e5
    beta = torch.full((M,), 1.0 / M, device=dev)
    coef = (torch.rand(3 * M + 1, device=dev, generator=g) + 0.5) * 1e-4
    n1 = max((j_hi - j_lo) * (hi - lo) for lo, hi, j_lo, j_hi, mir in jobs)
    n2 = max(max(1, j_hi - mir) * (hi - lo) for lo, hi, j_lo, j_hi, mir in jobs)
    m1 = [torch.empty(n1, device=dev) for _ in range(M)]
    m2 = [torch.empty(n2, device=dev) for _ in range(M)]
    gsc = torch.empty(slots + 1, nt, 8, device=dev, dtype=torch.float64)
    gam2 = torch.empty(slots, M, device=dev, dtype=torch.float64)
    out = torch.empty(slots * (nt + 2 * M), device=dev, dtype=torch.float64)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    total, work, busy = 0.0, 0.0, 0.0
    for lo, hi, j_lo, j_hi, mir in jobs:
        t = []
        for r in range(reps + 1):
            e[0].record()
            _lib.check(L.sga_loss_anchor_multi_bwd_symx_bf16x6(_ptr_array(imgs), M, _p(beta), A, 0, 0, _p(sums), 0.5, 0.1, 1.0, _p(coef), _ptr_array(m1),
                                                               _ptr_array(m2), _p(gsc), _p(gam2), lo, hi, j_lo, j_hi, mir, _p(out), st), 'planes')
            e[1].record()
            torch.cuda.synchronize()
            if r:
                t.append(e[0].elapsed_time(e[1]))
        ms = float(np.median(t))
        total += ms
        plan = ''
        if hasattr(L, 'sga_loss_anchor_plan'):
            p = (ct.c_int32 * 8)()
            _lib.check(L.sga_loss_anchor_plan(1, M, A, lo, hi, j_lo, j_hi, cus, p), 'plan')
            rows, shares, nib, nib1, s1, s2, wgs, steps = p
            cost = [len(range(s, steps, s1)) + 1 for _ in range(nib1) for s in range(s1)] + [len(range(s, steps, s2)) + 1 for _ in range(nib - nib1) for s in range(s2)]
            free = [0] * min(cus, len(cost))
            for c in cost:          # greedy hand-out in launch order
                k = free.index(min(free))
                free[k] += c
            fill = sum(cost) / (cus * max(free))
            work += sum(cost); busy += cus * max(free)
            plan = f'{nib1:4d} x {s1:2d} + {nib - nib1:3d} x {s2:2d} = {wgs:5d} workgroups, modelled fill {fill:.3f} | '
        print(f'rows {hi - lo:6d} ({(hi - lo + 31) // 32:4d} row blocks) x columns [{j_lo}, {j_hi}): {plan}{ms:8.3f} ms | checksums {float(out[:nt + 2 * M].sum()):.9e} '
              f'{float(m1[0][:(j_hi - j_lo) * (hi - lo)].abs().sum()):.6e}', flush=True)
    print(f'walk M={M} A={A}: {len(jobs)} launches, {total:.3f} ms' + (f', modelled fill {work / busy:.4f} (work-weighted)' if busy else ''))


if mode == 'walk':
    walk(A, M, reps)
    sys.exit(0)
if mode == 'classes':                # the two tile classes, 8192 x 8192 each: all own-square (ordered epilogue) against all mirrored
    walk(A, M, reps, jobs=[(A - 8192, A, A - 8192, A, A), (0, 8192, 8192, 16384, 8192)])
    sys.exit(0)
if mode == 'crossover':
    for a in (1024, 2048, 4096, 8192, 19456, 38912):
        (f32, pl), cs = sym_block(a, 1024, M, reps, True)
        print(f'crossover M={M} symmetric 1024 x {a}: fp32 {f32:.3f} ms | three-plane {pl:.3f} ms | ratio {pl / f32:.3f} | checksums {cs[0][0]:.6e} {cs[1][0]:.6e}')
    sys.exit(0)
if mode == 'planes':
    (f32, pl), cs = sym_block(A, NS, M, reps, True)
    print(f'symmetric block M={M} {NS} x {A}: fp32 entry {f32:.3f} ms | three-plane entry {pl:.3f} ms | ratio {pl / f32:.3f} | term checksums {cs[0][0]:.9e} {cs[1][0]:.9e} '
          f'| stash checksums {cs[0][1]:.6e} {cs[1][1]:.6e}')
    sys.exit(0)
g = torch.Generator(device=dev).manual_seed(0)
zs = []
for m in range(M):
    z = torch.zeros(2 * A + 32, 104, device=dev)
    z[:2 * A, :100] = torch.nn.functional.normalize(torch.randn(2 * A, 100, device=dev, generator=g), dim=1)
    zs.append(z)
nt = M + 1
slots = 1 + L.sga_loss_slots()
sums = torch.rand(nt, 8, device=dev, dtype=torch.float64, generator=g) * 1e5 + 1e5
beta = torch.full((M,), 1.0 / M, device=dev)
coef = (torch.rand(3 * M + 1, device=dev, generator=g) + 0.5) * 1e-4
m1 = [torch.empty(A * NS, device=dev) for _ in range(M)]
gsc = torch.empty(slots + 1, nt, 8, device=dev, dtype=torch.float64)
gam2 = torch.empty(slots, M, device=dev, dtype=torch.float64)
out = torch.empty(slots * (nt + 2 * M), device=dev, dtype=torch.float64)
dz = [torch.zeros(2 * A + 32, 104, device=dev) for _ in range(M)]
zarr = _ptr_array(zs)
e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
tk, tg = [], []
for r in range(reps + 1):
    e[0].record()
    _lib.check(L.sga_loss_anchor_multi_bwd(zarr, M, _p(beta), A, _p(sums), 0.5, 0.1, 1.0, _p(coef), _ptr_array(m1), _p(gsc), _p(gam2), 0, NS, _p(out), st), 'aa')
    e[1].record()
    for k in range(M):
        _lib.check(L.sga_loss_stash_grad(_p(m1[k]), _p(zs[k]), A, 104, _p(dz[k]), 0, NS, st), 'sg')
    e[2].record()
    torch.cuda.synchronize()
    if r:
        tk.append(e[0].elapsed_time(e[1])); tg.append(e[1].elapsed_time(e[2]))
el = float(NS) * A
print(f'A x A kernel (M={M}, {NS} rows x {A} anchors): {np.median(tk):.3f} ms = {np.median(tk) * 1e6 / el:.4f} ns per (i, j) pair; stash GEMMs {np.median(tg):.3f} ms '
      f'({2.0 * 2 * M * el * 104 / np.median(tg) / 1e9:.1f} TFLOP/s); checksum {float(out[:nt + 2 * M].sum()):.6e} {float(m1[0].abs().sum()):.6e}')
# symmetric block: rows [0, NS) x columns [0, A), both elements of every pair -> compare HALF its time with the ordinary block above
if M <= 4 and NS % 32 == 0:
    m1s = [torch.empty(A * NS, device=dev) for _ in range(M)]
    m2s = [torch.empty((A - NS) * NS, device=dev) for _ in range(M)]
    ts, tgs = [], []
    for r in range(reps + 1):
        e[0].record()
        _lib.check(L.sga_loss_anchor_multi_bwd_symx(zarr, M, _p(beta), A, _p(sums), 0.5, 0.1, 1.0, _p(coef), _ptr_array(m1s), _ptr_array(m2s), _p(gsc), _p(gam2),
                                                    0, NS, 0, A, NS, _p(out), st), 'sym')
        e[1].record()
        for k in range(M):
            _lib.check(L.sga_loss_stash_grad_symx(_p(m1s[k]), _p(m2s[k]), _p(zs[k]), A, 104, _p(dz[k]), 0, NS, 0, A, NS, st), 'sgs')
        e[2].record()
        torch.cuda.synchronize()
        if r:
            ts.append(e[0].elapsed_time(e[1])); tgs.append(e[1].elapsed_time(e[2]))
    pairs = float(NS) * A * 2 - float(NS) * NS
    print(f'symmetric block: kernel {np.median(ts):.3f} ms = {np.median(ts) * 1e6 / pairs:.4f} ns per ordered pair; stash GEMMs {np.median(tgs):.3f} ms')
