"""In-tree build of the HIP C-ABI library: hipcc --offload-arch=gfx950 csrc/*.hip -> csrc/libsga_hip.so.

Cross-compiles without a GPU (used by __graft_entry__.build()).  Objects are rebuilt only when their
source (or a header) is newer; the .so travels to the GPU box with the gpurun snapshot.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
LIB = os.path.join(CSRC, 'libsga_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=fast', '-munsafe-fp-atomics',
         '-Wno-unused-result', '-Wno-unused-value', '-I', CSRC]


def _newer(src_list, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


# Per-source flags.  The loss kernels (contrastive.hip, loss_pertable.hip, loss_anchor.hip, anchor3.hip): SLP-packed v_pk_mul/v_pk_fma_f32 (+ the v_movs that assemble their operand pairs) in the sweep
# epilogues are slower beside fp32 MFMAs than the scalar instructions they replace (MI355X_MICROARCH guide; measured here: backward sweep
# 0.767 -> 0.770 of peak, configs[2] step 7.243 -> 7.226 s).
FILE_FLAGS = {'contrastive.hip': ['-fno-slp-vectorize'],
              'loss_pertable.hip': ['-fno-slp-vectorize'],
              'loss_anchor.hip': ['-fno-slp-vectorize'],
              'sweep3.hip': ['-fno-slp-vectorize'],
              'anchor3.hip': ['-fno-slp-vectorize'],
              'pointnet.hip': ['-fno-slp-vectorize'],
              # nnsearch.hip: every fp64 operation rounded on its own -- the distances are bit-identical to the host KD-tree's (no FMA)
              'nnsearch.hip': ['-ffp-contract=off'],
              # featnn.hip: the fp64 distance to the chosen row is a sequential sum of separately rounded squares (no FMA)
              'featnn.hip': ['-ffp-contract=off'],
              # fpfh.hip: neighbour-list distances bit-identical to nnsearch.hip's, and the FPFH weighting's pinned fp64 operation order (no FMA)
              'fpfh.hip': ['-ffp-contract=off'],
              # voxel.hip: cell coordinates and voxel means bit-identical to their NumPy restatement, list distances to fpfh.hip's (no FMA)
              'voxel.hip': ['-ffp-contract=off'],
              # icp.hip: moved queries and distances bit-identical to their NumPy restatement and to nnsearch.hip's (no FMA)
              'icp.hip': ['-ffp-contract=off'],
              # ransac_geo.hip: the search's arithmetic, and a residual that NumPy recomputes bit for bit from the stored model (no FMA)
              'ransac_geo.hip': ['-ffp-contract=off'],
              # visibility.hip: same -- the frustum tests are bit-identical to the NumPy restatement of the reference's projection
              'visibility.hip': ['-ffp-contract=off']}


def _compile(src, obj, extra):
    cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + extra + ['-c', src, '-o', obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed for {src}:\n{r.stdout}\n{r.stderr}')
    return src


def build_lib(verbose: bool = True, extra_flags=()) -> str:
    srcs = sorted(glob.glob(os.path.join(CSRC, '*.hip')))
    hdrs = sorted(glob.glob(os.path.join(CSRC, '*.h'))) + sorted(glob.glob(os.path.join(CSRC, '..', '..', 'include', '*.h')))
    jobs = []
    objs = []
    for s in srcs:
        o = s[:-4] + '.o'
        objs.append(o)
        if _newer([s] + hdrs, o):
            jobs.append((s, o))
    if jobs:
        with cf.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            for done in ex.map(lambda so: _compile(so[0], so[1], list(extra_flags)), jobs):
                if verbose:
                    print('[sga build] compiled', os.path.basename(done), flush=True)
    if jobs or _newer(objs, LIB):
        r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stdout}\n{r.stderr}')
        if verbose:
            print('[sga build] linked', LIB, flush=True)
    return LIB


if __name__ == '__main__':
    build_lib(extra_flags=sys.argv[1:])
