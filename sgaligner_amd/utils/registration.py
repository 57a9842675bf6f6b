"""Registration and mosaicking metrics with the reference's signatures (utils/registration.py), the nearest-neighbour searches on the
GPU (csrc/nnsearch.hip through utils/point_cloud.py).  The searches return exact fp64 distances -- bit-identical to the KD-tree's -- and
every mean is taken by numpy on the host from those arrays, so the figures equal the reference's bit for bit.  The transform those
metrics judge comes from the second half of the file: RANSAC rigid registration from point correspondences, batched over pairs
(csrc/ransac.hip), with the shift and composition of src/engine/registration_evaluator.py:176-192 around it.  Nothing here falls back to
the host: without a HIP device the functions that need one raise."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import device_tensor, prefix_offsets, upload
from .point_cloud import _cloud64, _need_device, _nn_numpy, apply_transform, get_nearest_neighbor


def compute_modified_chamfer_distance(src_points, ref_points, raw_points, est_transform, gt_transform):
    """utils/registration.py:9-17: mean distance aligned-source -> raw plus mean distance reference -> raw moved by est * gt^-1."""
    _need_device('compute_modified_chamfer_distance')
    moved_src = apply_transform(src_points, est_transform)
    d_pq = get_nearest_neighbor(moved_src, raw_points).mean()
    moved_raw = apply_transform(raw_points, np.matmul(est_transform, np.linalg.inv(gt_transform)))
    d_qp = get_nearest_neighbor(ref_points, moved_raw).mean()
    return d_pq + d_qp


def compute_inlier_ratio(ref_corr_points, src_corr_points, transform, positive_radius=0.1):
    """utils/registration.py:19-24: share of correspondences closer than positive_radius after the transform."""
    diff = ref_corr_points - apply_transform(src_corr_points, transform)
    return np.mean(np.sqrt((diff ** 2).sum(1)) < positive_radius)


def compute_registration_rmse(ref_points, src_points, transform):
    """utils/registration.py:26-29."""
    moved = apply_transform(src_points, transform)
    return np.sqrt(((ref_points - moved) ** 2).sum() / moved.shape[0])


def get_rotation_translation_from_transform(transform, inverse_trans=False):
    """utils/registration.py:31-39: (R, t) of a 4x4; inverse_trans reads t from the last ROW (a transposed transform)."""
    return transform[:3, :3], (transform[3, :3] if inverse_trans else transform[:3, 3])


def compute_relative_rotation_error(gt_rotation: np.ndarray, est_rotation: np.ndarray):
    """Isotropic rotation error in degrees: acos((trace(est^T gt) - 1) / 2)."""
    c = np.clip(0.5 * (np.trace(np.matmul(est_rotation.T, gt_rotation)) - 1.0), -1.0, 1.0)
    return 180.0 * np.arccos(c) / np.pi


def compute_relative_translation_error(gt_translation: np.ndarray, est_translation: np.ndarray):
    """Isotropic translation error: |t_gt - t_est|."""
    return np.linalg.norm(gt_translation - est_translation)


def compute_registration_error(gt_transform: np.ndarray, est_transform: np.ndarray, inverse_trans=False):
    """(RRE in degrees, RTE) of two 4x4 transforms (utils/registration.py:91-105)."""
    gt_r, gt_t = get_rotation_translation_from_transform(gt_transform)
    est_r, est_t = get_rotation_translation_from_transform(est_transform, inverse_trans)
    return compute_relative_rotation_error(gt_r, est_r), compute_relative_translation_error(gt_t, est_t)


def _nn_lists(dist, idx):
    return [int(i) for i in idx], [d for d in dist]          # numpy float64 scalars, as np.sqrt(dist[0]) gives in the reference


def nn_correspondence(verts1, verts2):
    """utils/registration.py:107-129: for each vertex of verts2 the nearest vertex of verts1 -> ([indices], [distances]), the distances
    already rooted.  One launch instead of one KD-tree query per vertex; equal minima resolve to the lowest index."""
    if len(verts1) == 0 or len(verts2) == 0:
        return [], []
    _need_device('nn_correspondence')
    dist, idx = get_nearest_neighbor(verts2, verts1, return_index=True)
    return _nn_lists(dist, idx)


def compute_mosaicking_error(verts_pred, verts_gt, threshold=0.05):
    """utils/registration.py:131-143: precision / recall / F-score at `threshold` plus accuracy and completeness (mean distances).  Both
    directions go to the device in one upload and one launch."""
    if len(verts_pred) == 0 or len(verts_gt) == 0:
        dist1 = dist2 = np.array([])
    else:
        _need_device('compute_mosaicking_error')
        (dist1, _), (dist2, _) = _nn_numpy([_cloud64(verts_pred, 'verts_pred'), _cloud64(verts_gt, 'verts_gt')], [(1, 0), (0, 1)])
    precision = np.mean((dist2 < threshold).astype('float'))
    recall = np.mean((dist1 < threshold).astype('float'))
    return {'prec': precision, 'recall': recall, 'acc': np.mean(dist1), 'comp': np.mean(dist2),
            'fscore': 2 * precision * recall / (precision + recall)}


# ---- RANSAC rigid registration from point correspondences (src/engine/registration_evaluator.py:129-208, utils/open3d.py:172-201) ----------
RANSAC_CHUNK = None           # rows per workgroup pass of ransac_score_kernel; None = chosen per call (_ransac_chunk).  Tests lower it to
                              # force several chunks with a ragged last one on small inputs.
RANSAC_HYP_TILE = 1024        # hypotheses per workgroup of ransac_score_kernel (256 lanes x 4)
RANSAC_MIN_CHUNK = 128        # never split the rows finer than this: half an LDS tile, below it the staging barriers dominate


def _ransac_chunk(sizes_n, sizes_h) -> int:
    """Chunk size for a job list, by _nn_chunk's rule: split the rows just far enough that the grid fills the device a few times over
    (about 16 workgroups per CU), no further -- the count workspace is 4 B x n_chunks x total hypotheses.  A grid of more than one
    workgroup per CU is then trimmed to a whole number of workgroups per CU: the scoring kernel keeps three workgroups resident per CU,
    and a grid a few workgroups above that (785 on 256 CUs for one 20000 x 5000 job) pays a whole second round for them."""
    tiles = int(sum(-(-int(h) // RANSAC_HYP_TILE) for h in sizes_h)) or 1
    n_max = int(max(sizes_n, default=0))
    cus = int(_lib.lib().sga_device_cus())
    n_chunks = max(1, min(-(-16 * cus // tiles), -(-n_max // RANSAC_MIN_CHUNK)))
    if tiles * n_chunks > cus:
        n_chunks = max(1, (tiles * n_chunks // cus) * cus // tiles)
    return max(RANSAC_MIN_CHUNK, -(-n_max // n_chunks))


def find_rigid_transform_batch(corr, offsets, samples, hyp_offsets, threshold, refine_rounds=2, chunk=None):
    """corr [sum n, 6] float64 HIP tensor (jobs packed back to back; a row = source xyz | reference xyz), offsets [n_jobs+1] host ints,
    samples [sum H, 3] int32 HIP tensor of job-local row indices, hyp_offsets [n_jobs+1] host ints.  One launch set for all jobs, no shift,
    no random numbers: the result is a pure function of the arguments.  Returns a dict of HIP tensors: transform [n_jobs, 4, 4] float64
    (column-vector convention: apply_transform(src, T) ~ ref), inlier_count / best_hyp / status [n_jobs] int32 (status 1 = no model: identity,
    count 0, best_hyp -1), inlier_mask [sum n] uint8, hyp_count [sum H] int32 (the inlier count of every hypothesis).  refine_rounds = -1
    stops after the scoring: only hyp_count is meaningful then (score_hypotheses_batch)."""
    cr = device_tensor(corr, 'corr', torch.float64)
    if cr.dim() != 2 or cr.shape[1] != 6:
        raise ValueError(f'corr must be [N,6], got {tuple(cr.shape)}')
    dev = cr.device
    sm = samples if isinstance(samples, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int32))
    sm = sm.to(device=dev, dtype=torch.int32).contiguous().reshape(-1, 3)
    off = prefix_offsets(offsets, 'offsets', int(cr.shape[0]))
    hoff = prefix_offsets(hyp_offsets, 'hyp_offsets', int(sm.shape[0]))
    n_jobs = len(off) - 1
    if len(hoff) != n_jobs + 1:
        raise ValueError(f'offsets names {n_jobs} jobs, hyp_offsets {len(hoff) - 1}')
    if cr.shape[0] >= 2 ** 31 // 6 or sm.shape[0] >= 2 ** 31 // 3:
        raise ValueError('find_rigid_transform_batch indexes with int32: fewer than 2^31 / 6 rows and 2^31 / 3 hypotheses per call')
    threshold, refine_rounds = float(threshold), int(refine_rounds)
    if refine_rounds < -1:
        raise ValueError(f'refine_rounds must be >= 0 (or -1: scoring only), got {refine_rounds}')
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError(f'threshold must be finite and >= 0, got {threshold}')
    from .. import ops
    if ops.VALIDATE and cr.numel() and not bool(torch.isfinite(cr).all()):
        raise RuntimeError('sgaligner_amd: `corr` holds NaN or infinite coordinates')
    sizes_n, sizes_h = np.diff(off), np.diff(hoff)
    total, total_h = int(cr.shape[0]), int(sm.shape[0])
    out = {'transform': torch.empty((n_jobs, 4, 4), device=dev, dtype=torch.float64),
           'inlier_count': torch.empty((n_jobs,), device=dev, dtype=torch.int32),
           'best_hyp': torch.empty((n_jobs,), device=dev, dtype=torch.int32),
           'status': torch.empty((n_jobs,), device=dev, dtype=torch.int32),
           'inlier_mask': torch.empty((total,), device=dev, dtype=torch.uint8),
           'hyp_count': torch.empty((total_h,), device=dev, dtype=torch.int32)}
    if n_jobs == 0:
        return out
    chunk = int(chunk if chunk is not None else RANSAC_CHUNK if RANSAC_CHUNK is not None else _ransac_chunk(sizes_n, sizes_h))
    if chunk < 1:
        raise ValueError(f'chunk must be >= 1, got {chunk}')
    L = _lib.lib()
    h_off, h_hoff = off.astype(np.int32), hoff.astype(np.int32)
    d_off, d_hoff = upload([h_off, h_hoff], dev)                              # one small upload
    max_n, max_h = int(sizes_n.max()), int(sizes_h.max())
    ws_bytes = int(L.sga_ransac_workspace_bytes(n_jobs, total_h, max_n, chunk))
    ws = torch.empty((max((ws_bytes + 7) // 8, 1),), device=dev, dtype=torch.float64)
    rc = L.sga_ransac_rigid(_p(cr) if total else None, _p(d_off), n_jobs, total, _p(sm) if total_h else None, _p(d_hoff), total_h, max_n, max_h,
                            chunk, h_off.ctypes.data, h_hoff.ctypes.data, threshold, int(refine_rounds), _p(out['transform']),
                            _p(out['inlier_count']), _p(out['best_hyp']), _p(out['status']), _p(out['inlier_mask']) if total else None,
                            _p(out['hyp_count']) if total_h else None, _p(ws), ws_bytes, _stream())
    _lib.check(rc, 'sga_ransac_rigid')
    return out


def score_hypotheses_batch(corr, offsets, samples, hyp_offsets, threshold, chunk=None):
    """The scoring stage of find_rigid_transform_batch alone (same arguments): hyp_count [sum H] int32 HIP tensor, the number of rows each
    hypothesis' three-point model brings within `threshold`; 0 for an invalid sample."""
    return find_rigid_transform_batch(corr, offsets, samples, hyp_offsets, threshold, refine_rounds=-1, chunk=chunk)['hyp_count']


def draw_samples(sizes, iters, seed):
    """`iters` sample triples per job on the host, numpy.random.default_rng(seed): three DISTINCT row indices each (drawn from n, n-1 and
    n-2 values and shifted past the earlier picks, so no rejection loop).  A job with fewer than three rows gets no hypotheses.  The
    generator starts afresh from `seed` for every job, so a job's samples -- and with them its result -- do not depend on which other jobs
    share the call.  -> (samples [total, 3] int32, hyp_offsets [n_jobs+1] int64)."""
    iters = int(iters)
    parts, off = [], [0]
    for n in sizes:
        n = int(n)
        if n < 3 or iters <= 0:
            off.append(off[-1])
            continue
        rng = np.random.default_rng(seed)
        a, b, c = rng.integers(0, n, iters), rng.integers(0, n - 1, iters), rng.integers(0, n - 2, iters)
        b = b + (b >= a)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        c = c + (c >= lo)
        c = c + (c >= hi)
        parts.append(np.stack([a, b, c], axis=1))
        off.append(off[-1] + iters)
    samples = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 3), dtype=np.int32)
    return samples, np.asarray(off, dtype=np.int64)


def _corr64(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError(f'{name} must be [N, 6] (source xyz | reference xyz), got {a.shape}')
    return np.ascontiguousarray(a, dtype=np.float64)


def _ransac_numpy(packed, off, samples, hoff, threshold, refine_rounds):
    """numpy in, numpy out around find_rigid_transform_batch: one upload, one launch set, one download."""
    res = find_rigid_transform_batch(torch.from_numpy(packed).cuda(), off, torch.from_numpy(samples).cuda(), hoff, threshold, refine_rounds)
    return {k: v.cpu().numpy() for k, v in res.items()}


def find_rigid_transform_pairs(list_of_corrs, threshold=0.03, iters=5000, seed=0, refine_rounds=2):
    """find_rigid_transform for many correspondence arrays at once: one upload, one launch set, one download.  -> [(transform or None,
    info), ...] in the order given."""
    _need_device('find_rigid_transform_pairs')
    corrs = [_corr64(c, f'list_of_corrs[{i}]') for i, c in enumerate(list_of_corrs)]
    if not corrs:
        return []
    # registration_evaluator.py:176-177: the estimator sees the rows minus their per-column minimum
    shifts = [c.min(axis=0) if len(c) else np.zeros(6) for c in corrs]
    sizes = [len(c) for c in corrs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    samples, hoff = draw_samples(sizes, iters, seed)
    packed = np.concatenate([c - s for c, s in zip(corrs, shifts)])
    res = _ransac_numpy(packed, off, samples, hoff, threshold, refine_rounds)
    out = []
    for j, shift in enumerate(shifts):
        info = {'inlier_count': int(res['inlier_count'][j]), 'inlier_mask': res['inlier_mask'][off[j]:off[j + 1]].astype(bool),
                'best_hyp': int(res['best_hyp'][j]), 'status': int(res['status'][j]), 'shift': shift}
        if info['status'] != 0:
            out.append((None, info))
            continue
        # registration_evaluator.py:186-192 (T1 @ est @ T2inv, transposed) in the column convention: r = R (s - a) + t + b
        T = res['transform'][j].copy()
        T[:3, 3] = T[:3, 3] - T[:3, :3] @ shift[:3] + shift[3:]
        out.append((T, info))
    return out


def find_rigid_transform(corrs, threshold=0.03, iters=5000, seed=0, refine_rounds=2):
    """pygcransac.findRigidTransform as registration_evaluator.py:176-192 uses it (fixed iteration count, no spatial coherence), shift
    included: corrs [n, 6] numpy (source xyz | reference xyz) -> (transform [4, 4] with apply_transform(src, T) ~ ref, or None when there
    is no model; info = dict(inlier_count, inlier_mask, best_hyp, status, shift))."""
    _need_device('find_rigid_transform')
    return find_rigid_transform_pairs([corrs], threshold, iters, seed, refine_rounds)[0]


def registration_with_ransac_from_correspondences(src_points, ref_points, correspondences=None, distance_threshold=0.05, ransac_n=3,
                                                  num_iterations=10000):
    """utils/open3d.py:172-201 on the same kernel: src_points / ref_points [N, 3]; correspondences [M, 2] (source index, reference index),
    None = row i of one with row i of the other.  -> 4x4 transform (identity when no model is found)."""
    if ransac_n != 3:
        raise ValueError(f'registration_with_ransac_from_correspondences: only ransac_n == 3 is implemented (got {ransac_n})')
    _need_device('registration_with_ransac_from_correspondences')
    src, ref = _cloud64(src_points, 'src_points'), _cloud64(ref_points, 'ref_points')
    if correspondences is None:
        if len(src) != len(ref):
            raise ValueError(f'without correspondences src_points and ref_points pair row by row: {len(src)} != {len(ref)} rows')
        corr = np.concatenate([src, ref], axis=1)
    else:
        idx = np.asarray(correspondences, dtype=np.int64).reshape(-1, 2)
        corr = np.concatenate([src[idx[:, 0]], ref[idx[:, 1]]], axis=1)
    T, _ = find_rigid_transform(corr, threshold=distance_threshold, iters=num_iterations)
    return np.eye(4) if T is None else T
