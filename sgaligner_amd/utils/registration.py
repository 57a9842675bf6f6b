"""Registration and mosaicking metrics with the reference's signatures (utils/registration.py), the nearest-neighbour searches on the
GPU (csrc/nnsearch.hip through utils/point_cloud.py).  The searches return exact fp64 distances -- bit-identical to the KD-tree's -- and
every mean is taken by numpy on the host from those arrays, so the figures equal the reference's bit for bit.  The transform those
metrics judge comes from the second half of the file: RANSAC rigid registration from point correspondences, batched over pairs
(csrc/ransac.hip), with the shift and composition of src/engine/registration_evaluator.py:176-192 around it.  The last part is registration from per-point
descriptors (utils/open3d.py:137-170): an exact nearest-neighbour search in feature space on the fp32 matrix cores (csrc/featnn.hip),
the mutual filter and Open3D's edge-length checker as gathers and compares on the device, then the same RANSAC; and ICP refinement with
the geometric score of a transform (csrc/icp.hip: a nearest-neighbour search across clouds through a cell grid, batched over pairs);
and that score as RANSAC's own criterion, fused over thousands of hypotheses (csrc/ransac_geo.hip).  Nothing here falls back
to the host: without a HIP device the functions that need one raise."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import HypJobs, PairJobs, check_finite, device_tensor, pair_ids, prefix_offsets, resolve_chunk, split_chunk, upload, workspace
from .point_cloud import _cloud64, _need_device, _nn_numpy, _search_grid, apply_transform, get_nearest_neighbor


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
    """Chunk size for a job list, by packed.split_chunk: about 16 workgroups per CU, no further -- the count workspace is 4 B x n_chunks x
    total hypotheses -- in whole rounds: the scoring kernel keeps three workgroups resident per CU, and a grid a few workgroups above that
    (785 on 256 CUs for one 20000 x 5000 job) pays a whole second round for them."""
    tiles = sum(-(-int(h) // RANSAC_HYP_TILE) for h in sizes_h)
    return split_chunk(tiles, max(sizes_n, default=0), _lib.lib().sga_device_cus(), 16, RANSAC_MIN_CHUNK, whole_rounds=True)


def find_rigid_transform_batch(corr, offsets, samples, hyp_offsets, threshold, refine_rounds=2, chunk=None):
    """corr [sum n, 6] float64 HIP tensor (jobs packed back to back; a row = source xyz | reference xyz), offsets [n_jobs+1] host ints,
    samples [sum H, 3] int32 HIP tensor of job-local row indices, hyp_offsets [n_jobs+1] host ints.  One launch set for all jobs, no shift,
    no random numbers: the result is a pure function of the arguments.  Returns a dict of HIP tensors: transform [n_jobs, 4, 4] float64
    (column-vector convention: apply_transform(src, T) ~ ref), inlier_count / best_hyp / status [n_jobs] int32 (status 1 = no model: identity,
    count 0, best_hyp -1), inlier_mask [sum n] uint8, hyp_count [sum H] int32 (the inlier count of every hypothesis).  refine_rounds = -1
    stops after the scoring: only hyp_count is meaningful then (score_hypotheses_batch)."""
    J = HypJobs(corr, offsets, samples, hyp_offsets, convert_samples=True)
    J.check_int32('find_rigid_transform_batch', 3)
    cr, sm, dev, n_jobs, total, total_h = J.corr, J.samples, J.corr.device, J.n_jobs, J.total, J.total_h
    threshold, refine_rounds = float(threshold), int(refine_rounds)
    if refine_rounds < -1:
        raise ValueError(f'refine_rounds must be >= 0 (or -1: scoring only), got {refine_rounds}')
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError(f'threshold must be finite and >= 0, got {threshold}')
    check_finite(cr, 'corr', 'coordinates')
    out = {'transform': torch.empty((n_jobs, 4, 4), device=dev, dtype=torch.float64),
           'inlier_count': torch.empty((n_jobs,), device=dev, dtype=torch.int32),
           'best_hyp': torch.empty((n_jobs,), device=dev, dtype=torch.int32),
           'status': torch.empty((n_jobs,), device=dev, dtype=torch.int32),
           'inlier_mask': torch.empty((total,), device=dev, dtype=torch.uint8),
           'hyp_count': torch.empty((total_h,), device=dev, dtype=torch.int32)}
    if n_jobs == 0:
        return out
    chunk = resolve_chunk(chunk, RANSAC_CHUNK, lambda: _ransac_chunk(J.sizes_n, J.sizes_h))
    L = _lib.lib()
    d_off, d_hoff = upload([J.h_off, J.h_hoff], dev)                          # one small upload
    ws_bytes = int(L.sga_ransac_workspace_bytes(n_jobs, total_h, J.max_n, chunk))
    ws = workspace(ws_bytes, dev)
    rc = L.sga_ransac_rigid(_p(cr) if total else None, _p(d_off), n_jobs, total, _p(sm) if total_h else None, _p(d_hoff), total_h, J.max_n, J.max_h,
                            chunk, J.h_off.ctypes.data, J.h_hoff.ctypes.data, threshold, int(refine_rounds), _p(out['transform']),
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


# ---- registration from per-point descriptors (utils/open3d.py:137-170; src/engine/registration_evaluator.py:92-127) ----------------------
FEATNN_CHUNK = None           # support rows per workgroup pass of csrc/featnn.hip; None = chosen per call (_featnn_chunk).  Tests lower it to
                              # force the split (chunked + folded) form on small inputs.
FEATNN_QUERY_TILE = 128       # queries per workgroup of featnn_kernel (4 waves x 32)
FEATNN_SUPPORT_TILE = 128     # support rows per staged LDS tile
FEATNN_MIN_CHUNK = 1024       # never split a support finer than this: 8 staged tiles, below it the partial workspace and the fold cost
                              # more than idle CUs


def _featnn_chunk(sizes_q, sizes_s) -> int:
    """Chunk size for a job list, by packed.split_chunk: about 4 workgroups per CU (the kernel keeps two resident), no further -- the partial
    workspace is 8 B x n_chunks x total queries.  A whole number of staged tiles, so that only a support's last tile is ragged."""
    tiles = sum(-(-int(q) // FEATNN_QUERY_TILE) for q in sizes_q)
    return split_chunk(tiles, max(sizes_s, default=0), _lib.lib().sga_device_cus(), 4, FEATNN_MIN_CHUNK, round_to=FEATNN_SUPPORT_TILE)


def _featnn_tiles(nq, ns, chunk):
    """The grid of featnn_kernel as a list: (job, query tile, chunk) for every tile a job has; the chunk-0 entries first (they also drive
    the closing kernel).  -> (tiles [n, 3] int32, number of chunk-0 entries)."""
    q_tiles = -(-np.asarray(nq, dtype=np.int64) // FEATNN_QUERY_TILE)
    chunks = np.where(np.asarray(ns) <= chunk, 1, -(-np.asarray(ns, dtype=np.int64) // chunk))
    job = np.repeat(np.arange(len(q_tiles), dtype=np.int64), q_tiles)
    qt = np.arange(len(job), dtype=np.int64) - np.repeat(np.cumsum(q_tiles) - q_tiles, q_tiles)
    reps = chunks[job]
    c = np.arange(int(reps.sum()), dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
    full = np.stack([np.repeat(job, reps), np.repeat(qt, reps), c], axis=1)
    order = np.argsort(c != 0, kind='stable')
    return np.ascontiguousarray(full[order], dtype=np.int32), int(len(job))


def feature_nn_batch(feats, offsets, pairs, chunk=None):
    """feats [sum N, C] float32 HIP tensor (feature sets packed back to back), offsets [n_sets+1] host ints, pairs [n_pairs, 2] host ints
    (query set, support set).  One small upload and one launch set for all jobs.  Returns (idx [sum nq] int32, d2 [sum nq] float64,
    out_offsets [n_pairs+1] int64 numpy): job p's results are idx[out_offsets[p]:out_offsets[p+1]].  idx is support-set-local: the arg-min
    of the fp32 score |b|^2 - 2 a.b (csrc/featnn.hip), the LOWEST index among exactly equal scores, -1 for an empty support; d2 is the
    fp64 squared distance to that row, summed in ascending column order (+inf with -1).  A width that is no multiple of 4 is padded with
    zero columns, which change neither."""
    ft = device_tensor(feats, 'feats', torch.float32)
    if ft.dim() != 2 or ft.shape[1] < 1:
        raise ValueError(f'feats must be [N, C] with C >= 1, got {tuple(ft.shape)}')
    J = PairJobs(offsets, ft.shape[0], pairs, 'feature_nn_batch', 'set')
    check_finite(ft, 'feats', 'values')
    dev = ft.device
    idx = torch.empty((J.total_q,), device=dev, dtype=torch.int32)
    d2 = torch.empty((J.total_q,), device=dev, dtype=torch.float64)
    if J.total_q == 0:
        return idx, d2, J.out_off
    if ft.shape[1] % 4:
        ft = torch.nn.functional.pad(ft, (0, 4 - ft.shape[1] % 4))
    if ft.data_ptr() % 16:
        ft = ft.clone()
    chunk = resolve_chunk(chunk, FEATNN_CHUNK, lambda: _featnn_chunk(J.nq, J.ns))
    L = _lib.lib()
    h_tiles, n_qt = _featnn_tiles(J.nq, J.ns, chunk)
    d_off, d_pr, d_oo, d_tiles = upload(J.host_parts() + [h_tiles], dev)                     # one small upload
    total, C = int(ft.shape[0]), int(ft.shape[1])
    ws_bytes = int(L.sga_featnn_workspace_bytes(total, J.total_q, J.max_s, chunk))
    ws = workspace(ws_bytes, dev)
    rc = L.sga_featnn_search(_p(ft), C, _p(d_off), J.n_sets, total, _p(d_pr), J.n_pairs, _p(d_oo), _p(d_tiles), len(h_tiles), n_qt, J.total_q,
                             J.max_q, J.max_s, chunk, J.h_off.ctypes.data, J.h_pr.ctypes.data, h_tiles.ctypes.data, _p(idx), _p(d2), _p(ws),
                             ws_bytes, _stream())
    _lib.check(rc, 'sga_featnn_search')
    return idx, d2, J.out_off


def _feat32(a, name):
    """One feature set as a float32 [n, C] HIP tensor: a device tensor as it is, a numpy array uploaded; a CPU tensor is refused."""
    if isinstance(a, torch.Tensor):
        t = device_tensor(a, name, torch.float32)
    else:
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError(f'{name} must be [n, C], got {a.shape}')
        _need_device(name)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    if t.dim() != 2:
        raise ValueError(f'{name} must be [n, C], got {tuple(t.shape)}')
    return t


def match_features_pairs(list_of_feats, mutual=True):
    """list_of_feats: [(src_feats [n, C], ref_feats [m, C]), ...] (float32 HIP tensors, or numpy arrays that are uploaded; every set of the
    call has the same C).  Both directions of every pair go to the device in ONE feature_nn_batch call.  mutual=True keeps (i, j) iff
    nn(i) = j and nn(j) = i -- a gather and a compare on the device; mutual=False keeps every source row with its nearest reference row
    (what Open3D's registration_ransac_based_on_feature_matching does when the reference calls it: no mutual filter).  -> per pair
    (correspondences [k, 2] int64 sorted by source index, d2 [k] float64), HIP tensors."""
    sets = [_feat32(f, f'list_of_feats[{i}][{j}]') for i, p in enumerate(list_of_feats) for j, f in enumerate(p)]
    if not sets:
        return []
    if len({int(t.shape[1]) for t in sets}) != 1:
        raise ValueError('every feature set of one call must have the same width')
    n_pairs = len(sets) // 2
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t in sets])]).astype(np.int64)
    pairs = [(2 * p, 2 * p + 1) for p in range(n_pairs)] + ([(2 * p + 1, 2 * p) for p in range(n_pairs)] if mutual else [])
    idx, d2, oo = feature_nn_batch(torch.cat(sets) if len(sets) > 1 else sets[0], off, pairs)
    idx = idx.long()
    out = []
    for p in range(n_pairs):
        fwd, dist = idx[oo[p]:oo[p + 1]], d2[oo[p]:oo[p + 1]]
        keep = fwd >= 0
        if mutual:
            back = idx[oo[n_pairs + p]:oo[n_pairs + p + 1]]
            if back.numel():
                keep &= back[fwd.clamp(min=0)] == torch.arange(fwd.numel(), device=fwd.device)
        src = torch.nonzero(keep).reshape(-1)                                        # ascending: sorted by source index
        out.append((torch.stack([src, fwd[src]], dim=1), dist[src]))
    return out


def edge_length_filter(corr, offsets, samples, hyp_offsets, similarity=0.9):
    """Open3D's CorrespondenceCheckerBasedOnEdgeLength on a packed hypothesis list, on the device (arguments as find_rigid_transform_batch
    takes them).  A triple passes iff for each of its three point pairs d_src >= similarity * d_ref and d_ref >= similarity * d_src, d the
    fp64 distance sqrt((dx*dx + dy*dy) + dz*dz) between the two rows on that side.  A failing triple is overwritten with an invalid one
    (its first index three times), which sga_ransac_rigid scores 0 and never selects: hypothesis indices keep their meaning.  -> samples
    [sum H, 3] int32 HIP tensor (a new one)."""
    J = HypJobs(corr, offsets, samples, hyp_offsets, corr_shape=False)
    cr, sm = J.corr, J.samples
    if sm.shape[0] == 0:
        return sm.clone()
    sizes = torch.from_numpy(np.repeat(J.sizes_n, J.sizes_h)).to(cr.device)
    base = torch.from_numpy(np.repeat(J.off[:-1], J.sizes_h)).to(cr.device)
    local = sm.long()
    ok = ((local >= 0) & (local < sizes[:, None])).all(dim=1)
    rows = cr[(local.clamp(min=0) + base[:, None]).clamp(max=max(int(cr.shape[0]) - 1, 0))]      # [H, 3, 6]
    for a, b in ((0, 1), (1, 2), (2, 0)):
        d = rows[:, a] - rows[:, b]
        sq = d * d
        d_src = torch.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        d_ref = torch.sqrt((sq[:, 3] + sq[:, 4]) + sq[:, 5])
        ok &= (d_src >= similarity * d_ref) & (d_ref >= similarity * d_src)
    return torch.where(ok[:, None], sm, sm[:, :1].expand(-1, 3)).contiguous()


def registration_with_ransac_from_feats_pairs(list_of_clouds, distance_threshold=0.05, ransac_n=3, num_iterations=50000, val_iterations=1000,
                                              mutual=False, seed=0, score='correspondence', return_info=False):
    """registration_with_ransac_from_feats for many pairs: list_of_clouds = [(src_points, ref_points, src_feats, ref_feats), ...].  One
    matching launch set and one RANSAC launch set for all of them.  -> [4x4 transform, ...] in the order given; with return_info
    [(transform, info), ...]."""
    if ransac_n != 3:
        raise ValueError(f'registration_with_ransac_from_feats: only ransac_n == 3 is implemented (got {ransac_n})')
    if score not in RANSAC_SCORES:
        raise ValueError(f'score must be one of {RANSAC_SCORES}, got {score!r}')
    _need_device('registration_with_ransac_from_feats')
    clouds = [(_cloud64(s, f'list_of_clouds[{i}][0]'), _cloud64(r, f'list_of_clouds[{i}][1]'), sf, rf)
              for i, (s, r, sf, rf) in enumerate(list_of_clouds)]
    if not clouds:
        return []
    for i, (s, r, sf, rf) in enumerate(clouds):
        if len(s) != len(sf) or len(r) != len(rf):
            raise ValueError(f'list_of_clouds[{i}]: one feature row per point ({len(s)} / {len(sf)} source, {len(r)} / {len(rf)} reference)')
    matches = match_features_pairs([(sf, rf) for _, _, sf, rf in clouds], mutual=mutual)
    dev = matches[0][0].device
    pts = torch.from_numpy(np.concatenate([np.concatenate([s, r]) for s, r, _, _ in clouds])).to(dev)
    rows, base = [], 0
    for (s, r, _, _), (cij, _) in zip(clouds, matches):
        rows.append(torch.cat([pts[base + cij[:, 0]], pts[base + len(s) + cij[:, 1]]], dim=1))
        base += len(s) + len(r)
    sizes = [int(c.shape[0]) for c in rows]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    samples, hoff = draw_samples(sizes, num_iterations, seed)
    corr = torch.cat(rows)
    checked = edge_length_filter(corr, off, torch.from_numpy(samples).to(dev), hoff)
    if score == 'geometric':
        # cloud 2p is pair p's source (the queries), cloud 2p + 1 its reference (the support): `pts` is packed that way
        c_off = np.concatenate([[0], np.cumsum([len(c) for s, r, _, _ in clouds for c in (s, r)])]).astype(np.int64)
        res = ransac_geometric_batch(pts, c_off, [(2 * p, 2 * p + 1) for p in range(len(clouds))], corr, off, checked, hoff, distance_threshold,
                                     val_iterations)
        keys = ('fitness', 'inlier_rmse', 'best_hyp', 'n_validated')
    else:
        res = find_rigid_transform_batch(corr, off, checked, hoff, distance_threshold)
        keys = ('inlier_count', 'best_hyp')
    status, transform = res['status'].cpu().numpy(), res['transform'].cpu().numpy()
    out = [np.eye(4) if status[j] != 0 else transform[j] for j in range(len(clouds))]
    if not return_info:
        return out
    host = {k: res[k].cpu().numpy() for k in keys}
    return [(T, {'status': int(status[j]), **{k: host[k][j].item() for k in keys}}) for j, T in enumerate(out)]


def registration_with_ransac_from_feats(src_points, ref_points, src_feats, ref_feats, distance_threshold=0.05, ransac_n=3,
                                        num_iterations=50000, val_iterations=1000, mutual=False, seed=0, score='correspondence',
                                        return_info=False):
    """utils/open3d.py:137-170 (Open3D's registration_ransac_based_on_feature_matching) on the device: the reference signature plus
    `mutual`, `seed`, `score` and `return_info`.  src_points / ref_points [N, 3], src_feats / ref_feats [N, C] (numpy, or float32 HIP
    tensors for the features).  -> 4x4 transform with apply_transform(src, T) ~ ref, identity when no model is found; with return_info
    (transform, info).
      1. correspondences from match_features_pairs: every source row with its nearest reference row in feature space (mutual=False, as
         the reference's call), or the mutual nearest neighbours only;
      2. `num_iterations` sample triples of correspondences from draw_samples (numpy.random.default_rng(seed));
      3. Open3D's edge-length checker (0.9) on the triples (edge_length_filter), before scoring;
      4. score='correspondence' (the default): find_rigid_transform_batch with threshold = distance_threshold;
         score='geometric': ransac_geometric_batch with max_validation = val_iterations.
    ransac_n != 3 and an unknown score raise ValueError.
    Against Open3D.  score='geometric' is Open3D's rule: a hypothesis must also pass the distance checker (its three sampled pairs within
    distance_threshold under its own model); the first val_iterations hypotheses that pass both checkers, in the order drawn, are each
    scored by a nearest-neighbour search of ALL source points against the reference cloud (evaluate_registration at distance_threshold);
    the best fitness wins, then the smaller inlier RMSE, then the earlier hypothesis; and the three-point model is returned as it is,
    without a refit.  What remains different: the iteration count is fixed -- all num_iterations triples are drawn and checked, Open3D's
    confidence-based early stop is not reproduced -- and the random numbers are numpy's, so single results differ from Open3D's run by run.
    score='correspondence' departs further, as it always has: a model is scored on the feature correspondences (the rows its transform
    brings within distance_threshold), every hypothesis is scored in full so the distance checker is not needed and not applied,
    val_iterations is unused, and the winner is refitted on its inliers (find_rigid_transform_batch).
    info (return_info=True): status, best_hyp, and fitness / inlier_rmse / n_validated ('geometric') or inlier_count ('correspondence')."""
    return registration_with_ransac_from_feats_pairs([(src_points, ref_points, src_feats, ref_feats)], distance_threshold, ransac_n,
                                                     num_iterations, val_iterations, mutual, seed, score, return_info)[0]


# ---- ICP refinement and the geometric score of a transform (csrc/icp.hip) ------------------------------------------------------------------
ICP_METHODS = {'point': 0, 'plane': 1}
ICP_STATUS_TEXT = {0: 'ok', 1: 'too few correspondences for an update', 2: 'the update could not be solved', 3: 'bad job'}


def _model12(T):
    """4x4 (or 3x4) transforms [..., 4, 4] -> the kernels' row-major [R | t] rows [..., 12]."""
    T = np.asarray(T, dtype=np.float64)
    return np.concatenate([T[..., :3, :3].reshape(T.shape[:-2] + (9,)), T[..., :3, 3]], axis=-1)


def _matrix44(m):
    """[n, 12] model rows -> [n, 4, 4]."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 12)
    T = np.tile(np.eye(4), (len(m), 1, 1))
    T[:, :3, :3] = m[:, :9].reshape(-1, 3, 3)
    T[:, :3, 3] = m[:, 9:]
    return T


def icp_batch(points, offsets, pairs, transforms, max_distance, method='point', normals=None, max_iters=30, relative_fitness=1e-6,
              relative_rmse=1e-6, cell=None):
    """The device-resident form of icp_pairs: points [sum N, 3] float64 HIP tensor (clouds packed back to back), offsets [n_clouds + 1] host
    ints, pairs [n_pairs, 2] host ints (source cloud, reference cloud), transforms [n_pairs, 12] float64 HIP tensor (row-major R | t, the
    initial estimates; not modified), normals [sum N, 3] float64 HIP tensor (read at the reference clouds' rows; method 'plane').  The grid
    of every cloud is built once (cell: None = point_cloud.nn_grid_cell), the pivots are the reference clouds' box minima, then ONE sga_icp call: 3
    (max_iters + 1) launches on torch's current stream and no synchronisation.  -> dict of HIP tensors: transform [n_pairs, 12], fitness,
    inlier_rmse [n_pairs] float64, iterations, status [n_pairs] int32, trace [n_pairs, max_iters + 1, 2], idx [sum nq] int32, d2 [sum nq]
    float64 (the correspondences of the FINAL transform, reference-cloud-local, -1 / +inf without one), and out_offsets (host)."""
    if method not in ICP_METHODS:
        raise ValueError(f'method must be one of {tuple(ICP_METHODS)}, got {method!r}')
    max_iters, max_distance = int(max_iters), float(max_distance)
    if max_iters < 0:
        raise ValueError(f'max_iters must be >= 0, got {max_iters}')
    if not max_distance > 0.0:
        raise ValueError(f'max_distance must be > 0 (inf: no limit), got {max_distance}')
    if method == 'plane' and normals is None:
        raise ValueError("method 'plane' needs the reference clouds' normals")
    pts = device_tensor(points, 'points', torch.float64)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f'points must be [N, 3], got {tuple(pts.shape)}')
    J = PairJobs(offsets, pts.shape[0], pairs, 'icp_batch', 'cloud')
    T = device_tensor(transforms, 'transforms', torch.float64).reshape(-1, 12).clone()
    if T.shape[0] != J.n_pairs:
        raise ValueError(f'transforms must be [{J.n_pairs}, 12], got {tuple(transforms.shape)}')
    nr = None
    if normals is not None:
        nr = device_tensor(normals, 'normals', torch.float64)
        if tuple(nr.shape) != tuple(pts.shape):
            raise ValueError(f'normals must be {tuple(pts.shape)}, got {tuple(nr.shape)}')
    check_finite(pts, 'points', 'coordinates')
    dev, n = pts.device, J.n_pairs
    out = {'transform': T, 'fitness': torch.zeros((n,), device=dev, dtype=torch.float64),
           'inlier_rmse': torch.zeros((n,), device=dev, dtype=torch.float64), 'iterations': torch.zeros((n,), device=dev, dtype=torch.int32),
           'status': torch.zeros((n,), device=dev, dtype=torch.int32),
           'trace': torch.full((n, max_iters + 1, 2), float('nan'), device=dev, dtype=torch.float64),
           'idx': torch.full((J.total_q,), -1, device=dev, dtype=torch.int32),
           'd2': torch.full((J.total_q,), float('inf'), device=dev, dtype=torch.float64), 'out_offsets': J.out_off}
    if n == 0:
        return out
    L = _lib.lib()
    C, G = _search_grid(pts, J.off, max_distance, cell)
    _, d_pr, d_oo = upload(J.host_parts(), dev)
    box = torch.empty((J.n_sets, 6), device=dev, dtype=torch.float64)
    _lib.check(L.sga_cloud_bounds(_p(pts), *C.args(), _p(box), 1.0, None, _stream()), 'sga_cloud_bounds')
    pivot = box[d_pr.view(-1, 2)[:, 1].long(), :3]
    pivot = torch.where(torch.isfinite(pivot), pivot, torch.zeros_like(pivot)).contiguous()       # a reference cloud without a kept point
    ws_bytes = int(L.sga_icp_workspace_bytes(n, J.max_q))
    ws = workspace(ws_bytes, dev)
    rc = L.sga_icp(_p(pts), _p(C.d_off), J.n_sets, int(pts.shape[0]), _p(d_pr), n, _p(d_oo), J.total_q, J.max_q, J.h_off.ctypes.data,
                   J.h_pr.ctypes.data, *G.search_args(), max_distance * max_distance, ICP_METHODS[method], _p(nr), _p(pivot), max_iters,
                   float(relative_fitness), float(relative_rmse), _p(T), _p(out['fitness']), _p(out['inlier_rmse']), _p(out['iterations']),
                   _p(out['status']), _p(out['trace']), _p(out['idx']), _p(out['d2']), _p(ws), ws_bytes, _stream())
    _lib.check(rc, 'sga_icp')
    return out


def icp_pairs(list_of_pairs, init_transforms=None, max_distance=0.05, method='point', ref_normals=None, max_iters=30, relative_fitness=1e-6,
              relative_rmse=1e-6, cell=None):
    """ICP refinement of many (source, reference) cloud pairs at once -- Open3D's registration_icp loop, point-to-point or point-to-plane:
    list_of_pairs = [(src_points [n, 3], ref_points [m, 3]), ...] numpy; init_transforms: one 4x4 per pair (None: identity); ref_normals:
    one [m, 3] array per pair for method 'plane' (None: estimated on the device from the reference clouds' 30 nearest neighbours through the
    grid, features.estimate_normals_batch(search='grid')).  One upload, one launch set, one download.  -> per pair a dict: transformation
    [4, 4] with apply_transform(src, T) ~ ref, fitness (share of source points with a reference point within max_distance), inlier_rmse,
    correspondence_set [k, 2] int64 (source index, reference index) of the final transform, iterations, status (0 ok; 1 too few
    correspondences and 2 an unsolvable update: the transform is the last good one), trace [evaluations, 2] (fitness, rmse of each)."""
    _need_device('icp_pairs')
    if method not in ICP_METHODS:
        raise ValueError(f'method must be one of {tuple(ICP_METHODS)}, got {method!r}')
    if int(max_iters) < 0:
        raise ValueError(f'max_iters must be >= 0, got {max_iters}')
    prs = [(_cloud64(s, f'list_of_pairs[{i}][0]'), _cloud64(r, f'list_of_pairs[{i}][1]')) for i, (s, r) in enumerate(list_of_pairs)]
    n = len(prs)
    if n == 0:
        return []
    init = np.tile(np.eye(4), (n, 1, 1)) if init_transforms is None else np.asarray(init_transforms, dtype=np.float64).reshape(-1, 4, 4)
    if len(init) != n:
        raise ValueError(f'init_transforms must hold one 4x4 per pair ({n}), got {len(init)}')
    clouds = [c for p in prs for c in p]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    parts = [np.concatenate(clouds), _model12(init)]
    if method == 'plane' and ref_normals is not None:
        if len(ref_normals) != n:
            raise ValueError(f'ref_normals must hold one array per pair ({n}), got {len(ref_normals)}')
        nrm = []
        for i, (s, r) in enumerate(prs):
            nr = _cloud64(ref_normals[i], f'ref_normals[{i}]')
            if nr.shape != r.shape:
                raise ValueError(f'ref_normals[{i}] must be {r.shape}, got {nr.shape}')
            nrm += [np.zeros_like(s), nr]
        parts.append(np.concatenate(nrm))
    dev = torch.device('cuda', torch.cuda.current_device())
    d_parts = upload(parts, dev)                                                                   # one upload
    pts, T0 = d_parts[0].view(-1, 3), d_parts[1].view(-1, 12)
    normals = None
    if method == 'plane':
        if ref_normals is not None:
            normals = d_parts[2].view(-1, 3)
        else:
            from .features import estimate_normals_batch
            normals = estimate_normals_batch(pts, off, None, 30, search='grid')[0]
    res = icp_batch(pts, off, [(2 * p, 2 * p + 1) for p in range(n)], T0, max_distance, method, normals, max_iters, relative_fitness,
                    relative_rmse, cell)
    keys = ('transform', 'fitness', 'inlier_rmse', 'iterations', 'status', 'trace', 'idx', 'd2')
    flat = torch.cat([res[k].reshape(-1).double() for k in keys]).cpu().numpy()                    # one download (int32 is exact in fp64)
    host, at = {}, 0
    for k in keys:
        host[k] = flat[at:at + res[k].numel()].reshape(tuple(res[k].shape))
        at += res[k].numel()
    oo, T = res['out_offsets'], _matrix44(host['transform'])
    out = []
    for p in range(n):
        idx = host['idx'][oo[p]:oo[p + 1]].astype(np.int64)
        src = np.flatnonzero(idx >= 0)
        evals = int(host['iterations'][p]) + 1
        out.append({'transformation': T[p], 'fitness': float(host['fitness'][p]), 'inlier_rmse': float(host['inlier_rmse'][p]),
                    'correspondence_set': np.stack([src, idx[src]], axis=1), 'iterations': int(host['iterations'][p]),
                    'status': int(host['status'][p]), 'trace': host['trace'][p][:evals].copy()})
    return out


def icp(src_points, ref_points, init=None, max_distance=0.05, method='point', ref_normals=None, max_iters=30, relative_fitness=1e-6,
        relative_rmse=1e-6, cell=None):
    """icp_pairs for one pair: -> the dict of that pair."""
    _need_device('icp')
    return icp_pairs([(src_points, ref_points)], None if init is None else [init], max_distance, method,
                     None if ref_normals is None else [ref_normals], max_iters, relative_fitness, relative_rmse, cell)[0]


def evaluate_registration_pairs(list_of_pairs, transforms, max_distance):
    """Open3D's evaluate_registration for many pairs: the geometric score of given transforms -- fitness, inlier_rmse and the
    correspondence set at max_distance, by a nearest-neighbour search of every moved source point in its reference cloud's grid.  It is
    icp_pairs with max_iters = 0: same dicts, the transformation returned as given."""
    _need_device('evaluate_registration_pairs')
    return icp_pairs(list_of_pairs, transforms, max_distance, max_iters=0)


# ---- feature-matching RANSAC scored geometrically (csrc/ransac_geo.hip) ---------------------------------------------------------------------
RANSAC_SCORES = ('correspondence', 'geometric')


def hypothesis_models_batch(corr, offsets, samples, hyp_offsets):
    """The three-point models of a packed hypothesis list as an output of their own (arguments as find_rigid_transform_batch takes them;
    sga_ransac_models).  -> dict of HIP tensors: models [sum H, 12] float64 (row-major R | t; NaN where invalid), valid [sum H] int32,
    resid2 [sum H] float64 -- the largest |R s + t - r|^2 of the three sampled rows in the grid search's arithmetic (no fma), +inf where
    invalid: what Open3D's distance checker compares with the threshold."""
    return _hypothesis_models(HypJobs(corr, offsets, samples, hyp_offsets))


def _hypothesis_models(J):
    """hypothesis_models_batch of a checked hypothesis list."""
    J.check_int32('hypothesis_models_batch', 12)
    cr, dev, n_jobs, total, total_h = J.corr, J.corr.device, J.n_jobs, J.total, J.total_h
    check_finite(cr, 'corr', 'coordinates')
    out = {'models': torch.full((total_h, 12), float('nan'), device=dev, dtype=torch.float64),
           'valid': torch.zeros((total_h,), device=dev, dtype=torch.int32),
           'resid2': torch.full((total_h,), float('inf'), device=dev, dtype=torch.float64)}
    if n_jobs == 0 or total_h == 0:
        return out
    d_off, d_hoff = upload([J.h_off, J.h_hoff], dev)                          # one small upload
    rc = _lib.lib().sga_ransac_models(_p(cr) if total else None, _p(d_off), n_jobs, total, _p(J.samples), _p(d_hoff), total_h, J.max_h,
                                      J.h_off.ctypes.data, J.h_hoff.ctypes.data, _p(out['models']), _p(out['valid']), _p(out['resid2']), _stream())
    _lib.check(rc, 'sga_ransac_models')
    return out


def score_transforms_batch(points, offsets, pairs, transforms, max_distance, live=None, cell=None, _checked=False):
    """Open3D's evaluate_registration for MANY transforms per cloud pair, without the per-query results (sga_score_transforms_grid): points
    [sum N, 3] float64 HIP tensor (clouds packed back to back), offsets [n_clouds + 1] host ints, pairs [n_jobs, 2] host ints (source cloud,
    reference cloud; any number of jobs may share both), transforms [n_jobs, 12] float64 HIP tensor (row-major R | t), live [n_jobs] int32
    HIP tensor or None (0: the job is skipped and scores 0).  The grid of every cloud is built once (cell: None = point_cloud.nn_grid_cell;
    a speed choice only).  -> (count [n_jobs] int32, sum_d2 [n_jobs] float64) HIP tensors: the number of moved source points with a
    reference point within max_distance (inf: no limit) and the sum of their squared distances to the nearest, in a fixed order -- the same
    bits in two calls, for a job alone or in a batch, and for every cell.  No synchronisation."""
    max_distance = float(max_distance)
    if not max_distance > 0.0:
        raise ValueError(f'max_distance must be > 0 (inf: no limit), got {max_distance}')
    pts = device_tensor(points, 'points', torch.float64)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f'points must be [N, 3], got {tuple(pts.shape)}')
    dev = pts.device
    off = prefix_offsets(offsets, 'offsets', int(pts.shape[0]))
    n_sets = len(off) - 1
    pr = pair_ids(pairs, n_sets, 'cloud')
    n = len(pr)
    T = device_tensor(transforms, 'transforms', torch.float64)
    if tuple(T.shape) != (n, 12):
        raise ValueError(f'transforms must be [{n}, 12] (row-major R | t per job), got {tuple(T.shape)}')
    lv = None
    if live is not None:
        lv = device_tensor(live, 'live', torch.int32)
        if tuple(lv.shape) != (n,):
            raise ValueError(f'live must be [{n}], got {tuple(lv.shape)}')
    if not _checked:                                                                       # ransac_geometric_batch has looked already
        check_finite(pts, 'points', 'coordinates')
    count = torch.zeros((n,), device=dev, dtype=torch.int32)
    sum_d2 = torch.zeros((n,), device=dev, dtype=torch.float64)
    if n == 0:
        return count, sum_d2
    max_q = int(np.diff(off)[pr[:, 0]].max())
    if -(-max_q // 1024) * n >= 2 ** 24:
        raise ValueError(f'score_transforms_batch: {n} jobs of up to {max_q} queries exceed the grid limit; split the job list')
    L = _lib.lib()
    C, G = _search_grid(pts, off, max_distance, cell)
    h_off, h_pr = off.astype(np.int32), pr.astype(np.int32)
    d_pr, = upload([h_pr], dev)
    ws_bytes = int(L.sga_score_transforms_workspace_bytes(n, max_q))
    ws = workspace(ws_bytes, dev)
    rc = L.sga_score_transforms_grid(_p(pts), _p(C.d_off), n_sets, int(pts.shape[0]), _p(d_pr), n, max_q, h_off.ctypes.data, h_pr.ctypes.data,
                                     *G.search_args(), _p(T), _p(lv) if lv is not None else None, max_distance * max_distance, _p(count),
                                     _p(sum_d2), _p(ws), ws_bytes, _stream())
    _lib.check(rc, 'sga_score_transforms_grid')
    return count, sum_d2


def ransac_geometric_batch(points, offsets, pairs, corr, corr_offsets, samples, hyp_offsets, distance_threshold, max_validation, cell=None):
    """Open3D's registration_ransac_based_on_feature_matching from given sample triples, for many cloud pairs at once and device-resident
    (no host synchronisation between the stages).  points / offsets / pairs: the clouds and one (source cloud, reference cloud) job per
    pair, as score_transforms_batch takes them; corr [sum n, 6] / corr_offsets / samples [sum H, 3] / hyp_offsets: job j's correspondences
    and sample triples, as find_rigid_transform_batch takes them (the caller has applied edge_length_filter).  Per job:
      1. the three-point model of every hypothesis (hypothesis_models_batch);
      2. Open3D's distance checker: valid and resid2 <= distance_threshold^2;
      3. the validated set: the first `max_validation` passing hypotheses in ascending index (Open3D's max_validation);
      4. every validated model scored on ALL source points against the reference cloud at distance_threshold (score_transforms_batch;
         the evaluation is sized by min(H_j, max_validation) slots per job, unused ones are not searched);
      5. selected: the largest count; among equal counts the smallest sum_d2; then the lowest index;
      6. the transform is that hypothesis' model, bit for bit -- no refit, as in Open3D (icp_pairs refines).
    -> dict of HIP tensors: transform [n_jobs, 4, 4] float64, fitness (count / source points), inlier_rmse (sqrt(sum_d2 / count), 0 without
    a pair) [n_jobs] float64, best_hyp (job-local), n_validated, status [n_jobs] int32 (1: no validated hypothesis or a best count below
    3 -- identity, fitness 0, rmse 0, best_hyp -1), hyp_count [sum H] int32 (-1 where the hypothesis was not validated), hyp_sum_d2 [sum H]
    float64 (+inf there), and models / valid / resid2 of step 1."""
    distance_threshold, max_validation = float(distance_threshold), int(max_validation)
    if not (np.isfinite(distance_threshold) and distance_threshold > 0):
        raise ValueError(f'distance_threshold must be finite and > 0, got {distance_threshold}')
    if max_validation < 1:
        raise ValueError(f'max_validation must be >= 1, got {max_validation}')
    pts = device_tensor(points, 'points', torch.float64)
    dev = pts.device
    check_finite(pts, 'points', 'coordinates')                                             # the only download, before the first stage
    HJ = HypJobs(corr, corr_offsets, samples, hyp_offsets)
    M = _hypothesis_models(HJ)
    hoff, H, n_jobs, total_h = HJ.hoff, HJ.sizes_h, HJ.n_jobs, HJ.total_h
    off = prefix_offsets(offsets, 'offsets', int(pts.shape[0]))
    pr = pair_ids(pairs)
    if len(pr) != n_jobs:
        raise ValueError(f'pairs names {len(pr)} jobs, hyp_offsets {n_jobs}')
    pair_ids(pr, len(off) - 1, 'cloud')
    K = np.minimum(H, max_validation)                                                      # evaluation slots per job: a host-side bound
    slot_off = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    S, k_max = int(slot_off[-1]), int(K.max()) if n_jobs else 0
    nq = np.diff(off)[pr[:, 0]].astype(np.float64) if n_jobs else np.zeros(0)
    eye = torch.eye(4, device=dev, dtype=torch.float64)
    out = {'transform': eye.repeat(n_jobs, 1, 1), 'fitness': torch.zeros((n_jobs,), device=dev, dtype=torch.float64),
           'inlier_rmse': torch.zeros((n_jobs,), device=dev, dtype=torch.float64),
           'best_hyp': torch.full((n_jobs,), -1, device=dev, dtype=torch.int32), 'n_validated': torch.zeros((n_jobs,), device=dev, dtype=torch.int32),
           'status': torch.ones((n_jobs,), device=dev, dtype=torch.int32),
           'hyp_count': torch.full((total_h,), -1, device=dev, dtype=torch.int32),
           'hyp_sum_d2': torch.full((total_h,), float('inf'), device=dev, dtype=torch.float64), **M}
    if S == 0:
        return out
    # host-known index arrays, one upload: the job and base of every hypothesis, the job of every slot, the slot of every (job, k)
    job_of_h = np.repeat(np.arange(n_jobs, dtype=np.int64), H)
    pad = slot_off[:-1, None] + np.arange(k_max, dtype=np.int64)[None, :]
    pad = np.where(np.arange(k_max)[None, :] < K[:, None], pad, S)                         # S: the dummy slot
    d_job, d_hbase, d_sbase, d_pad, d_nq, d_hoff = upload([job_of_h, hoff[:-1][job_of_h], slot_off[:-1][job_of_h], pad, nq, hoff[:-1].copy()], dev)
    d_pad = d_pad.view(n_jobs, k_max)
    # 2. + 3.: the distance checker, the rank of a passing hypothesis within its job, the first max_validation of them
    passing = (M['valid'] != 0) & (M['resid2'] <= distance_threshold * distance_threshold)
    incl = torch.cumsum(passing.to(torch.int64), 0)
    before = torch.cat([incl.new_zeros(1), incl])[d_hbase]                                 # passing hypotheses before the job's first
    rank = incl - passing.to(torch.int64) - before
    validated = passing & (rank < max_validation)
    slot = torch.where(validated, d_sbase + rank, torch.full_like(rank, S))                # a validated hypothesis' slot, else the dummy
    hyp_of_slot = torch.zeros((S + 1,), device=dev, dtype=torch.int64).scatter_(0, slot, torch.arange(total_h, device=dev, dtype=torch.int64))
    live = torch.zeros((S + 1,), device=dev, dtype=torch.int32).scatter_(0, slot, torch.ones((total_h,), device=dev, dtype=torch.int32))
    live[S] = 0
    hyp_of_slot, live = hyp_of_slot[:S], live[:S].contiguous()
    # 4.: one job per slot
    count, sum_d2 = score_transforms_batch(pts, off, np.repeat(pr, K, axis=0), M['models'][hyp_of_slot].contiguous(), distance_threshold, live, cell,
                                           _checked=True)
    cnt_x = torch.cat([torch.where(live != 0, count, torch.full_like(count, -1)), count.new_full((1,), -1)])
    sd2_x = torch.cat([torch.where(live != 0, sum_d2, torch.full_like(sum_d2, float('inf'))), sum_d2.new_full((1,), float('inf'))])
    out['hyp_count'], out['hyp_sum_d2'] = cnt_x[slot], sd2_x[slot]
    # 5.: lexicographic over the job's slots, which are in ascending hypothesis index
    c_pad, s_pad = cnt_x[d_pad], sd2_x[d_pad]
    c_best = c_pad.max(dim=1).values
    cand = c_pad == c_best[:, None]
    s_best = torch.where(cand, s_pad, torch.full_like(s_pad, float('inf'))).min(dim=1).values
    cand &= s_pad == s_best[:, None]
    k_best = torch.where(cand, torch.arange(k_max, device=dev)[None, :], k_max).min(dim=1).values
    found = c_best >= 3
    best_slot = d_pad.gather(1, k_best.clamp(max=k_max - 1)[:, None]).reshape(-1).clamp(max=S - 1)
    best_glob = hyp_of_slot[best_slot]
    # 6.
    m = M['models'][best_glob]
    T = eye.repeat(n_jobs, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = m[:, :9].reshape(-1, 3, 3), m[:, 9:]
    cf = c_best.to(torch.float64)
    out['transform'] = torch.where(found[:, None, None], T, eye)
    out['fitness'] = torch.where(found & (d_nq > 0), cf / d_nq.clamp(min=1.0), torch.zeros_like(cf))
    out['inlier_rmse'] = torch.where(found, torch.sqrt(s_best / cf.clamp(min=1.0)), torch.zeros_like(cf))
    out['best_hyp'] = torch.where(found, best_glob - d_hoff, torch.full_like(best_glob, -1)).to(torch.int32)
    out['n_validated'] = (c_pad >= 0).sum(dim=1).to(torch.int32)
    out['status'] = torch.where(found, 0, 1).to(torch.int32)
    return out
