"""Registration and mosaicking metrics with the reference's signatures (utils/registration.py), the nearest-neighbour searches on the
GPU (csrc/nnsearch.hip through utils/point_cloud.py).  The searches return exact fp64 distances -- bit-identical to the KD-tree's -- and
every mean is taken by numpy on the host from those arrays, so the figures equal the reference's bit for bit.  Nothing here falls back
to a host search: without a HIP device the functions that need one raise."""
from __future__ import annotations

import numpy as np

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
