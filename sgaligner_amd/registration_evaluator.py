"""Registration of a scan pair from the aligner's node matches (src/engine/registration_evaluator.py:47-56, 129-208), the estimator on the
GPU (csrc/ransac.hip through utils/registration.py).

For every matched node pair the two objects' points go to an external point matcher; the point correspondences it returns are cut to the
best-scored share, pooled over all nodes and handed to RANSAC; the transform is scored with the metrics of utils/registration.py.  The point
matcher (GeoTransformer in the reference) is not part of this package: it is injected as a callable

    point_matcher(src_pts [n, 3], ref_pts [m, 3], gt_transform [4, 4]) -> None, or
        {'src_corr_points': [k, 3], 'ref_corr_points': [k, 3], 'corr_scores': [k]}

`run_aligner_registration_batch` runs the matcher for every pair first and then solves all pairs in one launch set -- what a loop over the
subscan pairs of a scan wants."""
from __future__ import annotations

import numpy as np

from .utils import registration


class RegistrationEvaluator:
    RESULT_KEYS = ('CD', 'IR', 'RRE', 'RTE', 'recall', 'FMR')

    def __init__(self, point_matcher, num_p2p_corrs=20000, ransac_threshold=0.03, ransac_iters=5000, inlier_ratio_thresh=0.05,
                 rmse_thresh=0.2, min_object_points=50, seed=0):
        if not callable(point_matcher):
            raise TypeError('point_matcher must be callable: (src_pts, ref_pts, gt_transform) -> dict or None')
        self.point_matcher = point_matcher
        self.num_p2p_corrs = int(num_p2p_corrs)
        self.ransac_threshold = float(ransac_threshold)
        self.ransac_iters = int(ransac_iters)
        self.inlier_ratio_thresh = inlier_ratio_thresh
        self.rmse_thresh = rmse_thresh
        self.min_object_points = int(min_object_points)
        self.seed = int(seed)

    def evaluate_registration(self, src_points, ref_points, raw_points, est_transform, gt_transform, src_corr_points, ref_corr_points,
                              gt_src_corr_points, gt_ref_corr_points):
        """-> (chamfer distance, inlier ratio under the TRUE transform, RRE, RTE, accepted, feature-matching recall)."""
        chamfer = registration.compute_modified_chamfer_distance(src_points, ref_points, raw_points, est_transform, gt_transform)
        inlier_ratio = registration.compute_inlier_ratio(ref_corr_points, src_corr_points, gt_transform)
        rre, rte = registration.compute_registration_error(gt_transform, est_transform)
        rmse = registration.compute_registration_rmse(gt_ref_corr_points, gt_src_corr_points, est_transform)
        return chamfer, inlier_ratio, rre, rte, float(rmse < self.rmse_thresh), float(inlier_ratio >= self.inlier_ratio_thresh)

    def collect_correspondences(self, reg_data_dict):
        """The [n, 6] array RANSAC sees (source xyz | reference xyz), or None when no node pair yields any: per node pair the points whose
        objectId matches, pairs with a too small object skipped, the matcher's output cut to its num_p2p_corrs // len(node_corrs)
        best-scored rows."""
        node_corrs = reg_data_dict['node_corrs']
        src_points, ref_points = reg_data_dict['src_points'], reg_data_dict['ref_points']
        src_ids, ref_ids = reg_data_dict['src_plydata']['objectId'], reg_data_dict['ref_plydata']['objectId']
        gt_transform = reg_data_dict['gt_transform']
        src_rows, ref_rows = [], []
        for src_id, ref_id in node_corrs:
            obj_src, obj_ref = src_points[src_ids == src_id], ref_points[ref_ids == ref_id]
            if min(obj_src.shape[0], obj_ref.shape[0]) < self.min_object_points:
                continue
            matched = self.point_matcher(obj_src, obj_ref, gt_transform)
            if matched is None:
                continue
            src_c, ref_c, scores = (np.asarray(matched[k]) for k in ('src_corr_points', 'ref_corr_points', 'corr_scores'))
            budget = self.num_p2p_corrs // len(node_corrs)
            if scores.shape[0] > budget:
                keep = np.argsort(-scores)[:budget]
                src_c, ref_c = src_c[keep], ref_c[keep]
            src_rows.append(src_c)
            ref_rows.append(ref_c)
        if not src_rows:
            return None
        return np.concatenate([np.concatenate(src_rows), np.concatenate(ref_rows)], axis=1)

    def _finish(self, reg_data_dict, corr, est_transform, evaluate_registration):
        if est_transform is None:
            return None
        if not evaluate_registration:
            return est_transform
        values = self.evaluate_registration(reg_data_dict['src_points'], reg_data_dict['ref_points'], reg_data_dict.get('raw_points'),
                                            est_transform, reg_data_dict['gt_transform'], corr[:, :3], corr[:, 3:],
                                            reg_data_dict.get('gt_src_corr_points'), reg_data_dict.get('gt_ref_corr_points'))
        return dict(zip(self.RESULT_KEYS, values))

    def _solve(self, corrs):
        return registration.find_rigid_transform_pairs(corrs, threshold=self.ransac_threshold, iters=self.ransac_iters, seed=self.seed)

    def run_aligner_registration(self, reg_data_dict, evaluate_registration=True):
        """One scan pair -> None (no correspondences or no model), the 4x4 transform (evaluate_registration=False), or the dict of
        CD / IR / RRE / RTE / recall / FMR."""
        corr = self.collect_correspondences(reg_data_dict)
        if corr is None:
            return None
        (est_transform, _), = self._solve([corr])
        return self._finish(reg_data_dict, corr, est_transform, evaluate_registration)

    def run_aligner_registration_batch(self, list_of_reg_data_dicts, evaluate_registration=True):
        """[run_aligner_registration(d) for d in the list], the matcher run for every pair first and all pairs solved in one call."""
        corrs = [self.collect_correspondences(d) for d in list_of_reg_data_dicts]
        live = [i for i, c in enumerate(corrs) if c is not None]
        solved = dict(zip(live, self._solve([corrs[i] for i in live]))) if live else {}
        return [None if i not in solved else self._finish(d, corrs[i], solved[i][0], evaluate_registration)
                for i, d in enumerate(list_of_reg_data_dicts)]
