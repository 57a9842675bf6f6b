"""Registration of a scan pair from the aligner's node matches (src/engine/registration_evaluator.py:47-56, 129-208), the estimator on the
GPU (csrc/ransac.hip through utils/registration.py).

For every matched node pair the two objects' points go to an external point matcher; the point correspondences it returns are cut to the
best-scored share, pooled over all nodes and handed to RANSAC; the transform is scored with the metrics of utils/registration.py.  The point
matcher (GeoTransformer in the reference) is not part of this package: it is injected as a callable

    point_matcher(src_pts [n, 3], ref_pts [m, 3], gt_transform [4, 4]) -> None, or
        {'src_corr_points': [k, 3], 'ref_corr_points': [k, 3], 'corr_scores': [k]}

`run_aligner_registration_batch` runs the matcher for every pair first and then solves all pairs in one launch set -- what a loop over the
subscan pairs of a scan wants.

`FeatureMatcher` is a point matcher that ships with the package: nearest neighbours in the space of an injected per-point descriptor
(`descriptor(points [n, 3]) -> [n, C]`: `utils.features.FPFHDescriptor`, which ships with the package and computes FPFH on the device
(csrc/fpfh.hip), a learned backbone, ...), searched on the device (csrc/featnn.hip through utils/registration.match_features_pairs).  A
descriptor that has `many(list of clouds)` is asked for all clouds of a call at once.  Besides the call above it has `match_many`, which matches
a list of pairs in one launch set; `collect_correspondences` uses it when the matcher has it, and `run_normal_registration` /
`run_registration` (src/engine/registration_evaluator.py:92-127, 211-220), which match the two whole clouds, need it."""
from __future__ import annotations

import numpy as np

from .utils import registration


class FeatureMatcher:
    """point_matcher by nearest neighbours in descriptor space.  descriptor(points [n, 3] numpy) -> [n, C] array, one row per point.
    mutual=True keeps the mutual nearest neighbours only.  corr_scores = exp(-d2), d2 the squared descriptor distance: monotone in the
    distance and in (0, 1]; the evaluator only uses the order of the scores and their mean."""

    def __init__(self, descriptor, mutual=True):
        if not callable(descriptor):
            raise TypeError('descriptor must be callable: points [n, 3] -> features [n, C]')
        self.descriptor = descriptor
        self.mutual = bool(mutual)

    def match_many(self, list_of_pairs):
        """[(src_pts, ref_pts), ...] -> [None or {'src_corr_points', 'ref_corr_points', 'corr_scores'}, ...]: every pair matched in one
        launch set, one download."""
        pairs = [(np.asarray(s), np.asarray(r)) for s, r in list_of_pairs]
        if not pairs:
            return []
        if hasattr(self.descriptor, 'many'):                                        # all 2 * len(pairs) clouds in one launch set
            flat = [np.ascontiguousarray(f, dtype=np.float32) for f in self.descriptor.many([p for pair in pairs for p in pair])]
            feats = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(pairs))]
        else:
            feats = [tuple(np.ascontiguousarray(self.descriptor(p), dtype=np.float32) for p in pair) for pair in pairs]
        for (s, r), (fs, fr) in zip(pairs, feats):
            if fs.ndim != 2 or fr.ndim != 2 or len(fs) != len(s) or len(fr) != len(r):
                raise ValueError(f'descriptor must return one feature row per point: {fs.shape} for {s.shape}, {fr.shape} for {r.shape}')
        out = []
        for (s, r), (cij, d2) in zip(pairs, registration.match_features_pairs(feats, mutual=self.mutual)):
            cij, d2 = cij.cpu().numpy(), d2.cpu().numpy()
            out.append(None if len(cij) == 0 else {'src_corr_points': s[cij[:, 0]], 'ref_corr_points': r[cij[:, 1]], 'corr_scores': np.exp(-d2)})
        return out

    def __call__(self, src_pts, ref_pts, gt_transform=None):
        return self.match_many([(src_pts, ref_pts)])[0]


class RegistrationEvaluator:
    NORMAL_MAX_POINTS = 10000          # perform_registration's npoint: larger clouds are subsampled before they are matched
    RESULT_KEYS = ('CD', 'IR', 'RRE', 'RTE', 'recall', 'FMR')

    def __init__(self, point_matcher, num_p2p_corrs=20000, ransac_threshold=0.03, ransac_iters=5000, inlier_ratio_thresh=0.05,
                 rmse_thresh=0.2, min_object_points=50, seed=0, voxel_size=None, refine=None, refine_distance=None):
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
        # voxel_size: clouds are down-sampled by voxels of this edge on the device (utils/voxel.py) before they are matched -- the two
        # whole clouds of run_normal_registration instead of the random draw of 10 000 rows, every eligible object cloud of
        # collect_correspondences in one call.  None: no voxel step anywhere.
        self.voxel_size = None if voxel_size is None else float(voxel_size)
        if self.voxel_size is not None and not (self.voxel_size > 0.0 and np.isfinite(self.voxel_size)):
            raise ValueError(f'voxel_size must be > 0 and finite, or None (got {voxel_size})')
        # refine: ICP ('point' or 'plane', utils.registration.icp_pairs) on the RANSAC transform -- in run_normal_registration on the
        # clouds the matcher saw, in run_aligner_registration[_batch] on the whole src_points / ref_points down-sampled by the same rule
        # (voxels, or the draw of 10 000 rows).  refine_distance: ICP's maximal correspondence distance; None: ransac_threshold, the
        # evaluator's own "this close counts as matched".  None: no refinement, every result as without the argument.
        if refine not in (None, 'point', 'plane'):
            raise ValueError(f"refine must be None, 'point' or 'plane' (got {refine!r})")
        self.refine = refine
        self.refine_distance = self.ransac_threshold if refine_distance is None else float(refine_distance)
        if not self.refine_distance > 0.0:
            raise ValueError(f'refine_distance must be > 0 (got {refine_distance})')

    def _refine_clouds(self, list_of_clouds):
        """The clouds ICP refines on: down-sampled by the rule run_normal_registration applies before matching."""
        if self.voxel_size is not None:
            from .utils.voxel import voxel_downsample_many
            return voxel_downsample_many(list_of_clouds, self.voxel_size)
        out = []
        for k in range(0, len(list_of_clouds), 2):                                   # per pair: the generator starts afresh, as there
            rng = np.random.default_rng(self.seed)
            out += [self._subsample(c, rng) for c in list_of_clouds[k:k + 2]]
        return out

    def _refine(self, pairs, transforms):
        """[(src, ref), ...] and their RANSAC transforms -> the ICP-refined transforms, all pairs in ONE icp_pairs call.  A pair whose ICP
        stops early (too few correspondences, an unsolvable update) keeps the last transform it reached."""
        res = registration.icp_pairs(pairs, transforms, self.refine_distance, method=self.refine)
        return [r['transformation'] for r in res]

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
        src_rows, ref_rows, eligible = [], [], []
        for src_id, ref_id in node_corrs:
            obj_src, obj_ref = src_points[src_ids == src_id], ref_points[ref_ids == ref_id]
            if min(obj_src.shape[0], obj_ref.shape[0]) < self.min_object_points:
                continue
            eligible.append((obj_src, obj_ref))
        if self.voxel_size is not None and eligible:                                 # min_object_points was tested on the raw counts
            from .utils.voxel import voxel_downsample_many
            flat = voxel_downsample_many([c for pair in eligible for c in pair], self.voxel_size)
            eligible = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(eligible))]
        if hasattr(self.point_matcher, 'match_many'):
            results = self.point_matcher.match_many(eligible)                       # all node pairs of the call in one launch set
        else:
            results = (self.point_matcher(obj_src, obj_ref, gt_transform) for obj_src, obj_ref in eligible)
        for matched in results:
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

    def _subsample(self, points, rng):
        points = np.asarray(points)
        if points.shape[0] <= self.NORMAL_MAX_POINTS:
            return points
        return points[rng.choice(points.shape[0], self.NORMAL_MAX_POINTS, replace=False)]

    def run_normal_registration(self, reg_data_dict, evaluate_registration=True):
        """src/engine/registration_evaluator.py:92-127: registration of the two WHOLE clouds, without the aligner's node matches.  Each
        cloud is subsampled to 10 000 rows when larger (numpy.random.default_rng(self.seed)) -- or, with voxel_size, down-sampled by voxels
        instead --, the matcher's match_many matches them, and
        the transform is estimated by RANSAC on those correspondences with the evaluator's threshold and iteration count.  (The reference
        takes GeoTransformer's own estimate, output_dict['estimated_transform'], at this point; a matcher here yields correspondences
        only.)  -> None (no correspondences or no model), (transform, mean correspondence score) with evaluate_registration=False, or the
        dict of CD / IR / RRE / RTE / recall / FMR."""
        if not hasattr(self.point_matcher, 'match_many'):
            raise TypeError('run_normal_registration matches whole clouds: the point matcher needs match_many (FeatureMatcher has it)')
        if self.voxel_size is not None:
            from .utils.voxel import voxel_downsample_many
            src, ref = voxel_downsample_many([reg_data_dict['src_points'], reg_data_dict['ref_points']], self.voxel_size)
        else:
            rng = np.random.default_rng(self.seed)
            src, ref = self._subsample(reg_data_dict['src_points'], rng), self._subsample(reg_data_dict['ref_points'], rng)
        matched, = self.point_matcher.match_many([(src, ref)])
        if matched is None:
            return None
        corr = np.concatenate([np.asarray(matched['src_corr_points']), np.asarray(matched['ref_corr_points'])], axis=1)
        (est_transform, _), = self._solve([corr])
        if est_transform is None:
            return None
        if self.refine is not None:
            est_transform, = self._refine([(src, ref)], [est_transform])
        if not evaluate_registration:
            return est_transform, np.mean(matched['corr_scores'])
        return self._finish(reg_data_dict, corr, est_transform, True)

    def run_registration(self, reg_data_dict):
        """src/engine/registration_evaluator.py:211-220 -> (normal result dict, aligner result dict), (None, None) when the normal
        registration yields nothing."""
        normal = self.run_normal_registration(reg_data_dict)
        if normal is None:
            return None, None
        return normal, self.run_aligner_registration(reg_data_dict)

    def run_aligner_registration(self, reg_data_dict, evaluate_registration=True):
        """One scan pair -> None (no correspondences or no model), the 4x4 transform (evaluate_registration=False), or the dict of
        CD / IR / RRE / RTE / recall / FMR."""
        corr = self.collect_correspondences(reg_data_dict)
        if corr is None:
            return None
        (est_transform, _), = self._solve([corr])
        if self.refine is not None and est_transform is not None:
            src, ref = self._refine_clouds([reg_data_dict['src_points'], reg_data_dict['ref_points']])
            est_transform, = self._refine([(src, ref)], [est_transform])
        return self._finish(reg_data_dict, corr, est_transform, evaluate_registration)

    def run_aligner_registration_batch(self, list_of_reg_data_dicts, evaluate_registration=True):
        """[run_aligner_registration(d) for d in the list], the matcher run for every pair first and all pairs solved in one call."""
        corrs = [self.collect_correspondences(d) for d in list_of_reg_data_dicts]
        live = [i for i, c in enumerate(corrs) if c is not None]
        solved = dict(zip(live, self._solve([corrs[i] for i in live]))) if live else {}
        found = [i for i in live if solved[i][0] is not None]
        if self.refine is not None and found:                                        # every solved pair in one icp_pairs call
            flat = self._refine_clouds([list_of_reg_data_dicts[i][k] for i in found for k in ('src_points', 'ref_points')])
            refined = self._refine([(flat[2 * j], flat[2 * j + 1]) for j in range(len(found))], [solved[i][0] for i in found])
            for i, T in zip(found, refined):
                solved[i] = (T, solved[i][1])
        return [None if i not in solved else self._finish(d, corrs[i], solved[i][0], evaluate_registration)
                for i, d in enumerate(list_of_reg_data_dicts)]
