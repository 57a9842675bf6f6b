"""Drop-in for the reference's `utils.alignment` (utils/alignment.py) + the FPS step of `utils.point_cloud`.
With `<root>/sgaligner_amd` on sys.path this package is found as top-level `utils`; only `utils.alignment` is taken
over then -- every other `utils.*` module (torch_util, common, scan3r, the full point_cloud ...) keeps resolving to
the reference tree further down sys.path (see sgaligner_amd/_dropin.py).

`sgaligner_amd.utils.point_cloud` also carries the exact nearest-neighbour helpers (get_nearest_neighbor, compute_pcl_overlap[_pairs],
apply_transform) and `sgaligner_amd.utils.registration` the chamfer / mosaicking / registration metrics built on them (csrc/nnsearch.hip)
and the estimator those metrics judge: batched RANSAC rigid registration from point correspondences (csrc/ransac.hip) as
find_rigid_transform[_pairs / _batch], draw_samples, score_hypotheses_batch and registration_with_ransac_from_correspondences, and the
registration from per-point descriptors (csrc/featnn.hip): feature_nn_batch, match_features_pairs, edge_length_filter and
registration_with_ransac_from_feats[_pairs].
Neither is aliased: callers import them from `sgaligner_amd.utils...` explicitly."""
if __name__ == 'utils':
    import os as _os
    import sys as _sys
    _root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
    if _root not in _sys.path:
        _sys.path.append(_root)
    from sgaligner_amd._dropin import alias as _alias
    _alias('utils', ['alignment'], ours_first=False)
