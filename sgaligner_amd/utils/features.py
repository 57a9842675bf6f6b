"""Per-point descriptors on the GPU (csrc/fpfh.hip): exact neighbour lists, normals, the SPFH census and FPFH -- the descriptor side of
the reference's utils/open3d.py (estimate_normals :61-66, the FPFH features of :78-86 that :137-170 matches).  The chain

    points -> neighbour_lists -> estimate_normals_batch -> spfh_counts -> fpfh_from_counts -> registration.feature_nn_batch -> RANSAC

runs on the device from end to end, batched over clouds packed back to back (packed.py).  `fpfh_batch` is the chain in one call,
`FPFHDescriptor` the callable `registration_evaluator.FeatureMatcher` wants, `estimate_normals` the single-cloud counterpart of
utils/open3d.py:61-66.

Open3D is not a dependency of this package and equality with its output is not tested anywhere: the contract written in
include/sgaligner_hip.h is the definition, and tests/fpfh_ref.py restates it in numpy.  Nothing here falls back to the host: without a
HIP device the functions raise."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import PackedLayout, check_dtype, device_tensor, upload
from .point_cloud import _cloud64, _need_device

MAX_NN = 128          # longest neighbour list of csrc/fpfh.hip
BINS = 33             # 3 groups of 11
LD = 36               # row width of the fp32 descriptors: 33 padded to a multiple of 4, what sga_featnn_search reads


class _Clouds(PackedLayout):
    """Offsets of one call's clouds, checked once (pt_off, h_pt, n_scans = the clouds, total_points) with their device copy d_off: one small
    upload.  With `points` it also holds pts [total, 3] float64 on the device; fpfh_from_counts has none and names total and device itself."""

    def __init__(self, points, offsets, total=None, device=None):
        self.pts = None if points is None else device_tensor(points, 'points', torch.float64)
        if self.pts is not None:
            if self.pts.dim() != 2 or self.pts.shape[1] != 3:
                raise ValueError(f'points must be [N, 3], got {tuple(self.pts.shape)}')
            total, device = self.pts.shape[0], self.pts.device
        super().__init__(offsets, total, 'offsets')
        self.dev, (self.d_off,) = device, upload([self.h_pt], device)

    def args(self):
        return _p(self.d_off), self.n_scans, self.total_points, self.h_pt.ctypes.data


def _clouds(points, offsets):
    return points if isinstance(points, _Clouds) else _Clouds(points, offsets)


def _check_max_nn(max_nn) -> int:
    max_nn = int(max_nn)
    if not 1 <= max_nn <= MAX_NN:
        raise ValueError(f'max_nn must be in [1, {MAX_NN}], got {max_nn}')
    return max_nn


class NeighbourLists(tuple):
    """The (count, idx, d2) triple of neighbour_lists; it remembers the offsets of the clouds it was built for (idx is cloud-local)."""
    offsets = None


def _list_dtypes(lists):
    """Every dtype of the triple, before any device check: a wrong dtype can be told apart on a machine without a device."""
    if not isinstance(lists, (tuple, list)) or len(lists) != 3:
        raise ValueError('lists must be the (count, idx, d2) triple of neighbour_lists')
    for t, name, dt in zip(lists, ('lists.count', 'lists.idx', 'lists.d2'), (torch.int32, torch.int32, torch.float64)):
        check_dtype(t, name, dt)


def _lists(lists, total, dev):
    """(count [total] int32, idx [total, max_nn] int32, d2 [total, max_nn] float64) device tensors -> the same, checked, plus max_nn."""
    _list_dtypes(lists)
    count, idx, d2 = (device_tensor(t, name, dt) for t, name, dt in
                      zip(lists, ('lists.count', 'lists.idx', 'lists.d2'), (torch.int32, torch.int32, torch.float64)))
    if count.shape != (total,) or idx.dim() != 2 or idx.shape[0] != total or d2.shape != idx.shape:
        raise ValueError(f'lists of {total} points: got count {tuple(count.shape)}, idx {tuple(idx.shape)}, d2 {tuple(d2.shape)}')
    return count, idx, d2, _check_max_nn(idx.shape[1])


SEARCHES = ('brute', 'grid')


def _check_search(search) -> str:
    if search not in SEARCHES:
        raise ValueError(f'search must be one of {SEARCHES}, got {search!r}')
    return search


def neighbour_lists(points, offsets, radius=None, max_nn=30, search='brute', cell=None):
    """points [sum N, 3] float64 HIP tensor (clouds packed back to back), offsets [n_clouds + 1] host ints.  For every point the first
    `max_nn` of the points of ITS cloud within `radius` (None: no radius, pure k-NN), sorted ascending by (squared distance, index); the
    point itself is entry 0 unless a duplicate with a lower index precedes it.  -> (count [total] int32, idx [total, max_nn] int32
    cloud-local, -1 past count, d2 [total, max_nn] float64, +inf past count), HIP tensors.  Exact (brute force): d2 = (dx*dx + dy*dy) +
    dz*dz with every operation rounded on its own, the arithmetic of nearest_neighbor_batch; a NaN distance never enters a list.
    search='grid' looks only at the cells around each point (csrc/voxel.hip through utils/voxel.py) and gives the SAME lists, bit for
    bit, whatever `cell` is: the cell edge, one for all clouds or one per cloud; None: voxel.default_cell (the radius where one is
    given, else a per-cloud edge from the bounding box, the point count and max_nn: half a list per cell of a surface).  It is the route for clouds far above 20 000 points."""
    C = _clouds(points, offsets)
    max_nn = _check_max_nn(max_nn)
    _check_search(search)
    r2 = float('inf') if radius is None else float(radius) * float(radius)
    if not r2 >= 0.0:
        raise ValueError(f'radius must be >= 0 or None, got {radius}')
    if search == 'grid':
        from . import voxel
        out = NeighbourLists(voxel.grid_lists(C, None, r2, max_nn, cell, radius))
        out.offsets = C.pt_off
        return out
    count = torch.empty((C.total_points,), device=C.dev, dtype=torch.int32)
    idx = torch.empty((C.total_points, max_nn), device=C.dev, dtype=torch.int32)
    d2 = torch.empty((C.total_points, max_nn), device=C.dev, dtype=torch.float64)
    if C.total_points:
        rc = _lib.lib().sga_knn_lists(_p(C.pts), *C.args(), r2, max_nn, _p(count), _p(idx), _p(d2), _stream())
        _lib.check(rc, 'sga_knn_lists')
    out = NeighbourLists((count, idx, d2))
    out.offsets = C.pt_off
    return out


def estimate_normals_batch(points, offsets, radius=None, max_nn=30, viewpoints=None, lists=None, search='brute', cell=None):
    """Normals of every point from its neighbour list (`lists`, or neighbour_lists(points, offsets, radius, max_nn)): the unit eigenvector
    of the smallest eigenvalue of the neighbours' covariance.  viewpoints [n_clouds, 3] (HIP float64 tensor or host array): the normal is
    turned towards its cloud's viewpoint; None: turned so that its component of largest magnitude is positive.  A point with fewer than 3
    neighbours gets (0, 0, 1) and status 1.  search / cell: how neighbour_lists builds the lists when none are given.
    -> (normals [total, 3] float64, status [total] int32), HIP tensors."""
    check_dtype(points, 'points', torch.float64)
    if lists is not None:
        _list_dtypes(lists)
    C = _clouds(points, offsets)
    if lists is None:
        lists = neighbour_lists(C, None, radius, max_nn, search, cell)
    count, idx, _, width = _lists(lists, C.total_points, C.dev)
    vp = None
    if viewpoints is not None:
        if isinstance(viewpoints, torch.Tensor):
            vp = device_tensor(viewpoints, 'viewpoints', torch.float64)
        else:
            vp = torch.from_numpy(np.ascontiguousarray(viewpoints, dtype=np.float64)).to(C.dev)
        if tuple(vp.shape) != (C.n_scans, 3):
            raise ValueError(f'viewpoints must be [{C.n_scans}, 3], got {tuple(vp.shape)}')
    normals = torch.empty((C.total_points, 3), device=C.dev, dtype=torch.float64)
    status = torch.empty((C.total_points,), device=C.dev, dtype=torch.int32)
    if C.total_points:
        rc = _lib.lib().sga_normals(_p(C.pts), *C.args(), _p(count), _p(idx), width, _p(vp) if vp is not None and vp.numel() else None,
                                    _p(normals), _p(status), _stream())
        _lib.check(rc, 'sga_normals')
    return normals, status


def spfh_counts(points, normals, offsets, lists):
    """The SPFH census: counts [total, 33] int32 HIP tensor, per point three histograms of 11 bins over its list entries 1 .. m-1 (the pair
    features of the point and each neighbour, from `normals` [total, 3] float64); each group sums to m - 1."""
    check_dtype(points, 'points', torch.float64)
    check_dtype(normals, 'normals', torch.float64)
    _list_dtypes(lists)
    C = _clouds(points, offsets)
    nr = device_tensor(normals, 'normals', torch.float64)
    if tuple(nr.shape) != (C.total_points, 3):
        raise ValueError(f'normals must be [{C.total_points}, 3], got {tuple(nr.shape)}')
    count, idx, d2, width = _lists(lists, C.total_points, C.dev)
    counts = torch.empty((C.total_points, BINS), device=C.dev, dtype=torch.int32)
    if C.total_points:
        rc = _lib.lib().sga_spfh_counts(_p(C.pts), _p(nr), *C.args(), _p(count), _p(idx), _p(d2), width, _p(counts), _stream())
        _lib.check(rc, 'sga_spfh_counts')
    return counts


def fpfh_from_counts(counts, lists, want_f64=False, offsets=None):
    """FPFH from the census: every point's SPFH (its counts scaled to 100) plus the SPFHs of its neighbours weighted by 1 / squared
    distance, each bin group scaled to 100.  counts [total, 33] int32 and `lists` are HIP tensors; offsets [n_clouds + 1] host ints (None:
    the offsets `lists` was built with, one cloud for a plain tuple).  -> [total, 36] float32 HIP tensor (columns 33-35 zero: the width sga_featnn_search reads), or with want_f64 the pair
    (that, [total, 33] float64).  The float32 values are the rounded float64 values."""
    check_dtype(counts, 'counts', torch.int32)
    _list_dtypes(lists)
    cn = device_tensor(counts, 'counts', torch.int32)
    if cn.dim() != 2 or cn.shape[1] != BINS:
        raise ValueError(f'counts must be [N, {BINS}], got {tuple(cn.shape)}')
    total, dev = int(cn.shape[0]), cn.device
    count, idx, d2, width = _lists(lists, total, dev)
    if offsets is None:
        offsets = getattr(lists, 'offsets', None)
    C = _Clouds(None, [0, total] if offsets is None else offsets, total, dev)
    out32 = torch.empty((total, LD), device=dev, dtype=torch.float32)
    out64 = torch.empty((total, BINS), device=dev, dtype=torch.float64) if want_f64 else None
    if total:
        rc = _lib.lib().sga_fpfh(_p(cn), *C.args(), _p(count), _p(idx), _p(d2), width, _p(out64) if want_f64 else None, _p(out32), LD, _stream())
        _lib.check(rc, 'sga_fpfh')
    return (out32, out64) if want_f64 else out32


def fpfh_batch(points, offsets, normals=None, radius_normal=None, max_nn_normal=30, radius_feature=None, max_nn_feature=100, viewpoints=None,
               search='brute', cell=None):
    """The whole chain for clouds packed back to back: points [sum N, 3] float64 HIP tensor, offsets [n_clouds + 1] host ints.  Normals
    (when none are given) from lists of (radius_normal, max_nn_normal), oriented by `viewpoints`; features from lists of (radius_feature,
    max_nn_feature).  search / cell: the route of both neighbour_lists calls; the result does not depend on them.
    -> [total, 36] float32 HIP tensor, bitwise what the four stages give when called one by one."""
    check_dtype(points, 'points', torch.float64)
    if normals is not None:
        check_dtype(normals, 'normals', torch.float64)
    C = _clouds(points, offsets)
    if normals is None:
        normals, _ = estimate_normals_batch(C, None, radius_normal, max_nn_normal, viewpoints, search=search, cell=cell)
    lists = neighbour_lists(C, None, radius_feature, max_nn_feature, search, cell)
    return fpfh_from_counts(spfh_counts(C, normals, None, lists), lists, offsets=C.pt_off)


def estimate_normals(points, radius=None, max_nn=30, viewpoint=None, search='brute', cell=None):
    """utils/open3d.py:61-66 for one cloud: points [n, 3] numpy -> normals [n, 3] float64 numpy.  The defaults are the reference's
    (pcd.estimate_normals(): the 30 nearest neighbours, no radius)."""
    _need_device('estimate_normals')
    p = _cloud64(points, 'points')
    if len(p) == 0:
        return np.zeros((0, 3))
    vp = None if viewpoint is None else np.asarray(viewpoint, dtype=np.float64).reshape(1, 3)
    normals, _ = estimate_normals_batch(torch.from_numpy(p).cuda(), [0, len(p)], radius, max_nn, vp, search=search, cell=cell)
    return normals.cpu().numpy()


class FPFHDescriptor:
    """descriptor(points [n, 3]) -> [n, 33] float32 numpy, the callable FeatureMatcher wants.  Normals from (radius_normal,
    max_nn_normal), oriented towards `viewpoint` (one fixed point for every cloud -- the evaluator's two clouds share one frame -- or
    None), features from (radius_feature, max_nn_feature).  `many` computes a list of clouds in one launch set and one download.
    search / cell: the route of the neighbour lists ('grid' for large clouds); the descriptors do not depend on them."""

    def __init__(self, radius_normal=None, max_nn_normal=30, radius_feature=None, max_nn_feature=100, viewpoint=None, search='brute', cell=None):
        self.search, self.cell = _check_search(search), cell
        self.radius_normal, self.max_nn_normal = radius_normal, _check_max_nn(max_nn_normal)
        self.radius_feature, self.max_nn_feature = radius_feature, _check_max_nn(max_nn_feature)
        self.viewpoint = None if viewpoint is None else np.asarray(viewpoint, dtype=np.float64).reshape(3)

    def many(self, list_of_clouds):
        _need_device('FPFHDescriptor')
        clouds = [_cloud64(c, f'list_of_clouds[{i}]') for i, c in enumerate(list_of_clouds)]
        if not clouds:
            return []
        off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        if off[-1] == 0:
            return [np.zeros((0, BINS), dtype=np.float32) for _ in clouds]
        pts = torch.from_numpy(np.concatenate(clouds) if len(clouds) > 1 else clouds[0]).cuda()
        vps = None if self.viewpoint is None else np.tile(self.viewpoint, (len(clouds), 1))
        feats = fpfh_batch(pts, off, None, self.radius_normal, self.max_nn_normal, self.radius_feature, self.max_nn_feature, vps,
                           self.search, self.cell)
        feats = feats[:, :BINS].cpu().numpy()
        return [np.ascontiguousarray(feats[off[i]:off[i + 1]]) for i in range(len(clouds))]

    def __call__(self, points):
        return self.many([points])[0]
