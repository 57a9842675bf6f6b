"""A uniform cell grid over packed clouds on the GPU (csrc/voxel.hip) and its two consumers: voxel down-sampling -- the reference's
utils/open3d.py:68-76 -- and the grid route of utils.features.neighbour_lists.

    points -> sga_voxel_keys -> torch.sort(keys, stable=True) -> sga_voxel_cells -> sga_voxel_downsample | sga_knn_lists_grid

The 64-bit sort is the one borrowed step (torch.sort); the library verifies the order it is handed, so a wrong one yields status 3 for that
cloud and never an out-of-bounds access.  Open3D is not a dependency and equality with its output is not tested: the contract written in
include/sgaligner_hip.h is the definition, and tests/voxel_ref.py restates it in numpy.  In particular the voxels of a cloud come in
ascending (kx, ky, kz) order, NOT in Open3D's hash-map order, and colours are not carried.  Nothing here falls back to the host: without
a HIP device the functions raise."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import check_dtype, device_tensor, workspace
from .point_cloud import _cloud64, _need_device

STATUS_TEXT = {2: 'the grid is too fine (a cell coordinate reaches 65535, or more than 32767 clouds)', 3: 'the sort order is not the stable argsort of the keys'}


class VoxelGrid:
    """What sga_voxel_keys and sga_voxel_cells give for one packed call, all HIP tensors: cell [C] and origin [C, 3] float64, dims [C, 3]
    int32, keys / sorted_keys [total] int64, order [total] int32, voxel_of_point [total] int32 (cloud-local, -1: dropped),
    voxel_offsets [C + 1] int32, voxel_first [total + 1] int32, status [C] int32 (0 ok, 2 grid too fine, 3 bad order); `clouds` holds
    the points and offsets."""

    def check(self):
        """One small download (voxel_offsets and status) -> voxel_offsets as host int64; ValueError naming the first cloud without a grid."""
        C = self.clouds
        host = torch.cat([self.voxel_offsets, self.status]).cpu().numpy()
        voff, status = host[:C.n_scans + 1].astype(np.int64), host[C.n_scans + 1:]
        bad = np.flatnonzero(status != 0)
        if len(bad):
            raise ValueError(f'voxel grid: cloud {int(bad[0])}: {STATUS_TEXT.get(int(status[bad[0]]), f"status {int(status[bad[0]])}")}')
        return voff

    def search_args(self):
        """The six pointers every grid search takes, in the order of the C ABI: cell, origin, dims, status, order, sorted_keys."""
        return [_p(t) for t in (self.cell, self.origin, self.dims, self.status, self.order, self.sorted_keys)]


def _cell_tensor(cell, n_clouds, dev):
    """cell: one edge for every cloud, or one per cloud (sequence, numpy array or tensor) -> ([C] float64 device tensor, host copy or None)."""
    if isinstance(cell, torch.Tensor) and cell.is_cuda:
        check_dtype(cell, 'cell', torch.float64)
        d = cell.reshape(-1).contiguous()
        if d.numel() != n_clouds:
            raise ValueError(f'cell must hold one edge per cloud ({n_clouds}), got {d.numel()}')
        return d, None
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(cell.cpu() if isinstance(cell, torch.Tensor) else cell, dtype=np.float64).reshape(-1),
                                             (n_clouds,)) if n_clouds else np.zeros(0))
    if not ((h > 0) & np.isfinite(h)).all():
        raise ValueError(f'the cell edge (voxel size) must be > 0 and finite, got {cell}')
    return torch.from_numpy(np.concatenate([h, [0.0]])).to(dev)[:n_clouds], h


def build_grid(points, offsets, cell, order=None) -> VoxelGrid:
    """The cell grid of clouds packed back to back: points [sum N, 3] float64 HIP tensor, offsets [n_clouds + 1] host ints, cell as in
    _cell_tensor.  order: the stable argsort of the keys as an int32 HIP tensor when the caller has one (it is verified either way);
    None: torch.sort(keys, stable=True)."""
    from .features import _clouds
    check_dtype(points, 'points', torch.float64)
    C = _clouds(points, offsets)
    n, total, dev = C.n_scans, C.total_points, C.dev
    G = VoxelGrid()
    G.clouds = C
    G.cell, cell_host = _cell_tensor(cell, n, dev)
    G.origin = torch.zeros((n, 3), device=dev, dtype=torch.float64)
    G.dims = torch.zeros((n, 3), device=dev, dtype=torch.int32)
    G.status = torch.zeros((n,), device=dev, dtype=torch.int32)
    G.keys = torch.empty((total,), device=dev, dtype=torch.int64)
    G.sorted_keys = torch.empty((total,), device=dev, dtype=torch.int64)
    G.voxel_of_point = torch.empty((total,), device=dev, dtype=torch.int32)
    G.voxel_offsets = torch.zeros((n + 1,), device=dev, dtype=torch.int32)
    G.voxel_first = torch.zeros((total + 1,), device=dev, dtype=torch.int32)
    L = _lib.lib()
    if n:
        rc = L.sga_voxel_keys(_p(C.pts), *C.args(), _p(G.cell), None if cell_host is None else cell_host.ctypes.data, _p(G.origin), _p(G.dims),
                              _p(G.keys), _p(G.status), _stream())
        _lib.check(rc, 'sga_voxel_keys')
    if order is None:
        order = torch.sort(G.keys, stable=True)[1].to(torch.int32)
    G.order = device_tensor(order, 'order', torch.int32)
    if tuple(G.order.shape) != (total,):
        raise ValueError(f'order must be [{total}], got {tuple(G.order.shape)}')
    if n:
        nbytes = L.sga_voxel_workspace_bytes(n, total)
        ws = workspace(nbytes, dev)
        rc = L.sga_voxel_cells(*C.args(), _p(G.keys), _p(G.order), _p(G.sorted_keys), _p(G.voxel_of_point), _p(G.voxel_offsets),
                               _p(G.voxel_first), _p(G.status), _p(ws), ws.numel() * 8, _stream())
        _lib.check(rc, 'sga_voxel_cells')
    return G


POINTS_PER_CELL = 0.5        # of max_nn: the default cell of the grid route without a radius (default_cell)


def default_cell(points, offsets, radius=None, max_nn=30):
    """The cell edge the grid route of neighbour_lists takes when none is given -- a speed choice only, the lists do not depend on it.
    With a radius: the radius (the 3 x 3 x 3 block then holds the whole ball of most queries).  Without: per cloud the edge at which an
    occupied cell holds about max_nn / 2 points if the cloud is a surface spread across its bounding box -- scans are --, from the box's
    two largest extents and the point count (sga_cloud_bounds): sqrt(e1 e2 (max_nn / 2) / n).  Half a list per cell was the fastest of
    the edges measured on surfaces; in a cloud that fills its box such cells are nearly empty, and the search then grows its
    block up to 33 cells wide before it gives up on the grid -- pass `cell` there.  -> [n_clouds] float64 HIP tensor, no download."""
    from .features import _clouds
    C = _clouds(points, offsets)
    if radius is not None and float(radius) > 0.0 and np.isfinite(float(radius)):
        return torch.full((C.n_scans,), float(radius), device=C.dev, dtype=torch.float64)
    box = torch.empty((C.n_scans, 6), device=C.dev, dtype=torch.float64)
    edge = torch.ones((C.n_scans,), device=C.dev, dtype=torch.float64)
    if C.n_scans:
        rc = _lib.lib().sga_cloud_bounds(_p(C.pts), *C.args(), _p(box), POINTS_PER_CELL * float(max_nn), _p(edge), _stream())
        _lib.check(rc, 'sga_cloud_bounds')
    return edge


def grid_lists(points, offsets, r2, max_nn, cell=None, radius=None):
    """The grid route of features.neighbour_lists: (count, idx, d2) HIP tensors, bit for bit those of sga_knn_lists.  A cloud whose grid is
    too fine for the key (status 2) is walked whole by the kernel itself, so nothing is downloaded and nothing is refused here."""
    from .features import _clouds
    C = _clouds(points, offsets)
    G = build_grid(C, None, default_cell(C, None, radius, max_nn) if cell is None else cell)
    count = torch.empty((C.total_points,), device=C.dev, dtype=torch.int32)
    idx = torch.empty((C.total_points, max_nn), device=C.dev, dtype=torch.int32)
    d2 = torch.empty((C.total_points, max_nn), device=C.dev, dtype=torch.float64)
    if C.total_points:
        rc = _lib.lib().sga_knn_lists_grid(_p(C.pts), *C.args(), *G.search_args(), r2, max_nn, _p(count), _p(idx), _p(d2), _stream())
        _lib.check(rc, 'sga_knn_lists_grid')
    return count, idx, d2


def voxel_downsample_batch(points, offsets, voxel_size, normals=None):
    """Voxel down-sampling of clouds packed back to back: points [sum N, 3] float64 HIP tensor, offsets [n_clouds + 1] host ints,
    voxel_size one edge for all clouds or one per cloud, normals [sum N, 3] float64 HIP tensor or None.  One output point per occupied
    voxel: the mean of the voxel's points, summed in ascending original index; the normals likewise, NOT re-normalised.  Points with a
    non-finite coordinate are dropped.  The voxels of a cloud come in ascending (kx, ky, kz) -- not Open3D's order.
    -> (out_points [n_vox, 3] float64, out_offsets [n_clouds + 1] host int64, out_normals [n_vox, 3] or None, counts [n_vox] int32,
    voxel_of_point [sum N] int32: the cloud-local voxel of every input point, -1 for a dropped one); HIP tensors but for out_offsets.
    One small download (the voxel prefix and the status) sizes the outputs; ValueError names a cloud whose grid is too fine."""
    check_dtype(points, 'points', torch.float64)
    if normals is not None:
        check_dtype(normals, 'normals', torch.float64)
    G = build_grid(points, offsets, voxel_size)
    C = G.clouds
    nr = None
    if normals is not None:
        nr = device_tensor(normals, 'normals', torch.float64)
        if tuple(nr.shape) != (C.total_points, 3):
            raise ValueError(f'normals must be [{C.total_points}, 3], got {tuple(nr.shape)}')
    voff = G.check()
    out_pts = torch.empty((C.total_points, 3), device=C.dev, dtype=torch.float64)
    out_nr = torch.empty((C.total_points, 3), device=C.dev, dtype=torch.float64) if nr is not None else None
    out_count = torch.empty((C.total_points,), device=C.dev, dtype=torch.int32)
    if C.total_points and C.n_scans:
        rc = _lib.lib().sga_voxel_downsample(_p(C.pts), _p(nr) if nr is not None else None, *C.args(), _p(G.order), _p(G.sorted_keys),
                                             _p(G.voxel_offsets), _p(G.voxel_first), _p(G.status), _p(out_pts),
                                             _p(out_nr) if nr is not None else None, _p(out_count), _stream())
        _lib.check(rc, 'sga_voxel_downsample')
    n_vox = int(voff[-1])
    return out_pts[:n_vox], voff, None if out_nr is None else out_nr[:n_vox], out_count[:n_vox], G.voxel_of_point


def voxel_downsample_many(list_of_clouds, voxel_size):
    """[points [n_i, 3] numpy, ...] -> their down-sampled clouds as float64 numpy arrays: one upload, one launch set, one download."""
    _need_device('voxel_downsample')
    clouds = [_cloud64(c, f'list_of_clouds[{i}]') for i, c in enumerate(list_of_clouds)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    if not clouds or off[-1] == 0:
        return [np.zeros((0, 3)) for _ in clouds]
    pts = torch.from_numpy(np.concatenate(clouds) if len(clouds) > 1 else clouds[0]).cuda()
    out, voff, _, _, _ = voxel_downsample_batch(pts, off, voxel_size)
    out = out.cpu().numpy()
    return [np.ascontiguousarray(out[voff[i]:voff[i + 1]]) for i in range(len(clouds))]


def voxel_downsample(points, voxel_size, normals=None):
    """utils/open3d.py:68-76 for one cloud: points [n, 3] numpy (and normals [n, 3]) -> points [n_vox, 3] float64 numpy, or the pair
    (points, normals)."""
    _need_device('voxel_downsample')
    p = _cloud64(points, 'points')
    nr = None if normals is None else _cloud64(normals, 'normals')
    if nr is not None and nr.shape != p.shape:
        raise ValueError(f'normals must be {p.shape}, got {nr.shape}')
    if len(p) == 0:
        return p if nr is None else (p, nr)
    out, _, out_nr, _, _ = voxel_downsample_batch(torch.from_numpy(p).cuda(), [0, len(p)], voxel_size,
                                                  None if nr is None else torch.from_numpy(nr).cuda())
    return out.cpu().numpy() if nr is None else (out.cpu().numpy(), out_nr.cpu().numpy())
