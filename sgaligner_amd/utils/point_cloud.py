"""Host-side mirror of the reference's utils/point_cloud.py sampling and nearest-neighbour helpers, backed by the HIP kernels.

`pcl_farthest_sample(point, npoint, return_idxs)` keeps the reference signature and semantics (utils/point_cloud.py:
61-89): N < npoint -> random draw with replacement on the host (np.random.choice, :70-73); otherwise the first sample is
drawn with np.random.randint(0, N) (:77) and the remaining ones come from csrc/fps.hip (bit-identical index sequence).
`farthest_point_sample_batch` is the batched form preprocessing wants: all objects of a scan (or of many scans) in
one launch.

`get_nearest_neighbor`, `compute_pcl_overlap` and `apply_transform` keep the reference signatures (utils/point_cloud.py:136-157,
91-103); `nearest_neighbor_batch` / `compute_pcl_overlap_pairs` are the batched forms (csrc/nnsearch.hip: exact fp64 brute force,
distances bit-identical to cKDTree's, ties to the lowest index; search='grid': the same answers through the support cloud's cell grid,
with a radius and a transform per job, csrc/icp.hip).

`inverse_relative` and `get_visible_pts_from_cam_pose` keep the reference signatures (utils/point_cloud.py:105-134);
`visible_masks_batch` is the packed form (csrc/visibility.hip: every frame of every scan in one launch, bit masks out)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import PackedLayout, PairJobs, check_dtype, check_finite, device_tensor, prefix_offsets, resolve_chunk, split_chunk, upload, workspace

SMALL_MAX, MID_MAX = 2048, 8192          # register-resident kernel variants (8 / 32 points per lane)


def farthest_point_sample_batch(points, offsets, npoint: int, start) -> torch.Tensor:
    """points [sum N, 3] float32 CUDA tensor (objects packed back to back), offsets [n_obj+1] (host ints or tensor),
    start [n_obj] first sample per object.  Returns idx [n_obj, npoint] int32 (object-local), on the GPU."""
    pts = device_tensor(points, 'points', torch.float32)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f'points must be [N,3], got {tuple(pts.shape)}')
    off = prefix_offsets(offsets, 'offsets', pts.shape[0])
    n_obj = len(off) - 1
    sizes = np.diff(off)
    if (sizes < npoint).any():
        raise ValueError('every object needs N >= npoint (the N < npoint branch is a host-side random draw)')
    st = np.asarray(start.cpu() if isinstance(start, torch.Tensor) else start, dtype=np.int64)
    if st.shape != (n_obj,) or (st < 0).any() or (st >= sizes).any():
        raise ValueError('start must hold one in-range index per object')
    dev = pts.device
    ids = np.arange(n_obj, dtype=np.int32)
    small, mid, large = ids[sizes <= SMALL_MAX], ids[(sizes > SMALL_MAX) & (sizes <= MID_MAX)], ids[sizes > MID_MAX]
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    d_off, d_start = to_dev(off), to_dev(st)
    d_small, d_mid, d_large = to_dev(small), to_dev(mid), to_dev(large)
    out = torch.empty((n_obj, npoint), device=dev, dtype=torch.int32)
    L = _lib.lib()
    scratch = torch.empty((L.sga_fps_scratch_floats(int(pts.shape[0])) if len(large) else 1,), device=dev, dtype=torch.float32)
    if n_obj:
        rc = L.sga_fps(_p(pts), _p(d_off), n_obj, _p(d_start), npoint, _p(d_small), len(small), _p(d_mid), len(mid),
                       _p(d_large), len(large), _p(out), _p(scratch), _stream())
        _lib.check(rc, 'sga_fps')
    return out


def pcl_farthest_sample(point, npoint, return_idxs=False):
    """Reference signature (utils/point_cloud.py:61): point [N, D] numpy array -> sampled [npoint, D] (and the indices)."""
    N, D = point.shape
    if N < npoint:
        indices = np.random.choice(point.shape[0], npoint)
        return point[indices]
    farthest = np.random.randint(0, N)
    xyz = torch.from_numpy(np.ascontiguousarray(point[:, :3], dtype=np.float32)).cuda()
    idx = farthest_point_sample_batch(xyz, [0, N], npoint, [farthest])[0].cpu().numpy().astype(np.int32)
    if return_idxs:
        return point[idx], idx
    return point[idx]


# ---- convex-hull barycentre (preprocessing/scan3r/preprocess.py:93-96) ---------------------------------------------------
def hull_candidate_mask_batch(points, offsets):
    """points [sum N, 3] float32 CUDA tensor (objects packed back to back), offsets [n_obj+1] host ints.  Returns
    (keep [sum N] bool CUDA tensor, n_planes [n_obj] int32 CUDA tensor): points that can be hull vertices (csrc/hull.hip)."""
    pts = device_tensor(points, 'points', torch.float32)
    off = prefix_offsets(offsets, 'offsets', pts.shape[0])
    n_obj = len(off) - 1
    d_off = torch.from_numpy(off.astype(np.int32)).to(pts.device)
    keep = torch.empty((max(int(pts.shape[0]), 1),), device=pts.device, dtype=torch.uint8)
    npl = torch.zeros((max(n_obj, 1),), device=pts.device, dtype=torch.int32)
    _lib.check(_lib.lib().sga_hull_candidates(_p(pts), _p(d_off), n_obj, _p(keep), _p(npl), _stream()), 'sga_hull_candidates')
    return keep[:pts.shape[0]].bool(), npl[:n_obj]


HULL_ON_DEVICE = True          # tests flip it to cross-check the device hull against Qhull on the same candidates


def hull_vertices_device(cand64, offsets):
    """The device-resident form of hull_vertices_batch: cand64 [sum n, 3] float64 CUDA tensor, offsets [n_obj+1] host ints (n_obj >= 1,
    at least one point).  Returns (is_vertex [sum n] uint8, status [n_obj] int32) CUDA tensors; nothing is downloaded."""
    d_pts = device_tensor(cand64, 'cand64', torch.float64)
    off = prefix_offsets(offsets, 'offsets', d_pts.shape[0])
    n_obj = len(off) - 1
    if n_obj <= 0 or off[-1] == 0:
        raise ValueError('offsets must cover the points of at least one object')
    d_off = torch.from_numpy(off.astype(np.int32)).to(d_pts.device)
    isv = torch.zeros((int(off[-1]),), device=d_pts.device, dtype=torch.uint8)
    status = torch.full((n_obj,), -1, device=d_pts.device, dtype=torch.int32)
    _lib.check(_lib.lib().sga_hull_vertices(_p(d_pts), _p(d_off), n_obj, _p(isv), _p(status), _stream()), 'sga_hull_vertices')
    return isv, status


def hull_vertices_batch(cand64, offsets):
    """cand64 [sum n, 3] float64 numpy (objects packed back to back), offsets [n_obj+1].  Returns (is_vertex [sum n] bool numpy,
    status [n_obj] int numpy): the device gift-wrapping hull with its certificate (csrc/hull.hip, sga_hull_vertices); status != 0
    marks the objects the caller has to hand to Qhull."""
    off = np.asarray(offsets, dtype=np.int64)
    n_obj = len(off) - 1
    if n_obj <= 0 or off[-1] == 0:
        return np.zeros((int(off[-1]) if len(off) else 0,), dtype=bool), np.ones((max(n_obj, 0),), dtype=np.int32)
    isv, status = hull_vertices_device(torch.from_numpy(np.ascontiguousarray(cand64, dtype=np.float64)).cuda(), off)
    return isv.cpu().numpy().astype(bool), status.cpu().numpy()


def _hull_means(cand, coff, counts, n_obj, verts, qhull_points):
    """The tail the two barycentre functions share.  cand [sum n, 3] float64 host candidates packed by coff / counts; verts: None (no device
    hull) or (is_vertex bool [sum n], status [n_obj]); qhull_points(i): object i's candidates in its own values, for the objects the device
    declined.  Returns (barycentres [n_obj, 3] float64, number of objects that went to Qhull)."""
    out = np.zeros((n_obj, 3))
    todo = np.ones((n_obj,), dtype=bool)
    if verts is not None:
        isv, status = verts
        ok = status == 0
        if ok.any():
            w = isv.astype(np.float64)
            seg = np.minimum(coff[:-1], max(len(w) - 1, 0))
            nz = counts > 0
            nv = np.where(nz, np.add.reduceat(w, seg), 0.0)
            for c in range(3):
                sm = np.where(nz, np.add.reduceat(cand[:, c] * w, seg), 0.0)
                out[ok, c] = sm[ok] / nv[ok]
            todo = ~ok
    n_q = 0
    if todo.any():
        from scipy.spatial import ConvexHull
        for i in np.flatnonzero(todo):
            hull = ConvexHull(qhull_points(i))
            v = hull.points[hull.vertices]
            out[i] = (np.mean(v[:, 0]), np.mean(v[:, 1]), np.mean(v[:, 2]))
            n_q += 1
    return out, n_q


def convex_hull_barycenters_batch(point_list, return_info=False):
    """Barycentre of the convex-hull vertices of every object (list of [N_i, 3] numpy arrays), as preprocess.py:93-96 computes
    it per object: cx, cy, cz = mean of hull.points[hull.vertices, 0 / 1 / 2].  Three steps, no per-object host loop on the common path:
    (1) one launch filters all objects down to their hull candidates (sga_hull_candidates); (2) one launch wraps every object's
    candidates into its hull vertices in fp64, with a certificate (sga_hull_vertices); (3) the vertex means are segment sums.  Objects
    the device declines (fewer than 4 or more than 512 candidates, coplanar / near-degenerate facets: lattices, flat objects) go to
    Qhull -- scipy, the reference's own dependency -- on their candidates, so every answer is the reference's."""
    sizes = [int(p.shape[0]) for p in point_list]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_obj = len(point_list)
    if off[-1] == 0:
        return (np.zeros((n_obj, 3)), {'device': 0, 'qhull': 0}) if return_info else np.zeros((n_obj, 3))
    src = np.concatenate([np.asarray(p)[:, :3] for p in point_list])          # the objects' own values (float32 scans stay float32)
    flat = src if src.dtype == np.float32 else src.astype(np.float32)
    keep, _ = hull_candidate_mask_batch(torch.from_numpy(np.ascontiguousarray(flat)).cuda(), off)
    keep = keep.cpu().numpy()
    # fp32 can merge distinct fp64 points; the filter only ever DISCARDS points that are interior by a margin far above that rounding
    idx = np.flatnonzero(keep)
    counts = np.add.reduceat(keep.astype(np.int64), np.minimum(off[:-1], len(keep) - 1)) * (np.diff(off) > 0)
    coff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cand = src[idx].astype(np.float64, copy=False)                            # exact: float32 -> float64
    verts = hull_vertices_batch(cand, coff) if HULL_ON_DEVICE else None
    # Qhull sees the candidates in the object's own dtype / values
    out, n_q = _hull_means(cand, coff, counts, n_obj, verts, lambda i: np.asarray(point_list[i])[keep[off[i]:off[i + 1]]])
    if return_info:
        return out, {'device': int(n_obj - n_q), 'qhull': int(n_q)}
    return out


def convex_hull_barycenters_device(points, offsets, return_info=False):
    """The device-resident form of convex_hull_barycenters_batch: points [sum N, 3] float32 CUDA tensor (objects packed back to back, e.g.
    the output of preprocessing.scene_graphs.object_partition_batch), offsets [n_obj+1] host ints.  Same three steps and the same answers;
    the points are never uploaded again.  Downloads: the candidates' indices (their number per object sizes the second launch), then the
    candidates themselves with their vertex flags -- a few per cent of the points.  Objects the device hull declines go to Qhull on the
    downloaded candidates (float32 values, the scan's own)."""
    pts = device_tensor(points, 'points', torch.float32)
    off = prefix_offsets(offsets, 'offsets', pts.shape[0])
    n_obj = len(off) - 1
    if off[-1] == 0:
        return (np.zeros((n_obj, 3)), {'device': 0, 'qhull': 0}) if return_info else np.zeros((n_obj, 3))
    keep, _ = hull_candidate_mask_batch(pts, off)
    d_idx = torch.nonzero(keep).reshape(-1)
    idx = d_idx.cpu().numpy()                                                  # ascending: the candidates stay packed per object
    coff = np.searchsorted(idx, off).astype(np.int64)
    counts = np.diff(coff)
    d_cand = pts[d_idx]
    verts = None
    if HULL_ON_DEVICE and len(idx):
        isv, status = hull_vertices_device(d_cand.double(), coff)              # exact: float32 -> float64
        verts = (isv.cpu().numpy().astype(bool), status.cpu().numpy())
    cand32 = d_cand.cpu().numpy()
    out, n_q = _hull_means(cand32.astype(np.float64), coff, counts, n_obj, verts, lambda i: cand32[coff[i]:coff[i + 1]])
    if return_info:
        return out, {'device': int(n_obj - n_q), 'qhull': int(n_q)}
    return out


def convex_hull_barycenter(obj_pcl):
    """Single-object form: (cx, cy, cz) exactly as preprocess.py:93-96 binds them."""
    c = convex_hull_barycenters_batch([obj_pcl])[0]
    return float(c[0]), float(c[1]), float(c[2])


# ---- exact nearest neighbours (utils/point_cloud.py:91-103, 136-147; utils/registration.py:107-129) -------------------------
NN_CHUNK = None           # support points per workgroup pass of csrc/nnsearch.hip; None = chosen per call (_nn_chunk).  Tests lower it
                          # to force the split (chunked + merged) form on mid-sized inputs.
NN_QUERY_TILE = 1024      # queries per workgroup of nn_kernel (256 lanes x 4)
NN_MIN_CHUNK = 2048       # never split a support finer than this: below it the partial workspace costs more than idle CUs


def _nn_chunk(sizes_q, sizes_s) -> int:
    """Chunk size for a job list, by packed.split_chunk: about 16 workgroups per CU, no further -- the partial workspace is 12 B x n_chunks
    x total queries."""
    tiles = sum(-(-int(q) // NN_QUERY_TILE) for q in sizes_q)
    return split_chunk(tiles, max(sizes_s, default=0), _lib.lib().sga_device_cus(), 16, NN_MIN_CHUNK)


NN_SEARCHES = ('brute', 'grid')
NN_GRID_POINTS_PER_CELL = 16     # the default cell of the cross-cloud grid search: the fastest of 0.5 .. 64 measured on surfaces


def nn_grid_cell(clouds, radius=None):
    """The cell edge the cross-cloud grid search takes when none is given -- a speed choice only, the results do not depend on it: per
    cloud the edge at which an occupied cell of a surface holds about NN_GRID_POINTS_PER_CELL points (voxel.default_cell), capped at the
    radius where one is given (beyond it the 3 x 3 x 3 block holds more than the ball).  -> [n_clouds] float64 HIP tensor, no download."""
    from . import voxel
    edge = voxel.default_cell(clouds, None, None, int(NN_GRID_POINTS_PER_CELL / voxel.POINTS_PER_CELL))
    if radius is not None and float(radius) > 0.0 and np.isfinite(float(radius)):
        edge = torch.clamp(edge, max=float(radius))
    return edge


def _search_grid(pts, off, radius, cell):
    """What every cross-cloud grid search starts from: the clouds of the call and their grid (utils/voxel.build_grid) at `cell`, or at
    nn_grid_cell's edge when none is given.  -> (clouds, grid)"""
    from . import voxel
    from .features import _Clouds
    C = _Clouds(pts, off)
    return C, voxel.build_grid(C, None, nn_grid_cell(C, radius) if cell is None else cell)


def _nn_grid(pts, J, radius, transforms, cell, squared, dist, idx):
    """The grid route of nearest_neighbor_batch (csrc/icp.hip): the grid of every cloud of the call (utils/voxel.build_grid), then one
    launch for all jobs.  The cell edge is a speed choice only (nn_grid_cell)."""
    r2 = float('inf') if radius is None else float(radius) * float(radius)
    if not r2 >= 0.0:
        raise ValueError(f'radius must be >= 0 or None, got {radius}')
    tr = None
    if transforms is not None:
        tr = device_tensor(transforms, 'transforms', torch.float64)
        if tuple(tr.shape) != (J.n_pairs, 12):
            raise ValueError(f'transforms must be [{J.n_pairs}, 12] (row-major R | t per job), got {tuple(tr.shape)}')
    C, G = _search_grid(pts, J.off, radius, cell)
    _, d_pr, d_oo = upload(J.host_parts(), pts.device)
    rc = _lib.lib().sga_nn_search_grid(_p(pts), _p(C.d_off), J.n_sets, int(pts.shape[0]), _p(d_pr), J.n_pairs, _p(d_oo), J.total_q, J.max_q,
                                       J.h_off.ctypes.data, J.h_pr.ctypes.data, *G.search_args(), _p(tr) if tr is not None else None, r2,
                                       1 if squared else 0, _p(dist), _p(idx), _stream())
    _lib.check(rc, 'sga_nn_search_grid')


def nearest_neighbor_batch(points, offsets, pairs, chunk=None, squared=False, search='brute', radius=None, transforms=None, cell=None):
    """points [sum N, 3] float64 CUDA tensor (clouds packed back to back), offsets [n_clouds+1] host ints, pairs [n_pairs, 2] host ints
    (query cloud, support cloud).  One launch for all jobs.  Returns (dist [sum nq] float64, idx [sum nq] int32, out_offsets
    [n_pairs+1] int64 numpy): job p's results are dist[out_offsets[p]:out_offsets[p+1]]; idx is support-cloud-local, the LOWEST index among
    exactly equal minima; an empty support gives (+inf, -1).  dist is the correctly rounded sqrt of (dx*dx + dy*dy) + dz*dz (bit-identical
    to cKDTree(s).query(q)[0]); squared=True returns that sum itself.
    search='grid' looks only at the cells of the support cloud's grid around each query (csrc/icp.hip) and gives the SAME outputs, bit for
    bit, whatever `cell` is (one edge for all clouds or one per cloud; None: nn_grid_cell -- about 16 points per occupied cell of a surface,
    never above the radius).  Only that route takes radius (a query without a support point within it gets (+inf, -1); None: no radius) and transforms
    ([n_pairs, 12] float64 HIP tensor, row-major R | t: job p's queries are moved by it first, ((m0 x + m1 y) + m2 z) + m9 ..., no fma)."""
    if search not in NN_SEARCHES:
        raise ValueError(f'search must be one of {NN_SEARCHES}, got {search!r}')
    if search == 'brute' and (radius is not None or transforms is not None or cell is not None):
        raise ValueError("radius, transforms and cell belong to search='grid'")
    if transforms is not None:
        check_dtype(transforms, 'transforms', torch.float64)
    pts = device_tensor(points, 'points', torch.float64)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f'points must be [N,3], got {tuple(pts.shape)}')
    J = PairJobs(offsets, pts.shape[0], pairs, 'nearest_neighbor_batch', 'cloud')
    check_finite(pts, 'points', 'coordinates')
    dev = pts.device
    dist = torch.empty((J.total_q,), device=dev, dtype=torch.float64)
    idx = torch.empty((J.total_q,), device=dev, dtype=torch.int32)
    if J.total_q == 0:
        return dist, idx, J.out_off
    if search == 'grid':
        _nn_grid(pts, J, radius, transforms, cell, squared, dist, idx)
        return dist, idx, J.out_off
    chunk = resolve_chunk(chunk, NN_CHUNK, lambda: _nn_chunk(J.nq, J.ns))
    L = _lib.lib()
    d_off, d_pr, d_oo = upload(J.host_parts(), dev)                                           # one small upload
    ws_bytes = int(L.sga_nn_workspace_bytes(J.total_q, J.max_s, chunk))
    ws = workspace(ws_bytes, dev)
    rc = L.sga_nn_search(_p(pts), _p(d_off), J.n_sets, int(pts.shape[0]), _p(d_pr), J.n_pairs, _p(d_oo), J.total_q, J.max_q, J.max_s, chunk,
                         J.h_off.ctypes.data, J.h_pr.ctypes.data, 1 if squared else 0, _p(dist), _p(idx), _p(ws), ws_bytes, _stream())
    _lib.check(rc, 'sga_nn_search')
    return dist, idx, J.out_off


def _need_device(what: str):
    if not torch.cuda.is_available():
        raise RuntimeError(f'sgaligner_amd: `{what}` needs a HIP device (torch.cuda.is_available() is False); there is no CPU path')


def _cloud64(a, name: str):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError(f'{name} must be [N, 3], got {a.shape}')
    return np.ascontiguousarray(a[:, :3], dtype=np.float64)


def _nn_numpy(clouds, pairs):
    """clouds: list of [N_i, 3] float64 numpy arrays; one upload, one launch, one download.  -> list of (dist, idx int64) per pair."""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(clouds) if len(clouds) > 1 else clouds[0]).cuda()
    dist, idx, oo = nearest_neighbor_batch(pts, off, pairs)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    return [(dist[oo[p]:oo[p + 1]], idx[oo[p]:oo[p + 1]]) for p in range(len(pairs))]


def get_nearest_neighbor(q_points: np.ndarray, s_points: np.ndarray, return_index: bool = False):
    """Reference signature (utils/point_cloud.py:136): the distance from every query point to its nearest support point (float64
    numpy, bit-identical to cKDTree(s_points).query(q_points, k=1)[0] for 3-D input) and, with return_index, that point's index (int64;
    the lowest one among exactly equal minima, where cKDTree's choice is arbitrary)."""
    _need_device('get_nearest_neighbor')
    q, s = _cloud64(q_points, 'q_points'), _cloud64(s_points, 's_points')
    if len(s) == 0:
        raise ValueError('get_nearest_neighbor: s_points is empty')
    dist, idx = _nn_numpy([q, s], [(0, 1)])[0]
    return (dist, idx) if return_index else dist


def _overlap_of(dist, n_source: int, threshold: float):
    common = np.flatnonzero(dist <= threshold).astype(np.int64)          # sorted and unique by construction, as np.unique returns them
    return round(common.shape[0] / n_source, 4), common


def compute_pcl_overlap(source, target, threshold=1e-7):
    """Reference signature (utils/point_cloud.py:91): (round(ratio, 4), common_pts_idx_src) -- the source points that have a target point
    within `threshold` (fp64), as sorted unique int64 indices, and their share of the source.  A source point is common iff the distance
    to its NEAREST target point is <= threshold.  The reference asks open3d's RadiusSearch; whether that includes a neighbour exactly AT
    the radius is not pinned here (open3d is not available to compare against) -- with the default 1e-7 on scan data the question does
    not arise: shared points are bitwise copies (distance 0), all others are millimetres apart."""
    _need_device('compute_pcl_overlap')
    return compute_pcl_overlap_pairs([source, target], [(0, 1)], threshold)[0]


def compute_pcl_overlap_pairs(clouds, pairs, threshold=1e-7):
    """The batched form preprocessing/scan3r/subgenscan3r.py:107-118 wants: clouds = the subscans of a scan (list of [N_i, 3] arrays),
    pairs = [(source, target), ...] cloud ids.  One upload and one launch for all pairs; returns [compute_pcl_overlap(clouds[s],
    clouds[t], threshold) for s, t in pairs]."""
    _need_device('compute_pcl_overlap_pairs')
    cl = [_cloud64(c, f'clouds[{i}]') for i, c in enumerate(clouds)]
    pairs = [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if len(cl[a]) == 0 or len(cl[b]) == 0:
            raise ValueError(f'compute_pcl_overlap: cloud {a if len(cl[a]) == 0 else b} is empty')
    if not pairs:
        return []
    return [_overlap_of(d, len(cl[a]), threshold) for (d, _), (a, _b) in zip(_nn_numpy(cl, pairs), pairs)]


def apply_transform(points: np.ndarray, transform: np.ndarray, normals=None):
    """Reference signature (utils/point_cloud.py:149): points @ R^T + t for a 4x4 rigid transform (numpy, on the host)."""
    rot, trans = transform[:3, :3], transform[:3, 3]
    moved = np.matmul(points, rot.T) + trans
    if normals is None:
        return moved
    return moved, np.matmul(normals, rot.T)


# ---- frame visibility (utils/point_cloud.py:105-134; the frame loop of preprocessing/scan3r/subgenscan3r.py:188-234) ---------------------
def inverse_relative(pose1To2):
    """Reference signature (utils/point_cloud.py:105): the inverse of a rigid 4x4 pose, on the host.  The result is a FLOAT32 array, as in
    the reference -- the world-to-camera matrix the visibility test sees is float32-valued."""
    pose1To2 = np.asarray(pose1To2)
    rot_t = np.transpose(pose1To2[:3, :3])
    pose2To1 = np.zeros((4, 4), dtype='float32')
    pose2To1[:3, :3] = rot_t
    pose2To1[:3, 3:4] = -np.dot(rot_t, pose1To2[:3, 3:4])
    pose2To1[3, 3] = 1
    return pose2To1


def intrinsic_row(intrinsic_info) -> np.ndarray:
    """fx, fy, cx, cy, u_max, v_max (float64) of a load_intrinsics() dict.  The reference compares the FIRST image coordinate against
    `height` and the second against `width` (utils/point_cloud.py:130-131); that is reproduced on purpose: u_max = height, v_max = width."""
    mat = np.asarray(intrinsic_info['intrinsic_mat'])
    return np.array([mat[0, 0], mat[1, 1], mat[0, 2], mat[1, 2], intrinsic_info['height'], intrinsic_info['width']], dtype=np.float64)


def world_to_cam_rows(cam_2_world_poses) -> np.ndarray:
    """[F, 4, 4] camera-to-world poses -> [F, 12] float64: rows 0-2 of inverse_relative(pose), row-major (float32 values, widened)."""
    poses = np.asarray(cam_2_world_poses)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f'poses must be [F, 4, 4], got {poses.shape}')
    out = np.empty((poses.shape[0], 12), dtype=np.float64)
    for f in range(poses.shape[0]):
        out[f] = inverse_relative(poses[f])[:3].reshape(12)
    return out


def visibility_offsets(pt_off, fr_off):
    """Host prefix arrays of the packed bit matrices: (words per row W [S], vis_off [S + 1] int64 = prefix sum of F_s * W_s)."""
    pt_off, fr_off = np.asarray(pt_off, dtype=np.int64), np.asarray(fr_off, dtype=np.int64)
    words = (np.diff(pt_off) + 63) // 64
    return words, np.concatenate([[0], np.cumsum(np.diff(fr_off) * words)]).astype(np.int64)


class ScanLayout(PackedLayout):
    """Point and frame offsets of a list of scans: pt_off / fr_off [S + 1] (h_pt / h_fr int32 on the host, d_pt / d_fr on the device), words
    per bit-matrix row W [S], vis_off [S + 1] int64 (d_vis on the device, as int32 pairs)."""

    def __init__(self, pt_off, fr_off, total_points: int, total_frames: int, device=None, meta=None):
        super().__init__(pt_off, total_points)
        self.fr_off, self.h_fr, self.total_frames, self.max_frames = self._second(fr_off, 'fr_off', total_frames)
        self.words, self.vis_off = visibility_offsets(self.pt_off, self.fr_off)
        self.total_words = int(self.vis_off[-1])
        views = self._device_views(device, meta)
        if views:
            self.d_vis, self.d_pt, self.d_fr = views

    def host_parts(self):
        return [self.vis_off, self.h_pt, self.h_fr]

    def host_args(self):
        return self.h_pt.ctypes.data, self.h_fr.ctypes.data, self.vis_off.ctypes.data


def _bit_matrix(t, name: str, total_words: int):
    t = device_tensor(t, name, torch.int64)
    if t.dim() != 1 or t.numel() < total_words:
        raise ValueError(f'{name} must be a flat int64 tensor of at least {total_words} words, got {tuple(t.shape)}')
    return t


def visible_masks_batch(points, pt_off, w2c, fr_off, intr, out=None, layout=None):
    """The packed form (csrc/visibility.hip, sga_frame_visibility): points [sum N, 3] float32, w2c [sum F, 12] float64 (world_to_cam_rows),
    intr [S, 6] float64 (intrinsic_row) HIP device tensors, scans packed back to back; pt_off / fr_off [S + 1] host ints (or a ScanLayout
    that already holds them).  One launch.  Returns (vis, vis_off): vis [total_words] int64 device tensor holding every scan's bit matrix --
    scan s's F_s rows of W_s = ceil(N_s / 64) words start at vis_off[s] (int64 numpy, [S + 1]); bit p % 64 of word p / 64 of a row is point
    p, padding bits 0."""
    for t, name, dt in ((points, 'points', torch.float32), (w2c, 'w2c', torch.float64), (intr, 'intr', torch.float64)):
        check_dtype(t, name, dt)                                              # every dtype before any device: told apart without a device
    pts, m, k = device_tensor(points, 'points', torch.float32), device_tensor(w2c, 'w2c', torch.float64), device_tensor(intr, 'intr', torch.float64)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f'points must be [N, 3], got {tuple(pts.shape)}')
    if m.dim() != 2 or m.shape[1] != 12:
        raise ValueError(f'w2c must be [F, 12], got {tuple(m.shape)}')
    L = layout if layout is not None else ScanLayout(pt_off, fr_off, pts.shape[0], m.shape[0], device=pts.device)
    if L.total_points != pts.shape[0] or L.total_frames != m.shape[0] or tuple(k.shape) != (L.n_scans, 6):
        raise ValueError(f'{L.n_scans} scans of {L.total_points} points and {L.total_frames} frames: got points {tuple(pts.shape)}, w2c '
                         f'{tuple(m.shape)}, intr {tuple(k.shape)} (intr must be [S, 6])')
    out = torch.empty((L.total_words,), device=pts.device, dtype=torch.int64) if out is None else _bit_matrix(out, 'out', L.total_words)
    if L.n_scans == 0 or L.total_words == 0:
        return out, L.vis_off
    rc = _lib.lib().sga_frame_visibility(_p(pts), _p(L.d_pt), _p(m), _p(L.d_fr), _p(k), _p(L.d_vis), L.n_scans, L.total_points, L.total_frames,
                                         L.total_words, L.max_points, L.max_frames, *L.host_args(), _p(out), _stream())
    _lib.check(rc, 'sga_frame_visibility')
    return out, L.vis_off


def unpack_mask_words(words, n_points: int) -> np.ndarray:
    """Host: [..., ceil(n / 64)] 64-bit words (numpy, any 8-byte integer dtype) -> bool [..., n]."""
    words = np.ascontiguousarray(words)
    lead = words.shape[:-1]
    bits = np.unpackbits(words.view(np.uint8).reshape(lead + (-1,)), axis=-1, bitorder='little')
    return bits[..., :n_points].astype(bool)


def get_visible_pts_from_cam_pose(scene_pts, cam_2_world_pose, intrinsic_info):
    """Reference signature (utils/point_cloud.py:112): the bool mask [N] of the scene points that project into the frame with positive
    depth.  One frame per call: upload, launch, download -- preprocessing.subscans.generate_subscan_masks runs all frames of many scans at once."""
    _need_device('get_visible_pts_from_cam_pose')
    pts = np.asarray(scene_pts)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError(f'scene_pts must be [N, 3], got {pts.shape}')
    n = int(pts.shape[0])
    if n == 0:
        return np.zeros((0,), dtype=bool)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float32)).cuda()
    d_m = torch.from_numpy(world_to_cam_rows(np.asarray(cam_2_world_pose)[None])).cuda()
    d_k = torch.from_numpy(intrinsic_row(intrinsic_info)[None]).cuda()
    vis, _ = visible_masks_batch(d_pts, [0, n], d_m, [0, 1], d_k)
    return unpack_mask_words(vis.cpu().numpy(), n)
