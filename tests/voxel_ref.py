"""NumPy fp64 yardstick of the voxel grid and of voxel down-sampling (csrc/voxel.hip through utils/voxel.py): a restatement of the
contract in include/sgaligner_hip.h -- bounds, origin, cell coordinates, keys, the stable argsort, heads, voxel ids, and the means by
explicit ascending loops.  Every operation is rounded on its own, as NumPy's elementwise fp64 arithmetic does.  Open3D is not available
to compare against: that contract, not Open3D's output, is what the kernels are held to (the voxels are numbered in ascending
(kx, ky, kz), not in Open3D's hash-map order).  The yardstick of the grid neighbour lists is fpfh_ref.lists_ref itself."""
import numpy as np

DROPPED = 65535
MAX_CLOUDS = 32767


def grid_ref(p, h):
    """One cloud, cell edge h -> (origin [3], dims [3] int32, cells [n, 3] int64 with 65535 for a dropped point, status 0 / 2)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    h = np.float64(h)
    n = len(p)
    kept = np.isfinite(p).all(1)
    origin, dims = np.zeros(3), np.zeros(3, dtype=np.int32)
    cells = np.full((n, 3), DROPPED, dtype=np.int64)
    if not (h > 0 and np.isfinite(h)):
        return origin, dims, cells, 2
    if kept.any():
        with np.errstate(over='ignore', invalid='ignore'):
            origin = p[kept].min(0) - 0.5 * h
            kmax = np.floor((p[kept].max(0) - origin) / h)
        if not ((kmax >= 0) & (kmax < DROPPED)).all():
            return origin, dims, cells, 2
        dims = (kmax + 1).astype(np.int32)
        cells[kept] = np.floor((p[kept] - origin) / h).astype(np.int64)
    return origin, dims, cells, 0


def voxels_ref(clouds, cell, normals=None):
    """Clouds packed back to back, cell: one edge for all or one per cloud -> dict with origin [C, 3], dims [C, 3], status [C], keys
    [total] int64, order [total] int32 (stable argsort), sorted_keys, voxel_of_point [total] int32 (-1: dropped), voxel_offsets [C + 1]
    int32, voxel_first [n_vox] int32, counts [n_vox] int32, out_points [n_vox, 3] and, with `normals` (packed [total, 3]), out_normals
    [n_vox, 3]: the plain mean, not re-normalised."""
    clouds = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds]
    C = len(clouds)
    hs = np.broadcast_to(np.asarray(cell, dtype=np.float64), (C,))
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    total = int(off[-1])
    pts = np.concatenate(clouds) if C else np.zeros((0, 3))
    origin, dims, status = np.zeros((C, 3)), np.zeros((C, 3), dtype=np.int32), np.zeros(C, dtype=np.int32)
    keys = np.zeros(total, dtype=np.int64)
    for c, p in enumerate(clouds):
        origin[c], dims[c], cells, status[c] = grid_ref(p, hs[c])
        if C > MAX_CLOUDS:
            status[c], dims[c], cells = 2, 0, np.full_like(cells, DROPPED)
        cf = c if C <= MAX_CLOUDS else 0
        keys[off[c]:off[c + 1]] = (cf << 48) | (cells[:, 0] << 32) | (cells[:, 1] << 16) | cells[:, 2]
    order = np.argsort(keys, kind='stable').astype(np.int32)
    sk = keys[order]
    dropped = (sk & 0xFFFFFFFFFFFF) == 0xFFFFFFFFFFFF
    first_of_cloud = np.zeros(total, dtype=bool)
    first_of_cloud[off[:-1][np.diff(off) > 0]] = True
    head = ~dropped & (first_of_cloud | (np.concatenate([[-1], sk[:-1]]) != sk))
    vid = np.cumsum(head) - 1                                               # global voxel id of each sorted position's run
    n_vox = int(head.sum())
    voxel_offsets = np.concatenate([[0], np.cumsum(head)])[off].astype(np.int32)
    voxel_first = np.flatnonzero(head).astype(np.int32)
    voxel_of_point = np.full(total, -1, dtype=np.int32)
    cloud_of_pos = np.repeat(np.arange(C), np.diff(off))
    voxel_of_point[order[~dropped]] = (vid[~dropped] - voxel_offsets[cloud_of_pos[~dropped]]).astype(np.int32)
    counts = np.bincount(vid[~dropped], minlength=n_vox).astype(np.int32)
    out = dict(origin=origin, dims=dims, status=status, keys=keys, order=order, sorted_keys=sk, voxel_of_point=voxel_of_point,
               voxel_offsets=voxel_offsets, voxel_first=voxel_first, counts=counts, offsets=off)
    for name, src in (('out_points', pts), ('out_normals', normals)):
        if src is None:
            continue
        src = np.asarray(src, dtype=np.float64).reshape(total, 3)
        acc = np.zeros((n_vox, 3))
        for s in range(int(counts.max()) if n_vox else 0):                  # the s-th member of every voxel that has one, s ascending
            live = np.flatnonzero(counts > s)
            with np.errstate(invalid='ignore', over='ignore'):
                acc[live] = acc[live] + src[order[voxel_first[live] + s]]
        with np.errstate(invalid='ignore', over='ignore'):
            out[name] = acc / counts.astype(np.float64)[:, None]
    return out


def downsample_ref(points, voxel_size, normals=None):
    """One cloud -> points [n_vox, 3], or (points, normals)."""
    v = voxels_ref([points], voxel_size, normals)
    if v['status'][0] != 0:
        raise ValueError('grid too fine')
    return v['out_points'] if normals is None else (v['out_points'], v['out_normals'])
