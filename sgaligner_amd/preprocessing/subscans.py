"""Subscan generation on the device: the frame loop of the reference's preprocessing/scan3r/subgenscan3r.py:159-234 for a whole list of scans.

For every scan the reference tests every vertex against every camera frame (utils/point_cloud.py:112-134), ORs the per-frame masks while it
walks the frames, closes a subscan whenever the running union reaches the drawn point budget, and builds that subscan's scene graph from
per-object visible-point counts (gen_scene_graph, :51-85).  Here the three steps are three launches of csrc/visibility.hip over all scans:
sga_frame_visibility (bit masks), sga_subscan_walk (in place: row seg_end[k] becomes subscan k's mask) and sga_subscan_object_counts.

Traffic of generate_subscan_masks / generate_subscans: one packed upload of everything the kernels read; one small download of the walk's
integers (a few per frame), which decide WHICH rows are subscans; then only those rows (and their object counts, whose row list is a second,
tiny upload) come back in one download.  The bit matrices themselves never leave the device.  There is no CPU path and no file I/O."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import device_tensor, upload
from ..utils import point_cloud as PC

# dtype of a subscan's `pcl` entry (the reference's utils/scan3r.py:143-144)
PLY_DTYPE = [('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('objectId', 'h'), ('globalId', 'h'),
             ('NYU40', 'u1'), ('Eigen13', 'u1'), ('RIO27', 'u1')]


def object_count_lds_slots() -> int:
    """Largest n_slots for which sga_subscan_object_counts keeps its histogram in LDS; above it the kernel uses global atomics."""
    return int(_lib.lib().sga_subscan_lds_slots())


def draw_max_pts(n_points: int, rng) -> int:
    """The point budget of a scan as the reference draws it (subgenscan3r.py:188); `rng` is the `random` module or a random.Random."""
    return rng.randint(int(0.2 * n_points), int(0.5 * n_points))


def subscan_walk_batch(vis, layout: PC.ScanLayout, max_pts, in_place: bool = True):
    """sga_subscan_walk over the bit matrices `vis` (visible_masks_batch) of the scans in `layout`; max_pts [S] int32 device tensor.
    Per scan: cur |= vis[f]; cum[f] = cur; frame_count[f] = popcount(cur); a count >= max_pts closes subscan k (seg_end[k] = f, seg_count[k])
    and empties cur; the unclosed tail is discarded.  Returns (cum, out): cum is `vis` itself when in_place, else a new matrix; out is ONE
    int32 device tensor [3 * total_frames + S] = seg_end | seg_count | frame_count (each [total_frames], scan s's entries from fr_off[s],
    seg_end scan-local) | n_seg [S] -- split_walk_output() slices it.  Entries past n_seg[s] are unspecified."""
    vis = PC._bit_matrix(vis, 'vis', layout.total_words)
    mp = device_tensor(max_pts, 'max_pts', torch.int32)
    if tuple(mp.shape) != (layout.n_scans,):
        raise ValueError(f'max_pts must be [{layout.n_scans}], got {tuple(mp.shape)}')
    cum = vis if in_place else torch.empty_like(vis)
    tf, s = layout.total_frames, layout.n_scans
    out = torch.empty((3 * tf + s,), device=vis.device, dtype=torch.int32)
    if s:
        rc = _lib.lib().sga_subscan_walk(_p(vis), _p(cum), _p(layout.d_pt), _p(layout.d_fr), _p(layout.d_vis), _p(mp), s, layout.total_points, tf,
                                         layout.total_words, *layout.host_args(), _p(out[:tf]), _p(out[tf:2 * tf]), _p(out[2 * tf:3 * tf]),
                                         _p(out[3 * tf:]), _stream())
        _lib.check(rc, 'sga_subscan_walk')
    return cum, out


def split_walk_output(out, layout: PC.ScanLayout):
    """The walk's packed integers (numpy, downloaded) -> per scan (seg_end [n_seg], seg_count [n_seg], frame_count [F]) int64 arrays."""
    out = np.asarray(out)
    tf = layout.total_frames
    res = []
    for s in range(layout.n_scans):
        f0, f1, k = int(layout.fr_off[s]), int(layout.fr_off[s + 1]), int(out[3 * tf + s])
        empty = f1 == f0 or layout.pt_off[s + 1] == layout.pt_off[s]                   # nothing but n_seg = 0 is written for such a scan
        res.append((out[f0:f0 + k].astype(np.int64), out[tf + f0:tf + f0 + k].astype(np.int64),
                    np.zeros(0, dtype=np.int64) if empty else out[2 * tf + f0:2 * tf + f1].astype(np.int64)))
    return res


def object_counts_batch(bits, layout: PC.ScanLayout, rows, slot, n_slots: int):
    """sga_subscan_object_counts: rows [n_rows, 2] host ints (scan, scan-local frame row of `bits`), slot [sum N] int32 device tensor (the dense
    object slot of every point, np.unique(objectId, return_inverse=True)[1]).  Returns counts [n_rows, n_slots] int32 device tensor: the number
    of set bits of each row per slot.  Exact: integer atomics."""
    bits = PC._bit_matrix(bits, 'bits', layout.total_words)
    sl = device_tensor(slot, 'slot', torch.int32)
    if tuple(sl.shape) != (layout.total_points,):
        raise ValueError(f'slot must be [{layout.total_points}], got {tuple(sl.shape)}')
    h_rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)
    n_rows, n_slots = len(h_rows), int(n_slots)
    if n_slots < 0 or n_rows * max(n_slots, 1) >= 2 ** 31:
        raise ValueError(f'n_slots must be >= 0 and rows x slots below 2^31 (got {n_rows} x {n_slots})')
    if n_rows and (h_rows[:, 0].min() < 0 or h_rows[:, 0].max() >= layout.n_scans or h_rows[:, 1].min() < 0 or
                   (h_rows[:, 1] >= np.diff(layout.fr_off)[h_rows[:, 0]]).any()):
        raise ValueError('rows must name (scan, frame row) pairs inside the layout')
    counts = torch.empty((n_rows, n_slots), device=bits.device, dtype=torch.int32)
    if n_rows and n_slots:
        d_rows = torch.from_numpy(h_rows).to(bits.device)
        rc = _lib.lib().sga_subscan_object_counts(_p(bits), _p(layout.d_pt), _p(layout.d_fr), _p(layout.d_vis), layout.n_scans, layout.total_points,
                                                  layout.total_frames, layout.total_words, layout.max_points, _p(d_rows), n_rows, _p(sl), n_slots,
                                                  *layout.host_args(), h_rows.ctypes.data, _p(counts), _stream())
        _lib.check(rc, 'sga_subscan_object_counts')
    return counts


def _run(scans, max_pts, slots=None, n_slots=0):
    """scans: [(vertices [N, 3], cam-to-world poses [F, 4, 4], intrinsics dict)]; slots: optional [sum N] int32 host array.  Returns per scan
    (seg_end, seg_count, masks bool [n_seg, N], counts int32 [n_seg, n_slots] or None)."""
    n_scans = len(scans)
    max_pts = np.asarray(max_pts, dtype=np.int64).reshape(-1)
    if len(max_pts) != n_scans:
        raise ValueError(f'{n_scans} scans need {n_scans} point budgets, got {len(max_pts)}')
    if n_scans and (max_pts.min() < 0 or max_pts.max() >= 2 ** 31):
        raise ValueError('max_pts must be in [0, 2^31)')
    PC._need_device('generate_subscans')
    pts, w2c, intr = [], [], []
    for i, (v, poses, info) in enumerate(scans):
        v = np.asarray(v)
        if v.ndim != 2 or v.shape[1] < 3:
            raise ValueError(f'scans[{i}]: vertices must be [N, 3], got {v.shape}')
        pts.append(np.ascontiguousarray(v[:, :3], dtype=np.float32))
        w2c.append(PC.world_to_cam_rows(np.asarray(poses).reshape(-1, 4, 4)))
        intr.append(PC.intrinsic_row(info))
    if n_scans == 0:
        return []
    pt_off = np.concatenate([[0], np.cumsum([len(p) for p in pts])])
    fr_off = np.concatenate([[0], np.cumsum([len(m) for m in w2c])])
    L = PC.ScanLayout(pt_off, fr_off, int(pt_off[-1]), int(fr_off[-1]))
    parts = [np.concatenate(w2c).reshape(-1), np.stack(intr).reshape(-1), L.host_meta(), max_pts.astype(np.int32), np.concatenate(pts).reshape(-1)]
    if slots is not None:
        parts.append(np.ascontiguousarray(slots, dtype=np.int32))
    d_w2c, d_intr, d_meta, d_max, d_pts, *d_slot = upload(parts, 'cuda')               # the one upload
    L = PC.ScanLayout(pt_off, fr_off, L.total_points, L.total_frames, meta=d_meta)
    vis, _ = PC.visible_masks_batch(d_pts.view(-1, 3), None, d_w2c.view(-1, 12), None, d_intr.view(-1, 6), layout=L)
    cum, walk = subscan_walk_batch(vis, L, d_max, in_place=True)
    segs = split_walk_output(walk.cpu().numpy(), L)                                    # small: 3 ints per frame; decides which rows are subscans
    rows = [(s, int(f)) for s in range(n_scans) for f in segs[s][0]]
    pieces = [cum[int(L.vis_off[s]) + f * int(L.words[s]):int(L.vis_off[s]) + (f + 1) * int(L.words[s])] for s, f in rows]
    n_words = sum(int(p.numel()) for p in pieces)
    counts = None
    if slots is not None and rows:
        counts = object_counts_batch(cum, L, rows, d_slot[0], n_slots)
        flat = counts.reshape(-1)
        if flat.numel() % 2:
            flat = torch.cat([flat, flat.new_zeros(1)])
        pieces.append(flat.view(torch.int64))
    host = torch.cat(pieces).cpu().numpy() if pieces else np.zeros(0, dtype=np.int64)  # the subscan rows (and their counts) in one download
    h_counts = host[n_words:].view(np.int32)[:len(rows) * n_slots].reshape(len(rows), n_slots) if counts is not None else None
    out, pos, r = [], 0, 0
    for s in range(n_scans):
        seg_end, seg_count, _ = segs[s]
        n, w, k = int(pt_off[s + 1] - pt_off[s]), int(L.words[s]), len(seg_end)
        masks = PC.unpack_mask_words(host[pos:pos + k * w].reshape(k, w), n) if k else np.zeros((0, n), dtype=bool)
        pos += k * w
        c = None
        if slots is not None:
            c = h_counts[r:r + k] if h_counts is not None else np.zeros((0, n_slots), dtype=np.int32)
        r += k
        out.append((seg_end, seg_count, masks, c))
    return out


def generate_subscan_masks(scans, max_pts):
    """scans: a list of (vertices [N, 3] as the ply stores them (float32), camera-to-world poses [F, 4, 4], intrinsics dict with
    'intrinsic_mat', 'width', 'height' as utils/scan3r.load_intrinsics returns it); max_pts: one point budget per scan (draw_max_pts).
    Returns per scan (seg_end [n_seg] int64: the frame that closed each subscan, seg_count [n_seg] int64: its number of points,
    masks bool [n_seg, N]) -- what the reference's loop hands to gen_scene_graph as `curr_visible_mask`, for every subscan of every scan."""
    return [(e, c, m) for e, c, m, _ in _run(scans, max_pts)]


def generate_subscans(ply_vertex, poses, intrinsics, max_pts, objects_json, relationships_json, min_obj_points, scan_id='scan'):
    """One scan, as SubGenScan3R.__getitem__ + gen_scene_graph produce it.  ply_vertex: the ply's vertex element (structured array or mapping
    with the fields of PLY_DTYPE); poses [F, 4, 4] camera-to-world; intrinsics as load_intrinsics returns them; max_pts: the point budget
    (the reference draws it: draw_max_pts); objects_json: the scan's 'objects' list of objects.json; relationships_json: the scan's
    'relationships' list of relationships.json; min_obj_points: cfg.preprocess.min_obj_points.  Returns the list of subscan dicts
    {'pcl', 'subscan_id', 'relationships', 'objects'}: pcl the visible vertices as a PLY_DTYPE array; objects the json entries whose id has
    at least one visible point; relationships the triples whose two ends both have MORE than min_obj_points visible points."""
    x, y, z = (np.asarray(ply_vertex[k]) for k in 'xyz')
    scene_pts = np.stack((x, y, z)).transpose()
    if scene_pts.shape[0] == 0:
        return []
    object_id = np.asarray(ply_vertex['objectId'])
    ids, slot = np.unique(object_id, return_inverse=True)
    (seg_end, seg_count, masks, counts), = _run([(scene_pts, poses, intrinsics)], [max_pts], slots=slot.reshape(-1), n_slots=len(ids))
    subscans = []
    for idx in range(len(seg_end)):
        subscan_id = '{}_{}'.format(scan_id, idx)
        visible_pts_idx = np.where(masks[idx])[0]
        pcl = np.empty(len(visible_pts_idx), dtype=PLY_DTYPE)
        for name, code in PLY_DTYPE:
            pcl[name] = np.asarray(ply_vertex[name])[visible_pts_idx].astype(code)
        n_visible = {int(i): int(c) for i, c in zip(ids, counts[idx])}
        objs = [o for o in objects_json if n_visible.get(int(o['id']), 0) > 0]
        rels = [[sub_id, ob_id, rel_id, rel_name] for (sub_id, ob_id, rel_id, rel_name) in relationships_json
                if n_visible.get(int(sub_id), 0) > min_obj_points and n_visible.get(int(ob_id), 0) > min_obj_points]
        subscans.append({'pcl': pcl, 'subscan_id': subscan_id, 'relationships': {'relationships': rels, 'scan': subscan_id},
                         'objects': {'scan': subscan_id, 'objects': objs}})
    return subscans
