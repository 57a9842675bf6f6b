"""Scene-graph records on the device: the reference's preprocessing/scan3r/preprocess.py process_scan (:40-211) and its two bag-of-words
passes (:280-361) for a whole list of (sub)scans.

process_scan splits every object from the scan with its own np.where, takes its convex-hull barycentre and its farthest-point samples,
filters the listed relationships, supplements every unlisted ordered pair with a `none` edge by a linear search of a growing list, and the
bag-of-words passes count relation names per subject (with the edge index applied to the TRIPLES list, which is longer than the edge list
whenever a pair is listed with two relations -- reproduced here) and attribute words per object.  Here the split is sga_object_counts +
sga_object_partition, hulls and samples run on the packed device points (csrc/hull.hip, csrc/fps.hip), and the supplement with the relation
bag-of-words is sga_graph_complete -- one launch each over all scans of the call (csrc/scenegraph.hip).

Traffic of process_scans: one packed upload of points + slots + offsets; a small download of the per-slot point counts, which decide on the
host which objects are kept (objects_json order, count >= min_obj_points) and every random draw; a small upload of the destination
offsets; the hull candidates' indices, then the candidates themselves with their vertex flags come back (a few per cent of the points);
small uploads of the FPS offsets / start indices and of the drawn indices of objects below the resolution; the samples come back once per
resolution; one small upload of the graph-local pairs and relation ids, one download of edges + counts.  The points are uploaded once.
JSON strings (names, attributes, ids typed as strings) stay on the host.  There is no CPU path and no file I/O except write_records.

Random draws: the reference consumes np.random per kept object, in object order, once per resolution -- np.random.choice(N, res) if
N < res, else np.random.randint(0, N), N being the previous resolution from the second resolution on (obj_pcl is overwritten inside the
loop, :98-100: later resolutions sample the earlier sample).  All draws depend only on the downloaded counts; they are made here from
np.random in exactly that order, scans in list order, so the same seed gives the reference's own samples -- for a batch the sequence of
the scans processed one after the other.

Not here: the four augmentation switches of the reference's command line (--remove_nodes, --remove_edges, --change_node_semantic,
--change_edge_semantic).  They are edits of the objects / relationships lists; a caller applies them to the json before the call."""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from ..packed import PackedLayout, check_dtype, device_tensor, upload
from ..utils import point_cloud as PC


def graph_max_nodes() -> int:
    """Largest number of objects sga_graph_complete serves: the adjacency bit matrix and one counter per row fit the LDS of a workgroup."""
    return int(_lib.lib().sga_graph_max_nodes())


def partition_tile() -> int:
    """Points per tile of sga_object_partition."""
    return int(_lib.lib().sga_scenegraph_tile())


def partition_max_slots() -> int:
    """Largest number of slots of one scan sga_object_partition serves (its per-tile tables live in LDS)."""
    return int(_lib.lib().sga_scenegraph_lds_slots())


class SlotLayout(PackedLayout):
    """Point and slot offsets of a list of scans: pt_off / slot_off [S + 1] (h_pt / h_slot int32 on the host, d_pt / d_slot on the device)."""

    def __init__(self, pt_off, slot_off, device=None, meta=None):
        super().__init__(pt_off)
        self.slot_off, self.h_slot, self.total_slots, self.max_slots = self._second(slot_off, 'slot_off')
        views = self._device_views(device, meta)
        if views:
            self.d_pt, self.d_slot = views

    def host_parts(self):
        return [self.h_pt, self.h_slot]

    def host_args(self):
        return self.h_pt.ctypes.data, self.h_slot.ctypes.data


def object_counts_batch(slot, layout: SlotLayout):
    """sga_object_counts: slot [sum N] int32 device tensor (each point's dense object slot within its scan; a value outside the scan's slot
    range, e.g. -1, belongs to no object).  Returns counts [sum slots] int32 device tensor.  Exact: integer atomics."""
    sl = device_tensor(slot, 'slot', torch.int32)
    if tuple(sl.shape) != (layout.total_points,):
        raise ValueError(f'slot must be [{layout.total_points}], got {tuple(sl.shape)}')
    counts = torch.empty((layout.total_slots,), device=sl.device, dtype=torch.int32)
    if layout.n_scans and layout.total_slots:
        rc = _lib.lib().sga_object_counts(_p(sl), _p(layout.d_pt), _p(layout.d_slot), layout.n_scans, layout.total_points, layout.total_slots,
                                          layout.max_points, *layout.host_args(), _p(counts), _stream())
        _lib.check(rc, 'sga_object_counts')
    return counts


def object_partition_batch(points, slot, layout: SlotLayout, dest_off, counts):
    """sga_object_partition, the stable split: points [sum N, 3] float32 and slot [sum N] int32 device tensors; dest_off [sum slots] host ints
    (the start of the slot's points in the packed output, -1 = dropped); counts [sum slots] host ints (object_counts_batch, downloaded).
    Returns (perm [n_kept] int32, pts_out [n_kept, 3] float32) device tensors, n_kept = the kept slots' points:
    perm[dest_off[k] : dest_off[k] + counts[k]] == np.flatnonzero(slot_s == k), scan-local, ascending.  A pure function of the input."""
    for t, name, dt in ((points, 'points', torch.float32), (slot, 'slot', torch.int32)):
        check_dtype(t, name, dt)
    h_dest = np.ascontiguousarray(dest_off, dtype=np.int64).reshape(-1)
    h_cnt = np.ascontiguousarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.int64).reshape(-1)
    if len(h_dest) != layout.total_slots or len(h_cnt) != layout.total_slots:
        raise ValueError(f'dest_off and counts must be [{layout.total_slots}], got {len(h_dest)} and {len(h_cnt)}')
    if layout.max_slots > partition_max_slots():
        raise ValueError(f'a scan has {layout.max_slots} slots; sga_object_partition serves at most {partition_max_slots()}')
    kept = h_dest >= 0
    n_kept = int(h_cnt[kept].sum())
    if (h_cnt < 0).any() or h_cnt.sum() > layout.total_points:
        raise ValueError('counts must be non-negative and sum to at most the number of points')
    full = kept & (h_cnt > 0)                                # an empty object has no range to collide with
    if full.any():
        order = np.argsort(h_dest[full], kind='stable')
        lo, hi = h_dest[full][order], (h_dest[full] + h_cnt[full])[order]
        if hi.max() > n_kept or (lo[1:] < hi[:-1]).any():
            raise ValueError('dest_off must give the kept objects disjoint ranges that tile [0, kept points)')
    pts = device_tensor(points, 'points', torch.float32)
    sl = device_tensor(slot, 'slot', torch.int32)
    if tuple(pts.shape) != (layout.total_points, 3) or tuple(sl.shape) != (layout.total_points,):
        raise ValueError(f'points / slot must be [{layout.total_points}, 3] / [{layout.total_points}], got {tuple(pts.shape)} / {tuple(sl.shape)}')
    perm = torch.empty((n_kept,), device=pts.device, dtype=torch.int32)
    out = torch.empty((n_kept, 3), device=pts.device, dtype=torch.float32)
    if n_kept:
        L = _lib.lib()
        h_dest32, h_cnt32 = h_dest.astype(np.int32), h_cnt.astype(np.int32)
        d_dest = torch.from_numpy(h_dest32).to(pts.device)
        ws_bytes = int(L.sga_object_partition_ws_bytes(layout.n_scans, layout.max_points, layout.max_slots))
        ws = torch.empty((max((ws_bytes + 3) // 4, 1),), device=pts.device, dtype=torch.int32)
        rc = L.sga_object_partition(_p(pts), _p(sl), _p(layout.d_pt), _p(layout.d_slot), _p(d_dest), layout.n_scans, layout.total_points,
                                    layout.total_slots, layout.max_points, layout.max_slots, n_kept, *layout.host_args(), h_dest32.ctypes.data,
                                    h_cnt32.ctypes.data, _p(perm), _p(out), _p(ws), ws_bytes, _stream())
        _lib.check(rc, 'sga_object_partition')
    return perm, out


def graph_complete_batch(n_nodes, pairs, rels, none_id: int, vocab: int, device='cuda'):
    """sga_graph_complete for a list of graphs in one launch.  n_nodes: objects per graph; pairs: per graph the listed pairs [P, 2]
    (graph-local ints, list order); rels: per graph the relation ids of the listed triples [Tr >= P]; none_id: the id of `none`; vocab: V.
    Returns per graph (edges [n_edges, 2] int64, bow [N, V] int32) numpy arrays: the listed pairs, then every unlisted ordered pair (i, j),
    i != j, row-major; bow[edges[idx][0], rel(idx)] += 1 with rel(idx) the idx-th entry of the triples list (listed, then `none`).
    One upload, one launch, one download.  Raises before launching when a graph has more than graph_max_nodes() objects."""
    n_nodes = np.asarray(n_nodes, dtype=np.int64).reshape(-1)
    G = len(n_nodes)
    if len(pairs) != G or len(rels) != G:
        raise ValueError(f'{G} graphs need {G} pair lists and relation lists, got {len(pairs)} and {len(rels)}')
    if G and n_nodes.max() > graph_max_nodes():
        raise ValueError(f'a graph has {int(n_nodes.max())} objects; sga_graph_complete serves at most {graph_max_nodes()} '
                         f'(its adjacency bit matrix lives in LDS)')
    if G and n_nodes.min() < 0:
        raise ValueError('n_nodes must be non-negative')
    vocab, none_id = int(vocab), int(none_id)
    if not 0 <= none_id < vocab:
        raise ValueError(f'the id of `none` ({none_id}) must be inside the vocabulary of {vocab}')
    h_pairs = [np.ascontiguousarray(p, dtype=np.int64).reshape(-1, 2) for p in pairs]
    h_rels = [np.ascontiguousarray(r, dtype=np.int64).reshape(-1) for r in rels]
    for g in range(G):
        if len(h_rels[g]) < len(h_pairs[g]):
            raise ValueError(f'graph {g} lists {len(h_rels[g])} triples for {len(h_pairs[g])} pairs (every pair comes from a triple)')
        if h_pairs[g].size and (h_pairs[g].min() < 0 or h_pairs[g].max() >= n_nodes[g]):
            raise ValueError(f'graph {g}: pairs must name objects in [0, {int(n_nodes[g])})')
        if h_rels[g].size and (h_rels[g].min() < 0 or h_rels[g].max() >= vocab):
            raise ValueError(f'graph {g}: relation ids must be in [0, {vocab})')
    PC._need_device('graph_complete_batch')
    if G == 0:
        return []
    n_p = np.array([len(p) for p in h_pairs], dtype=np.int64)
    prefix = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int64)
    node_off, pair_off, trip_off = prefix(n_nodes), prefix(n_p), prefix([len(r) for r in h_rels])
    edge_off = prefix(n_p + n_nodes * (n_nodes - 1))
    if max(edge_off[-1], node_off[-1] * vocab, trip_off[-1]) >= 2 ** 31:
        raise ValueError('sga_graph_complete indexes with int32: split the graph list')
    h_off = np.concatenate([node_off, pair_off, trip_off, edge_off]).astype(np.int32)
    h_pr = (np.concatenate(h_pairs) if G else np.zeros((0, 2))).astype(np.int32).reshape(-1)
    h_rl = np.concatenate(h_rels).astype(np.int32)
    d_off, d_pr, d_rl = upload([h_off, h_pr, h_rl], device)                            # the one upload
    n = G + 1
    te, tn = int(edge_off[-1]), int(node_off[-1])
    # one output buffer, one download: edges (int64) | bow | n_edges (int32)
    out = torch.empty((te * 2 + (tn * vocab + G + 1) // 2 + 1,), device=d_off.device, dtype=torch.int64)
    d_edges = out[:te * 2]
    tail = out[te * 2:].view(torch.int32)
    d_bow, d_ne = tail[:tn * vocab], tail[tn * vocab:tn * vocab + G]
    ho = [h_off[i * n:(i + 1) * n] for i in range(4)]
    rc = _lib.lib().sga_graph_complete(_p(d_off[:n]), _p(d_off[n:2 * n]), _p(d_off[2 * n:3 * n]), _p(d_off[3 * n:4 * n]), G, _p(d_pr), _p(d_rl), none_id,
                                       vocab, ho[0].ctypes.data, ho[1].ctypes.data, ho[2].ctypes.data, ho[3].ctypes.data, h_pr.ctypes.data,
                                       h_rl.ctypes.data, _p(d_edges), _p(d_ne), _p(d_bow), _stream())
    _lib.check(rc, 'sga_graph_complete')
    host = out.cpu().numpy()
    h_edges = host[:te * 2].reshape(-1, 2)
    h_tail = host[te * 2:].view(np.int32)
    h_bow, h_ne = h_tail[:tn * vocab].reshape(tn, vocab), h_tail[tn * vocab:tn * vocab + G]
    return [(h_edges[edge_off[g]:edge_off[g] + int(h_ne[g])].copy(), h_bow[node_off[g]:node_off[g + 1]].copy()) for g in range(G)]


def bow_counts(rows, cols, n_rows: int, vocab: int, device='cuda') -> np.ndarray:
    """sga_bow_counts: out [n_rows, vocab] int32 with out[rows[i], cols[i]] += 1 (host int arrays in, numpy out; integer atomics, exact).
    An entry outside the matrix is refused before anything is launched."""
    h_r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    h_c = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
    n_rows, vocab = int(n_rows), int(vocab)
    if len(h_r) != len(h_c):
        raise ValueError(f'rows and cols must have one length, got {len(h_r)} and {len(h_c)}')
    if n_rows < 0 or vocab < 0 or n_rows * vocab >= 2 ** 31 or len(h_r) >= 2 ** 31:
        raise ValueError(f'n_rows x vocab must be in [0, 2^31) (got {n_rows} x {vocab})')
    if len(h_r) and (h_r.min() < 0 or h_r.max() >= n_rows):
        raise ValueError(f'rows must be in [0, {n_rows})')
    if len(h_c) and (h_c.min() < 0 or h_c.max() >= vocab):
        raise ValueError(f'cols must be in [0, {vocab})')
    PC._need_device('bow_counts')
    out = torch.empty((n_rows, vocab), device=device, dtype=torch.int32)
    if n_rows and vocab:
        h_rc = np.concatenate([h_r, h_c]).astype(np.int32)
        d_rc = torch.from_numpy(h_rc).to(out.device) if len(h_rc) else torch.zeros((2,), device=out.device, dtype=torch.int32)
        n = len(h_r)
        rc = _lib.lib().sga_bow_counts(_p(d_rc[:n]) if n else None, _p(d_rc[n:]) if n else None, n, n_rows, vocab, h_rc[:n].ctypes.data if n else None,
                                       h_rc[n:].ctypes.data if n else None, _p(out), _stream())
        _lib.check(rc, 'sga_bow_counts')
    return out.cpu().numpy()


# ---- the record ------------------------------------------------------------------------------------------------------------------------
RECORD_KEYS = ('scan_id', 'objects_id', 'global_objects_id', 'objects_cat', 'triples', 'pairs', 'edges', 'obj_points', 'objects_count',
               'edges_count', 'object_id2idx', 'object_attributes', 'edges_cat', 'rel_trans', 'root_obj_id')          # preprocess.py:195-211


def relation_columns(rel2idx):
    """The column of every relation id in the edge bag-of-words (preprocess.py:285-290: word = position of the NAME among rel2idx's keys, the
    name looked up from the id).  -> {relation id: column}."""
    idx_2_rel = {idx: name for name, idx in rel2idx.items()}
    word = {name: k for k, name in enumerate(rel2idx.keys())}
    return {int(idx): word[name] for idx, name in idx_2_rel.items()}


def filter_relationships(relationships, objects_ids, rel2idx):
    """The host side of the triples loop (preprocess.py:133-159) on raw json triples [sub, obj, rel id, rel name]: keep the triples whose two
    ends are kept objects; a pair joins `pairs` unless the RAW first two entries already equal a listed pair (Python list equality: ints
    de-duplicate, ids typed as strings never equal the stored ints and never do).  Returns (triples, pairs, edges_cat)."""
    kept = set(objects_ids)
    triples, pairs, edges_cat, seen = [], [], [], set()
    for triple in relationships:
        sub, obj = int(triple[0]), int(triple[1])
        rel_name = triple[3]
        if rel_name not in rel2idx:
            raise ValueError(f'relationship name {rel_name!r} is not in rel2idx')
        rel_id = int(rel2idx[rel_name])
        if sub in kept and obj in kept:
            if rel_name == 'inside':
                raise ValueError("the reference refuses the relation 'inside' between kept objects (preprocess.py:151-152)")
            triples.append([sub, obj, rel_id])
            edges_cat.append(rel2idx[rel_name])
            raw = triple[:2]
            # `raw not in pairs` with pairs holding int pairs: a set gives the same answer exactly when both raw entries are plain ints
            # (or compare equal to them: bool, integral float); anything else falls back to the list search itself
            if type(raw) is list and all(type(v) is int for v in raw):
                new = (sub, obj) not in seen
            else:
                new = raw not in pairs
            if new:
                pairs.append([sub, obj])
                seen.add((sub, obj))
    return triples, pairs, edges_cat


def _scan_arrays(i, vertices):
    try:
        x, y, z = (np.asarray(vertices[k]) for k in 'xyz')
        object_id = np.asarray(vertices['objectId']).reshape(-1)
    except (KeyError, ValueError, IndexError, TypeError) as e:
        raise ValueError(f'scans[{i}]: vertices must be a structured array or mapping with x, y, z, objectId') from e
    pts = np.stack([x, y, z]).transpose((1, 0))
    if pts.ndim != 2 or pts.shape[0] != len(object_id):
        raise ValueError(f'scans[{i}]: x, y, z, objectId must be flat arrays of one length')
    return np.ascontiguousarray(pts, dtype=np.float32), object_id


def process_scans(scans, rel2idx, pc_resolutions=(512,), min_obj_points=50, return_info=False):
    """scans: a list of (scan_id, vertices, objects_json, relationships_json) -- vertices the structured data.npy array or any mapping with
    x, y, z, objectId (float32 coordinates, as the ply stores them); objects_json / relationships_json the scan's 'objects' /
    'relationships' lists of objects.json / relationships.json.  rel2idx: relation name -> id (the reference's relationships.txt);
    pc_resolutions: cfg.preprocess.pc_resolutions; min_obj_points: cfg.preprocess.min_obj_points.

    Returns one entry per scan: the record dict of preprocess.py:195-211 (RECORD_KEYS) plus 'bow_vec_object_edge_feats' (float64 [N, V], what
    calculate_bow_node_edge_feats adds), or -1 in the reference's three cases: no relationships, fewer than 2 kept objects, no pair between
    kept objects.  With return_info also {'hull_device', 'hull_qhull', 'fps', 'random'}: how many objects went through the device hull,
    Qhull, the FPS kernel and the N < resolution draw (first resolution).

    Uploads, downloads and the order of the np.random draws: see the module docstring."""
    pc_resolutions = [int(r) for r in pc_resolutions]
    if not pc_resolutions or min(pc_resolutions) < 1:
        raise ValueError('pc_resolutions must name at least one positive resolution')
    if 'none' not in rel2idx:
        raise ValueError("rel2idx must hold the relation 'none'")
    rel_col = relation_columns(rel2idx)
    vocab = len(rel2idx)
    results = [-1] * len(scans)
    live = []                                                # (position in `scans`, scan id, points, slots, ids, objects, relationships)
    for i, (scan_id, vertices, objects_json, relationships_json) in enumerate(scans):
        if len(relationships_json) == 0:                     # :43-44, before anything is drawn
            continue
        pts, object_id = _scan_arrays(i, vertices)
        ids, slot = np.unique(object_id, return_inverse=True)
        live.append((i, scan_id, pts, slot.reshape(-1).astype(np.int32), ids, objects_json, relationships_json))
    info = {'hull_device': 0, 'hull_qhull': 0, 'fps': 0, 'random': 0}
    PC._need_device('process_scans')
    if not live:
        return (results, info) if return_info else results

    # 1. one packed upload
    L = SlotLayout(np.concatenate([[0], np.cumsum([len(s[2]) for s in live])]), np.concatenate([[0], np.cumsum([len(s[4]) for s in live])]))
    d_meta, d_slot, d_pts = upload([L.host_meta(), np.concatenate([s[3] for s in live]), np.concatenate([s[2] for s in live])], 'cuda')
    L = SlotLayout(L.pt_off, L.slot_off, meta=d_meta)
    d_pts = d_pts.view(-1, 3)
    # 2. counts
    counts = object_counts_batch(d_slot, L).cpu().numpy().astype(np.int64)

    # 3. the host walks objects_json in its own order (:74-106)
    per_scan = []                                            # kept objects per live scan: dicts of lists
    kept_slot, kept_n = [], []                               # global slot and point count of every kept object, in draw order
    for li, (_, scan_id, _, _, ids, objects_json, _) in enumerate(live):
        k0 = int(L.slot_off[li])
        slot_of = {int(v): k for k, v in enumerate(ids)}
        rec = {'objects_id': [], 'global_objects_id': [], 'attributes': [], 'first': len(kept_slot)}
        for obj in objects_json:
            object_id = int(obj['id'])
            k = slot_of.get(object_id)
            n = int(counts[k0 + k]) if k is not None else 0
            if n < min_obj_points:
                continue
            if k is None:
                raise ValueError(f'scan {scan_id!r}: object {object_id} has no points (min_obj_points must be at least 1)')
            if object_id in rec['objects_id']:
                raise ValueError(f'scan {scan_id!r}: objects_json lists object {object_id} twice')
            rec['objects_id'].append(object_id)
            rec['global_objects_id'].append(int(obj['global_id']))
            rec['attributes'].append([item for sublist in obj['attributes'].values() for item in sublist])
            kept_slot.append(k0 + k)
            kept_n.append(n)
        per_scan.append(rec)
    n_obj = len(kept_slot)
    kept_n = np.asarray(kept_n, dtype=np.int64)

    # the draws, in the reference's order: object by object, resolution by resolution
    res0 = pc_resolutions[0]
    starts = [np.zeros(n_obj, dtype=np.int64) for _ in pc_resolutions]                 # FPS start per object and level (where FPS applies)
    drawn = [dict() for _ in pc_resolutions]                                           # object -> drawn indices (the N < res branch)
    for o in range(n_obj):
        n = int(kept_n[o])
        for lv, res in enumerate(pc_resolutions):
            if n < res:
                drawn[lv][o] = np.random.choice(n, res)
            else:
                starts[lv][o] = np.random.randint(0, n)
            n = res

    obj_points = [np.zeros((0, r, 3), dtype=np.float32) for r in pc_resolutions]
    bary = np.zeros((0, 3))
    if n_obj:
        # 4. the stable split; objects the first FPS launch serves are packed first, so that it sees one contiguous prefix
        is_fps = kept_n >= res0
        order = np.concatenate([np.flatnonzero(is_fps), np.flatnonzero(~is_fps)])      # packed position -> object
        pos_of = np.empty(n_obj, dtype=np.int64)
        pos_of[order] = np.arange(n_obj)
        p_off = np.concatenate([[0], np.cumsum(kept_n[order])]).astype(np.int64)       # packed offsets, packing order
        dest = np.full(L.total_slots, -1, dtype=np.int64)
        dest[np.asarray(kept_slot)[order]] = p_off[:-1]
        _, d_obj = object_partition_batch(d_pts, d_slot, L, dest, counts)
        # 5. hulls and samples on the packed device points
        bc, hinfo = PC.convex_hull_barycenters_device(d_obj, p_off, return_info=True)
        bary = bc[pos_of]
        info['hull_device'], info['hull_qhull'] = hinfo['device'], hinfo['qhull']
        n_fps = int(is_fps.sum())
        info['fps'], info['random'] = n_fps, n_obj - n_fps
        cur, cur_off = d_obj, p_off                                                    # the level's input, packing order
        for lv, res in enumerate(pc_resolutions):
            idx = torch.empty((n_obj, res), device=d_obj.device, dtype=torch.int64)    # object-local sample indices, packing order
            if lv == 0:
                fps_pos = np.arange(n_fps)
            else:
                fps_pos = np.arange(n_obj) if pc_resolutions[lv - 1] >= res else np.zeros(0, dtype=np.int64)
            if len(fps_pos):
                k = len(fps_pos)                                                       # a prefix of the packing order on every level
                out = PC.farthest_point_sample_batch(cur[:int(cur_off[k])], cur_off[:k + 1], res, starts[lv][order[:k]])
                idx[:k] = out.long()
            if len(fps_pos) < n_obj:
                rest = order[len(fps_pos):]
                idx[len(fps_pos):] = torch.from_numpy(np.stack([drawn[lv][int(o)] for o in rest]).astype(np.int64)).to(d_obj.device)
            base = torch.from_numpy(cur_off[:-1].astype(np.int64)).to(d_obj.device)
            cur = cur[(base[:, None] + idx).reshape(-1)]                               # [n_obj * res, 3]: the next level samples this sample
            cur_off = np.arange(n_obj + 1, dtype=np.int64) * res
            obj_points[lv] = cur.view(n_obj, res, 3).cpu().numpy()[pos_of]

    # the triples loop, the root object and the graph inputs
    graphs = []                                              # (live scan, triples, pairs, edges_cat, listed pair count)
    for li, (i, scan_id, _, _, _, _, relationships_json) in enumerate(live):
        rec = per_scan[li]
        if len(rec['objects_id']) < 2:                       # :111-112
            continue
        triples, pairs, edges_cat = filter_relationships(relationships_json, rec['objects_id'], rel2idx)
        if len(pairs) == 0:                                  # :161-162
            continue
        graphs.append((li, triples, pairs, edges_cat))
    if graphs:
        g_nodes, g_pairs, g_rels = [], [], []
        for li, triples, pairs, _ in graphs:
            id2idx = {v: k for k, v in enumerate(per_scan[li]['objects_id'])}
            g_nodes.append(len(id2idx))
            g_pairs.append(np.array([[id2idx[s], id2idx[o]] for s, o in pairs], dtype=np.int64))
            g_rels.append(np.array([rel_col[t[2]] for t in triples], dtype=np.int64))
        if max(g_nodes) > graph_max_nodes():
            raise ValueError(f'a scan keeps {max(g_nodes)} objects; the edge completion serves at most {graph_max_nodes()} per scan')
        none_id = rel2idx['none']
        completed = graph_complete_batch(g_nodes, g_pairs, g_rels, rel_col[int(none_id)], vocab)
        for (li, triples, pairs, edges_cat), (edges, bow) in zip(graphs, completed):
            i, scan_id = live[li][0], live[li][1]
            rec = per_scan[li]
            objects_ids = rec['objects_id']
            first, n = rec['first'], len(objects_ids)
            object_id2idx = {v: k for k, v in enumerate(objects_ids)}
            # root object: highest degree among the LISTED pairs (:165-167); rel_trans in fp64 (:170-174)
            root_obj_id = np.argmax(np.bincount(np.array(pairs).flatten()))
            bc = bary[first:first + n]
            rel_trans = np.array([np.subtract(bc[object_id2idx[root_obj_id]], b) for b in bc])
            ids_arr = np.asarray(objects_ids, dtype=np.int64)
            extra = ids_arr[edges[len(pairs):]].tolist()                               # the supplemented pairs, as object ids
            triples = triples + [[a, b, none_id] for a, b in extra]
            all_pairs = pairs + extra
            edges_cat = edges_cat + [none_id] * len(extra)
            results[i] = {
                'scan_id': scan_id,
                'objects_id': np.array(objects_ids),
                'global_objects_id': np.array(rec['global_objects_id']),
                'objects_cat': np.array(rec['global_objects_id']),
                'triples': triples,
                'pairs': all_pairs,
                'edges': edges,
                'obj_points': {res: obj_points[lv][first:first + n].copy() for lv, res in enumerate(pc_resolutions)},
                'objects_count': n,
                'edges_count': len(edges),
                'object_id2idx': object_id2idx,
                'object_attributes': rec['attributes'],
                'edges_cat': edges_cat,
                'rel_trans': rel_trans,
                'root_obj_id': root_obj_id,
                'bow_vec_object_edge_feats': bow.astype(np.float64),
            }
    return (results, info) if return_info else results


def process_scan(scan_id, vertices, objects_json, relationships_json, rel2idx, pc_resolutions=(512,), min_obj_points=50):
    """The single-scan form of process_scans: the record dict, or -1."""
    return process_scans([(scan_id, vertices, objects_json, relationships_json)], rel2idx, pc_resolutions, min_obj_points)[0]


def bow_attr_feats(records, word_2_ix):
    """calculate_bow_node_attr_feats (preprocess.py:328-361) for a list of records (-1 entries are skipped): the vocabulary grows on the host
    exactly as :333-342 -- records in the order of their sorted scan ids, new words appended in encounter order -- then one sga_bow_counts
    launch counts every object's words.  Returns (feats, vocabulary): feats[k] the float64 [N, V] matrix of records[k] (None for a -1
    entry), also stored in the record as 'bow_vec_object_attr_feats'; vocabulary the extended copy of word_2_ix."""
    vocabulary = dict(word_2_ix)
    live = sorted((k for k, r in enumerate(records) if not isinstance(r, int)), key=lambda k: records[k]['scan_id'])
    for k in live:
        for object_attr in records[k]['object_attributes']:
            for attr in object_attr:
                if attr not in vocabulary:
                    vocabulary[attr] = len(vocabulary)
    rows, cols, row0, n_rows = [], [], {}, 0
    for k in live:
        row0[k] = n_rows
        for j, object_attr in enumerate(records[k]['object_attributes']):
            rows.extend([n_rows + j] * len(object_attr))
            cols.extend(vocabulary[a] for a in object_attr)
        n_rows += len(records[k]['object_attributes'])
    out = bow_counts(rows, cols, n_rows, len(vocabulary)).astype(np.float64)
    feats = [None] * len(records)
    for k in live:
        feats[k] = out[row0[k]:row0[k] + len(records[k]['object_attributes'])].copy()
        records[k]['bow_vec_object_attr_feats'] = feats[k]
    return feats, vocabulary


def write_records(records, out_dir, mode='orig'):
    """Write every record (-1 entries are skipped) to <out_dir>/files/<mode>/data/<scan_id>.pkl, the layout datasets/scan3r.py reads (and
    process_data writes, preprocess.py:249).  Returns the scan ids written, in list order."""
    data_dir = os.path.join(out_dir, 'files', mode, 'data')
    os.makedirs(data_dir, exist_ok=True)
    written = []
    for rec in records:
        if isinstance(rec, int):
            continue
        with open(os.path.join(data_dir, rec['scan_id'] + '.pkl'), 'wb') as fh:
            pickle.dump(rec, fh, protocol=pickle.HIGHEST_PROTOCOL)
        written.append(rec['scan_id'])
    return written
