"""The packed-segment contract of the batched geometry ops, host side: segments (objects, clouds, jobs, scans) packed back to back, an
[n + 1] prefix array that is validated here before the C ABI validates its host copy again (csrc/packed.h), tensors that must already live
on the device, and small host arrays that travel in ONE upload; on top of it the job list of the nearest-neighbour searches (PairJobs,
csrc/pair_jobs.h), the hypothesis list of the RANSAC entries (HypJobs) and the one chunk rule (split_chunk).  Used by utils/point_cloud, registration, features and preprocessing/subscans, scene_graphs."""
from __future__ import annotations

import numpy as np
import torch


def prefix_offsets(a, name: str, total=None) -> np.ndarray:
    """The host prefix check: `a` (tensor or sequence) -> contiguous int64 [n + 1], starting at 0, never decreasing, ending at `total` when
    one is given, and below 2^31 (the kernels index with int32)."""
    off = np.ascontiguousarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or (np.diff(off) < 0).any() or (total is not None and off[-1] != total):
        raise ValueError(f'{name} must be a monotone prefix array starting at 0' + (f' and covering all {total} entries' if total is not None else ''))
    if off[-1] >= 2 ** 31:
        raise ValueError(f'{name} is indexed with int32: fewer than 2^31 entries per call')
    return off


def check_dtype(t, name: str, dtype):
    if isinstance(t, torch.Tensor) and t.dtype != dtype:
        raise RuntimeError(f'sgaligner_amd: `{name}` must be {dtype} (got {t.dtype})')


def device_tensor(t, name: str, dtype):
    """`t` as a contiguous HIP device tensor of `dtype`, or RuntimeError.  The dtype is reported first, so that a wrong dtype can be told
    apart on a machine without a device."""
    check_dtype(t, name, dtype)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'sgaligner_amd: `{name}` must be a HIP device tensor (got {t.device if isinstance(t, torch.Tensor) else type(t)}); '
                           f'there is no CPU path and no CPU fallback')
    return t.contiguous()


def upload(parts, device):
    """Host arrays -> flat device views of ONE buffer, each typed like its part and starting at a multiple of 8 bytes: one upload."""
    parts = [np.ascontiguousarray(a).reshape(-1) for a in parts]
    starts = np.cumsum([0] + [(a.nbytes + 7) // 8 * 8 for a in parts])
    buf = np.zeros(max(int(starts[-1]), 8), dtype=np.uint8)
    for a, o in zip(parts, starts):
        buf[o:o + a.nbytes] = a.view(np.uint8)
    d_buf = torch.from_numpy(buf).to(device)
    return [d_buf[o:o + a.nbytes].view(torch.from_numpy(a[:0]).dtype) for a, o in zip(parts, starts)]


def check_finite(t, name: str, noun: str):
    """The ops.VALIDATE guard of a float device tensor: RuntimeError when it holds a NaN or an infinity (`noun`: "coordinates", "values")."""
    from . import ops
    if ops.VALIDATE and t.numel() and not bool(torch.isfinite(t).all()):
        raise RuntimeError(f'sgaligner_amd: `{name}` holds NaN or infinite {noun}')


def workspace(nbytes: int, device):
    """An 8-byte-aligned device workspace of at least `nbytes` bytes (never empty: its pointer is always valid)."""
    return torch.empty((max((int(nbytes) + 7) // 8, 1),), device=device, dtype=torch.float64)


def split_chunk(tiles, longest, cus, per_cu, min_chunk, round_to=1, whole_rounds=False) -> int:
    """The one chunk rule of the kernels that split their long axis over workgroups: `tiles` workgroups cover the job list's other axis; the
    longest segment (`longest` rows) is split just far enough that the grid holds about `per_cu` workgroups per CU, never finer than
    `min_chunk` rows and in multiples of `round_to`.  whole_rounds: a grid above one workgroup per CU is trimmed to whole rounds of them."""
    tiles, longest, cus = int(tiles) or 1, int(longest), int(cus)
    n_chunks = max(1, min(-(-per_cu * cus // tiles), -(-longest // min_chunk)))
    if whole_rounds and tiles * n_chunks > cus:
        n_chunks = max(1, (tiles * n_chunks // cus) * cus // tiles)
    return -(-max(min_chunk, -(-longest // n_chunks)) // round_to) * round_to


def resolve_chunk(arg, module_default, rule) -> int:
    """The caller's `chunk`, else the module's constant (tests set it), else rule(); ValueError below 1."""
    chunk = int(arg if arg is not None else module_default if module_default is not None else rule())
    if chunk < 1:
        raise ValueError(f'chunk must be >= 1, got {chunk}')
    return chunk


def pair_ids(pairs, n_sets=None, unit='cloud') -> np.ndarray:
    """`pairs` (tensor or sequence) -> contiguous int64 [n_pairs, 2]; with n_sets, ValueError unless every id names one of the `unit`s."""
    pr = np.ascontiguousarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
    if n_sets is not None and pr.size and (pr.min() < 0 or pr.max() >= n_sets):
        raise ValueError(f'pairs must name {unit}s in [0, {n_sets})')
    return pr


class PairJobs:
    """(query set, support set) jobs over sets packed back to back, what csrc/pair_jobs.h checks again behind the C ABI: off (int64
    [n_sets + 1] over `total` rows), pr (int64 [n_pairs, 2]), per job nq / ns, out_off (int64 [n_pairs + 1]: job p's results start at
    out_off[p]), total_q (below 2^31), the int32 host copies h_off / h_pr / h_oo and max_q / max_s.  `what` / `unit` word the refusals."""

    def __init__(self, offsets, total, pairs, what: str, unit: str):
        self.off = prefix_offsets(offsets, 'offsets', total)
        self.n_sets = len(self.off) - 1
        self.pr = pair_ids(pairs, self.n_sets, unit)
        self.nq, self.ns = (np.diff(self.off)[self.pr[:, k]] for k in (0, 1))
        self.out_off = np.concatenate([[0], np.cumsum(self.nq)]).astype(np.int64)
        self.n_pairs, self.total_q = len(self.pr), int(self.out_off[-1])
        if self.total_q >= 2 ** 31:
            raise ValueError(f'{what} indexes with int32: fewer than 2^31 queries per call')
        self.h_off, self.h_pr, self.h_oo = self.off.astype(np.int32), self.pr.astype(np.int32), self.out_off[:-1].astype(np.int32)
        self.max_q, self.max_s = (int(self.nq.max()), int(self.ns.max())) if self.n_pairs else (0, 0)

    def host_parts(self):                                   # what the kernels read, for the caller's ONE upload (it may append its own)
        return [self.h_off, self.h_pr, self.h_oo]


class HypJobs:
    """A packed hypothesis list as the RANSAC entries take it (csrc/ransac.hip, csrc/ransac_geo.hip), checked in the order dtype, device,
    shape: corr [N, 6] float64 and samples [H, 3] int32 HIP tensors (job-local row indices), offsets / hyp_offsets the two [n_jobs + 1]
    prefix arrays over them.  Holds corr, samples, off / hoff (int64), their int32 host copies h_off / h_hoff, n_jobs, total / total_h,
    the per-job sizes_n / sizes_h and max_n / max_h.  corr_shape=False leaves corr's shape to the caller; convert_samples=True takes
    samples from numpy or any integer tensor and converts it instead of refusing."""

    def __init__(self, corr, offsets, samples, hyp_offsets, corr_shape=True, convert_samples=False):
        self.corr = device_tensor(corr, 'corr', torch.float64)
        if corr_shape and (self.corr.dim() != 2 or self.corr.shape[1] != 6):
            raise ValueError(f'corr must be [N,6], got {tuple(self.corr.shape)}')
        if convert_samples:
            sm = samples if isinstance(samples, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int32))
            sm = sm.to(device=self.corr.device, dtype=torch.int32).contiguous()
        else:
            sm = device_tensor(samples, 'samples', torch.int32)
        self.samples = sm.reshape(-1, 3)
        self.total, self.total_h = int(self.corr.shape[0]), int(self.samples.shape[0])
        self.off = prefix_offsets(offsets, 'offsets', self.total)
        self.hoff = prefix_offsets(hyp_offsets, 'hyp_offsets', self.total_h)
        self.n_jobs = len(self.off) - 1
        if len(self.hoff) != self.n_jobs + 1:
            raise ValueError(f'offsets names {self.n_jobs} jobs, hyp_offsets {len(self.hoff) - 1}')
        self.h_off, self.h_hoff = self.off.astype(np.int32), self.hoff.astype(np.int32)
        self.sizes_n, self.sizes_h = np.diff(self.off), np.diff(self.hoff)
        self.max_n, self.max_h = (int(self.sizes_n.max()), int(self.sizes_h.max())) if self.n_jobs else (0, 0)

    def check_int32(self, what: str, per_hyp: int):
        """ValueError unless corr's 6 columns and `per_hyp` values per hypothesis can be indexed with int32."""
        if self.total >= 2 ** 31 // 6 or self.total_h >= 2 ** 31 // per_hyp:
            raise ValueError(f'{what} indexes with int32: fewer than 2^31 / 6 rows and 2^31 / {per_hyp} hypotheses per call')


class PackedLayout:
    """Offsets of S scans packed back to back, on the host and on the device.  The base holds the points: pt_off (int64 numpy), h_pt (its
    int32 host copy, what the C ABI checks), total_points, max_points, n_scans.  A subclass adds its second [S + 1] prefix array with
    _second(), lists in host_parts() the arrays the kernels read, and takes their device views from _device_views().  `name` is what the
    refusals call the array."""

    def __init__(self, pt_off, total_points=None, name='pt_off'):
        self.pt_off = prefix_offsets(pt_off, name, total_points)
        self.h_pt = self.pt_off.astype(np.int32)
        self.n_scans = len(self.pt_off) - 1
        self.total_points, self.max_points = int(self.pt_off[-1]), self._max_len(self.pt_off)

    @staticmethod
    def _max_len(off) -> int:
        return int(np.diff(off).max()) if len(off) > 1 else 0

    def _second(self, a, name: str, total=None):
        """A second prefix array over the same scans -> (int64 offsets, int32 host copy, total, longest segment)."""
        off = prefix_offsets(a, name, total)
        if len(off) != self.n_scans + 1:
            raise ValueError(f'pt_off names {self.n_scans} scans, {name} {len(off) - 1}')
        return off, off.astype(np.int32), int(off[-1]), self._max_len(off)

    def host_meta(self) -> np.ndarray:
        """host_parts() as one int32 array (an int64 part as int32 pairs; such parts come first, for their alignment)."""
        return np.concatenate([a.view(np.int32) for a in self.host_parts()])

    def _device_views(self, device, meta):
        """int32 device views of host_parts(), in that order, or None without a device.  `meta`, when given, is an int32 device tensor that
        already holds host_meta() (a caller can fold the offsets into a larger upload); with `device` alone the layout uploads it."""
        if meta is None and device is not None:
            meta = torch.from_numpy(self.host_meta()).to(device)                      # one small upload
        if meta is None:
            return None
        return meta.split([a.nbytes // 4 for a in self.host_parts()])
