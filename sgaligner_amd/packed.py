"""The packed-segment contract of the batched geometry ops, host side: segments (objects, clouds, jobs, scans) packed back to back, an
[n + 1] prefix array that is validated here before the C ABI validates its host copy again (csrc/packed.h), tensors that must already live
on the device, and small host arrays that travel in ONE upload.  Used by utils/point_cloud.py, utils/registration.py,
preprocessing/subscans.py and preprocessing/scene_graphs.py."""
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


class PackedLayout:
    """Offsets of S scans packed back to back, on the host and on the device.  The base holds the points: pt_off (int64 numpy), h_pt (its
    int32 host copy, what the C ABI checks), total_points, max_points, n_scans.  A subclass adds its second [S + 1] prefix array with
    _second(), lists in host_parts() the arrays the kernels read, and takes their device views from _device_views()."""

    def __init__(self, pt_off, total_points=None):
        self.pt_off = prefix_offsets(pt_off, 'pt_off', total_points)
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
