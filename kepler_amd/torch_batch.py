"""Device-resident batches via PyTorch (plumbing only: device memory + streams).

The engine's C ABI takes raw device pointers; torch tensors provide the HBM
allocations and the stream the kernel is launched on.  Unsigned arrays are
moved as same-width signed views (only the bytes matter).
"""

from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .accel import KaccInterval, KaccTopRows, make_interval

_VIEW = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def to_device(arrays: Dict[str, np.ndarray], device: str = "cuda") -> Dict[str, torch.Tensor]:
    out = {}
    for name, a in arrays.items():
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        v = a.view(_VIEW.get(a.dtype, a.dtype))
        out[name] = torch.from_numpy(v).to(device, non_blocking=False)
    return out


def interval_from_tensors(tensors: Dict[str, torch.Tensor], sizes: dict, flags: int = 0) -> KaccInterval:
    return make_interval(tensors, sizes, flags, ptr=lambda t: t.data_ptr())


_KIND_PREFIX = ("proc", "ctr", "vm", "pod")  # kacc_kind order


def top_rows_from_tensors(tensors: Dict[str, torch.Tensor], kind: int, listed: bool = True) -> KaccTopRows:
    """kacc_top_rows of one workload kind (KACC_KIND_*) out of an interval's device tensors: its
    offsets, slot words and, unless ``listed`` is False, the batch's node_status (read-error nodes
    list nothing).  The caller keeps the tensors alive while the descriptor is in use."""
    p = _KIND_PREFIX[kind]
    off, slot = tensors[f"{p}_off"], tensors[f"{p}_slot"]
    status = tensors.get("node_status") if listed else None
    r = KaccTopRows()
    r.n_nodes = off.numel() - 1
    r.n_rows = slot.numel()
    r.row_off = off.data_ptr()
    r.slot = slot.data_ptr() or None
    r.node_status = status.data_ptr() if status is not None else None
    return r


def current_stream_handle() -> int:
    return torch.cuda.current_stream().cuda_stream
