"""Device-resident entry points (torch tensors in HBM -> labels in HBM).

torch is plumbing here (allocation, streams); all compute is libdbscan_hip.so."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _p(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def fit_tensors(x: torch.Tensor, y: torch.Tensor, eps: float, min_points: int, mode: int,
                handle: _lib.Handle, cluster: torch.Tensor = None, flag: torch.Tensor = None):
    """Fit device float64 tensors; returns (cluster int32, flag uint8, n_clusters).

    The caller's pending torch work on x/y must be complete: we synchronize torch's current
    stream before handing the pointers to the library's own stream."""
    assert x.is_cuda and y.is_cuda and x.dtype == torch.float64 and y.dtype == torch.float64
    assert x.shape == y.shape and x.dim() == 1 and x.is_contiguous() and y.is_contiguous()
    n = x.numel()
    if cluster is None:
        cluster = torch.empty(n, dtype=torch.int32, device=x.device)
    if flag is None:
        flag = torch.empty(n, dtype=torch.uint8, device=x.device)
    torch.cuda.current_stream(x.device).synchronize()
    k = ctypes.c_int32(0)
    _lib.check(_lib.load().dbscan_fit_device(handle.ptr, _p(x), _p(y), n, float(eps),
                                             int(min_points), int(mode), _p(cluster), _p(flag),
                                             ctypes.byref(k)))
    return cluster, flag, int(k.value)


def fit_tensors_async(x: torch.Tensor, y: torch.Tensor, eps: float, min_points: int, mode: int,
                      handle: _lib.Handle, cluster: torch.Tensor, flag: torch.Tensor,
                      n_clusters: torch.Tensor = None) -> None:
    """Enqueue a fit on the handle's stream and return at once (dbscan_fit_device_async).
    n_clusters (int32 device tensor of one element) receives the cluster count; call
    handle.sync() (or synchronize the device) before reading any output.  x/y must not be
    written by other streams until then."""
    assert x.is_cuda and y.is_cuda and x.dtype == torch.float64 and y.dtype == torch.float64
    assert x.shape == y.shape and x.dim() == 1 and x.is_contiguous() and y.is_contiguous()
    n = x.numel()
    assert cluster.numel() == n and flag.numel() == n and cluster.dtype == torch.int32 \
        and flag.dtype == torch.uint8
    nk = _p(n_clusters) if n_clusters is not None else None
    _lib.check(_lib.load().dbscan_fit_device_async(handle.ptr, _p(x), _p(y), n, float(eps),
                                                   int(min_points), int(mode), _p(cluster),
                                                   _p(flag), nk))


def fit_batch_tensors_async(x: torch.Tensor, y: torch.Tensor, offsets, eps: float,
                            min_points: int, mode: int, handle: _lib.Handle,
                            cluster: torch.Tensor, flag: torch.Tensor,
                            n_clusters: torch.Tensor) -> None:
    """Enqueue a batch of partition fits (dbscan_fit_batch_device_async): partition p is
    x[offsets[p]:offsets[p+1]] (offsets: host int64 array); n_clusters: int32 device tensor of
    n_parts entries.  handle.sync() before reading the outputs."""
    import numpy as np

    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1 or offs[0] < 0 or np.any(np.diff(offs) < 0):
        raise ValueError("offsets: n_parts + 1 non-decreasing values from >= 0")
    total = int(offs[-1])
    for name, t, dt, need in (("x", x, torch.float64, total), ("y", y, torch.float64, total),
                              ("cluster", cluster, torch.int32, total),
                              ("flag", flag, torch.uint8, total),
                              ("n_clusters", n_clusters, torch.int32, offs.size - 1)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.device == x.device
                and t.numel() >= need):
            raise ValueError(f"{name}: contiguous {dt} tensor of >= {need} values on {x.device}")
    if x.numel() != y.numel():
        raise ValueError("x and y differ in length")
    _lib.check(_lib.load().dbscan_fit_batch_device_async(
        handle.ptr, _p(x), _p(y), offs.ctypes.data_as(ctypes.c_void_p), offs.size - 1,
        float(eps), int(min_points), int(mode), _p(cluster), _p(flag), _p(n_clusters)))


def _check_tensor(name: str, t, dtype, device, numel=None) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: a torch tensor is required")
    if not (t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.dtype == dtype):
        raise ValueError(f"{name}: contiguous 1-D {dtype} device tensor required")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: {t.numel()} values, expected {numel}")


def build_index_tensors(x: torch.Tensor, y: torch.Tensor, cluster: torch.Tensor,
                        flag: torch.Tensor, eps: float, handle: _lib.Handle):
    """A ClusterIndex over a model held in device tensors (float64 x / y, int32 cluster, uint8
    flag; dbscan_index_build_device).  Synchronous; the index copies what it needs, so the
    tensors may be freed afterwards."""
    from .assign import ClusterIndex

    if not isinstance(handle, _lib.Handle):
        raise ValueError("handle: a dbscan_amd.Handle is required")
    _check_tensor("x", x, torch.float64, None)
    n = x.numel()
    if x.device.index != handle.device:
        raise ValueError(f"x: on {x.device}, the handle is on device {handle.device}")
    _check_tensor("y", y, torch.float64, x.device, n)
    _check_tensor("cluster", cluster, torch.int32, x.device, n)
    _check_tensor("flag", flag, torch.uint8, x.device, n)
    torch.cuda.current_stream(x.device).synchronize()
    out = ctypes.c_void_p()
    _lib.check(_lib.load().dbscan_index_build_device(handle.ptr, _p(x), _p(y), _p(cluster),
                                                     _p(flag), n, float(eps), ctypes.byref(out)))
    return ClusterIndex._from_ptr(out, handle, float(eps))


def _assign_args(index, qx, qy, handle, cluster, flag, nearest):
    from .assign import ClusterIndex

    if not isinstance(index, ClusterIndex):
        raise ValueError("index: a ClusterIndex is required")
    if not isinstance(handle, _lib.Handle):
        raise ValueError("handle: a dbscan_amd.Handle is required")
    _check_tensor("qx", qx, torch.float64, None)
    m = qx.numel()
    if qx.device.index != handle.device:
        raise ValueError(f"qx: on {qx.device}, the handle is on device {handle.device}")
    _check_tensor("qy", qy, torch.float64, qx.device, m)
    _check_tensor("cluster", cluster, torch.int32, qx.device, m)
    _check_tensor("flag", flag, torch.uint8, qx.device, m)
    if nearest is not None:
        _check_tensor("nearest", nearest, torch.int32, qx.device, m)
    return m


def assign_tensors(index, qx: torch.Tensor, qy: torch.Tensor, handle: _lib.Handle,
                   cluster: torch.Tensor = None, flag: torch.Tensor = None,
                   nearest: torch.Tensor = None, want_nearest: bool = False):
    """Assign device float64 queries against a ClusterIndex (dbscan_assign_device; returns after
    the handle's stream has drained): (cluster int32, flag uint8, nearest int32 or None) in
    query order.  The caller's pending torch work on qx/qy is synchronized first."""
    if isinstance(qx, torch.Tensor) and qx.is_cuda:
        if cluster is None:
            cluster = torch.empty(qx.numel(), dtype=torch.int32, device=qx.device)
        if flag is None:
            flag = torch.empty(qx.numel(), dtype=torch.uint8, device=qx.device)
        if nearest is None and want_nearest:
            nearest = torch.empty(qx.numel(), dtype=torch.int32, device=qx.device)
    m = _assign_args(index, qx, qy, handle, cluster, flag, nearest)
    torch.cuda.current_stream(qx.device).synchronize()
    _lib.check(_lib.load().dbscan_assign_device(
        handle.ptr, index.ptr, _p(qx), _p(qy), m, _p(cluster), _p(flag),
        _p(nearest) if nearest is not None else None))
    return cluster, flag, nearest


def assign_tensors_async(index, qx: torch.Tensor, qy: torch.Tensor, handle: _lib.Handle,
                         cluster: torch.Tensor, flag: torch.Tensor,
                         nearest: torch.Tensor = None) -> None:
    """Enqueue an assign on the handle's stream and return at once
    (dbscan_assign_device_async); handle.sync() before reading the outputs, and before the
    index is closed.  qx/qy must not be written by other streams until then."""
    m = _assign_args(index, qx, qy, handle, cluster, flag, nearest)
    _lib.check(_lib.load().dbscan_assign_device_async(
        handle.ptr, index.ptr, _p(qx), _p(qy), m, _p(cluster), _p(flag),
        _p(nearest) if nearest is not None else None))


def generate_blobs(n: int, noise: float, dense: float, seed: int, handle: _lib.Handle,
                   device=None):
    """SURVEY §8d generator on the device (no PCIe): returns (x, y) float64 tensors."""
    dev = device if device is not None else torch.device("cuda", handle.device)
    x = torch.empty(n, dtype=torch.float64, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    _lib.check(_lib.load().dbscan_generate_blobs_device(handle.ptr, _p(x), _p(y), n,
                                                        float(noise), float(dense), int(seed)))
    return x, y


def slab_fit(x: torch.Tensor, y: torch.Tensor, zone: torch.Tensor, eps: float, min_points: int,
             handle: _lib.Handle):
    """Slab fit phase 1 (node path): returns (core uint8, root int32) device tensors."""
    n = x.numel()
    core = torch.empty(n, dtype=torch.uint8, device=x.device)
    root = torch.empty(n, dtype=torch.int32, device=x.device)
    torch.cuda.current_stream(x.device).synchronize()
    _lib.check(_lib.load().dbscan_slab_fit_device(handle.ptr, _p(x), _p(y), _p(zone), n,
                                                  float(eps), int(min_points), _p(core),
                                                  _p(root)))
    return core, root


def slab_merge_roots(zone: torch.Tensor, gid: torch.Tensor, root: torch.Tensor,
                     parent: torch.Tensor, gs_of_root: torch.Tensor, own_roots: torch.Tensor,
                     handle: _lib.Handle) -> int:
    """After a slab fit and the merge union: gs_of_root[p] for every local root p; the global
    roots owned here into own_roots (increasing gid); returns their count."""
    k = ctypes.c_int64(0)
    torch.cuda.current_stream(zone.device).synchronize()
    _lib.check(_lib.load().dbscan_slab_merge_roots_device(handle.ptr, zone.numel(), _p(zone),
                                                          _p(gid), _p(root), _p(parent),
                                                          _p(gs_of_root), _p(own_roots),
                                                          ctypes.byref(k)))
    return int(k.value)


def slab_label(zone: torch.Tensor, gid: torch.Tensor, gs_of_root: torch.Tensor,
               all_roots: torch.Tensor, mode: int, handle: _lib.Handle, cluster=None,
               flag=None):
    """Slab fit phase 2 (after the global merge): (cluster int32, flag uint8) in slab order;
    only zone-0 entries are written.  all_roots: every global component's s(K), sorted."""
    n = zone.numel()
    if cluster is None:
        cluster = torch.zeros(n, dtype=torch.int32, device=zone.device)
    if flag is None:
        flag = torch.full((n,), 3, dtype=torch.uint8, device=zone.device)
    all_roots = all_roots.to(torch.int64).contiguous()
    torch.cuda.current_stream(zone.device).synchronize()
    _lib.check(_lib.load().dbscan_slab_label_device(handle.ptr, _p(zone), _p(gid),
                                                    _p(gs_of_root), _p(all_roots),
                                                    all_roots.numel(), int(mode), _p(cluster),
                                                    _p(flag)))
    return cluster, flag
