"""Out-of-sample assignment: ClusterIndex, a core-point index over a fitted model.

The reference names the operation (DBSCAN.predict, DBSCAN.scala:300-302) and leaves it
unimplemented; here a new point takes the label the Archery border rule
(LocalDBSCANArchery.scala:103-106) would give a non-core point at its position: the smallest
cluster id among the model's cores within eps under the exact fp64 predicate
(DBSCANPoint.scala:26-30), flag Border; cluster 0, flag Noise when there is none.  Everything is
computed by the gfx950 kernels of assign.hip; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib

INDEX_STAT_KEYS = ["n", "cores", "max_cluster", "cells", "nx", "ny", "grid_mode", "device"]


def _vec(a, name: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D array")
    return a


class ClusterIndex:
    """A dbscan_index over the cores (flag == Core) of a model fitted in mode NAIVE or ARCHERY:
    x, y, cluster, flag of n points plus eps.  It owns device buffers of its own (later fits on
    the handle leave it intact) and keeps its handle alive; close() synchronizes that handle
    before the index is destroyed.  A caller who queues asynchronous assigns on OTHER handles
    (device.assign_tensors_async) must sync those before close()."""

    def __init__(self, x, y, cluster, flag, eps: float, handle: Optional[_lib.Handle] = None):
        x, y = _vec(x, "x"), _vec(y, "y")
        cluster = np.ascontiguousarray(cluster)
        flag = np.ascontiguousarray(flag)
        if x.shape != y.shape:
            raise ValueError("x and y must be 1-D arrays of equal length")
        if cluster.shape != x.shape or cluster.dtype.kind not in "iu":
            raise ValueError("cluster: one integer per point")
        if flag.shape != x.shape or flag.dtype.kind not in "iu":
            raise ValueError("flag: one Flag ordinal per point")
        cluster = np.ascontiguousarray(cluster, dtype=np.int32)
        flag = np.ascontiguousarray(flag, dtype=np.uint8)
        self._idx = None
        self._handle = None
        if handle is None:
            from .local import default_handle

            handle = default_handle()
        vp = ctypes.c_void_p
        out = vp()
        _lib.check(_lib.load().dbscan_index_build(
            handle.ptr, x.ctypes.data_as(vp), y.ctypes.data_as(vp), cluster.ctypes.data_as(vp),
            flag.ctypes.data_as(vp), x.size, float(eps), ctypes.byref(out)))
        self._adopt(out, handle, float(eps))

    def _adopt(self, ptr, handle: _lib.Handle, eps: float) -> None:
        self._idx = ptr
        self._handle = handle
        self.eps = eps

    @classmethod
    def _from_ptr(cls, ptr, handle: _lib.Handle, eps: float) -> "ClusterIndex":
        self = cls.__new__(cls)
        self._adopt(ptr, handle, eps)
        return self

    @property
    def ptr(self):
        if not self._idx:
            raise _lib.DBSCANError("the ClusterIndex is closed")
        return self._idx

    @property
    def handle(self) -> _lib.Handle:
        return self._handle

    def assign(self, qx, qy, nearest: bool = False, handle: Optional[_lib.Handle] = None):
        """Labels of the queries, in query order: (cluster int32, flag uint8) and, with
        nearest=True, the model input index of each query's nearest core within eps (-1: none;
        ties go to the smallest index).  handle: the handle to run on (default: the index's
        own); several threads, each with its own handle, may assign from one index at once."""
        qx, qy = _vec(qx, "qx"), _vec(qy, "qy")
        if qx.shape != qy.shape:
            raise ValueError("qx and qy must be 1-D arrays of equal length")
        m = qx.size
        cl = np.zeros(m, np.int32)
        fl = np.full(m, 2, np.uint8)
        nr = np.full(m, -1, np.int32) if nearest else None
        vp = ctypes.c_void_p
        h = handle or self._handle
        _lib.check(_lib.load().dbscan_assign(
            h.ptr, self.ptr, qx.ctypes.data_as(vp), qy.ctypes.data_as(vp), m,
            cl.ctypes.data_as(vp), fl.ctypes.data_as(vp),
            nr.ctypes.data_as(vp) if nearest else None))
        return (cl, fl, nr) if nearest else (cl, fl)

    def stats(self) -> dict:
        """n, cores indexed, largest cluster id, occupied cells, grid nx / ny, grid mode
        (0 = grid, 1 = all pairs, 2 = no pairs), device."""
        buf = (ctypes.c_int64 * 8)()
        k = _lib.load().dbscan_index_stats(self.ptr, buf, 8)
        if k < 0:
            _lib.check(int(k))
        return {INDEX_STAT_KEYS[i]: int(buf[i]) for i in range(k)}

    def close(self) -> None:
        if self._idx:
            idx, self._idx = self._idx, None
            try:
                if self._handle is not None and self._handle.ptr:
                    self._handle.sync()  # dbscan_index_destroy waits for nothing
            finally:
                _lib.load().dbscan_index_destroy(idx)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
