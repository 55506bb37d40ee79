"""CPU tests of the out-of-sample assignment's boundary: the symbols exist, NULL arguments are
DBSCAN_EARG with a message, the Python wrappers validate their arguments before any native call,
and nothing computes without a GPU (the parity tests are in test_gpu_assign.py)."""
import ctypes

import numpy as np
import pytest

import dbscan_amd
from dbscan_amd import _lib

NEW_SYMBOLS = ["dbscan_index_build_device", "dbscan_index_build", "dbscan_index_destroy",
               "dbscan_index_stats", "dbscan_assign_device_async", "dbscan_assign_device",
               "dbscan_assign", "dbscan_set_assign_sort_min"]


def test_new_symbols_are_exported_and_declared():
    L = _lib.load()
    declared = {name for name, _, _ in _lib.SIGNATURES}
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
        assert s in declared, s
        assert s + "(" in header, s
    assert L.dbscan_version() == 100
    assert dbscan_amd.ClusterIndex is dbscan_amd.assign.ClusterIndex
    assert callable(dbscan_amd.DBSCAN.assign) and callable(dbscan_amd.DBSCAN.index)
    assert callable(_lib.Handle.set_assign_sort_min)


def test_null_arguments_are_earg_with_a_message():
    L = _lib.load()
    out = ctypes.c_void_p(0x1234)
    rc = L.dbscan_index_build(None, None, None, None, None, 0, 0.3, ctypes.byref(out))
    assert rc == _lib.DBSCAN_EARG and b"NULL handle" in L.dbscan_last_error()
    assert not out.value  # never left dangling
    rc = L.dbscan_index_build_device(None, None, None, None, None, 0, 0.3, None)
    assert rc == _lib.DBSCAN_EARG and b"NULL handle" in L.dbscan_last_error()
    for fn in (L.dbscan_assign, L.dbscan_assign_device, L.dbscan_assign_device_async):
        rc = fn(None, None, None, None, 0, None, None, None)
        assert rc == _lib.DBSCAN_EARG and b"NULL handle" in L.dbscan_last_error()
    buf = (ctypes.c_int64 * 8)()
    assert L.dbscan_index_stats(None, buf, 8) == _lib.DBSCAN_EARG
    assert b"NULL index" in L.dbscan_last_error()
    assert L.dbscan_set_assign_sort_min(None, 5) == _lib.DBSCAN_EARG
    assert b"NULL handle" in L.dbscan_last_error()
    L.dbscan_index_destroy(None)  # a no-op, like dbscan_destroy(NULL)


def test_cluster_index_validates_before_any_native_call():
    x = np.zeros(6)
    cl = np.ones(6, np.int32)
    fl = np.ones(6, np.uint8)
    bad = [
        (np.zeros(5), x, cl, fl),              # x and y differ in length
        (np.zeros((3, 2)), np.zeros((3, 2)), cl, fl),  # not 1-D
        (x, x, np.ones(5, np.int32), fl),      # short cluster
        (x, x, np.ones(6, np.float64), fl),    # float cluster ids
        (x, x, cl, np.ones(7, np.uint8)),      # long flag
        (x, x, cl, np.ones(6, np.float32)),    # float flags
    ]
    for a, b, c, f in bad:
        with pytest.raises(ValueError):
            dbscan_amd.ClusterIndex(a, b, c, f, 0.3)


def test_tensor_wrappers_validate_and_raise_value_error():
    import torch

    from dbscan_amd import device

    h = object.__new__(_lib.Handle)  # a Handle that owns nothing: validation comes first
    h._h, h.device = None, 0
    idx = object.__new__(dbscan_amd.ClusterIndex)
    idx._idx = idx._handle = None
    x = torch.zeros(4, dtype=torch.float64)  # host tensors: not on the device
    cl = torch.zeros(4, dtype=torch.int32)
    fl = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        device.build_index_tensors(x, x, cl, fl, 0.3, h)
    with pytest.raises(ValueError):
        device.build_index_tensors(x, x, cl, fl, 0.3, None)
    with pytest.raises(ValueError):
        device.assign_tensors(idx, x, x, h)
    with pytest.raises(ValueError):
        device.assign_tensors_async(idx, x, x, h, cl, fl)
    with pytest.raises(ValueError):
        device.assign_tensors_async(None, x, x, h, cl, fl)
    with pytest.raises(ValueError):
        device.assign_tensors_async(idx, [0.0], [0.0], h, cl, fl)


@pytest.mark.skipif(_lib.load().dbscan_device_count() > 0, reason="GPU present")
def test_cluster_index_without_gpu_fails_loudly():
    x = np.zeros(4)
    with pytest.raises(dbscan_amd.DBSCANError):
        dbscan_amd.ClusterIndex(x, x, np.ones(4, np.int32), np.ones(4, np.uint8), 0.3)
