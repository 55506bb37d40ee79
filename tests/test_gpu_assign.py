"""Out-of-sample assignment on the GPU (assign.hip): every comparison is exact.

The label a query gets is the label the Archery border rule gives a non-core point at its
position, so assigning a model's own points must reproduce the oracle's ARCHERY clusters; fresh
queries are checked against the chunked `d2 <= eps2` matrix built with numpy's plain `*` and
`+` (which never fuse), the predicate of DBSCANPoint.scala:26-30 taken literally (NaN and inf
included)."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle as O
from conftest import EPS_03F, ROOT, gen_blobs

pytestmark = pytest.mark.gpu

BORDER, CORE, NOISE = 0, 1, 2
NEVER = 1 << 40  # a sort threshold no batch reaches: every assign takes the unsorted form


def ref_assign(mx, my, mcl, mfl, eps, qx, qy, chunk=256):
    """numpy brute force over all (query, core) pairs: (cluster, flag, nearest)."""
    core = np.flatnonzero(np.asarray(mfl) == CORE)
    cx, cy, ccl = mx[core], my[core], np.asarray(mcl)[core].astype(np.int64)
    eps2 = np.float64(eps) * np.float64(eps)
    m = qx.size
    cl = np.zeros(m, np.int32)
    fl = np.full(m, NOISE, np.uint8)
    nr = np.full(m, -1, np.int32)
    if core.size == 0:
        return cl, fl, nr
    with np.errstate(all="ignore"):
        for a in range(0, m, chunk):
            b = min(m, a + chunk)
            dx = cx[None, :] - qx[a:b, None]
            dy = cy[None, :] - qy[a:b, None]
            np.multiply(dx, dx, out=dx)
            np.multiply(dy, dy, out=dy)
            d2 = np.add(dx, dy, out=dx)
            rows, cols = np.nonzero(d2 <= eps2)  # the matching pairs (few per query)
            if rows.size == 0:
                continue
            d = d2[rows, cols]
            # per query: the smallest cluster; the smallest (d2, input index) -- cores ascend
            order = np.lexsort((ccl[cols], rows))
            q, at = np.unique(rows[order], return_index=True)
            cl[a + q] = ccl[cols[order[at]]]
            fl[a + q] = BORDER
            order = np.lexsort((cols, d, rows))
            q, at = np.unique(rows[order], return_index=True)
            nr[a + q] = core[cols[order[at]]]
    return cl, fl, nr


def eps_for(n):
    return 2.55 * np.sqrt(n / 1e6) * 7


INPUTS = {
    "blobs20000": dict(n=20000, noise=0.2, seed=5, mp=10, counts=(1351, 13990, 4659), k=33,
                       naive_diff=12),
    "blobs4000": dict(n=4000, noise=0.3, seed=6, mp=4, counts=(353, 1973, 1674), k=93,
                      naive_diff=67),
}


@pytest.fixture(scope="module")
def handle():
    import dbscan_amd

    h = dbscan_amd.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for name, p in INPUTS.items():
        x, y = gen_blobs(p["n"], noise=p["noise"], seed=p["seed"])
        eps = eps_for(p["n"])
        acl, afl, ak = O.fit_grid(x, y, eps, p["mp"], 1)
        assert tuple(np.bincount(afl, minlength=3)[:3]) == p["counts"] and ak == p["k"]
        out[name] = dict(x=x, y=y, eps=eps, mp=p["mp"], acl=acl, afl=afl, p=p)
    return out


def both_forms(idx, h, qx, qy):
    """The assign in its sorted and its unsorted form (they must agree bit for bit)."""
    old = h.set_assign_sort_min(0)
    try:
        a = idx.assign(qx, qy, nearest=True, handle=h)
        h.set_assign_sort_min(NEVER)
        b = idx.assign(qx, qy, nearest=True, handle=h)
    finally:
        h.set_assign_sort_min(old)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    return a


def check(idx, h, model, eps, qx, qy):
    """Both forms against the numpy reference, all three outputs."""
    mx, my, mcl, mfl = model
    rcl, rfl, rnr = ref_assign(mx, my, mcl, mfl, eps, qx, qy)
    cl, fl, nr = both_forms(idx, h, qx, qy)
    np.testing.assert_array_equal(cl, rcl)
    np.testing.assert_array_equal(fl, rfl)
    np.testing.assert_array_equal(nr, rnr)
    return rcl, rfl, rnr


# ---- 1. own points against the oracle -----------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["naive_model", "archery_model"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_own_points_reproduce_the_archery_oracle(handle, inputs, name, mode):
    import dbscan_amd

    d = inputs[name]
    x, y, eps = d["x"], d["y"], d["eps"]
    mcl, mfl, _ = dbscan_amd.fit_arrays(x, y, eps, d["mp"], mode, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    if mode == 0:  # the test can tell the two border rules apart
        assert int((mcl != d["acl"]).sum()) == d["p"]["naive_diff"] > 0
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, eps, handle=handle)
    st = idx.stats()
    assert st["n"] == x.size and st["cores"] == d["p"]["counts"][1] and st["grid_mode"] == 0
    assert st["max_cluster"] == d["p"]["k"] and 0 < st["cells"] <= st["nx"] * st["ny"]
    cl, fl, nr = both_forms(idx, handle, x, y)
    np.testing.assert_array_equal(cl, d["acl"])
    np.testing.assert_array_equal(fl == NOISE, d["afl"] == NOISE)
    assert not (fl == CORE).any()
    core = np.flatnonzero(d["afl"] == CORE)
    np.testing.assert_array_equal(nr[core], core)
    idx.close()


# ---- 2. fresh queries against numpy brute force ---------------------------------------------

@pytest.fixture(scope="module")
def fresh(handle, inputs):
    """The 20000-point model (Naive fit), its index, the query batch and the numpy reference,
    computed once and shared (read-only)."""
    import dbscan_amd

    d = inputs["blobs20000"]
    x, y, eps = d["x"], d["y"], d["eps"]
    mcl, mfl, _ = dbscan_amd.fit_arrays(x, y, eps, d["mp"], 0, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    rng = np.random.default_rng(77)
    g = 3 * eps
    qx = rng.uniform(x.min() - g, x.max() + g, 30000)
    qy = rng.uniform(y.min() - g, y.max() + g, 30000)
    far = [1e6, -1e6, 1e300, -1e300]
    odd = [np.nan, np.inf, -np.inf]
    sx = [a for a in far for _ in far] + [a for a in odd for _ in range(4)] + [0.0] * 3 + \
        [a for a in odd for _ in odd]
    sy = [b for _ in far for b in far] + [b for _ in odd for b in (0.0, 1e6, x[0], -1e300)] + \
        odd + [b for _ in odd for b in odd]
    core = np.flatnonzero(mfl == CORE)
    dup = core[rng.integers(0, core.size, 200)]  # exact duplicates of model cores
    qx = np.concatenate([qx, sx, x[dup]])
    qy = np.concatenate([qy, sy, y[dup]])
    ref = ref_assign(x, y, mcl, mfl, eps, qx, qy)
    assert (ref[1] == BORDER).sum() > 3000 and (ref[1] == NOISE).sum() > 3000
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, eps, handle=handle)
    for a in (qx, qy, mcl, mfl) + ref:
        a.setflags(write=False)
    yield dict(model=(x, y, mcl, mfl), eps=eps, qx=qx, qy=qy, ref=ref, idx=idx, dup=dup)
    idx.close()


def test_fresh_queries_equal_numpy_brute_force(handle, fresh):
    cl, fl, nr = both_forms(fresh["idx"], handle, fresh["qx"], fresh["qy"])
    rcl, rfl, rnr = fresh["ref"]
    np.testing.assert_array_equal(cl, rcl)
    np.testing.assert_array_equal(fl, rfl)
    np.testing.assert_array_equal(nr, rnr)
    # a duplicate of a core is its own nearest core; far and non-finite queries are Noise
    np.testing.assert_array_equal(nr[-200:], fresh["dup"])
    assert (fl[30000:-200] == NOISE).all() and (nr[30000:-200] == -1).all()
    cl2, fl2 = fresh["idx"].assign(fresh["qx"], fresh["qy"])  # without the optional output
    np.testing.assert_array_equal(cl2, rcl)
    np.testing.assert_array_equal(fl2, rfl)


def test_duplicated_cores_break_nearest_ties_by_index(handle, inputs):
    import dbscan_amd

    d = inputs["blobs4000"]
    rng = np.random.default_rng(3)
    pick = rng.integers(0, d["x"].size, 600)
    order = rng.permutation(d["x"].size + 600)
    x = np.concatenate([d["x"], d["x"][pick]])[order]
    y = np.concatenate([d["y"], d["y"][pick]])[order]
    eps = d["eps"]
    mcl, mfl, _ = dbscan_amd.fit_arrays(x, y, eps, d["mp"], 1, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, eps, handle=handle)
    qx = np.concatenate([x, rng.uniform(x.min(), x.max(), 2000)])
    qy = np.concatenate([y, rng.uniform(y.min(), y.max(), 2000)])
    _, _, rnr = check(idx, handle, (x, y, mcl, mfl), eps, qx, qy)
    core = np.flatnonzero(mfl == CORE)
    twin = rnr[core] != core  # cores whose nearest is an earlier copy of themselves
    assert twin.sum() > 100 and (rnr[core][twin] < core[twin]).all()
    idx.close()


# ---- 3. the predicate's edge, straddling cell boundaries ------------------------------------

def lattice_case(scale, eps):
    gx, gy = np.meshgrid(np.arange(40.0), np.arange(20.0))
    x = np.concatenate([gx.ravel(), gx.ravel()]) * scale
    y = np.concatenate([gy.ravel(), gy.ravel() + 100.0]) * scale
    # cores on the blocks' edges and corners, and a few inside
    ex = np.array([0, 39, 0, 39, 17, 20, 0, 39, 5, 10, 15, 25], float)
    ey = np.array([0, 0, 19, 19, 0, 19, 7, 12, 5, 10, 15, 119], float)
    ey2 = np.array([100, 100, 119, 119, 100, 119, 107, 112, 105, 110, 115, 100], float)
    bx = np.concatenate([ex, ex])
    by = np.concatenate([ey, ey2])
    qx, qy = [], []
    for ox, oy in ((3, 4), (4, 3), (5, 0), (0, 5)):
        for sx in (1, -1):
            for sy in (1, -1):
                px, py = (bx + sx * ox) * scale, (by + sy * oy) * scale
                for ux in (-np.inf, None, np.inf):
                    for uy in (-np.inf, None, np.inf):
                        qx.append(px if ux is None else np.nextafter(px, ux))
                        qy.append(py if uy is None else np.nextafter(py, uy))
    # queries one ulp either side of the index grid's cell boundaries (side = |eps|(1 + 2^-20))
    side = abs(eps) * (1.0 + 2.0 ** -20)
    edges = side * np.arange(1, 9)
    for e in (edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)):
        for row in (0.0, 19.0 * scale, 24.0 * scale, 100.0 * scale):
            qx.append(e)
            qy.append(np.full(e.size, row))
            qx.append(np.full(e.size, row))
            qy.append(e)
    return x, y, np.concatenate(qx), np.concatenate(qy)


@pytest.mark.parametrize("scale,eps", [(1.0, 5.0), (EPS_03F / 5.0, EPS_03F), (1.0, -5.0),
                                       (EPS_03F / 5.0, -EPS_03F)],
                         ids=["unit", "eps03f", "unit_negative_eps", "eps03f_negative_eps"])
def test_predicate_edge_on_a_lattice(handle, scale, eps):
    import dbscan_amd

    x, y, qx, qy = lattice_case(scale, eps)
    mcl, mfl, k = dbscan_amd.fit_arrays(x, y, abs(eps), 4, 0, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    assert k == 2 and (mfl == CORE).all()
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, eps, handle=handle)
    rcl, rfl, _ = check(idx, handle, (x, y, mcl, mfl), eps, qx, qy)
    if scale == 1.0:  # d2 == eps*eps exactly is inside; one ulp further out may not be
        assert (rfl == BORDER).sum() > 1000 and (rfl == NOISE).sum() > 100
        assert set(np.unique(rcl)) == {0, 1, 2}
    idx.close()


# ---- 4. degenerate models and batches ------------------------------------------------------

def test_degenerate_models_and_batches(handle, inputs):
    import dbscan_amd
    from dbscan_amd import _lib

    d = inputs["blobs4000"]
    x, y, eps = d["x"][:1500].copy(), d["y"][:1500].copy(), d["eps"] * 2
    q = np.array([0.0, x[0], np.nan, np.inf, -np.inf, 1e300])
    qy = np.array([0.0, y[0], 0.0, 0.0, np.inf, -1e300])
    e = np.zeros(0)
    # n == 0
    idx = dbscan_amd.ClusterIndex(e, e, np.zeros(0, np.int32), np.zeros(0, np.uint8), eps,
                                  handle=handle)
    assert idx.stats()["grid_mode"] == 2 and idx.stats()["n"] == 0
    cl, fl, nr = both_forms(idx, handle, q, qy)
    assert (cl == 0).all() and (fl == NOISE).all() and (nr == -1).all()
    idx.close()
    # m == 0, and a model without cores (a huge minPoints)
    mcl, mfl, k = dbscan_amd.fit_arrays(x, y, eps, 1 << 30, 1, handle=handle)
    assert k == 0
    idx = dbscan_amd.ClusterIndex(x, y, mcl.copy(), mfl.copy(), eps, handle=handle)
    assert idx.stats()["cores"] == 0 and idx.stats()["grid_mode"] == 2
    cl, fl, nr = idx.assign(e, e, nearest=True)
    assert cl.size == fl.size == nr.size == 0
    cl, fl, nr = both_forms(idx, handle, np.concatenate([q, x]), np.concatenate([qy, y]))
    assert (cl == 0).all() and (fl == NOISE).all() and (nr == -1).all()
    idx.close()
    # eps = inf: all pairs, an inf query against finite cores included; eps = nan: none
    mcl, mfl, k = dbscan_amd.fit_arrays(x, y, np.inf, 10, 1, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    assert k == 1 and (mfl == CORE).all()
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, np.inf, handle=handle)
    assert idx.stats()["grid_mode"] == 1 and idx.stats()["cores"] == x.size
    rcl, rfl, rnr = check(idx, handle, (x, y, mcl, mfl), np.inf, q, qy)
    assert list(rfl) == [BORDER, BORDER, NOISE, BORDER, BORDER, BORDER] and rnr[1] == 0
    idx.close()
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, np.nan, handle=handle)
    assert idx.stats()["grid_mode"] == 2
    cl, fl, nr = both_forms(idx, handle, q, qy)
    assert (cl == 0).all() and (fl == NOISE).all() and (nr == -1).all()
    idx.close()
    # minPoints = 0: every point is a core, the NaN and inf ones too -- nobody's neighbours
    x2, y2 = x.copy(), y.copy()
    x2[7], y2[11], x2[13] = np.nan, np.inf, -np.inf
    mcl, mfl, _ = dbscan_amd.fit_arrays(x2, y2, eps, 0, 0, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    assert (mfl == CORE).all()
    idx = dbscan_amd.ClusterIndex(x2, y2, mcl, mfl, eps, handle=handle)
    assert idx.stats()["cores"] == x.size - 3
    qq = np.concatenate([q, x2])
    qqy = np.concatenate([qy, y2])
    _, rfl, rnr = check(idx, handle, (x2, y2, mcl, mfl), eps, qq, qqy)
    assert rfl[6 + 7] == NOISE and rfl[6 + 11] == NOISE and rnr[6 + 20] == 20
    idx.close()
    # ... and all of them take part when eps*eps is +inf (d2 = inf matches, d2 = NaN does not)
    idx = dbscan_amd.ClusterIndex(x2, y2, mcl, mfl, np.inf, handle=handle)
    assert idx.stats()["cores"] == x.size
    check(idx, handle, (x2, y2, mcl, mfl), np.inf, qq[:40], qqy[:40])
    # argument errors: a core without a cluster; negative sizes
    bad = mcl.copy()
    bad[5] = 0
    with pytest.raises(dbscan_amd.DBSCANError, match="cluster <= 0"):
        dbscan_amd.ClusterIndex(x, y, bad, mfl, eps, handle=handle)
    L, out = _lib.load(), ctypes.c_void_p()
    assert L.dbscan_index_build(handle.ptr, None, None, None, None, -1, eps,
                                ctypes.byref(out)) == _lib.DBSCAN_EARG
    assert b"n < 0" in L.dbscan_last_error()
    assert L.dbscan_assign(handle.ptr, idx.ptr, None, None, -1, None, None,
                           None) == _lib.DBSCAN_EARG
    assert b"m < 0" in L.dbscan_last_error()
    assert L.dbscan_assign(handle.ptr, idx.ptr, None, None, 3, None, None,
                           None) == _lib.DBSCAN_EARG
    idx.close()


# ---- 5. grid coarsening --------------------------------------------------------------------

def test_wide_sparse_model_coarsens_the_grid(handle):
    import dbscan_amd

    rng = np.random.default_rng(12)
    eps = 0.01
    x = np.concatenate([rng.normal(0, 0.02, 500), 1e9 + rng.normal(0, 0.02, 500)])
    y = np.concatenate([rng.normal(0, 0.02, 500), 3e5 + rng.normal(0, 0.02, 500)])
    mcl, mfl, k = dbscan_amd.fit_arrays(x, y, eps, 10, 0, handle=handle)
    mcl, mfl = mcl.copy(), mfl.copy()
    assert k >= 2 and (mfl == CORE).sum() > 500
    idx = dbscan_amd.ClusterIndex(x, y, mcl, mfl, eps, handle=handle)
    st = idx.stats()
    assert st["grid_mode"] == 0
    assert -(-st["nx"] // 8) * -(-st["ny"] // 8) <= 1 << 20  # the budget: 2^20 tiles of 8x8
    assert st["nx"] * st["ny"] < 1e9 / eps  # far fewer cells than an eps grid would take
    qx = np.concatenate([rng.normal(0, 0.04, 2000), 1e9 + rng.normal(0, 0.04, 2000),
                         np.linspace(-1e8, 1.1e9, 500), x])
    qy = np.concatenate([rng.normal(0, 0.04, 2000), 3e5 + rng.normal(0, 0.04, 2000),
                         np.linspace(-3e4, 3.3e5, 500), y])
    _, rfl, _ = check(idx, handle, (x, y, mcl, mfl), eps, qx, qy)
    assert (rfl[:4000] == BORDER).sum() > 500 and (rfl[:4000] == NOISE).sum() > 500
    idx.close()


# ---- 6. both forms agree -------------------------------------------------------------------

def test_small_batch_equals_the_head_of_the_full_batch(handle, fresh):
    from dbscan_amd import _lib

    L = _lib.load()
    default = handle.set_assign_sort_min(1000)  # 100 queries: unsorted; the full batch: sorted
    assert default == 1 << 20  # DBSCAN_ASSIGN_SORT_DEFAULT_QUERIES, the measured crossover
    try:
        full = fresh["idx"].assign(fresh["qx"], fresh["qy"], nearest=True, handle=handle)
        head = fresh["idx"].assign(fresh["qx"][:100], fresh["qy"][:100], nearest=True,
                                   handle=handle)
    finally:
        assert handle.set_assign_sort_min(default) == 1000
    for a, b, r in zip(full, head, fresh["ref"]):
        np.testing.assert_array_equal(a[:100], b)
        np.testing.assert_array_equal(a, r)
    assert L.dbscan_set_assign_sort_min(handle.ptr, -1) == _lib.DBSCAN_EARG


# ---- 7. index independence -----------------------------------------------------------------

def test_index_survives_fits_and_queued_work(inputs, fresh):
    import torch

    import dbscan_amd
    from dbscan_amd import device

    h = dbscan_amd.Handle(0)
    dev = torch.device("cuda", 0)
    x, y, mcl, mfl = (torch.from_numpy(np.array(a)).to(dev) for a in fresh["model"])
    idx = device.build_index_tensors(x, y, mcl, mfl, fresh["eps"], h)
    qx = torch.from_numpy(np.array(fresh["qx"])).to(dev)
    qy = torch.from_numpy(np.array(fresh["qy"])).to(dev)
    rcl, rfl, rnr = fresh["ref"]

    def same(out):
        np.testing.assert_array_equal(out[0].cpu().numpy(), rcl)
        np.testing.assert_array_equal(out[1].cpu().numpy(), rfl)
        np.testing.assert_array_equal(out[2].cpu().numpy(), rnr)

    same(device.assign_tensors(idx, qx, qy, h, want_nearest=True))
    # an unrelated fit on the same handle, through the tiled pipeline
    ux, uy = gen_blobs(20000, noise=0.1, seed=9)
    ueps = eps_for(20000)
    ocl, ofl, ok = O.fit_grid(ux, uy, ueps, 10, 0)
    tx, ty = torch.from_numpy(ux).to(dev), torch.from_numpy(uy).to(dev)
    old = h.set_small_max(0)
    fcl, ffl, fk = device.fit_tensors(tx, ty, ueps, 10, 0, h)
    assert fk == ok
    np.testing.assert_array_equal(fcl.cpu().numpy(), ocl)
    same(device.assign_tensors(idx, qx, qy, h, want_nearest=True))
    # three assigns queued back to back into distinct outputs, one sync
    m = qx.numel()
    outs = [(torch.full((m,), -7, dtype=torch.int32, device=dev),
             torch.full((m,), 9, dtype=torch.uint8, device=dev),
             torch.full((m,), -7, dtype=torch.int32, device=dev)) for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs:
        device.assign_tensors_async(idx, qx, qy, h, *o)
    h.sync()
    for o in outs:
        same(o)
    # a queued fit followed by a queued assign: neither disturbs the other
    fcl.fill_(-1)
    ffl.fill_(9)
    nk = torch.zeros(1, dtype=torch.int32, device=dev)
    o = (torch.empty(m, dtype=torch.int32, device=dev),
         torch.empty(m, dtype=torch.uint8, device=dev), None)
    torch.cuda.synchronize()
    device.fit_tensors_async(tx, ty, ueps, 10, 0, h, fcl, ffl, nk)
    device.assign_tensors_async(idx, qx, qy, h, o[0], o[1])
    h.sync()
    assert int(nk.item()) == ok and h.stats()["clusters"] == ok
    np.testing.assert_array_equal(fcl.cpu().numpy(), ocl)
    np.testing.assert_array_equal(ffl.cpu().numpy(), ofl)
    np.testing.assert_array_equal(o[0].cpu().numpy(), rcl)
    np.testing.assert_array_equal(o[1].cpu().numpy(), rfl)
    h.set_small_max(old)
    with pytest.raises(ValueError):
        device.assign_tensors_async(idx, qx, qy[:-1], h, o[0], o[1])
    with pytest.raises(ValueError):
        device.assign_tensors_async(idx, qx, qy, h, o[0].to(torch.int64), o[1])
    idx.close()
    h.close()


# ---- 8. one index shared by several handles ------------------------------------------------

def test_four_threads_share_one_index(fresh):
    import dbscan_amd

    qx, qy = fresh["qx"], fresh["qy"]
    m = qx.size
    cuts = [0, m // 5, m // 2, m - 1000, m]
    res, errs = [None] * 4, []

    def work(t):
        try:
            h = dbscan_amd.Handle(0)
            a, b = cuts[t], cuts[t + 1]
            for _ in range(3):
                res[t] = fresh["idx"].assign(qx[a:b], qy[a:b], nearest=True, handle=h)
            h.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for k, r in enumerate(fresh["ref"]):
        np.testing.assert_array_equal(np.concatenate([res[t][k] for t in range(4)]), r)


# ---- 9. the mirrors ------------------------------------------------------------------------

def test_train_assign_mirrors(tmp_path, labeled_data):
    import dbscan_amd
    from dbscan_amd import _lib

    x, y, lab = labeled_data
    acl, afl, ak = O.fit_sequential(x, y, EPS_03F, 10, 1)
    assert ak == 3 and int((afl == NOISE).sum()) == 18
    model = dbscan_amd.DBSCAN.train(np.stack([x, y], 1), eps=EPS_03F, minPoints=10,
                                    maxPointsPerPartition=250)
    cl, fl = model.assign(np.stack([x, y], 1))
    np.testing.assert_array_equal(cl, acl)
    np.testing.assert_array_equal(fl == NOISE, afl == NOISE)
    assert len(set(cl.tolist()) - {0}) == 3 and int((fl == NOISE).sum()) == 18
    assert model.index() is model.index()
    cl2, _ = model.assign([dbscan_amd.DBSCANPoint([a, b]) for a, b in zip(x[:50], y[:50])])
    np.testing.assert_array_equal(cl2, acl[:50])
    with pytest.raises(NotImplementedError):
        model.predict([0.0, 0.0])

    data = tmp_path / "pts.txt"
    np.savetxt(data, np.stack([x, y], 1), fmt="%.17g")
    src = tmp_path / "assign.cpp"
    src.write_text(r'''
#include <cstdio>
#include <fstream>
#include "dbscan_local.hpp"
int main(int argc, char** argv) {
    std::ifstream in(argv[1]);
    std::vector<dbscan::DBSCANPoint> pts;
    double a, b;
    while (in >> a >> b) pts.emplace_back(std::vector<double>{a, b});
    auto m = dbscan::DBSCAN::train(pts, (double)0.3f, 10, 250);
    for (int rep = 0; rep < 2; ++rep)
        for (const auto& p : m.assign(pts)) std::printf("%d %d %d\n", rep, p.cluster, (int)p.flag);
    try {
        m.predict({0.0, 0.0});
        return 3;
    } catch (const std::logic_error&) {
    }
    return 0;
}
''')
    exe = tmp_path / "assign"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-ldbscan_hip", f"-Wl,-rpath,{libdir}"],
                   check=True)
    out = subprocess.run([str(exe), str(data)], check=True, capture_output=True, text=True).stdout
    rows = np.array([[int(v) for v in l.split()] for l in out.splitlines()])
    assert rows.shape == (2 * x.size, 3)
    for rep in (0, 1):
        r = rows[rows[:, 0] == rep]
        np.testing.assert_array_equal(r[:, 1], cl)
        np.testing.assert_array_equal(r[:, 2], fl)
