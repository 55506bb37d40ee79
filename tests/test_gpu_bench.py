"""bench.py's plain run on the GPU, in-process at a small size: the result line's fields, what
stays out of a plain run, and --dump-outputs (the last timed step's labels: equal to the
oracle's on the same generated points, identical from run to run)."""
import json
import sys

import numpy as np
import pytest

import bench
import oracle as O

pytestmark = pytest.mark.gpu

N = 200_003  # (odd: no multiple of any tile or block size)


def _run(monkeypatch, capsys, *argv):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--points-per-gpu", str(N)]
                        + list(argv))
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {k: np.load(d / f"{k}.npy") for k in ("cluster", "flag", "n_clusters")}


def test_plain_run_line_and_dump(monkeypatch, capsys, tmp_path):
    d = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs",
             str(tmp_path / "a"))
    assert (d["steps"], d["warmup"], d["n_gpus"], d["full"]) == (3, 1, 1, False)
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == \
        (bench.METRIC, "points/s", True, "f64")
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(N / (d["ms_per_step"] * 1e-3), rel=1e-3)
    for leg in ("roofline", "valu", "end_to_end", "seam", "cpu_baseline"):
        assert d[leg] is None, leg
    assert d["kernels_ms_per_step"] == {}

    a = _load(tmp_path / "a")
    assert a["cluster"].dtype == np.float64 and a["flag"].dtype == np.float32
    assert a["cluster"].shape == a["flag"].shape == (N,)
    import dbscan_amd
    from dbscan_amd import device as D

    h = dbscan_amd.Handle(0)
    x, y = D.generate_blobs(N, 0.0, 1.0, 1, h)
    rc, rf, rk = O.fit_grid(x.cpu().numpy(), y.cpu().numpy(), 2.55, 10, 0)
    h.close()
    np.testing.assert_array_equal(a["cluster"], rc)
    np.testing.assert_array_equal(a["flag"], rf)
    assert a["n_clusters"].tolist() == [rk] and d["config"]["clusters"] == rk

    _run(monkeypatch, capsys, "--steps", "1", "--warmup", "0", "--dump-outputs",
         str(tmp_path / "b"))
    b = _load(tmp_path / "b")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
