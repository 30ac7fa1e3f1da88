"""bench.py's reporting helpers on the CPU: a secondary measurement that raises is reported in the
line and the run goes on (a failing cfg5 shard lost the whole bench line)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def test_secondary_failure_is_reported_and_the_run_goes_on():
    extra = {}

    def boom():
        raise RuntimeError("RCCL stand-in: rank 1 unreachable")

    assert bench.secondary(extra, "cfg5_shard", boom) is False
    assert "cfg5_shard" not in extra
    assert extra["cfg5_shard_error"] == "RuntimeError: RCCL stand-in: rank 1 unreachable"
    assert bench.secondary(extra, "cfg1", lambda: {"gibps": 1.0}) is True
    assert extra["cfg1"] == {"gibps": 1.0}
    # (a long message is cut to 300 characters: the line stays one line of JSON)
    bench.secondary(extra, "x", lambda: (_ for _ in ()).throw(ValueError("y" * 1000)))
    assert len(extra["x_error"]) == 300


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--no-cold"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d" and a.no_cold is True


def _rows(torch, n, extra):
    # n valid rows followed by `extra` rows the scan never wrote (alloc_rows leaves slack)
    i = torch.arange(n + extra, dtype=torch.int64)
    return {"pos": i * 5114 % (2 ** 31), "seq": i + 1, "vsz": (i % 4096 * 16 + 16).to(torch.int32),
            "ksz": torch.full((n + extra,), 16, dtype=torch.int16), "status": (i % 7 == 0).to(torch.uint8)}


def test_dump_outputs_small_count_writes_every_row(tmp_path):
    import numpy as np
    import torch
    rows = _rows(torch, 1000, 16)
    written = bench.dump_outputs(torch, str(tmp_path / "o"), rows, 1000, sample_rows=4096)
    got = {p.stem: np.load(p) for p in (tmp_path / "o").iterdir()}
    assert set(got) == {"count", "sample_index", "column_sums", *bench.ROW_COLUMNS}
    assert all(a.dtype == np.float64 for a in got.values())
    assert written == sum(a.nbytes for a in got.values())
    assert got["count"].tolist() == [1000.0]
    assert np.array_equal(got["sample_index"], np.arange(1000))
    for name in bench.ROW_COLUMNS:
        assert np.array_equal(got[name], rows[name][:1000].numpy().astype(np.float64)), name
    for c, name in enumerate(bench.ROW_COLUMNS):
        col = [int(v) for v in rows[name][:1000]]
        lo, hi, wlo, whi = (int(v) for v in got["column_sums"][c])
        assert lo + (hi << 32) == sum(col) % 2 ** 64
        assert wlo + (whi << 32) == sum(v * (i + 1) for i, v in enumerate(col)) % 2 ** 64


def test_dump_outputs_sample_is_fixed_distinct_and_sees_changes_outside_it(tmp_path):
    import numpy as np
    import torch
    rows = _rows(torch, 5000, 16)
    bench.dump_outputs(torch, str(tmp_path / "a"), rows, 5000, sample_rows=256)
    bench.dump_outputs(torch, str(tmp_path / "b"), rows, 5000, sample_rows=256, prefix="rank1_")
    a = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    b = {p.stem[len("rank1_"):]: np.load(p) for p in (tmp_path / "b").iterdir()}
    assert all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)
    idx = a["sample_index"].astype(np.int64)
    assert idx.size == 256 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 5000
    assert np.array_equal(a["seq"], idx + 1.0)
    # two rows outside the sample swapped: the plain sums agree, the weighted ones do not
    outside = [i for i in range(5000) if i not in set(idx.tolist())][:2]
    for t in rows.values():
        t[outside] = t[outside[::-1]].clone()
    bench.dump_outputs(torch, str(tmp_path / "c"), rows, 5000, sample_rows=256)
    c = np.load(tmp_path / "c" / "column_sums.npy")
    assert np.array_equal(c[:, :2], a["column_sums"][:, :2])
    assert not np.array_equal(c[1, 2:], a["column_sums"][1, 2:])


def test_watchdog_exit_status_is_not_success():
    # the watchdog prints the partial line and exits with 3, not 0 (bench.py main: os._exit(3))
    src = open(bench.__file__).read()
    assert "os._exit(3)" in src and "os._exit(0)" not in src
