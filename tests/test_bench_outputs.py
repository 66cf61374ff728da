"""bench.py's plain run and its --dump-outputs files (benchkit/lib.py: warmup_schedule / dump_outputs / device_slice), on the CPU: the
warm-up covers every launch shape of the timed schedule, the dumped arrays are the records' exact 32-bit words, a large output is cut to
the same seeded sample every time, and the files stay within 64 MB."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchkit import lib  # noqa: E402


@pytest.mark.parametrize("sizes, lanes, steps, want", [
    ([16, 4], 1, 5, ([16, 4], 1)),            # the driver's --steps 20 --warmup 5: one pass over the full group and the remainder
    ([16, 4], 1, 40, ([16, 4], 2)),
    ([16, 16, 16, 16], 1, 5, ([16], 1)),      # --steps 64: whole groups only; the warm-up is not --steps long
    ([4, 4, 4], 2, 1, ([4, 4], 1)),           # two groups in flight: both lanes
    ([8, 8, 3], 2, 19, ([8, 8, 3], 1)),
    ([16], 1, 0, ([16], 0)),                  # --warmup 0
])
def test_warmup_schedule(sizes, lanes, steps, want):
    assert lib.warmup_schedule(sizes, lanes, steps) == want


def test_parse_args_plain_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.min_time is None and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out", "--min-time", "0.5"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "out" and a.min_time == 0.5


def test_small_outputs_are_written_whole_and_exact(tmp_path):
    rng = np.random.default_rng(1)
    words = rng.integers(0, 1 << 32, size=(100, 96), dtype=np.uint64).astype("<u4")
    rows = rng.integers(0, 1 << 32, size=(300, 16), dtype=np.uint64).astype("<u4")
    n = lib.dump_outputs(str(tmp_path), [("gt", words.tobytes(), 384), ("g1", rows.tobytes(), 64)])
    gt, g1 = np.load(tmp_path / "gt.npy"), np.load(tmp_path / "g1.npy")
    assert gt.dtype == np.float64 and gt.shape == (100, 96) and (gt == words).all()
    assert g1.dtype == np.float64 and g1.shape == (300, 16) and (g1 == rows).all()
    assert gt.max() >= 2 ** 31          # the full 32-bit range survives float64
    assert n == gt.nbytes + g1.nbytes


def test_large_outputs_are_a_fixed_seeded_sample_within_the_budget(tmp_path):
    n_rec = lib.DUMP_MAX_RECORDS * 4
    data = np.arange(n_rec * 48, dtype="<u4").tobytes()          # record i starts with the word 48 i
    a, b = tmp_path / "a", tmp_path / "b"
    lib.dump_outputs(str(a), [("rows", data, 192)])
    lib.dump_outputs(str(b), [("rows", data, 192)])
    x, y = np.load(a / "rows.npy"), np.load(b / "rows.npy")
    assert x.shape == (lib.DUMP_MAX_RECORDS, 48) and (x == y).all()
    idx = x[:, 0] / 48
    assert (np.diff(idx) > 0).all() and idx[-1] < n_rec and (x[:, 47] == x[:, 0] + 47).all()
    assert idx[-1] > n_rec // 2          # a sample of the whole output, not its head


def test_the_budget_holds_for_wide_records(tmp_path):
    rec = 384 * 64          # records so wide that DUMP_MAX_RECORDS of them would pass 64 MB
    data = bytes(rec * (lib.DUMP_MAX_RECORDS // 4))
    n = lib.dump_outputs(str(tmp_path), [("wide", data, rec), ("wide2", data, rec)])
    assert n <= lib.DUMP_BUDGET == 64 << 20
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= lib.DUMP_BUDGET + 4096


def test_device_slice_stays_inside_the_buffer():
    buf = types.SimpleNamespace(ptr=ctypes.c_void_p(0x10000), nbytes=1024)
    v = lib.device_slice(buf, 256, 768)
    assert v.ptr.value == 0x10000 + 256 and v.nbytes == 768
    with pytest.raises(AssertionError):
        lib.device_slice(buf, 512, 768)
