"""bench.py on the GPU prints ONE stdout line -- the compact object the driver parses (benchkit/lib.py) -- and leaves the full object in
bench_detail.json; a short run of the default configuration with the informational legs switched off."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_compact_line_on_stdout_and_the_detail_beside_it():
    env = dict(os.environ, RABE_PAIRING_MODE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RABE_BENCH_FULL_LINE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--min-time", "0", "--full", "--cpu-sample", "2",
                          "--no-object-api", "--no-host-io-leg", "--no-single-batch", "--no-configs-leg", "--wide-window", "0"], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == 1 and len(lines[0]) < 4096, (len(lines), [len(l) for l in lines])
    d = json.loads(lines[0])
    assert d["metric"].startswith("ABE ops/sec") and d["value"] > 0 and d["n_gpus"] == 1 and d["steps"] == 4 and d["roundtrip_bit_exact"] is True
    rf, cb = d["roofline"], d["cpu_baseline"]
    assert rf["kernel"] and rf["kernel_ms"] > 0 and 0 < rf["frac"] < 1 and rf["peak"] > 0 and rf["traffic"] and os.path.exists(os.path.join(ROOT, rf["traffic_source"]))
    assert 0 < rf["frac_valu_issue"] < 1
    assert cb["value"] > 0 and cb["cores"] == 1 and cb["kind"] == "port"
    full = json.load(open(os.path.join(ROOT, "bench_detail.json")))
    assert full["value"] == d["value"] and full["roofline"]["kernels_ms"] and full["timed_regions"]["count"] >= 1
    assert out.stderr.decode().count("bench_detail: ") == 1


def _plain(out_dir, *extra):
    env = dict(os.environ, RABE_PAIRING_MODE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RABE_BENCH_FULL_LINE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
                         + list(extra), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("config, extra", [
    (2, ("--batch", "256", "--attrs", "8", "--g-window", "16")),
    (3, ("--batch", "64", "--attrs", "12", "--policies", "4")),
    (4, ("--batch", "64", "--attrs", "12", "--policies", "4")),
    (5, ("--batch", "64", "--attrs", "20", "--policies", "4")),
])
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_twice(tmp_path, config, extra):
    """a plain run: one timed region of exactly --steps steps, none of the --full legs, and the last step's outputs in --dump-outputs --
    the same files, value for value, from a second run with the same arguments"""
    import numpy as np
    runs = [_plain(tmp_path / str(i), "--config", str(config), *extra) for i in range(2)]
    d = runs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - d["config"]["batch_per_gpu"] * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    for k in ("roofline", "cpu_baseline", "configs", "roundtrip_bit_exact"):
        assert k not in d, k
    detail = json.load(open(os.path.join(ROOT, "bench_detail.json")))
    assert detail["timed_regions"]["count"] == 1 and detail["timed_regions"]["steps_each"] == 3
    for k in ("single_batch", "object_api", "host_io_leg", "value_wide_tables"):
        assert k not in detail, k
    names = sorted(os.listdir(tmp_path / "0"))
    assert names == sorted(os.listdir(tmp_path / "1")) and any(n.endswith("_decrypted_gt.npy") for n in names), names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "0" / n), np.load(tmp_path / "1" / n)
        assert a.dtype == np.float64 and a.ndim == 2 and a.shape[0] > 0, (n, a.dtype, a.shape)
        assert (a == b).all(), n
        assert (a >= 0).all() and (a < 2.0 ** 32).all() and (a == np.floor(a)).all() and a.any(), n
        total += os.path.getsize(tmp_path / "0" / n)
    assert total <= 64 << 20
    gt = np.load(tmp_path / "0" / [n for n in names if n.endswith("_decrypted_gt.npy")][0])
    assert gt.shape == (d["config"]["batch_per_gpu"], 96)
