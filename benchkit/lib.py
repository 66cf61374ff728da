"""Shared plumbing of bench.py's configurations: group splitting, repeated exactly-K-step timed regions, rank-consistent
loop control, torch-owned device buffers.  Measurement only -- no group arithmetic here."""
import ctypes
import json
import sys
import time

G1_GEN = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")
G2_GEN = b"".join(int(v).to_bytes(32, "little") for v in (
    10857046999023057135944570762232829481370756359578518086990519993285655852781,
    11559732032986387107991004021392285783925812861821192530917403151452391805634,
    8495653923123431417604973247489272438418190587263600148770280649306958101930,
    4082367875863433681332203403145435568316851327593401208105741076214120093531))
MAC_PER_FPMUL = 136          # 8-limb Montgomery multiplication: 2 * 8^2 + 8 32x32 multiply-adds


class ExtBuf:
    """A device buffer owned by a torch tensor (so that torch.distributed can gather it), seen as an engine buffer."""

    def __init__(self, torch_mod, nbytes, device):
        self.t = torch_mod.empty(max(int(nbytes), 4), dtype=torch_mod.uint8, device=device)
        self.ptr = ctypes.c_void_p(self.t.data_ptr())
        self.nbytes = int(nbytes)


def split_steps(k, gmax):
    """K steps -> group sizes: full groups of gmax first, the remainder last (a full group fills the chip exactly; for the
    driver's 20 steps 16 + 4 measures 982 k ops/s against 965 k for 10 + 10 and 959 k for one group of 20)."""
    sizes = [gmax] * (k // gmax)
    if k % gmax:
        sizes.append(k % gmax)
    return sizes


def warmup_schedule(sizes, lanes, steps):
    """--warmup W: (group sizes of one warm-up pass, passes).  A pass is the timed schedule's first `lanes` groups (one per group in flight)
    and its remainder group, so that every launch shape, lane, buffer and the remainder's overlap have run once before the timed region;
    passes are repeated until W steps are covered (0 passes for W = 0)."""
    one = list(sizes[:lanes])
    if len(sizes) > lanes and sizes[-1] != sizes[0]:
        one.append(sizes[-1])
    return one, (-(-steps // sum(one)) if steps > 0 else 0)


def device_slice(buf, offset, nbytes):
    """bytes [offset, offset + nbytes) of an engine buffer (DevBuf), as a buffer Engine.download accepts"""
    import types
    assert 0 <= offset and 0 <= nbytes and offset + nbytes <= buf.nbytes, (offset, nbytes, buf.nbytes)
    return types.SimpleNamespace(ptr=ctypes.c_void_p(buf.ptr.value + offset), nbytes=nbytes)


DUMP_BUDGET = 64 << 20          # bytes of .npy data that --dump-outputs may write in all
DUMP_MAX_RECORDS = 16384        # records kept per array; a larger output is cut to a fixed, seeded sample of its records
DUMP_SEED = 20251016


def dump_outputs(out_dir, arrays):
    """--dump-outputs DIR: every (name, data, record_bytes) -> DIR/<name>.npy, float64 of shape (records, record_bytes / 4): the
    little-endian 32-bit words of every record (exact in float64).  An array of more than DUMP_MAX_RECORDS records (fewer if the total
    would pass DUMP_BUDGET) keeps the records at a fixed, seeded sample of indices, in index order; the sample depends only on the record
    count, so two builds run with the same arguments write comparable files."""
    import os
    import numpy as np
    per_record = sum(8 * (rb // 4) for _, _, rb in arrays)
    cap = max(1, min(DUMP_MAX_RECORDS, DUMP_BUDGET // max(1, per_record)))
    os.makedirs(out_dir, exist_ok=True)
    written = 0
    for name, data, rb in arrays:
        assert rb % 4 == 0 and len(data) % rb == 0, (name, len(data), rb)
        words = np.frombuffer(data, dtype="<u4").reshape(-1, rb // 4)
        if words.shape[0] > cap:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(words.shape[0], cap, replace=False))
            words = words[idx]
        a = words.astype(np.float64)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written += a.nbytes
    assert written <= DUMP_BUDGET, written
    return written


def same_on_all_ranks(flag):
    """rank 0's decision, everywhere (loop control of the repeated timed regions)"""
    import torch
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized():
        return bool(flag)
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
    dist.broadcast(t, src=0)
    return bool(t.item())


def timed_regions(run_steps, sync_all, min_time, max_regions=200):
    """Repeats the region [barrier, run_steps() = exactly K steps, synchronize, barrier] until min_time seconds are covered;
    returns the list of max-over-ranks region times."""
    import torch
    import torch.distributed as dist
    from rabe_amd import shard

    def barrier():
        if dist.is_available() and dist.is_initialized():
            dist.barrier()

    regions = []
    while True:
        barrier()
        t0 = time.perf_counter()
        run_steps()
        sync_all()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        barrier()
        regions.append(shard.max_over_ranks(t1 - t0))
        if not same_on_all_ranks(sum(regions) < min_time and len(regions) < max_regions):
            break
    return regions


def regions_summary(regions, steps):
    mean = sum(regions) / len(regions)
    return {"count": len(regions), "steps_each": steps, "ms_min": round(1e3 * min(regions), 3), "ms_mean": round(1e3 * mean, 3),
            "ms_max": round(1e3 * max(regions), 3),
            "note": "every region times exactly --steps steps between barrier + synchronize; repeated until --min-time s are covered; value uses the mean"}


def cpu_model():
    """model name of the host CPU (stated with every CPU number)"""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


# ---------------------------------------------------------------------------------------------------------------- the printed line
# The driver keeps a bounded tail of stdout and parses its LAST line: round 5's 20 KB object did not survive that (BENCH_r05.parsed =
# null).  So stdout carries ONE compact JSON line (<= COMPACT_LIMIT bytes, the contract's keys + `roofline` + `cpu_baseline` + the
# headline's neighbours + configs 3-5); everything else -- prose notes, the object-level legs, ragged legs, per-kernel maps -- goes to
# bench_detail.json beside the script (and under gpurun_out/ when that exists) and, as one line, to STDERR.
COMPACT_LIMIT = 4096
_CONFIG_KEYS = ("workload", "batch_per_gpu", "attrs", "policies", "steps_per_launch_set", "parallelism", "device", "pairing_mode",
                "launch_sets_in_flight", "tree", "ragged")
_ROOFLINE_KEYS = ("bound", "kernel", "kernel_ms", "items_per_launch", "achieved", "peak", "unit", "frac", "frac_survey", "frac_valu_issue", "achieved_survey",
                  "traffic", "traffic_source", "kernels_ms_sum_per_step")
_CPU_KEYS = ("value", "unit", "cores", "cpu_model", "kind", "sample", "error")


def _num(v):
    """strict JSON has no NaN / Infinity: they become null"""
    if isinstance(v, float) and (v != v or v in (float("inf"), float("-inf"))):
        return None
    return v


def _clean(o):
    if isinstance(o, dict):
        return {str(k): _clean(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_clean(v) for v in o]
    return _num(o)


def _short(s, n):
    s = str(s)
    return s if len(s) <= n else s[:n - 1].rstrip() + "~"


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact_line(result):
    """The driver-parseable form of a bench result: contract keys, `roofline`, `cpu_baseline`, neighbours, configs 3-5.  Prose is cut to a
    few dozen characters; whatever does not fit COMPACT_LIMIT is dropped from the least important end (never the contract keys)."""
    r = _clean(result)
    out = {}
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline"):
        out[k] = r.get(k)
    out["dtype"] = _short(r.get("dtype", ""), 24)
    out["data"] = r.get("data")
    if "roundtrip_bit_exact" in r:
        out["roundtrip_bit_exact"] = r["roundtrip_bit_exact"]
    cfg = r.get("config") if isinstance(r.get("config"), dict) else {}
    c = _pick(cfg, _CONFIG_KEYS)
    if "workload" in c:
        c["workload"] = _short(c["workload"], 150)
    if "parallelism" in c:
        c["parallelism"] = _short(c["parallelism"], 60)
    out["config"] = c
    rf = r.get("roofline")
    if isinstance(rf, dict):
        o = _pick(rf, _ROOFLINE_KEYS)
        if "bound" in o:
            o["bound"] = _short(o["bound"], 64)
        if "traffic" not in o:
            o["traffic"] = None
        out["roofline"] = o
    cb = r.get("cpu_baseline")
    if isinstance(cb, dict):
        o = _pick(cb, _CPU_KEYS)
        if "sample" in o:
            o["sample"] = _short(o["sample"], 96)
        out["cpu_baseline"] = o
    mc = r.get("cpu_baseline_multicore")
    if isinstance(mc, dict) and "value" in mc:
        out["cpu_baseline_multicore"] = _pick(mc, ("value", "cores"))
    for k in ("value_lone_batch", "value_end_to_end", "value_end_to_end_inflight2"):
        if r.get(k) is not None:
            out[k] = r[k]
    if isinstance(r.get("gather"), dict):          # every field but prose: backend, collective, bytes, ms, matches_unsharded_order
        out["gather"] = {k: (v if not isinstance(v, str) else _short(v, 40)) for k, v in r["gather"].items()
                         if not isinstance(v, (dict, list)) and k not in ("note",)}
    cfs = r.get("configs")
    if isinstance(cfs, dict):
        oc = {}
        for k in sorted(cfs):
            v = cfs[k]
            if not isinstance(v, dict):
                continue
            if "error" in v and "value" not in v:
                oc[k] = {"error": _short(v["error"], 60)}
                continue
            rr = v.get("roofline") if isinstance(v.get("roofline"), dict) else {}
            e = {"value": v.get("value"), "ms_per_step": v.get("ms_per_step"), "steps": v.get("steps"), "batch_per_gpu": v.get("batch_per_gpu"),
                 "kernel_ms": rr.get("kernel_ms"), "frac": rr.get("frac"), "frac_survey": rr.get("frac_survey"),
                 "roundtrip_bit_exact": v.get("roundtrip_bit_exact")}
            if isinstance(v.get("cpu_baseline"), dict):
                e["cpu_baseline"] = _pick(v["cpu_baseline"], ("value", "cores", "kind"))
            oc[k] = {kk: vv for kk, vv in e.items() if vv is not None}
        out["configs"] = oc
    out["detail"] = "bench_detail.json"

    def size():
        return len(json.dumps(out, allow_nan=False, separators=(",", ":")))
    # shrink from the least important end; the contract keys, roofline and cpu_baseline are never touched
    if size() > COMPACT_LIMIT and "configs" in out:
        for k in [k for k in list(out["configs"]) if not k.isdigit()]:          # ragged / mixed neighbours of the BASELINE configs first
            del out["configs"][k]
            if size() <= COMPACT_LIMIT:
                break
    for k in ("cpu_baseline_multicore", "gather", "configs"):
        if size() > COMPACT_LIMIT and k in out:
            del out[k]
    if size() > COMPACT_LIMIT and "sample" in out.get("cpu_baseline", {}):
        del out["cpu_baseline"]["sample"]
    assert size() <= COMPACT_LIMIT, size()
    return out


def write_detail(result, root=None):
    """bench_detail.json: the full result object (every leg, every note) -- beside bench.py and, on a gpurun box, under gpurun_out/"""
    import os
    root = root or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = json.dumps(_clean(result), allow_nan=False)
    written = []
    for d in (root, os.path.join(root, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_detail.json"), "w") as f:
                    f.write(text + "\n")
                written.append(d)
            except OSError:
                pass
    return text, written


def emit_line(result):
    """rank 0's ONE JSON line, as the LAST line of stdout (and the only JSON on stdout): RCCL writes a version banner through C stdio,
    which would otherwise be flushed at exit -- after the line (found on the GPU box, RABE_FORCE_DIST run) -- so everything buffered is
    flushed first.  The full object goes to bench_detail.json and to stderr."""
    import ctypes
    import os
    if os.environ.get("RABE_BENCH_FULL_LINE"):          # a sub-run of bench.py's configs leg: the parent reads the whole object from the pipe
        sys.stdout.flush()
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(_clean(result), allow_nan=False), flush=True)
        return
    text, _ = write_detail(result)
    sys.stdout.flush()
    print("bench_detail: " + text, file=sys.stderr, flush=True)
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(compact_line(result), allow_nan=False, separators=(",", ":")), flush=True)
