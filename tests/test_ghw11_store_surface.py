"""The surface of the GHW11 key store that adds and revokes keys in place, without a GPU (include/rabe_host.h: rabe_ghw11_tk_store_open, _add,
_revoke, _stat; include/rabe_hip.h: rhip_g2_lines_reserve, _prepare_range, _scrub_range, _range_is_zero): both headers declare the eight
functions with their documented argument lists, the library exports exactly what the headers declare, the ABI version and the object kind
have not moved, the recorded table of rabe_*_packed symbols has not grown, the Python wrappers exist, and null arguments are refused before
any device is touched."""
import ctypes
import inspect
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NEW = ("rabe_ghw11_tk_store_open", "rabe_ghw11_tk_store_add", "rabe_ghw11_tk_store_revoke", "rabe_ghw11_tk_store_stat")
DEV_NEW = ("rhip_g2_lines_reserve", "rhip_g2_lines_prepare_range", "rhip_g2_lines_scrub_range", "rhip_g2_lines_range_is_zero")
RHIP_ERR_ARG = -3


def header(name):
    return " ".join(open(os.path.join(ROOT, "include", name)).read().split())


def test_both_headers_declare_the_eight_functions():
    host, dev = header("rabe_host.h"), header("rabe_hip.h")
    assert "int32_t rabe_ghw11_tk_store_open(rabe_host* h, uint64_t capacity_blocks, void** store);" in host
    assert ("int32_t rabe_ghw11_tk_store_add(rabe_host* h, void* store, size_t n_keys, const uint8_t* tk_blob, size_t tk_len, "
            "const uint64_t* tk_off /*[n_keys+1]*/, uint32_t flags, int32_t* key_status /*[n_keys]*/, uint32_t* key_id /*[n_keys]*/);") in host
    assert "int32_t rabe_ghw11_tk_store_revoke(rabe_host* h, void* store, size_t n, const uint32_t* key_id, int32_t* status /*[n]*/);" in host
    assert "int32_t rabe_ghw11_tk_store_stat(const void* store, uint64_t out[4]);" in host
    assert "int32_t rhip_g2_lines_reserve(rhip_ctx* ctx, size_t capacity, rhip_g2_lines** out);" in dev
    assert "int32_t rhip_g2_lines_prepare_range(rhip_ctx* ctx, rhip_g2_lines* lines, size_t first, size_t n, const rhip_g2* dev_q);" in dev
    assert "int32_t rhip_g2_lines_scrub_range(rhip_ctx* ctx, rhip_g2_lines* lines, size_t first, size_t n);" in dev
    assert "int32_t rhip_g2_lines_range_is_zero(rhip_ctx* ctx, const rhip_g2_lines* lines, size_t first, size_t n, int32_t* out_zero);" in dev
    assert "RABE_GHW11_TK_STORE = 47" in host
    assert "#define RABE_HOST_ABI_VERSION 5" in host          # additions only
    assert "The store is immutable" not in host


def test_exports_are_the_headers_and_no_packed_name_was_added():
    from rabe_amd import build
    syms = build.declared_symbols()
    for name in HOST_NEW + DEV_NEW:
        assert name in syms, name
    lib_path = build.build()
    lib = ctypes.CDLL(lib_path)
    for name in HOST_NEW + DEV_NEW:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, stdout=subprocess.PIPE).stdout.decode()
    exported = sorted(line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip() and line.split()[-1] != "RABE_AMD")
    assert exported == syms
    recorded = set(json.load(open(os.path.join(ROOT, "tests", "golden", "packed_abi_contract.json"))))
    packed = {s for s in syms if s.startswith("rabe_") and s.endswith("_packed")}
    assert packed <= recorded, sorted(packed - recorded)
    assert not any(name.endswith("_packed") for name in HOST_NEW)
    lib.rabe_host_abi_version.restype = ctypes.c_uint32
    assert lib.rabe_host_abi_version() == 5


def test_null_arguments_are_refused_without_a_device():
    from rabe_amd import build
    lib = ctypes.CDLL(build.build())
    out = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert lib.rabe_ghw11_tk_store_stat(None, out) != 0 and list(out) == [7, 7, 7, 7]
    handle = ctypes.c_void_p()
    assert lib.rabe_ghw11_tk_store_open(None, ctypes.c_uint64(16), ctypes.byref(handle)) == -1 and not handle.value
    assert lib.rabe_ghw11_tk_store_add(None, None, ctypes.c_size_t(0), None, ctypes.c_size_t(0), None, ctypes.c_uint32(0), None, None) == -1
    assert lib.rabe_ghw11_tk_store_revoke(None, None, ctypes.c_size_t(0), None, None) == -1
    sz = ctypes.c_size_t
    assert lib.rhip_g2_lines_reserve(None, sz(4), ctypes.byref(handle)) == RHIP_ERR_ARG and not handle.value
    assert lib.rhip_g2_lines_prepare_range(None, None, sz(0), sz(0), None) == RHIP_ERR_ARG
    assert lib.rhip_g2_lines_scrub_range(None, None, sz(0), sz(0)) == RHIP_ERR_ARG
    zero = ctypes.c_int32(5)
    assert lib.rhip_g2_lines_range_is_zero(None, None, sz(0), sz(0), ctypes.byref(zero)) == RHIP_ERR_ARG and zero.value == 5


def test_python_wrappers_exist():
    from rabe_amd import engine, hostlib
    from rabe_amd.schemes import ghw11
    assert list(inspect.signature(ghw11.tk_store_open).parameters) == ["host", "capacity_blocks"]
    assert list(inspect.signature(ghw11.TkStore.add).parameters) == ["self", "tk_blob", "tk_off", "trusted"]
    assert inspect.signature(ghw11.TkStore.add).parameters["trusted"].default is False
    assert list(inspect.signature(ghw11.TkStore.revoke).parameters) == ["self", "ids"]
    assert list(inspect.signature(ghw11.TkStore.stat).parameters) == ["self"]
    assert hostlib.KINDS["ghw11_tk_store"] == 47
    assert list(inspect.signature(engine.G2Lines.reserve).parameters) == ["eng", "capacity"]
    assert list(inspect.signature(engine.G2Lines.prepare_range).parameters) == ["self", "first", "n", "dq"]
    assert list(inspect.signature(engine.G2Lines.scrub_range).parameters) == ["self", "first", "n"]
    assert list(inspect.signature(engine.G2Lines.range_is_zero).parameters) == ["self", "first", "n"]
    lib = hostlib._lib()
    assert lib.rabe_ghw11_tk_store_open.argtypes[1] is ctypes.c_uint64
