"""The surface of the proxy's call for a mixed queue, without a GPU (include/rabe_host.h: rabe_ghw11_tk_store_create, rabe_ghw11_tk_store_bytes,
rabe_ghw11_transform_keyed; include/rabe_hip.h: rhip_ghw11_transform_batch_keyed, rhip_g2_lines_bytes): both headers declare the functions
with their documented argument lists, the library exports exactly what the headers declare, the recorded table of rabe_*_packed symbols has
not grown, and the Python wrappers exist."""
import ctypes
import inspect
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NEW = ("rabe_ghw11_tk_store_create", "rabe_ghw11_tk_store_bytes", "rabe_ghw11_transform_keyed")
DEV_NEW = ("rhip_ghw11_transform_batch_keyed", "rhip_g2_lines_bytes")


def header(name):
    return " ".join(open(os.path.join(ROOT, "include", name)).read().split())


def test_both_headers_declare_the_new_functions():
    host, dev = header("rabe_host.h"), header("rabe_hip.h")
    assert ("int32_t rabe_ghw11_tk_store_create(rabe_host* h, size_t n_keys, const uint8_t* tk_blob, size_t tk_len, const uint64_t* tk_off /*[n_keys+1]*/, "
            "uint32_t flags, int32_t* key_status /*[n_keys]*/, void** store);") in host
    assert "uint64_t rabe_ghw11_tk_store_bytes(const void* store);" in host
    assert ("int32_t rabe_ghw11_transform_keyed(rabe_host* h, const void* store, size_t n_items, const uint32_t* item_key /*[n_items]*/, "
            "const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, "
            "uint8_t* tct_buf, size_t tct_cap);") in host
    assert "RABE_GHW11_TK_STORE = 47" in host
    assert "#define RABE_HOST_ABI_VERSION 5" in host          # additions only
    assert "const uint32_t* dev_item_line_base /*[n_items]*/, const uint32_t* dev_item_ok /*[n_items], may be NULL*/, const rhip_g2_lines* store_lines," in dev
    assert "size_t rhip_g2_lines_bytes(const rhip_g2_lines* p);" in dev
    # the keyed call takes rhip_ghw11_transform_batch's arguments, in its order, in front of its own three
    plain = " ".join(re.sub(r"/\*.*?\*/", "", dev).split())
    args = lambda fn: [a.strip() for a in plain[plain.index("int32_t %s(" % fn):].split(");")[0].split("(", 1)[1].split(",")]
    one, many = args("rhip_ghw11_transform_batch"), args("rhip_ghw11_transform_batch_keyed")
    assert many[:len(one) - 2] == one[:-2] and many[-1] == one[-1] and len(many) == len(one) + 2
    assert many[-4:-1] == ["const uint32_t* dev_item_line_base", "const uint32_t* dev_item_ok", "const rhip_g2_lines* store_lines"]


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


def test_null_arguments_are_refused_without_a_device():
    from rabe_amd import build
    lib = ctypes.CDLL(build.build())
    lib.rabe_ghw11_tk_store_bytes.restype = ctypes.c_uint64
    assert lib.rabe_ghw11_tk_store_bytes(None) == 0
    lib.rhip_g2_lines_bytes.restype = ctypes.c_size_t
    assert lib.rhip_g2_lines_bytes(None) == 0
    assert lib.rhip_ghw11_transform_batch_keyed(*([None] * 18)) == -3          # RHIP_ERR_ARG: no context


def test_python_wrappers_exist():
    from rabe_amd import engine, hostlib
    from rabe_amd.schemes import ghw11
    assert list(inspect.signature(ghw11.tk_store_create).parameters) == ["host", "tk_blob", "tk_off", "trusted"]
    assert list(inspect.signature(ghw11.transform_keyed).parameters) == ["host", "store", "item_key", "ct_blob", "ct_off", "trusted"]
    assert callable(ghw11.TkStore.nbytes) and callable(ghw11.TkStore.free)
    assert hostlib.KINDS["ghw11_tk_store"] == 47
    assert list(inspect.signature(engine.ghw11_transform_keyed_dev).parameters)[-4:] == ["d_item_line_base", "d_item_ok", "store_lines", "d_out"]
    assert callable(engine.G2Lines.nbytes)
