"""CPU-side surface of the LSW one-key decrypt: both headers declare the new entry points, the built library exports them, and the Python
wrappers exist with the documented signatures.  No compute is launched."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rabe_amd import build
    return ctypes.CDLL(build.build())


def declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "%s does not declare %s" % (header, name)
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_headers_declare_the_one_sk_entry_points():
    dev = declaration("rabe_hip.h", "rhip_lsw_decrypt_batch_one_sk")
    # the selection groups are stated by the caller, the key's D2 rows come as prepared lines
    assert any("n_groups" in a for a in dev) and any("dev_group_off" in a for a in dev) and any("dev_item_group" in a for a in dev)
    assert any(a.startswith("const rhip_g2_lines*") for a in dev)
    host = declaration("rabe_host.h", "rabe_lsw_decrypt_one_sk_packed")
    assert host == ["rabe_host* h", "const void* sk", "size_t n_items", "const uint8_t* ct_blob", "size_t ct_len", "const uint64_t* ct_off",
                    "uint32_t flags", "int32_t* status", "uint8_t* pt_buf", "size_t pt_cap", "uint64_t* pt_off"]
    # the argument list of the bsw form: same conventions
    assert [a.split()[0:-1] for a in host] == [a.split()[0:-1] for a in declaration("rabe_host.h", "rabe_bsw_decrypt_packed")]


def test_abi_revision_is_unchanged():
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    assert re.search(r"#define\s+RABE_HOST_ABI_VERSION\s+5\b", text)


def test_library_exports_the_one_sk_entry_points(lib):
    for sym in ("rhip_lsw_decrypt_batch_one_sk", "rabe_lsw_decrypt_one_sk_packed"):
        assert hasattr(lib, sym), sym


def test_python_wrappers_have_the_documented_signatures():
    from rabe_amd import engine as E
    from rabe_amd.schemes import bsw, lsw
    sig = inspect.signature(lsw.decrypt_one_sk_packed)
    assert list(sig.parameters) == ["host", "sk", "ct_blob", "ct_off", "out", "trusted"]
    assert sig.parameters["out"].default is None and sig.parameters["trusted"].default is False
    assert list(sig.parameters) == list(inspect.signature(bsw.decrypt_packed).parameters)
    dev = list(inspect.signature(E.lsw_decrypt_one_sk_dev).parameters)
    assert dev[0] == "eng" and dev[-1] == "d_out"
    for name in ("n_groups", "d_group_off", "d_item_group", "sk_d2_lines"):
        assert name in dev
