"""CPU-side checks of GHW11's bulk provisioning: include/rabe_host.h declares rabe_ghw11_provision_packed and include/rabe_hip.h
rhip_ghw11_provision_batch with their documented argument lists, the built library exports both, and rabe_amd.schemes.ghw11 /
rabe_amd.engine wrap them; the Python wrapper refuses an empty attribute list and an item_set out of range before it touches a device.
No compute is launched."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/%s" % (name, header)
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_provision_packed():
    assert declaration("rabe_host.h", "rabe_ghw11_provision_packed") == [
        "rabe_host* h", "const void* pk", "const void* msk", "const char* const* attributes", "const size_t* counts", "size_t n_sets",
        "size_t n_items", "const uint32_t* item_set", "uint8_t* sk_buf", "size_t sk_cap", "uint64_t* sk_off", "uint8_t* tk_buf", "size_t tk_cap",
        "uint64_t* tk_off", "uint8_t* rk_buf"]


def test_header_declares_provision_batch():
    assert declaration("rabe_hip.h", "rhip_ghw11_provision_batch") == [
        "rhip_ctx* ctx", "rhip_ghw11_keys* keys", "size_t n_items", "size_t n_rows", "const uint32_t* dev_item_row_off",
        "const uint32_t* dev_item_hash_off", "const rhip_fr* dev_hash", "const rhip_fr* dev_r", "const rhip_fr* dev_z", "rhip_g2* dev_out_sk",
        "rhip_g2* dev_out_tk", "uint32_t* dev_flags"]


def test_provision_header_states_the_draw_order():
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    doc = text[:text.index("int32_t rabe_ghw11_provision_packed")].rsplit("/*", 1)[1]
    assert "DRAW ORDER: r_0 .. r_{n-1}, then z_0 .. z_{n-1}" in doc and "z = 0 fails the whole call" in doc and "sk_off = NULL" in doc


def test_the_library_exports_both():
    from rabe_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "rabe_ghw11_provision_packed") and hasattr(lib, "rhip_ghw11_provision_batch")
    # the calls it is defined by keep their signatures
    assert declaration("rabe_host.h", "rabe_ghw11_keygen_packed")[-3:] == ["uint8_t* sk_buf", "size_t sk_cap", "uint64_t* sk_off"]
    assert declaration("rabe_hip.h", "rhip_ghw11_keygen_batch")[1] == "const rhip_ghw11_keys* keys"


def test_python_wrappers():
    from rabe_amd.schemes import ghw11
    from rabe_amd.engine import Engine, Ghw11Keys
    pv = inspect.signature(ghw11.provision_packed).parameters
    assert list(pv) == ["host", "pk", "msk", "sets", "item_set", "want_sk"] and pv["want_sk"].default is True
    dv = inspect.signature(Engine.ghw11_provision_dev).parameters
    assert list(dv) == ["self", "keys", "item_row_off", "item_hash_off", "hashes", "r", "z", "want_sk"] and dv["want_sk"].default is True
    assert list(inspect.signature(Ghw11Keys.__init__).parameters) == ["self", "eng", "g2", "g2_a", "g2_alpha"]


def test_wrapper_refuses_bad_lists_without_a_device():
    """host, pk and msk are None: a wrapper that reached the library (or a device) with them would fail otherwise"""
    from rabe_amd.schemes import ghw11
    with pytest.raises(ValueError, match="empty attribute list"):
        ghw11.provision_packed(None, None, None, [["A"], []], [0, 0])
    with pytest.raises(ValueError, match="empty attribute list"):
        ghw11.provision_packed(None, None, None, [["A"], []], [0, 0], want_sk=False)
    with pytest.raises(ValueError, match="item_set out of range"):
        ghw11.provision_packed(None, None, None, [["A"], ["B", "C"]], [0, 2])
    with pytest.raises(ValueError, match="item_set out of range"):
        ghw11.provision_packed(None, None, None, [["A"]], [0, -1])


def test_device_wrapper_checks_its_offsets_before_the_device():
    from rabe_amd.engine import Engine
    eng = Engine.__new__(Engine)                       # no context: the checks come first
    h = [bytes(32)] * 2
    with pytest.raises(ValueError, match="item_row_off"):
        eng.ghw11_provision_dev(None, [0, 3, 6], [0], h, [bytes(32)], [bytes(32)])
    with pytest.raises(ValueError, match="at least one attribute row"):
        eng.ghw11_provision_dev(None, [0, 2], [0], h, [bytes(32)], [bytes(32)])
    with pytest.raises(ValueError, match="inside `hashes`"):
        eng.ghw11_provision_dev(None, [0, 5], [0], h, [bytes(32)], [bytes(32)])
