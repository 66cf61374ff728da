"""CPU-side checks of GHW11's packed service entry points: include/rabe_host.h declares rabe_ghw11_encrypt_packed and
rabe_ghw11_decrypt_out_packed with their documented argument lists (tests/test_abi_exports.py then checks that the built
library exports them), and rabe_amd.schemes.ghw11 wraps both.  No compute is launched."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declaration(name):
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/rabe_host.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_encrypt_packed():
    assert declaration("rabe_ghw11_encrypt_packed") == [
        "rabe_host* h", "const void* pk", "const char* const* policies", "size_t n_policies", "int32_t language", "size_t n_items",
        "const uint32_t* item_policy", "const uint8_t* pt_blob", "const uint64_t* pt_off", "uint8_t* ct_buf", "size_t ct_cap", "uint64_t* ct_off"]


def test_header_declares_decrypt_out_packed():
    assert declaration("rabe_ghw11_decrypt_out_packed") == [
        "rabe_host* h", "const void* rk", "size_t n_items", "const uint8_t* tct_buf", "const uint8_t* ct_blob", "size_t ct_len",
        "const uint64_t* ct_off", "uint32_t flags", "int32_t* status", "uint8_t* pt_buf", "size_t pt_cap", "uint64_t* pt_off"]


def test_device_level_surface_is_declared():
    text = open(os.path.join(ROOT, "include", "rabe_hip.h")).read()
    for name in ("rhip_ghw11_pk_create", "rhip_ghw11_pk_destroy", "rhip_ghw11_encrypt_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_python_wrappers():
    from rabe_amd.schemes import ghw11
    enc = inspect.signature(ghw11.encrypt_packed).parameters
    assert list(enc)[:7] == ["host", "pk", "policies", "item_policy", "pt_blob", "pt_off", "language"]
    dec = inspect.signature(ghw11.decrypt_out_packed).parameters
    assert list(dec) == ["host", "rk", "tct", "ct_blob", "ct_off", "trusted"]
    assert dec["trusted"].default is False
