"""CPU-side checks of the bulk key issuing of BDABE / MKE08: include/rabe_host.h declares the four packed calls with their documented argument
lists (tests/test_abi_exports.py then checks that the built library exports them), include/rabe_hip.h declares the device-level entry points,
and rabe_amd.schemes.{bdabe,mke08} / rabe_amd.engine wrap them.  No compute is launched."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declaration(name, header="rabe_host.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/%s" % (name, header)
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name, key", [("rabe_bdabe_keygen_packed", "ska"), ("rabe_mke08_keygen_packed", "msk")])
def test_header_declares_keygen_packed(name, key):
    assert declaration(name) == ["rabe_host* h", "const void* pk", "const void* %s" % key, "const char* const* names", "size_t n_items", "uint8_t* uk_buf",
                                 "size_t uk_cap", "uint64_t* uk_off"]


@pytest.mark.parametrize("name", ["rabe_bdabe_request_attribute_sk_packed", "rabe_mke08_request_authority_sk_packed"])
def test_header_declares_request_sk_packed(name):
    assert declaration(name) == [
        "rabe_host* h", "const void* ska", "const char* const* attributes", "const size_t* counts", "size_t n_sets", "size_t n_items",
        "const uint32_t* item_set", "const uint8_t* upk_blob", "size_t upk_len", "const uint64_t* upk_off", "uint32_t flags", "int32_t* status",
        "uint8_t* out_buf", "size_t out_cap", "uint64_t* out_off"]


def test_device_level_surface_is_declared():
    assert declaration("rhip_g1_mul_rows", "rabe_hip.h") == [
        "rhip_ctx* ctx", "size_t n_rows", "const uint32_t* dev_item_row_off", "const rhip_g1* dev_p", "size_t n_items", "const rhip_fr* dev_k",
        "rhip_g1* dev_out"]
    # the G2 entry point of the parent keeps its signature; the indexed forms sit beside it
    assert declaration("rhip_g2_mul_rows", "rabe_hip.h") == [
        "rhip_ctx* ctx", "size_t n_rows", "const uint32_t* dev_item_row_off", "const rhip_g2* dev_p", "size_t n_items", "const rhip_fr* dev_k",
        "rhip_g2* dev_out"]
    for g in ("g1", "g2"):
        assert declaration("rhip_%s_mul_rows_at" % g, "rabe_hip.h") == [
            "rhip_ctx* ctx", "size_t n_rows", "const uint32_t* dev_item_row_off", "const rhip_%s* dev_p" % g, "const uint32_t* dev_row_src", "size_t n_items",
            "const rhip_fr* dev_k", "const uint32_t* dev_row_dst", "rhip_%s* dev_out" % g]
    text = open(os.path.join(ROOT, "include", "rabe_hip.h")).read()
    for name in ("rhip_dnf_keys_create", "rhip_dnf_keys_destroy", "rhip_dnf_keygen_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_python_wrappers():
    from rabe_amd.engine import Engine
    from rabe_amd.schemes import bdabe, mke08
    assert list(inspect.signature(bdabe.keygen_packed).parameters) == ["host", "pk", "ska", "names", "out"]
    assert list(inspect.signature(mke08.keygen_packed).parameters) == ["host", "pk", "msk", "names", "out"]
    for fn in (bdabe.request_attribute_sk_packed, mke08.request_authority_sk_packed):
        p = inspect.signature(fn).parameters
        assert list(p) == ["host", "ska", "attr_sets", "item_set", "upk_blob", "upk_off", "trusted"] and p["trusted"].default is False
    assert list(inspect.signature(Engine.g1_mul_rows).parameters) == ["self", "points", "item_row_off", "scalars"]


@pytest.mark.parametrize("mod", ["bdabe", "mke08"])
def test_public_user_key_record_cuts_name_u1_u2(mod):
    import importlib
    m = importlib.import_module("rabe_amd.schemes." + mod)
    for name in (b"", b"u1", "zü".encode("utf-8") * 40):
        upk = len(name).to_bytes(4, "little") + name + bytes(range(64)) + bytes(range(128))
        tail = (2).to_bytes(4, "little") + b"rows that follow"
        assert m.public_user_key_record(b"\x11" * 64 + b"\x22" * 128 + upk + tail) == upk
    with pytest.raises(ValueError):
        m.public_user_key_record(b"\x00" * 100)
    with pytest.raises(ValueError):
        m.public_user_key_record(b"\x00" * 192 + (500).to_bytes(4, "little") + b"short")


def test_docs_name_the_new_calls():
    for doc in ("docs/boundary.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in ("rabe_bdabe_keygen_packed", "rabe_mke08_keygen_packed", "rabe_bdabe_request_attribute_sk_packed", "rabe_mke08_request_authority_sk_packed"):
            assert name in text, (doc, name)
    kernels = open(os.path.join(ROOT, "docs", "kernels.md")).read()
    for k in ("k_g1_mul_rows", "k_glv_masks", "k_g2_mul_rows_at", "k_dnf_keygen_g1", "k_dnf_keygen_g2"):
        assert k in kernels, k
