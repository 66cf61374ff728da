"""CPU-side checks of the packed encrypt of the two DNF schemes: include/rabe_host.h declares rabe_bdabe_encrypt_packed and
rabe_mke08_encrypt_packed with their documented argument lists (tests/test_abi_exports.py then checks that the built library exports
them), include/rabe_hip.h declares the device-level rhip_dnf_* surface, and rabe_amd.schemes.bdabe / mke08 wrap the entry points.
No compute is launched."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["rabe_host* h", "const void* pk", "const void* const* attr_pks", "size_t n_pks", "const char* const* policies", "size_t n_policies",
        "int32_t language", "size_t n_items", "const uint32_t* item_policy", "const uint8_t* pt_blob", "const uint64_t* pt_off", "uint8_t* ct_buf",
        "size_t ct_cap", "uint64_t* ct_off"]


def declaration(name):
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/rabe_host.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("scheme", ["bdabe", "mke08"])
def test_header_declares_encrypt_packed(scheme):
    assert declaration("rabe_%s_encrypt_packed" % scheme) == ARGS


def test_device_level_surface_is_declared():
    text = open(os.path.join(ROOT, "include", "rabe_hip.h")).read()
    for name in ("rhip_dnf_pk_create", "rhip_dnf_pk_destroy", "rhip_dnf_terms_create", "rhip_dnf_terms_destroy", "rhip_dnf_encrypt_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name


@pytest.mark.parametrize("scheme", ["bdabe", "mke08"])
def test_python_wrappers(scheme):
    import importlib
    from rabe_amd import hostlib
    mod = importlib.import_module("rabe_amd.schemes." + scheme)
    p = inspect.signature(mod.encrypt_packed).parameters
    assert list(p) == ["host", "pk", "attr_pks", "policies", "item_policy", "pt_blob", "pt_off", "language", "out"]
    assert p["language"].default == hostlib.JSON_POLICY and p["out"].default is None
