"""CPU-side checks of GHW11's bulk key issuing: include/rabe_host.h declares rabe_ghw11_keygen_packed and rabe_ghw11_tkgen_packed with their
documented argument lists (tests/test_abi_exports.py then checks that the built library exports them), include/rabe_hip.h declares the
device-level entry points, and rabe_amd.schemes.ghw11 / rabe_amd.engine wrap them.  No compute is launched."""
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


def test_header_declares_keygen_packed():
    assert declaration("rabe_ghw11_keygen_packed") == [
        "rabe_host* h", "const void* pk", "const void* msk", "const char* const* attributes", "const size_t* counts", "size_t n_sets",
        "size_t n_items", "const uint32_t* item_set", "uint8_t* sk_buf", "size_t sk_cap", "uint64_t* sk_off"]


def test_header_declares_tkgen_packed():
    assert declaration("rabe_ghw11_tkgen_packed") == [
        "rabe_host* h", "size_t n_items", "const uint8_t* sk_blob", "size_t sk_len", "const uint64_t* sk_off", "uint32_t flags",
        "int32_t* status", "uint8_t* tk_buf", "size_t tk_cap", "uint64_t* tk_off", "uint8_t* rk_buf"]


def test_header_declares_fr_split4():
    assert declaration("rabe_fr_split4") == ["const uint8_t k[32]", "uint8_t mag[4][16]", "uint8_t neg[4]"]


def test_tkgen_header_states_the_draw_order():
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    doc = text[:text.index("int32_t rabe_ghw11_tkgen_packed")].rsplit("/*", 1)[1]
    assert "DRAW ORDER" in doc and "decodes ON THE HOST" in doc and "z = 0" in doc


def test_device_level_surface_is_declared():
    text = open(os.path.join(ROOT, "include", "rabe_hip.h")).read()
    for name in ("rhip_ghw11_keygen_batch", "rhip_ghw11_keys_create", "rhip_ghw11_keys_destroy", "rhip_g2_mul_rows"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    # the existing create function keeps its signature
    assert re.search(r"rhip_ghw11_pk_create\(rhip_ctx\* ctx, const rhip_g1\* host_g1, const rhip_g1\* host_g1_a, const rhip_gt\* host_e_gg_alpha, "
                     r"rhip_ghw11_pk\*\* out\)", text)


def test_python_wrappers():
    from rabe_amd.schemes import ghw11
    from rabe_amd.engine import Engine
    kg = inspect.signature(ghw11.keygen_packed).parameters
    assert list(kg) == ["host", "pk", "msk", "attr_sets", "item_set", "out"] and kg["out"].default is None
    tk = inspect.signature(ghw11.tkgen_packed).parameters
    assert list(tk) == ["host", "sk_blob", "sk_off", "trusted"] and tk["trusted"].default is False
    assert list(inspect.signature(Engine.g2_mul_rows).parameters) == ["self", "points", "item_row_off", "scalars"]


def test_new_unit_is_built():
    from rabe_amd import build
    assert any(os.path.basename(s) == "engine_keys.hip" for s in build.SOURCES)
    assert [os.path.basename(s) for s in build.DEVICE_SOURCES] == ["engine.hip", "engine_jobs.hip", "engine_coop.hip", "engine_coop_w1.hip", "engine_rr.hip"]
