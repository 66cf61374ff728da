"""The surface of AW11 as a key encapsulation (include/rabe_host.h: rabe_aw11_{encaps,decaps}_packed; include/rabe_hip.h:
rhip_gt_multiexp_rows, rhip_aw11_decrypt_batch_w4): the symbols are declared and exported, the kernels live in the unit they belong to, the
Python wrappers exist.  No GPU needed."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_HOST = ("rabe_aw11_encaps_packed", "rabe_aw11_decaps_packed")
NEW_DEV = ("rhip_gt_multiexp_rows", "rhip_aw11_decrypt_batch_w4")


def header(name):
    return " ".join(open(os.path.join(ROOT, "include", name)).read().split())


def test_entry_points_are_declared_and_exported():
    from rabe_amd import build
    syms = set(build.declared_symbols())
    for name in NEW_HOST + NEW_DEV + ("rhip_aw11_decrypt_batch", "rhip_gt_pow_rows"):
        assert name in syms, name
    lib = ctypes.CDLL(build.build())
    for name in NEW_HOST + NEW_DEV:
        assert hasattr(lib, name), name
    assert not hasattr(lib, "rhip_gt_mexp4_run")          # the shared body is internal


def test_host_header_states_the_signatures_and_the_contracts():
    h = header("rabe_host.h")
    assert ("int32_t rabe_aw11_encaps_packed(rabe_host* h, const void* gk, const void* const* pks, size_t n_pks, const char* const* policies, "
            "size_t n_policies, int32_t language, size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, "
            "uint64_t* hdr_off /*[n_items+1]*/, uint8_t* key_buf /*32 n_items*/);") in h
    assert ("int32_t rabe_aw11_decaps_packed(rabe_host* h, const void* gk, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, "
            "const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);") in h
    assert "the AW11 KEM: rabe_aw11_encaps_packed, rabe_aw11_decaps_packed;" in h          # the SHARDED list
    assert "minus the AES nonce" in h and "neither read nor authenticated" in h
    assert "#define RABE_HOST_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "rabe_host.h")).read()          # additions only


def test_device_header_declares_the_multi_exponentiation():
    h = header("rabe_hip.h")
    assert ("int32_t rhip_gt_multiexp_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_gt* dev_a "
            "/*[n_rows]*/, const rhip_fr* dev_k /*[n_rows]*/, size_t n_items, const rhip_gt* dev_mul /*[n_items] or NULL*/, uint32_t flags, "
            "uint32_t chunk_terms /*0 = the engine's choice*/, rhip_gt* dev_out /*[n_items]*/);") in h
    assert "rhip_gt_pow + rhip_gt_product is the route" in h          # the membership precondition and the way round it
    assert "4 x 384 = 1536 bytes" in h          # the table's memory per row is stated


def test_kernels_live_in_the_gt_power_unit_and_the_yardstick_keeps_its_launches():
    from rabe_amd import build
    names = [os.path.basename(s) for s in build.SOURCES]
    csrc = os.path.join(ROOT, "rabe_amd", "csrc")
    unit = open(os.path.join(csrc, "engine_gtpow.hip")).read()
    for k in ("k_gtmexp4_digits", "k_gtmexp4_table", "k_gt_mexp4_partial", "k_gt_mexp4_finish", "gt_mexp4_chunk"):
        assert k in unit, k
    for other in names:
        if other.endswith(".hip") and other != "engine_gtpow.hip":
            assert "k_gt_mexp4" not in open(os.path.join(csrc, other)).read(), other
    jobs = open(os.path.join(csrc, "engine_jobs.hip")).read()
    assert jobs.count('KLAUNCH(ctx, "k_gt_multiexp_partial"') == 1 and jobs.count('KLAUNCH(ctx, "k_gt_lead"') == 1
    assert os.path.exists(os.path.join(csrc, "bn254", "gtmexp4.h"))
    chunks = open(os.path.join(csrc, "msm_chunks.h")).read()
    assert "rb_gtmexp4_chunks" not in chunks          # the sibling lives beside the routine it serves


def test_python_wrappers_exist():
    from rabe_amd import Engine
    from rabe_amd.schemes import aw11
    for fn in (aw11.encaps_packed, aw11.decaps_packed, Engine.gt_multiexp_rows):
        assert callable(fn)
    with pytest.raises(ValueError):
        Engine.gt_multiexp_rows(None, [b""], [0, 2], [b""])          # refused before the library is touched
