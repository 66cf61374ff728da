"""The surface of GHW11 as a key encapsulation (include/rabe_host.h: rabe_ghw11_{encaps,decaps_out,decaps}_packed; include/rabe_hip.h:
rhip_gt_pow_rows): the symbols are declared and exported, the new translation unit is built, the Python wrappers exist -- no GPU needed --
and, on a device, the null and short-buffer contracts of the three calls."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("rabe_ghw11_encaps_packed", "rabe_ghw11_decaps_out_packed", "rabe_ghw11_decaps_packed")


def header(name):
    return " ".join(open(os.path.join(ROOT, "include", name)).read().split())


def test_entry_points_are_declared_and_exported():
    from rabe_amd import build
    syms = set(build.declared_symbols())
    for name in NEW + ("rhip_gt_pow_rows", "rhip_gt_pow"):
        assert name in syms, name
    lib = ctypes.CDLL(build.build())
    for name in NEW + ("rhip_gt_pow_rows",):
        assert hasattr(lib, name), name
    assert "RHIP_GT_POW_INVERT" not in syms          # a macro, not a symbol


def test_host_header_states_the_signatures_and_the_contracts():
    h = header("rabe_host.h")
    assert ("int32_t rabe_ghw11_encaps_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, "
            "size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap, uint64_t* hdr_off /*[n_items+1]*/, "
            "uint8_t* key_buf /*32 n_items*/);") in h
    assert ("int32_t rabe_ghw11_decaps_out_packed(rabe_host* h, const void* rk, size_t n_items, const uint8_t* tct_buf /*768 n_items*/, "
            "uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);") in h
    assert ("int32_t rabe_ghw11_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, "
            "const uint64_t* ct_off /*[n_items+1]*/, uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);") in h
    assert "minus the AES nonce" in h and "its key is UNSPECIFIED" in h
    assert "the headers rabe_ghw11_encaps_packed writes" in h          # transform_packed's comment says that headers pass through it
    assert "#define RABE_HOST_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "rabe_host.h")).read()          # additions only


def test_device_header_declares_the_row_power():
    h = header("rabe_hip.h")
    assert ("int32_t rhip_gt_pow_rows(rhip_ctx* ctx, size_t n_rows, const uint32_t* dev_item_row_off /*[n_items+1]*/, const rhip_gt* dev_a "
            "/*[n_rows]*/, size_t n_items, const rhip_fr* dev_k /*[n_items]*/, const rhip_gt* dev_mul /*[n_rows] or NULL*/, uint32_t flags, "
            "rhip_gt* dev_out /*[n_rows]*/);") in h
    assert "#define RHIP_GT_POW_INVERT 1u" in h
    assert "the result is NOT a^k" in h          # the membership precondition is stated as it is for rhip_g2_mul_rows


def test_new_unit_is_built_and_the_measured_units_are_not_touched():
    from rabe_amd import build
    names = [os.path.basename(s) for s in build.SOURCES]
    assert "engine_gtpow.hip" in names
    assert [os.path.basename(s) for s in build.DEVICE_SOURCES] == ["engine.hip", "engine_jobs.hip", "engine_coop.hip", "engine_coop_w1.hip", "engine_rr.hip"]
    unit = open(os.path.join(ROOT, "rabe_amd", "csrc", "engine_gtpow.hip")).read()
    assert "k_gt_pow_rows" in unit and "gt_pow_split4" in unit
    for other in names:
        if other.endswith(".hip") and other != "engine_gtpow.hip":
            assert "k_gt_pow_rows" not in open(os.path.join(ROOT, "rabe_amd", "csrc", other)).read(), other


def test_python_wrappers_exist():
    from rabe_amd import Engine
    from rabe_amd.schemes import ghw11
    for fn in (ghw11.encaps_packed, ghw11.decaps_out_packed, ghw11.decaps_packed, Engine.gt_pow_rows):
        assert callable(fn)
    with pytest.raises(ValueError):
        ghw11.decaps_out_packed(None, None, bytes(767))          # refused before the library is touched


@pytest.mark.gpu
def test_null_and_short_buffer_contracts():
    import numpy as np
    from rabe_amd import hostlib as hl
    from rabe_amd.schemes import ghw11
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    host = hl.Host(0)
    try:
        pk, msk = ghw11.setup(host)
        sk = ghw11.keygen(host, pk, msk, ["A", "B"])
        _tk, rk = ghw11.tkgen(host, sk)
        pols = ['{"name": "A"}', '{"name": "and", "children": [{"name": "A"}, {"name": "B"}]}']
        item_pol = [0, 1, 0]
        tape = list(range(7, 7 + 3 + 5 + 3))          # exactly the draws of one call
        assert all(0 < v < R for v in tape)
        host.set_tape(tape)
        want_hdr, want_off, want_keys = ghw11.encaps_packed(host, pk, pols, item_pol)
        want_hdr, want_keys = want_hdr.copy(), want_keys.copy()
        need = int(want_off[3])
        arr, npol = hl._strs(pols)
        ip = np.ascontiguousarray(item_pol, dtype=np.uint32)
        ho = np.full(4, 99, dtype=np.uint64)
        buf = np.full(need, 0xAB, dtype=np.uint8)
        keys = np.full((3, 32), 0xCD, dtype=np.uint8)

        def encaps(hdr_buf, cap, off, key_buf):
            return host.lib.rabe_ghw11_encaps_packed(host.h, pk.ptr, arr, npol, hl.JSON_POLICY, ctypes.c_size_t(3), hl._np_ptr(ip), hdr_buf,
                                                     ctypes.c_size_t(cap), off, key_buf)
        host.set_tape(tape)          # a short call that drew anything would exhaust the tape for the full call below
        assert encaps(hl._np_ptr(buf), need - 1, hl._np_ptr(ho), hl._np_ptr(keys)) == 1
        assert ho.tolist() == want_off.tolist() and (buf == 0xAB).all() and (keys == 0xCD).all()
        ho[:] = 99
        assert encaps(None, 0, hl._np_ptr(ho), hl._np_ptr(keys)) == 1          # the sizing call
        assert int(ho[3]) == need and (keys == 0xCD).all()
        assert encaps(hl._np_ptr(buf), need, None, hl._np_ptr(keys)) == -1          # no offsets array: refused, nothing drawn
        assert encaps(hl._np_ptr(buf), need, hl._np_ptr(ho), None) == -1            # no key array
        assert (buf == 0xAB).all() and (keys == 0xCD).all()
        assert encaps(hl._np_ptr(buf), need, hl._np_ptr(ho), hl._np_ptr(keys)) == 0
        host.clear_tape()
        assert bytes(buf) == bytes(want_hdr) and (keys == want_keys).all()
        # the decaps calls: null arrays are refused with an error text, nothing is written
        status = np.full(3, 7, dtype=np.int32)
        tct = np.zeros(3 * 768, dtype=np.uint8)
        co = np.ascontiguousarray(want_off, dtype=np.uint64)
        out = host.lib.rabe_ghw11_decaps_out_packed
        dec = host.lib.rabe_ghw11_decaps_packed
        n3 = ctypes.c_size_t(3)
        flags = ctypes.c_uint32(0)
        assert out(host.h, rk.ptr, n3, None, flags, hl._np_ptr(status), hl._np_ptr(keys)) == -1
        assert out(host.h, rk.ptr, n3, hl._np_ptr(tct), flags, None, hl._np_ptr(keys)) == -1
        assert out(host.h, rk.ptr, n3, hl._np_ptr(tct), flags, hl._np_ptr(status), None) == -1
        assert dec(host.h, sk.ptr, n3, hl._np_ptr(buf), ctypes.c_size_t(need), None, flags, hl._np_ptr(status), hl._np_ptr(keys)) == -1
        assert dec(host.h, sk.ptr, n3, hl._np_ptr(buf), ctypes.c_size_t(need), hl._np_ptr(co), flags, None, hl._np_ptr(keys)) == -1
        assert dec(host.h, sk.ptr, n3, hl._np_ptr(buf), ctypes.c_size_t(need), hl._np_ptr(co), flags, hl._np_ptr(status), None) == -1
        assert (status == 7).all() and (keys == want_keys).all()
        assert (host.lib.rabe_host_last_error(None) or b"") != b""
        # all-zero records: every item fails alone, the call succeeds
        assert out(host.h, rk.ptr, n3, hl._np_ptr(tct), flags, hl._np_ptr(status), hl._np_ptr(keys)) == 0
        assert (status == -1).all() and not keys.any()
        # n_items = 0 touches nothing
        assert out(host.h, rk.ptr, ctypes.c_size_t(0), None, flags, None, None) == 0
        assert dec(host.h, sk.ptr, ctypes.c_size_t(0), None, ctypes.c_size_t(0), hl._np_ptr(co), flags, None, None) == 0
    finally:
        host.close()
