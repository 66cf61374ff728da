"""CPU-side checks of the key-encapsulation surface (include/rabe_host.h: rabe_{ac17_cp,bsw}_{encaps,decaps}_packed; include/rabe_hip.h:
rhip_gt_kdf_rows): the symbols are declared and exported, the Python wrappers exist, and a HEADER -- a ciphertext record whose sealed part has
length zero -- goes through the C++ reader and writer unchanged (the existing parser accepts it; only the tag check, which a decaps never
reaches, refuses an empty sealed part)."""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("rabe_ac17_cp_encaps_packed", "rabe_ac17_cp_decaps_packed", "rabe_bsw_encaps_packed", "rabe_bsw_decaps_packed")


def hb(s):
    return bytes.fromhex(s)


def u32(v):
    return int(v).to_bytes(4, "little")


def s_(text):
    return u32(len(text.encode())) + text.encode()


def test_entry_points_are_declared_and_exported():
    from rabe_amd import build
    syms = set(build.declared_symbols())
    for name in NEW + ("rhip_gt_kdf_rows", "rabe_host_kernel_timing", "rabe_host_kernel_timing_read"):
        assert name in syms, name
    lib = ctypes.CDLL(build.build())
    for name in NEW + ("rhip_gt_kdf_rows",):
        assert hasattr(lib, name), name
    host_h = open(os.path.join(os.path.dirname(HERE), "include", "rabe_host.h")).read()
    for scheme in ("ac17_cp", "bsw"):
        assert ("int32_t rabe_%s_encaps_packed(rabe_host* h, const void* pk, const char* const* policies, size_t n_policies, int32_t language, "
                "size_t n_items," % scheme) in host_h
        assert "int32_t rabe_%s_decaps_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len," % scheme in host_h
    assert "minus the AES nonce" in host_h          # the draw order is stated


def test_python_wrappers_exist():
    from rabe_amd.schemes import ac17, bsw
    from rabe_amd import hostlib, symlib
    for fn in (ac17.cp_encaps_packed, ac17.cp_decaps_packed, bsw.encaps_packed, bsw.decaps_packed, hostlib.packed_encaps, hostlib.packed_decaps,
               symlib.gt_kdf_rows):
        assert callable(fn)


def golden(name):
    with open(os.path.join(HERE, "golden", name + ".json")) as f:
        return json.load(f)["cases"][0]


def ac17_record(c, sealed):
    lang = {"json": 0, "human": 1}[c["language"]]
    out = s_(c["policy"]) + bytes([lang]) + u32(3) + b"".join(hb(x) for x in c["ct"]["c_0"]) + u32(len(c["ct"]["c"]))
    for name, vec in c["ct"]["c"]:
        out += s_(name) + u32(3) + b"".join(hb(x) for x in vec)
    return out + hb(c["ct"]["c_p"]) + u32(len(sealed)) + sealed


def bsw_record(c, sealed):
    lang = {"json": 0, "human": 1}[c["language"]]
    out = s_(c["policy"]) + bytes([lang]) + hb(c["ct"]["c"]) + hb(c["ct"]["c_p"]) + u32(len(c["ct"]["c_y"]))
    for name, g1, g2 in c["ct"]["c_y"]:
        out += s_(name) + hb(g1) + hb(g2)
    return out + u32(len(sealed)) + sealed


@pytest.mark.parametrize("kind,make,field", [("ac17_cp_ct", lambda: ac17_record(golden("ac17"), b""), "ct"),
                                             ("bsw_ct", lambda: bsw_record(golden("bsw"), b""), "data")])
def test_a_header_round_trips_through_the_cxx_reader(kind, make, field):
    from rabe_amd import hostlib as hl
    hdr = make()
    assert hdr[-4:] == bytes(4)
    obj = hl.Obj.deserialize(kind, hdr)
    assert obj.serialize() == hdr
    assert hl.parse_obj(kind, hdr)[field] == b""
    with pytest.raises(hl.RabeError):          # the length field must lie inside the record
        hl.Obj.deserialize(kind, hdr[:-1])


@pytest.mark.parametrize("kind,make", [("ac17_cp_ct", lambda s: ac17_record(golden("ac17"), s)), ("bsw_ct", lambda s: bsw_record(golden("bsw"), s))])
def test_a_full_record_is_its_header_plus_the_sealed_part(kind, make):
    from rabe_amd import hostlib as hl
    sealed = bytes(range(12)) + b"\x11" * 5 + bytes(16)
    full, hdr = make(sealed), make(b"")
    assert hl.Obj.deserialize(kind, full).serialize() == full
    assert full[:len(hdr) - 4] == hdr[:-4] and full[len(hdr) - 4:] == u32(len(sealed)) + sealed
