"""CPU-side checks of the BDABE / MKE08 key encapsulation: the four host calls and the device-level four-pair decrypt are declared with the
signatures they were specified with, exported by the built library and wrapped in Python; the ABI revision is unchanged (additions only);
the gather kernel lives in one translation unit."""
import glob
import os
import re
import subprocess

from rabe_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_CALLS = ["rabe_bdabe_kem_encaps", "rabe_bdabe_kem_decaps", "rabe_mke08_kem_encaps", "rabe_mke08_kem_decaps"]
DEVICE_CALL = "rhip_dnf_decrypt_batch_one_uk"

ENCAPS = """int32_t rabe_%s_kem_encaps(rabe_host* h, const void* pk, const void* const* attr_pks, size_t n_pks, const char* const* policies, size_t n_policies,
                              int32_t language, size_t n_items, const uint32_t* item_policy /*[n_items]*/, uint8_t* hdr_buf, size_t hdr_cap,
                              uint64_t* hdr_off /*[n_items+1]*/, uint8_t* key_buf /*32 n_items*/);"""
DECAPS = """int32_t rabe_%s_kem_decaps(rabe_host* h, const void* uk, size_t n_items, const uint8_t* ct_blob, size_t ct_len, const uint64_t* ct_off /*[n_items+1]*/,
                              uint32_t flags, int32_t* status /*[n_items]*/, uint8_t* key_buf /*32 n_items*/);"""
ONE_UK = """int32_t rhip_dnf_decrypt_batch_one_uk(rhip_ctx* ctx, size_t n_items, size_t n_classes, const uint32_t* dev_item_class /*[n_items]*/,
                                      const rhip_g1* dev_class_s1 /*[n_classes]*/, const uint8_t* dev_class_skip /*[n_classes]: bit 0 S1 = O, bit 1 S2 = O*/,
                                      const rhip_g1* dev_neg_u1 /*[1]*/, const rhip_g2_lines* key_lines /* block 0: sk.u2, block 1 + c: S2 of class c */,
                                      const rhip_g1* dev_ct_g1 /*[n_items][2]: e2, e4*/, const rhip_g2* dev_ct_g2 /*[n_items][2]: e3, e5*/,
                                      const rhip_gt* dev_lead /*[n_items]*/, rhip_gt* dev_out /*[n_items]*/);"""


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def squeeze(s):
    return " ".join(s.split())


def test_symbols_are_declared_and_exported():
    declared = build.declared_symbols()
    for name in HOST_CALLS + [DEVICE_CALL]:
        assert name in declared, name
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    for name in HOST_CALLS + [DEVICE_CALL]:
        assert name in exported, name


def test_signatures_stand_in_the_headers():
    host, hip = squeeze(text("include", "rabe_host.h")), squeeze(text("include", "rabe_hip.h"))
    for scheme in ("bdabe", "mke08"):
        assert squeeze(ENCAPS % scheme) in host, scheme
        assert squeeze(DECAPS % scheme) in host, scheme
    assert squeeze(ONE_UK) in hip


def test_abi_revision_is_unchanged():
    assert re.search(r"^#define RABE_HOST_ABI_VERSION 5$", text("include", "rabe_host.h"), flags=re.M)


def test_no_new_packed_symbol():
    """the table of rabe_*_packed symbols is a recorded contract (tests/test_gpu_packed_abi_contract.py): the KEM calls stay out of it"""
    assert not [s for s in build.declared_symbols() if "kem" in s and s.endswith("_packed")]


def test_the_gather_kernel_lives_in_one_unit():
    units = sorted(glob.glob(os.path.join(ROOT, "rabe_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "rabe_amd", "csrc", "**", "*.h"), recursive=True)
                   + glob.glob(os.path.join(ROOT, "rabe_amd", "csrc", "host", "*.cpp")))
    holders = [os.path.basename(u) for u in units if re.search(r"\bk_dnf_dec_pairs\s*\(", open(u).read())]
    assert holders == ["engine_jobs.hip"], holders


def test_the_device_group_paragraph_lists_the_calls():
    host = text("include", "rabe_host.h")
    sharded = host[host.index("The SHARDED calls:"):host.index("Each cuts its n_items")]
    for name in HOST_CALLS:
        assert name in sharded, name
    rest = host[host.index("NOT sharded, on devices[0]:"):host.index("Status: as rabe_host_create_checked.")]
    assert "rabe_{bdabe,mke08}_decrypt_packed" in rest          # the yardstick stays where it was


def test_python_wrappers_exist():
    from rabe_amd import engine, hostlib
    from rabe_amd.schemes import bdabe, mke08
    for mod in (bdabe, mke08):
        assert callable(mod.encaps_packed) and callable(mod.decaps_packed)
    assert callable(hostlib.packed_encaps) and callable(hostlib.packed_decaps)
    assert callable(engine.dnf_decrypt_one_uk_dev)
