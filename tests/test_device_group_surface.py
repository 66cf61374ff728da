"""The device group's surface, without a GPU: the library exports rabe_host_group_items, hostlib wraps it, the header's device-group
paragraph names every call that is cut over a group (and the ones that are deliberately not), and the draw order of a call with two runs
of draws that is cut into blocks (rabe_amd/csrc/host/predraw.h) holds in a stand-alone program."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHARDED = ["rabe_ghw11_transform_packed", "rabe_ghw11_decrypt_out_packed", "rabe_ghw11_decrypt_packed", "rabe_ac17_kp_decrypt_packed",
           "rabe_ac17_cp_decaps_packed", "rabe_bsw_decaps_packed", "rabe_ghw11_keygen_packed", "rabe_ac17_kp_encrypt_packed",
           "rabe_ac17_cp_encaps_packed", "rabe_bsw_encaps_packed", "rabe_ghw11_provision_packed",
           # sharded before, and still
           "rabe_ghw11_encrypt_packed", "rabe_bdabe_encrypt_packed", "rabe_mke08_encrypt_packed", "rabe_ac17_cp_encrypt_packed",
           "rabe_ac17_cp_decrypt_packed", "rabe_bsw_encrypt_packed", "rabe_bsw_decrypt_packed", "rabe_lsw_keygen_packed", "rabe_lsw_decrypt_packed",
           "rabe_lsw_decrypt_one_sk_packed", "rabe_aw11_encrypt_packed", "rabe_aw11_decrypt_packed"]
LEFT_ON_FIRST_DEVICE = ["rabe_ghw11_tkgen_packed", "rabe_bsw_delegate_packed", "request_*_sk_packed", "rabe_{bdabe,mke08}_decrypt_packed"]


@pytest.fixture(scope="module")
def lib():
    from rabe_amd import build
    return ctypes.CDLL(build.build())


def group_paragraph():
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    m = re.search(r"/\* ---- device group:.*?\*/", text, flags=re.S)
    assert m, "include/rabe_host.h has no device-group paragraph"
    return m.group(0)


def test_library_exports_group_items(lib):
    assert hasattr(lib, "rabe_host_group_items")
    # no host: refused, not a crash
    out = (ctypes.c_uint64 * 4)()
    assert lib.rabe_host_group_items(None, out, ctypes.c_size_t(4)) == -1


def test_header_declares_group_items():
    text = open(os.path.join(ROOT, "include", "rabe_host.h")).read()
    assert re.search(r"int32_t\s+rabe_host_group_items\s*\(\s*rabe_host\s*\*\s*h\s*,\s*uint64_t\s*\*\s*out[^,]*,\s*size_t\s+cap\s*\)\s*;", text)


def test_python_wrapper_has_the_documented_signature():
    from rabe_amd import hostlib as hl
    assert list(inspect.signature(hl.Host.group_items).parameters) == ["self"]
    assert "rabe_host_group_items" in (hl.Host.group_items.__doc__ or "")


@pytest.mark.parametrize("name", SHARDED)
def test_group_paragraph_names_the_sharded_call(name):
    para = group_paragraph()
    sharded = para[:para.index("NOT sharded")]
    assert re.search(r"\b%s\b" % re.escape(name), sharded), "%s is cut over a device group and the header does not say so" % name


def test_group_paragraph_names_what_stays_on_the_first_device():
    para = group_paragraph()
    assert "Every other entry point runs on devices[0]" not in para
    rest = para[para.index("NOT sharded"):]
    assert "devices[0]" in rest
    for name in LEFT_ON_FIRST_DEVICE:
        assert name in rest, name


def test_two_runs_of_draws_keep_their_order_when_the_batch_is_cut(tmp_path):
    """tests/native/predraw_blocks.cpp: r in block order, then z in block order, with a block that never starts; its header comment has
    the thread-sanitizer build line for a CPU machine.  Here: built plain and run -- no engine, no device."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "predraw_blocks")
    subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "rabe_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "native", "predraw_blocks.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert run.returncode == 0, run.stderr.decode()
    assert b"predraw_blocks ok" in run.stdout
