"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads without a GPU,
and exports every symbol include/rabe_hip.h declares.  No compute is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rabe_amd import build
    return ctypes.CDLL(build.build())


def declared_symbols():
    out = set()
    for header, prefix in (("rabe_hip.h", "rhip_"), ("rabe_host.h", "rabe_")):
        text = open(os.path.join(ROOT, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M)          # macros (rabe_host_open) are not symbols
        out |= set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text))
    return sorted(out)


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for must in ["rhip_ctx_create", "rhip_pairing_product", "rhip_ac17_cp_encrypt_batch", "rhip_ac17_cp_decrypt_batch",
                 "rhip_ac17_cp_keygen_batch", "rhip_g1_table_mul", "rhip_gt_pow", "rhip_ac17_sk_prepare",
                 "rhip_ac17_cp_decrypt_batch_prepared", "rhip_g1_table_add_wide", "rabe_ac17_cp_encrypt_batch", "rabe_bsw_encrypt_batch",
                 "rabe_bsw_decrypt_batch", "rabe_lsw_keygen_batch", "rabe_lsw_decrypt_batch", "rabe_aw11_encrypt_batch",
                 "rabe_aw11_decrypt_batch",
                 # device-level Level B of the other three schemes and what the rabe-bn replacement crate binds
                 "rhip_bsw_pk_create", "rhip_bsw_encrypt_batch", "rhip_bsw_sk_prepare", "rhip_bsw_decrypt_batch", "rhip_lsw_pk_create",
                 "rhip_bsw_decrypt_batch_one_sk", "rhip_lsw_keygen_batch", "rhip_lsw_decrypt_batch", "rhip_lsw_decrypt_batch_one_ct", "rhip_aw11_pk_create", "rhip_aw11_pk_table_form", "rhip_aw11_encrypt_batch", "rhip_aw11_decrypt_batch",
                 "rhip_g2_lines_prepare", "rhip_host_fr_pow", "rhip_host_g1_on_curve", "rhip_host_g2_on_curve",
                 # round 3: decoding checks (fast + by-order forms), packed entry points of every scheme, LSW negative leaves, pipelining hook
                 "rhip_g2_in_subgroup", "rhip_g2_in_subgroup_by_order", "rhip_gt_is_member", "rhip_gt_is_member_by_order", "rhip_flags_all", "rhip_ghw11_transform_batch",
                 "rhip_host_g2_in_subgroup", "rhip_host_gt_is_member", "rhip_lsw_keygen_batch_signed", "rhip_ctx_release_before_final_exp",
                 "rabe_ac17_cp_encrypt_packed", "rabe_ac17_cp_decrypt_packed", "rabe_bsw_encrypt_packed", "rabe_bsw_decrypt_packed",
                 "rabe_lsw_keygen_packed", "rabe_lsw_decrypt_packed", "rabe_aw11_encrypt_packed", "rabe_aw11_decrypt_packed"]:
        assert must in syms


def test_every_declared_symbol_is_exported(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert missing == []


def test_dynamic_symbol_table_is_exactly_the_two_headers():
    """rabe_amd/build.py links with a version script: nothing but the C API is exported -- no std:: / rabe:: C++ symbols, no kernel stubs
    (a Rust or C++ host that links the library must not inherit libstdc++ interposition; the C convention of src/ffi/bsw.rs:22-163)."""
    import subprocess
    from rabe_amd import build
    for path in (build.build(), build.LIB_SAFE):
        if not os.path.exists(path):
            continue
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE).stdout.decode()
        exported = sorted(line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip() and line.split()[-1] != "RABE_AMD")
        assert exported == declared_symbols() == build.declared_symbols(), (sorted(set(exported) ^ set(declared_symbols())), path)


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = ctypes.c_void_p()
    rc = lib.rhip_ctx_create(ctypes.c_int32(0), ctypes.byref(ctx))
    assert rc == -1 and not ctx.value          # RHIP_ERR_NO_DEVICE: the engine refuses to run
    from rabe_amd import Engine, EngineError
    with pytest.raises(EngineError):
        Engine(0)


def test_rabe_bn_shim_binds_only_exported_symbols(lib):
    """integration/rabe-bn-shim/src/lib.rs (not compiled here: no Rust) must only name functions the library exports, and
    must offer what rabe's call sites use (src/error.rs:60-69, src/utils/secretsharing/mod.rs:218, the serde / borsh derives)."""
    src = open(os.path.join(ROOT, "integration", "rabe-bn-shim", "src", "lib.rs")).read()
    block = src[src.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    for sym in re.findall(r"fn (rhip_[a-z0-9_]+)\(", block):
        assert hasattr(lib, sym), sym
    for needle in ["enum FieldError", "InvalidSliceLength", "InvalidU512Encoding", "NotMember", "pub fn pow(&self, exp: Fr) -> Fr",
                   "impl Serialize for", "impl BorshSerialize for", "impl BorshDeserialize for", "impl From<Gt> for Vec<u8>",
                   "pub fn from_str(s: &str) -> Option<Fr>", "pub fn inverse(&self) -> Option<Fr>"]:
        assert needle in src, needle
