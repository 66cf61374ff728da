"""The surface of GHW11's decrypt for a key holder without a proxy (include/rabe_host.h: rabe_ghw11_decrypt_packed, rabe_ghw11_decrypt,
rabe_ghw11_decrypt_gt; include/rabe_hip.h: rhip_ghw11_decrypt_batch) and the identity it rests on, on the oracle: for every z,
decrypt_out(transform(ct, tkgen(sk, z)), z) = c * t_1^-1 with t_1 the transform's own expression on the secret key's elements."""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def hb(s):
    return bytes.fromhex(s)


def test_entry_points_are_declared():
    from rabe_amd import build
    syms = set(build.declared_symbols())
    for name in ("rabe_ghw11_decrypt_packed", "rabe_ghw11_decrypt", "rabe_ghw11_decrypt_gt", "rhip_ghw11_decrypt_batch"):
        assert name in syms, name
    inc = os.path.join(os.path.dirname(HERE), "include")
    host_h = open(os.path.join(inc, "rabe_host.h")).read()
    hip_h = open(os.path.join(inc, "rabe_hip.h")).read()
    assert "int32_t rabe_ghw11_decrypt_packed(rabe_host* h, const void* sk, size_t n_items, const uint8_t* ct_blob, size_t ct_len," in host_h
    assert "int32_t rabe_ghw11_decrypt(rabe_host* h, const void* sk, const void* ct, uint8_t** plaintext, size_t* len);" in host_h
    assert "int32_t rabe_ghw11_decrypt_gt(rabe_host* h, const void* sk, const void* ct, uint8_t out_gt[384]);" in host_h
    assert "int32_t rhip_ghw11_decrypt_batch(rhip_ctx* ctx," in hip_h and "rabe_ghw11_decrypt_packed" not in hip_h


def test_python_wrappers_exist():
    from rabe_amd.schemes import ghw11
    for name in ("decrypt", "decrypt_gt", "decrypt_packed"):
        assert callable(getattr(ghw11, name)), name


def test_the_blinding_cancels_on_the_oracle():
    """the golden case's secret key read as a transform key (the record layouts agree) gives t_1; two random z give two transform keys"""
    from oracle import bn254 as bn
    from oracle import schemes as sch
    from oracle.tape import ListRng
    with open(os.path.join(HERE, "golden", "ghw11.json")) as f:
        c = json.load(f)["cases"][0]
    sk = {"k": bn.g2_from_le(hb(c["sk"]["k"])), "l": bn.g2_from_le(hb(c["sk"]["l"])),
          "attr_key": [{"string": n, "k_x": bn.g2_from_le(hb(k))} for n, k in c["sk"]["attr_key"]]}
    ct = {"policy": (c["policy"], c["language"]), "c": bn.gt_from_le(hb(c["ct"]["c"])), "c1": bn.g1_from_le(hb(c["ct"]["c1"])),
          "ci_di": [(n, bn.g1_from_le(hb(a)), bn.g1_from_le(hb(b))) for n, a, b in c["ct"]["ci_di"]]}
    t_1 = sch.ghw11_transform(ct, {"k_z": sk["k"], "l_z": sk["l"], "attr_key_z": sk["attr_key"]})["t"]
    msg = bn.gt_mul(ct["c"], bn.gt_inv(t_1))
    assert bn.gt_to_le(msg) == hb(c["msg"]) == hb(c["decrypted"])
    rnd = random.Random(1102)
    for _ in range(2):
        z = rnd.randrange(2, R)
        tk, rk = sch.ghw11_tkgen(sk, ListRng([z]))
        assert rk["z"] == z
        pct = sch.ghw11_transform(ct, tk)
        assert pct["t"] != t_1
        assert bn.gt_to_le(sch.ghw11_decrypt_out(pct, rk)) == bn.gt_to_le(msg)
