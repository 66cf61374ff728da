"""TEST INFRASTRUCTURE: builds and drives tests/hostsim/fp_dot2.cpp, the stand-alone host program around the two-term Montgomery
dot product of rabe_amd/csrc/bn254/fp.h (mont_dot2_raw) -- its carry-capture plan, the routine on raw residues, a g1_madd_inl walk."""
import os
import subprocess

from oracle import bn254 as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "fp_dot2.cpp")
EXE = os.path.join(ROOT, "build", "fp_dot2")
HDR_DIR = os.path.join(ROOT, "rabe_amd", "csrc", "bn254")
W = 0xFFFFFFFF
MODS = {"fp": bn.P, "fr": bn.R}


def build_program():
    deps = [SRC] + [os.path.join(HDR_DIR, f) for f in os.listdir(HDR_DIR)]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    # RABE_HOST_SANITIZE=address,undefined builds the program (host code, its own main) with those sanitizers
    san = os.environ.get("RABE_HOST_SANITIZE")
    extra = ["-fsanitize=" + san, "-fno-sanitize-recover=all", "-g"] if san else []
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-o", EXE, SRC] + extra, check=True, timeout=600)
    return EXE


def plan(field):
    """(safe[16], last_safe) of the dot product's ColumnPlan, from the header the kernels compile from"""
    out = subprocess.run([build_program(), "plan"], check=True, stdout=subprocess.PIPE, timeout=60).stdout.decode()
    assert "!" not in out, out                     # the accessors the routine reads and the ColumnPlan object agree
    nums = [int(x, 16) for x in out.splitlines()[0 if field == "fp" else 1].split()]
    assert len(nums) == 17
    return nums[:16], nums[16]


def le(x):
    return int(x).to_bytes(32, "little")


def dot2(field, quads):
    """quads of raw Montgomery residues (a0, b0, a1, b1) -> (return code, [(dot2 bytes, mul + mul + add bytes)], stderr)"""
    res = subprocess.run([build_program(), field], input=b"".join(le(x) for q in quads for x in q), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    out = res.stdout
    assert len(out) == 64 * len(quads), res.stderr.decode()
    return res.returncode, [(out[64 * i:64 * i + 32], out[64 * i + 32:64 * i + 64]) for i in range(len(quads))], res.stderr.decode()


def walk(points_raw):
    """affine points as 64 bytes of raw Montgomery limbs each -> (return code, g1_madd_inl walk bytes, jac_add_aff walk bytes)"""
    res = subprocess.run([build_program(), "walk"], input=b"".join(points_raw), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert len(res.stdout) == 128, res.stderr.decode()
    return res.returncode, res.stdout[:64], res.stdout[64:]


def edge_residues(mod, rnd, n_random=0):
    """residues < mod whose LIMBS are extreme: 0, 1, mod - 1, 2^256 mod mod (the Montgomery one), limbs of 0xFFFFFFFF wherever mod
    allows (the top limb can only reach mod's own), the limbs of mod +- 1, single saturated limbs, mixtures"""
    pl = [(mod >> (32 * i)) & W for i in range(8)]
    top = pl[7]
    out = [0, 1, 2, mod - 1, mod - 2, (1 << 256) % mod, (1 << 224) - 1, ((top - 1) << 224) | ((1 << 224) - 1),
           (top << 224) | ((1 << 192) - 1), (top << 224) | ((pl[6] - 1) << 192) | ((1 << 192) - 1)]
    for i in range(8):
        out.append(W << (32 * i) if i < 7 else (top - 1) << 224)          # one saturated limb
        out.append((((1 << 256) - 1) ^ (W << (32 * i))) % mod)            # all but one
        out.append((mod - 1) ^ (1 << (32 * i)))                           # the limbs of mod - 1, one of them off by one
    out.append(sum(((pl[i] + 1) & W) << (32 * i) for i in range(7)) | ((top - 1) << 224))     # every low limb of mod, plus one
    out.append(sum(((pl[i] - 1) & W) << (32 * i) for i in range(8)))                           # every limb of mod, minus one
    choices = lambda i: [0, 1, W, W - 1, 0x80000000, pl[i], (pl[i] - 1) & W, (pl[i] + 1) & W, rnd.getrandbits(32)]
    for _ in range(n_random):
        out.append(sum(rnd.choice(choices(i)) << (32 * i) for i in range(8)))
    return [x % mod for x in out]
