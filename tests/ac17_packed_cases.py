"""The table behind tests/test_gpu_ac17_packed_contract.py and tools/record_ac17_packed_contract.py: the four AC17 entry points that take many
records under one key -- rabe_ac17_{cp,kp}_{decrypt,decaps}_packed, each checked and trusted: eight LEGS -- and the batches each one is run on.

Shapes: N = 20 records (more than 16: the host's parallel_for takes its threaded path) under two policies / attribute lists in turn, every draw
from a tape.  CP: the policies '"A" and "B"' and '"C" or ("B" and "B")' -- the second names B twice, in the branch the pruning does not take:
the reference matches rows by NAME, so a selected attribute that two rows carry does not decrypt there either -- under a key with A, B, C.
KP: the lists [A, B] and [A, C, D] under a key with the policy '"A" and ("B" or "C")'.

A case is a function of the side's clean records that returns a Batch: the records (or blob + offsets), the victims, and what is known about
them beforehand: `ok` (damage that must still decrypt) and `dead` (damage no leg may accept).  Every case names the line of
ac17::decrypt_packed_core (host/packed.cpp) or of its record reader (host/ac17_record.h) that it reaches.  A case whose error TEXT is of
interest has ONE victim, at index 7: rabe_host_last_error holds the first failing item's message."""
import ctypes
import hashlib

import numpy as np

from rabe_amd import hostlib as hl

N = 20
VICTIM = 7
TAPE = [1000003 * (i + 11) + 23 for i in range(1500)]
PTS = [b"ac17 packed contract, item " + bytes([65 + i]) * (1 + i % 5) for i in range(N)]
CP_POLICIES = ['"A" and "B"', '"C" or ("B" and "B")']
CP_ATTRS, CP_OTHER_ATTRS = ["A", "B", "C"], ["A", "B", "C", "D"]
KP_LISTS = [["A", "B"], ["A", "C", "D"]]
KP_POLICY, KP_OTHER_POLICY = '"A" and ("B" or "C")', '"A" and ("C" or "B")'
PANIC_JSON = ['{"name": "and", "children": [{"name": "A"}]}',          # tests/test_gpu_packed_fuzz.py
              '{"name": "or", "children": [{"name": 7}, {"name": "A"}]}',
              '{"name": "and"']
LEGS = [(side, op, mode) for side in ("cp", "kp") for op in ("decrypt", "decaps") for mode in ("checked", "trusted")]


def leg_name(leg):
    return "%s_%s_%s" % leg


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(p) for p in items])]).astype(np.uint64)


def u32(v):
    return int(v).to_bytes(4, "little")


# ---------------------------------------------------------------- the record: Ac17CpCiphertext / Ac17KpCiphertext (host/ac17_record.h)
def fields(rec, kp):
    """[(name, offset, length)] of a well-formed record, in byte order.  CP head: pol_len, pol, lang; KP head: attr_cnt, then a<k>_len, a<k>;
    then c0_cnt, c0, row_cnt, per row r<k>_len, r<k>_name, r<k>_cnt, r<k>_el, then cp, sealed_len, sealed."""
    out, at = [], 0

    def take(name, n):
        nonlocal at
        assert at + n <= len(rec), (name, at, n, len(rec))
        out.append((name, at, n))
        at += n
        return int.from_bytes(rec[at - n:at], "little") if n == 4 else None

    if kp:
        for k in range(take("attr_cnt", 4)):
            take("a%d" % k, take("a%d_len" % k, 4))
    else:
        take("pol", take("pol_len", 4))
        take("lang", 1)
    assert take("c0_cnt", 4) == 3
    take("c0", 384)
    for r in range(take("row_cnt", 4)):
        take("r%d_name" % r, take("r%d_len" % r, 4))
        assert take("r%d_cnt" % r, 4) == 3
        take("r%d_el" % r, 192)
    take("cp", 384)
    take("sealed", take("sealed_len", 4))
    assert at == len(rec)
    return out


def where(rec, kp, name):
    for f, at, n in fields(rec, kp):
        if f == name:
            return at, n
    raise KeyError(name)


def put(rec, at, data):
    return rec[:at] + bytes(data) + rec[at + len(data):]


def head_end(rec, kp):
    return where(rec, kp, "c0_cnt")[0]


def with_policy(rec, text, lang_byte):
    """CP: the same record under another policy text"""
    raw = text.encode()
    return u32(len(raw)) + raw + bytes([lang_byte]) + rec[head_end(rec, False):]


def with_attrs(rec, attrs):
    """KP: the same record under another attribute list (the rows keep their names)"""
    return u32(len(attrs)) + b"".join(u32(len(a)) + a.encode() for a in attrs) + rec[head_end(rec, True):]


def rows_of(rec, kp):
    """(offset of the first row, [bytes of each row: length, name, count, elements], offset behind the last row)"""
    f = fields(rec, kp)
    n = int.from_bytes(rec[where(rec, kp, "row_cnt")[0]:][:4], "little")
    starts = [at for name, at, _ in f if name.startswith("r") and name.endswith("_len")] + [where(rec, kp, "cp")[0]]
    return starts[0], [rec[starts[r]:starts[r + 1]] for r in range(n)], starts[-1]


def with_rows(rec, kp, rows):
    first, _old, behind = rows_of(rec, kp)
    return put(rec[:first], where(rec, kp, "row_cnt")[0], u32(len(rows))) + b"".join(rows) + rec[behind:]


# ---------------------------------------------------------------- elements that are no members (tests/test_gpu_validation.py, test_gpu_walk_verdicts.py)
def non_members():
    from oracle import bn254 as bn
    from tests.test_gpu_validation import fp2_sqrt
    bp = bn.fp2_mul((3, 0), bn.fp2_inv(bn.XI))
    x = (1, 0)
    while True:          # a point ON the twist; its cofactor is huge, so it lies outside the r-torsion
        y = fp2_sqrt(bn.fp2_add(bn.fp2_mul(bn.fp2_mul(x, x), x), bp))
        if y is not None:
            break
        x = (x[0] + 1, 0)
    assert bn.g2_add(bn.g2_mul((x, y), bn.R - 1), (x, y)) is not None
    return {"twist": bn.g2_to_le((x, y)), "p": bn.P, "fq12": b"".join((i + 2).to_bytes(32, "little") for i in range(12))}


class Batch:
    def __init__(self, recs=None, victims=(), ok=(), dead=(), blob=None, off=None, key="own"):
        self.blob = b"".join(recs) if blob is None else blob
        self.off = offsets(recs) if off is None else np.array(off, dtype=np.uint64)
        self.n = len(self.off) - 1
        self.victims, self.ok, self.dead, self.key = set(victims), set(ok), set(dead), key
        self.by_leg = None          # {(op, mode): Batch}: a case whose bytes differ from leg to leg
        assert self.ok <= self.victims and self.dead <= self.victims and not (self.ok & self.dead)


def one(recs, rec, **kw):
    """the clean batch with the victim's record replaced"""
    kw.setdefault("victims", [VICTIM])
    return Batch(recs[:VICTIM] + [rec] + recs[VICTIM + 1:], **kw)


def build_cases(side, recs, bad):
    """{case name: Batch} of one side ("cp" / "kp"); recs: its N clean records; bad: non_members()"""
    kp = side == "kp"
    v = recs[VICTIM]
    names = [f[0] for f in fields(v, kp)]
    C = {}
    dead = dict(dead=[VICTIM])
    # ---- shapes of the call
    C["clean"] = Batch(recs)
    C["clean_again"] = Batch(recs)                                   # a hit in the cross-call cache (Ac17PlanCache::get)
    C["other_key"] = Batch(recs, key="other")                        # another fingerprint: another bucket
    C["clean_after_other_key"] = Batch(recs)
    C["n0"] = Batch([], blob=b"\0", off=[0])
    C["n1"] = Batch(recs[:1])
    C["all_fail"] = Batch([r[:10] for r in recs], victims=range(N), dead=range(N))          # m == 0: the early return
    # ---- offsets (check_offsets)
    o = offsets(recs)
    o[VICTIM] = o[VICTIM + 1] + 1          # off[7] > off[8]; item 6 then ends one byte inside record 8, and bytes behind a sealed part are nobody's
    C["off_not_monotone"] = Batch(blob=b"".join(recs), off=o, victims=[VICTIM], **dead)
    o = offsets(recs[:VICTIM + 1])
    o[VICTIM + 1] += 1                     # off[8] > len, item 7 being the last
    C["off_beyond_blob"] = Batch(blob=b"".join(recs[:VICTIM + 1]), off=o, victims=[VICTIM], **dead)
    # ---- truncation through the offsets: at every field boundary and one byte inside each field (Cursor::need at every read)
    row = "r1"          # "a row": the second one
    cut_fields = (["attr_cnt", "a1_len", "a1"] if kp else ["pol_len", "pol"]) + ["c0_cnt", "c0", "row_cnt", row + "_len", row + "_name", row + "_cnt", row + "_el",
                                                                                "cp", "sealed_len", "sealed"]
    for f in cut_fields:
        at, n = where(v, kp, f)
        C["cut_at_" + f] = one(recs, v[:at], **dead)
        C["cut_in_" + f] = one(recs, v[:at + 1], **dead)
    C["cut_sealed_short"] = one(recs, v[:-1], **dead)               # a sealed body one byte shorter than its length field
    # ---- counts
    for f, vals in (("c0_cnt", (2, 4)), (row + "_cnt", (2,))):
        for x in vals:
            C["%s_%d" % (f, x)] = one(recs, put(v, where(v, kp, f)[0], u32(x)), **dead)
    C["rows_x200_beyond"] = one(recs, put(v, where(v, kp, "row_cnt")[0], u32(len(v) // 200 + 1)), **dead)          # the pre-check in front of the row loop
    if kp:
        C["attrs_x4_beyond"] = one(recs, put(v, 0, u32(len(v) // 4 + 1)), **dead)                                  # the pre-check in front of the attribute loop
    for f in [n for n in names if n.endswith("_len") and n[:-4] in ("pol", "a1", row, "sealed")] + ["attr_cnt" if kp else None, "c0_cnt", "row_cnt", row + "_cnt"]:
        if f is None:
            continue
        for tag, x in (("ff", 0xFFFFFFFF), ("zero", 0), ("2len", 2 * len(v))):
            C["%s_%s" % (f, tag)] = one(recs, put(v, where(v, kp, f)[0], u32(x)), **({} if tag == "zero" else dead))
    # ---- policy (the plan maker)
    if kp:
        C["attrs_unsatisfied"] = one(recs, with_attrs(v, ["B", "C"]), **dead)          # the key's policy needs A
    else:
        for k, text in enumerate(PANIC_JSON):
            C["panic_policy_%d" % k] = one(recs, with_policy(v, text, 0), **dead)
        C["policy_unsatisfied"] = one(recs, with_policy(v, '"A" and "D"', 1), **dead)
    # ---- layout (the plan's shared row names against a record's own selection)
    at, n = where(v, kp, "r0_name")
    C["first_row_renamed"] = one(recs, put(v, at, b"Z"))
    _first, rows, _behind = rows_of(v, kp)
    C["rows_permuted"] = one(recs, with_rows(v, kp, rows[1:] + rows[:1]), ok=[VICTIM])
    extra = u32(2) + b"ZZ" + rows[0][-196:]
    C["extra_row"] = one(recs, with_rows(v, kp, rows + [extra]), ok=[VICTIM])
    # The plan LEARNS its row names from a non-standard record, and the standard ones then select on their own (shares_layout is false for
    # them, gather_record gets a null key).  The plan must be new when record 0 arrives, whatever ran before: per leg, all N records go under
    # a key text that occurs nowhere else -- CP: another spacing of the same policy; KP: one more attribute, E<leg>, behind the list.
    def fresh(k):
        if kp:
            out = [with_attrs(r, KP_LISTS[i % 2] + ["E%d" % k]) for i, r in enumerate(recs)]
        else:
            out = [with_policy(r, CP_POLICIES[i % 2].replace(" ", " " * (2 + k), 1), 1) for i, r in enumerate(recs)]
        _f0, rows0, _b0 = rows_of(out[0], kp)
        return Batch([with_rows(out[0], kp, rows0[1:] + rows0[:1])] + out[1:], victims=[0], ok=[0])
    C["victim_at_0"] = fresh(0)
    C["victim_at_0"].by_leg = {(op, mode): fresh(k) for k, (op, mode) in enumerate((o, m) for o in ("decrypt", "decaps") for m in ("checked", "trusted"))}
    # ---- members (checked legs: MemberChecks / WalkedG2; the trusted legs record what the parent makes of the same bytes)
    c0 = where(v, kp, "c0")[0]
    C["c0_outside_subgroup"] = one(recs, put(v, c0 + 128, bad["twist"]))
    x = int.from_bytes(v[c0:c0 + 32], "little") + bad["p"]
    assert x < 1 << 256
    C["c0_coordinate_ge_p"] = one(recs, put(v, c0, x.to_bytes(32, "little")))
    el = where(v, kp, row + "_el")[0]
    C["row_off_curve"] = one(recs, put(v, el + 33, bytes([v[el + 33] ^ 1])))
    C["cp_outside_subgroup"] = one(recs, put(v, where(v, kp, "cp")[0], bad["fq12"]))
    # ---- seal
    C["tag_bit"] = one(recs, v[:-1] + bytes([v[-1] ^ 1]))
    # ---- six damages in one batch
    six = list(recs)
    r = recs[1]
    six[1] = r[:where(r, kp, "c0")[0] + 5]
    r = recs[4]
    six[4] = put(r, where(r, kp, "c0_cnt")[0], u32(2))
    r = recs[7]
    six[7] = put(r, where(r, kp, "r0_name")[0], b"Z")
    r = recs[10]
    six[10] = r[:-1] + bytes([r[-1] ^ 1])
    r = recs[13]
    el = where(r, kp, "r0_el")[0]
    six[13] = put(r, el + 33, bytes([r[el + 33] ^ 1]))
    r = recs[16]
    six[16] = with_attrs(r, ["B", "C"]) if kp else with_policy(r, '"A" and "D"', 1)
    C["six_damages"] = Batch(six, victims=[1, 4, 7, 10, 13, 16], dead=[1, 4, 16])
    return C


# ---------------------------------------------------------------- keys, records, calls
class Setup:
    """keys and clean records of both sides, every draw from the tape"""
    def __init__(self, host):
        from rabe_amd.schemes import ac17
        pt_blob, pt_off = b"".join(PTS), offsets(PTS)
        items = [i % 2 for i in range(N)]

        def taped(fn, *a):
            host.set_tape(TAPE)
            try:
                return fn(host, *a)
            finally:
                host.clear_tape()

        self.pk, self.msk = taped(ac17.setup)
        self.keys = {("cp", "own"): taped(ac17.cp_keygen, self.msk, CP_ATTRS), ("cp", "other"): taped(ac17.cp_keygen, self.msk, CP_OTHER_ATTRS),
                     ("kp", "own"): taped(ac17.kp_keygen, self.msk, KP_POLICY, hl.HUMAN_POLICY),
                     ("kp", "other"): taped(ac17.kp_keygen, self.msk, KP_OTHER_POLICY, hl.HUMAN_POLICY)}
        blob, off = taped(ac17.cp_encrypt_packed, self.pk, CP_POLICIES, items, pt_blob, pt_off, hl.HUMAN_POLICY)
        cp = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(N)]
        blob, off = taped(ac17.kp_encrypt_packed, self.pk, KP_LISTS, items, pt_blob, pt_off)
        kp = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(N)]
        bad = non_members()
        self.records = {"cp": cp, "kp": kp}
        self.cases = {"cp": build_cases("cp", cp, bad), "kp": build_cases("kp", kp, bad)}


def marker(lib):
    """leaves a known text in the calling thread's last error: a call that sets none can be told from one that repeats the last one"""
    p = ctypes.c_void_p()
    assert lib.rabe_policy_parse(b"not a policy", hl.JSON_POLICY, hl.JSON_POLICY, ctypes.byref(p)) != 0
    return lib.rabe_host_last_error(None)


def run(host, setup, leg, name):
    """one call.  Returns (record for the golden file, status, per item: plaintext / key bytes)"""
    side, op, mode = leg
    b = setup.cases[side][name]
    b = b.by_leg[op, mode] if b.by_leg else b
    key = setup.keys[side, b.key]
    n = b.n
    ct = np.frombuffer(b.blob, dtype=np.uint8).copy()
    status = np.full(max(n, 1), 7, dtype=np.int32)
    quiet = marker(host.lib)
    head = (host.h, key.ptr, ctypes.c_size_t(n), hl._np_ptr(ct), ctypes.c_size_t(len(b.blob) if n else 0), hl._np_ptr(b.off),
            ctypes.c_uint32(1 if mode == "trusted" else 0), hl._np_ptr(status))
    if op == "decrypt":
        buf, po = np.full(len(b.blob) + 1, 0xAB, dtype=np.uint8), np.full(n + 1, 0x99, dtype=np.uint64)
        rc = getattr(host.lib, "rabe_ac17_%s_decrypt_packed" % side)(*head, hl._np_ptr(buf), ctypes.c_size_t(buf.size), hl._np_ptr(po))
        out = [buf[int(po[i]):int(po[i + 1])].tobytes() for i in range(n)] if rc == 0 else []
        written = buf[:int(po[n])].tobytes() + po.tobytes() if rc == 0 else b""
    else:
        keys = np.full((max(n, 1), 32), 0xEE, dtype=np.uint8)
        rc = getattr(host.lib, "rabe_ac17_%s_decaps_packed" % side)(*head, hl._np_ptr(keys))
        out = [keys[i].tobytes() for i in range(n)]
        written = keys[:n].tobytes()
    err = host.lib.rabe_host_last_error(None)
    st = [int(x) for x in status[:n]]
    rec = {"rc": int(rc), "status": st, "sha256": hashlib.sha256(written).hexdigest()}
    if rc != 0 or any(st):
        rec["err"] = "" if err == quiet else (err or b"").decode("utf-8", "replace")
    return rec, st, out


def run_leg(host, setup, leg):
    """{case: (record, status, outputs)} of one leg, in the table's order"""
    return {name: run(host, setup, leg, name) for name in setup.cases[leg[0]]}
