"""GPU checks of rhip_aw11_encrypt_batch (k_aw11_enc_scalars, k_aw11_enc_c1, k_aw11_enc_c3, the c2 table call) on the rows of
tests/aw11_row_cases.py -- r on the edges of every window walk, the Gt product started by a negative digit, the two-base G2 sum through its
doubling branch and through infinity, raw `rand` words, the last attribute, rows around the 64- and 128-thread blocks -- in every form the
per-attribute tables take.  rhip_aw11_pk_table_form says which form a handle got: a form that fell back to the 8-bit tables is skipped, with
the device's memory in the reason, and never counts as a pass.  Every comparison is of canonical bytes against oracle.bn254 alone (the
builder's window tables; tests/test_aw11_rows_precheck.py proves the rows and the builder on the CPU)."""
import pytest

from rabe_amd import Engine
from rabe_amd import engine as E
from rabe_amd import hostprep as hp
from tests import aw11_row_cases as ac

pytestmark = pytest.mark.gpu

GUARD = bytes([0xA5]) * 256
ENV = ("RABE_AW11_ATTR_BITS", "RABE_AW11_ATTR_W16")
FORM_CASES = [("default-signed-10", {}, 10), ("plain-8", {"RABE_AW11_ATTR_BITS": "8"}, 0), ("signed-9", {"RABE_AW11_ATTR_BITS": "9"}, 9),
              ("signed-14", {"RABE_AW11_ATTR_BITS": "14"}, 14), ("w16-per-attribute", {"RABE_AW11_ATTR_W16": "1"}, 1)]


class World:
    def __init__(self):
        self.cs = cs = ac.cases()
        self.eng = eng = Engine(0)
        self.dtt = E.DevTreeTables(eng, cs.tt)
        self.d_leaf_attr = eng.upload_u32(cs.leaf_attr)
        # expected bytes do not depend on the table form: once per module
        self.c0 = [cs.want_c0(i) for i in range(len(cs.items))]
        rows = [cs.want_row(t) for t in range(len(cs.rows))]
        self.c1, self.c2, self.c3 = ([r[j] for r in rows] for j in range(3))

    def pk(self, monkeypatch, env, form):
        """a handle built under `env`; skips unless it got the form asked for"""
        for name in ENV:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        cs = self.cs
        from oracle import bn254 as bn
        pk = E.Aw11Pk(self.eng, bn.g1_to_le(cs.g1), bn.g2_to_le(cs.g2), [ac.gt_le(x) for x in cs.egg_alpha], [ac.g2_le(x) for x in cs.g2_y])
        got = pk.table_form()
        if got != form:
            pk.destroy()
            import torch
            free_b, total_b = torch.cuda.mem_get_info(0)
            pytest.skip("asked for table form %d, the handle fell back to %d: %d of %d bytes of device memory free" % (form, got, free_b, total_b))
        return pk

    def run(self, pk, n_items=None):
        """one call over the first n_items items (all by default); (c0, c1, c2, c3) as lists of elements, the guard bytes behind each checked"""
        eng, a = self.eng, self.cs.call_arrays(n_items)
        n, total = a["n_items"], a["total_rows"]
        le = lambda xs: b"".join(hp.fr_le(x) for x in xs) or bytes(32)
        raw = b"".join(x.to_bytes(32, "little") for x in a["rand"]) or bytes(32)
        sizes = (n * 384, total * 384, total * 128, total * 128)
        outs = [eng.upload(GUARD * ((sz + 255) // 256) + GUARD) for sz in sizes]
        E.aw11_encrypt_dev(eng, pk, n, total, eng.upload_u32(a["row_off"]), eng.upload_u32(a["tree_leaf"] or [0]), eng.upload_u32(a["tree_gate"] or [0]),
                           eng.upload_u32(a["n_coef"] or [0]), self.dtt, self.d_leaf_attr, eng.upload(le(a["s"])), eng.upload(le(a["coefs"])),
                           eng.upload_u32(a["coef_off"] or [0]), eng.upload(raw), eng.upload(b"".join(a["msg"]) or bytes(384)), *outs)
        eng.sync()
        res = []
        for buf, sz, el in zip(outs, sizes, (384, 384, 128, 128)):
            b = eng.download(buf)
            assert set(b[sz:]) == {0xA5} and len(b) - sz >= 256, "bytes behind an output were written"
            res.append([b[i:i + el] for i in range(0, sz, el)])
        return res

    def differing(self, got):
        """the elements that differ from the builder's expected values, by name"""
        c0, c1, c2, c3 = got
        bad = ["c0 of item %d" % i for i in range(len(c0)) if c0[i] != self.c0[i]]
        for name, g, want in (("c1", c1, self.c1), ("c2", c2, self.c2), ("c3", c3, self.c3)):
            bad += ["%s of %s" % (name, self.cs.label(t)) for t in range(len(g)) if g[t] != want[t]]
        return bad


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()


@pytest.mark.parametrize("env,form", [c[1:] for c in FORM_CASES], ids=[c[0] for c in FORM_CASES])
def test_every_row_equals_the_oracle(world, env, form, monkeypatch):
    pk = world.pk(monkeypatch, env, form)
    try:
        got = world.run(pk)
        assert [len(x) for x in got] == [len(world.cs.items)] + [len(world.cs.rows)] * 3
        bad = world.differing(got)
        assert bad == [], "%d elements differ under table form %d: %s" % (len(bad), form, "; ".join(bad[:12]))
    finally:
        pk.destroy()


def test_leading_sub_lists_guards_and_the_empty_call(world, monkeypatch):
    """the default form on the head of the list at row counts around the 64-thread blocks of c1 and the 128-thread blocks of c3 (whose shadow
    lanes repeat the last row), cut at item boundaries; nothing is written behind an output; n_items = 0 is served and writes nothing"""
    pk = world.pk(monkeypatch, {}, 10)
    try:
        bad = []
        for rows in ac.HEADS:
            got = world.run(pk, world.cs.items_for_rows(rows))
            assert [len(x) for x in got[1:]] == [rows] * 3
            bad += ["%d rows: %s" % (rows, b) for b in world.differing(got)]
        assert bad == [], "%d elements differ: %s" % (len(bad), "; ".join(bad[:12]))
        assert world.run(pk, 0) == [[], [], [], []]                      # run() checks that every byte of the four buffers still holds the guard
    finally:
        pk.destroy()
