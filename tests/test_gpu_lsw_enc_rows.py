"""GPU checks of the fused LSW row kernel (include/rabe_hip.h: rhip_lsw_encrypt_rows, k_lsw_enc_rows) against the path lsw::encrypt_packed runs
today on the same scalars, byte for byte: four rhip_g1_table_mul launches fed the host-formed products h secret, sx, sx h, plus rhip_g1_add.

Row counts 1, 63, 64, 65 and 130 in items of 1, 2 and 5 rows (a ragged row_off); the scalar cases of tests/lsw_row_cases.py (sx = 0, which the row
of a one-attribute list has, secret = 0, sx = r - 1, rows whose e4 and e5 are the identity while e3 is not, the reverse, all three); and keys whose g1_b2 and
h_b are the same point or opposite points, so that the two halves of e5 meet in the doubling and the cancelling case of the mixed addition
(proved on the logs before the launch).  The identity must come out as 64 zero bytes without touching the other elements of its lane."""
import pytest

from oracle import bn254 as bn
from rabe_amd import Engine
from rabe_amd import engine as E
from tests import lsw_row_cases as lc

pytestmark = pytest.mark.gpu


def le(x):
    return int(x).to_bytes(32, "little")


@pytest.fixture(scope="module")
def world():
    """the engine and one window table per distinct base of the three keys (the tables are built from the keys' public bytes)"""
    eng = Engine(0)
    tables = {}
    out = {}
    for key in lc.keys():
        tbls = []
        for pt in key.points():
            if pt not in tables:
                t = eng.g1_table(pt)
                t.add_w16()
                tables[pt] = t
            tbls.append(tables[pt])
        out[key.name] = (key, tbls)
    yield eng, out
    for t in tables.values():
        t.destroy()
    eng.close()


def fused(eng, tbls, call):
    d_out = eng.alloc(call.n_rows * 192)
    E.lsw_encrypt_rows_dev(eng, tbls[0], tbls[1], tbls[2], tbls[3], call.n_items, call.n_rows, eng.upload_u32(call.row_off),
                           eng.upload_u32(call.hash_off), eng.upload(b"".join(le(h) for h in call.hash)),
                           eng.upload(b"".join(le(s) for s in call.secret)), eng.upload(b"".join(le(s) for s in call.sx)), d_out)
    raw = eng.download(d_out, call.n_rows * 192)
    return [raw[64 * i:64 * i + 64] for i in range(3 * call.n_rows)]


def four_launches(eng, tbls, call):
    ka, kb, kc = call.host_products()
    e3 = tbls[0].mul([le(k) for k in ka])
    e4 = tbls[1].mul([le(k) for k in kb])
    t1 = tbls[2].mul([le(k) for k in kc])
    t2 = tbls[3].mul([le(k) for k in kb])
    e5 = eng.g1_add(t1, t2)
    return [e for row in zip(e3, e4, e5) for e in row]


def check(eng, tbls, call):
    got, want = fused(eng, tbls, call), four_launches(eng, tbls, call)
    logs = call.want_logs()
    for t in range(call.n_rows):
        for j in range(3):
            assert got[3 * t + j] == want[3 * t + j], (call.key.name, t, j, call.note[t])
            assert (got[3 * t + j] == bytes(64)) == (logs[t][j] == 0), (call.key.name, t, j, call.note[t])


@pytest.mark.parametrize("total", lc.ROW_COUNTS)
def test_rows_equal_the_four_table_launches_and_the_addition(world, total):
    eng, keys = world
    key, tbls = keys["random"]
    call = lc.scalar_call(key, total, "gpu")
    if total >= 63:          # every scalar case is among the rows
        assert set(lc.KINDS) <= set(call.note)
    check(eng, tbls, call)


@pytest.mark.parametrize("name", ["random", "same", "opposite"])
def test_e5_special_cases_of_the_addition(world, name):
    eng, keys = world
    key, tbls = keys[name]
    call = lc.special_call(key)
    lc.check_special(call)
    check(eng, tbls, call)
    if name == "opposite":          # a cancelled e5 between live neighbours: the lane's e3 and e4 stand
        got, logs = fused(eng, tbls, call), call.want_logs()
        for t in (0, 1, 2, 3):
            assert got[3 * t + 2] == bytes(64)
            assert got[3 * t] == bn.g1_to_le(bn.g1_mul(bn.G1_GEN, logs[t][0])) and got[3 * t + 1] == bn.g1_to_le(bn.g1_mul(bn.G1_GEN, logs[t][1]))


def test_scalar_cases_under_the_degenerate_keys(world):
    eng, keys = world
    for name in ("same", "opposite"):
        key, tbls = keys[name]
        check(eng, tbls, lc.scalar_call(key, 65, "gpu"))


def test_empty_call_and_tables_without_wide_windows(world):
    eng, keys = world
    key, tbls = keys["random"]
    d_out = eng.alloc(192)
    z = eng.upload(bytes(32))
    off = eng.upload_u32([0, 0])
    E.lsw_encrypt_rows_dev(eng, tbls[0], tbls[1], tbls[2], tbls[3], 0, 0, off, off, z, z, z, d_out)          # nothing to do: no launch
    plain = eng.g1_table(key.points()[0])          # 8-bit windows only: refused, not walked
    try:
        with pytest.raises(E.EngineError):
            E.lsw_encrypt_rows_dev(eng, plain, tbls[1], tbls[2], tbls[3], 1, 1, eng.upload_u32([0, 1]), eng.upload_u32([0]), z, z, z, d_out)
    finally:
        plain.destroy()
