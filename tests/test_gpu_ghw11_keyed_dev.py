"""rhip_ghw11_transform_batch_keyed driven directly (include/rabe_hip.h): ONE prepared-lines handle over the elements of two keys, a line base
per item.  Its output must be rhip_ghw11_transform_batch's under the item's key's own handle on the same device arrays, bit for bit; an item
whose dev_item_ok is 0 comes back as zeros.  The arrays are the synthetic ones of tests/decrypt_launch_cases.py (multiples of the generators, a
coefficient above r / 2 in every selection); the shapes reach the uniform, the lane = pair and the tiled gather maps."""
import pytest

from oracle import bn254 as bn
from rabe_amd import engine as E
from tests import decrypt_launch_cases as cases

pytestmark = pytest.mark.gpu
GT = cases.GT
ELEMENTS = 2 + cases.ROWS          # k_z, l_z, k_x[0 .. 3]


@pytest.fixture(scope="module")
def world():
    eng = E.Engine(0)
    yield cases.World(eng)
    eng.close()


@pytest.mark.parametrize("shape", ["uniform3", "ragged5", "tiled65", "empty"])
def test_keyed_equals_the_one_key_call_per_key(world, shape):
    w, eng = world, world.eng
    s = cases.Selection(w, shape)
    mx, total, d_off = s.pairs(w, 1, 2)
    keys = [w.g2_list(ELEMENTS, 9), w.g2_list(ELEMENTS, 4)]
    own = [E.G2Lines(eng, ELEMENTS, eng.upload(b"".join(k))) for k in keys]
    store = E.G2Lines(eng, 2 * ELEMENTS, eng.upload(b"".join(keys[0] + keys[1])))
    assert store.nbytes() == 2 * own[0].nbytes() and own[0].nbytes() in (ELEMENTS * (88 * 192 + 1), ELEMENTS * (88 * 192 + 1 + 88 * 144))
    args = (s.n, mx, total, s.n_sel, d_off, s.d_start, s.d_a, s.d_b, s.d_coeff, w.g1(s.n, 3), w.g1(cases.ROWS * s.n, 5), w.g1(cases.ROWS * s.n, 10), s.d_row_off)
    ref = []
    for lines in own:
        d_out = eng.upload(bytes(s.n * GT))
        E.ghw11_transform_dev(eng, *args, lines, d_out)
        ref.append(eng.download(d_out, s.n * GT))
    assert ref[0] != ref[1]
    item_key = [(i // 2 + i) % 2 for i in range(s.n)]          # 0, 1, 1, 0, 0, 1, ...: both keys inside every wave
    skipped = 1 if s.n > 1 else None
    ok = [0 if i == skipped else 1 for i in range(s.n)]
    d_base = w.u32([ELEMENTS * u for u in item_key])
    for d_ok in (None, w.u32(ok)):
        d_out = eng.upload(bytes(s.n * GT))
        E.ghw11_transform_keyed_dev(eng, *args, d_base, d_ok, store, d_out)
        got = eng.download(d_out, s.n * GT)
        for i in range(s.n):
            want = bytes(GT) if d_ok is not None and not ok[i] else ref[item_key[i]][GT * i:GT * (i + 1)]
            assert got[GT * i:GT * (i + 1)] == want, (shape, i, d_ok is not None)
    # a base beyond the handle reads nothing: the item is skipped like one that is not ok, its neighbours are served
    d_out = eng.upload(bytes(s.n * GT))
    E.ghw11_transform_keyed_dev(eng, *args, w.u32([2 * ELEMENTS if i == 0 else ELEMENTS * item_key[i] for i in range(s.n)]), None, store, d_out)
    got = eng.download(d_out, s.n * GT)
    assert got[GT:] == b"".join(ref[item_key[i]][GT * i:GT * (i + 1)] for i in range(1, s.n))
    assert got[:GT] == bn.gt_to_le(bn.GT_ONE)          # every pair of item 0 skipped, no dev_item_ok: the empty product
    with pytest.raises(E.EngineError):
        E.ghw11_transform_keyed_dev(eng, *args, None, None, store, d_out)          # no line bases: RHIP_ERR_ARG
    for h in own + [store]:
        h.destroy()
