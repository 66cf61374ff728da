"""rhip_assemble_records and rhip_gather_parts (k_assemble_records, k_gather_parts: every record of a packed encrypt is written by the first,
every part of a packed decrypt is pulled out by the second) driven with layouts of the test's own, byte for byte -- guard bytes included --
against the plain Python of tests/record_mover_cases.py.  The first test needs no GPU: it proves the case tables well-formed."""
import array
import ctypes

import pytest

from rabe_amd import Engine, EngineError
from tests import record_mover_cases as rc

RHIP_ERR_ARG = -3
FILL = rc.FILL


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_case_tables_are_well_formed_and_the_reference_inverts_itself():
    """no table indexes outside its arrays, records and guards do not overlap, and gathering what the reference assembled returns every
    source byte a record read"""
    for name, make in rc.ASSEMBLE_CASES.items():
        case, guards = make()
        rc.check_assemble(case, guards)
        out = rc.assemble_ref(**case)
        assert len(out) == case["out_size"]
        for at, length in guards:
            assert out[at:at + length] == bytes([FILL]) * length, name
        back, read = rc.inverse_parts(case)
        rc.check_gather(dict(back, blob=out), guard=0, overlap=True)
        assert rc.gather_ref(blob=out, **back) == read, name
        assert any(r != bytes([FILL]) * len(r) for r in read)
    case, guards = rc.marker_case()
    assert len(case["sources"]) == rc.N_SRC_MAX and max(v >> 24 for v in case["map_words"] if v >> 24 != 0xFF) == rc.N_SRC_MAX - 1
    assert rc.lit(0xFF) == 0xFF0000FF and rc.lit(0xFF) in case["map_words"]
    case, _ = rc.lengths_case()
    assert sorted({case["layout_off"][l + 1] - case["layout_off"][l] for l in case["layout"]}) == [0, 1, 255, 256, 257, 511, 513, 3000]
    case, _ = rc.offsets_case()
    assert max(v & 0xFFFFFF for v in case["map_words"] if v >> 24 == 0) == 69999
    gather = rc.gather_case()
    rc.check_gather(gather)
    got = rc.gather_ref(**gather)
    assert got[5] == bytes([FILL]) * gather["dst_sizes"][5]
    assert all(d[:rc.GUARD] == d[-rc.GUARD:] == bytes([FILL]) * rc.GUARD for d in got)
    assert sorted(set(gather["part_len"])) == [0, 1, 31, 33, 64, 255, 256, 257, 1025] and 0 in gather["layout_off"][1:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rc.ASSEMBLE_CASES))
def test_assemble_records(eng, name):
    """record lengths around the block's 256-byte stride at odd output offsets; the literal marker beside the largest source index; source
    offsets past 2^16 and per-item offsets in any order -- the whole output, guards included"""
    case, _ = rc.ASSEMBLE_CASES[name]()
    assert eng.assemble_records(fill=FILL, **case) == rc.assemble_ref(**case)


@pytest.mark.gpu
def test_assemble_records_source_count_limit(eng):
    """254 sources are taken (the marker case above), 255 are RHIP_ERR_ARG: the top byte 0xFF of a map word is the literal marker"""
    case, _ = rc.marker_case(rc.N_SRC_MAX + 1)
    rc.check_assemble(case)
    with pytest.raises(EngineError, match=r"\(%d\)" % RHIP_ERR_ARG):
        eng.assemble_records(fill=FILL, **case)


@pytest.mark.gpu
def test_gather_parts(eng):
    """a layout without parts, parts of 0 .. 1025 bytes, overlapping reads, adjacent writes, odd record offsets, seven destinations of
    which one receives nothing -- every destination whole, guards included"""
    case = rc.gather_case()
    assert eng.gather_parts(fill=FILL, **case) == rc.gather_ref(**case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lengths", "offsets"])
def test_round_trip_on_the_device(eng, name):
    """assemble_records, then gather_parts on its output with the inverse part list: every source byte a record read comes back"""
    case, _ = rc.ASSEMBLE_CASES[name]()
    back, read = rc.inverse_parts(case)
    blob = eng.assemble_records(fill=FILL, **case)
    assert eng.gather_parts(blob=blob, fill=FILL, **back) == read


@pytest.mark.gpu
def test_empty_calls_and_null_pointers(eng):
    assert eng.assemble_records(16, [], [], [0], [], [], [], fill=FILL) == bytes([FILL]) * 16
    assert eng.gather_parts(b"abc", [], [], [0], [], [], [], [], [8], [], fill=FILL) == [bytes([FILL]) * 8]
    keep = []          # the device buffers of the argument lists below, alive until the end

    def u64(values):
        keep.append(eng.upload(array.array("Q", values).tobytes()))
        return keep[-1].ptr

    def u32(values):
        keep.append(eng.upload_u32(values))
        return keep[-1].ptr

    src, dst, out = eng.upload(b"\x11" * 4), eng.upload(bytes([FILL]) * 4), eng.upload(bytes([FILL]) * 4)
    one, zero = ctypes.c_size_t(1), ctypes.c_size_t(0)
    # one record of two bytes: a literal and byte 1 of source 0
    args = [out.ptr, u64([1]), u32([0]), u32([0, 2]), u32([rc.lit(0x77), rc.src(0, 1)]), ctypes.c_uint32(1), u64([src.ptr.value]), u64([0])]
    for j in (0, 1, 2, 3, 4, 6, 7):
        assert eng.lib.rhip_assemble_records(eng.ctx, one, *[None if i == j else a for i, a in enumerate(args)]) == RHIP_ERR_ARG, j
    assert eng.lib.rhip_assemble_records(eng.ctx, zero, *[a if i == 5 else None for i, a in enumerate(args)]) == 0
    assert eng.download(out, 4) == bytes([FILL]) * 4
    assert eng.lib.rhip_assemble_records(eng.ctx, one, *args) == 0
    assert eng.download(out, 4) == bytes([FILL, 0x77, 0x11, FILL])
    # one record, one part: two bytes from record offset 1 to destination offset 1
    args = [out.ptr, u64([0]), u32([0]), u32([0, 1]), u32([1]), u32([1]), u32([2]), u32([0]), u64([dst.ptr.value]), u64([0])]
    for j in range(len(args)):
        assert eng.lib.rhip_gather_parts(eng.ctx, one, *[None if i == j else a for i, a in enumerate(args)]) == RHIP_ERR_ARG, j
    assert eng.lib.rhip_gather_parts(eng.ctx, zero, *[None] * len(args)) == 0
    assert eng.download(dst, 4) == bytes([FILL]) * 4
    assert eng.lib.rhip_gather_parts(eng.ctx, one, *args) == 0
    assert eng.download(dst, 4) == bytes([FILL, 0x77, 0x11, FILL])
