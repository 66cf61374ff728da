"""rhip_assemble_records / rhip_gather_parts restated in plain Python from the comment in include/rabe_hip.h, and the case tables of
tests/test_gpu_record_movers.py.  A case is the keyword arguments of Engine.assemble_records / Engine.gather_parts (and of the reference
here); check_assemble / check_gather walk a table the way the kernels do and fail on any index outside its arrays, on records that
overlap and on guard bytes that a record covers, so the tables are proven well-formed without a GPU."""
import random

FILL = 0xA5
GUARD = 8


def lit(v):
    return 0xFF000000 | v


def src(k, o):
    return k << 24 | o


def assemble_ref(out_size, out_off, layout, layout_off, map_words, sources, src_item_off, fill=FILL):
    """byte b of item i's record = map_words[layout_off[layout[i]] + b]: 0xFF0000vv the literal vv, k << 24 | o byte o of item i's part in
    source k, which starts at src_item_off[k * n + i]"""
    n = len(out_off)
    out = bytearray([fill]) * out_size
    for i in range(n):
        words = map_words[layout_off[layout[i]]:layout_off[layout[i] + 1]]
        for b, v in enumerate(words):
            k, o = v >> 24, v & 0xFFFFFF
            out[out_off[i] + b] = v & 0xFF if k == 0xFF else sources[k][src_item_off[k * n + i] + o]
    return bytes(out)


def gather_ref(blob, rec_off, layout, layout_off, part_src, part_dst, part_len, part_k, dst_sizes, dst_item_off, fill=FILL):
    """part p of item i's layout copies part_len[p] bytes from record offset part_src[p] to destination k = part_k[p] at
    dst_item_off[k * n + i] + part_dst[p]"""
    n = len(rec_off)
    dst = [bytearray([fill]) * s for s in dst_sizes]
    for i in range(n):
        for p in range(layout_off[layout[i]], layout_off[layout[i] + 1]):
            k, s, d = part_k[p], rec_off[i] + part_src[p], dst_item_off[part_k[p] * n + i] + part_dst[p]
            dst[k][d:d + part_len[p]] = blob[s:s + part_len[p]]
    return [bytes(d) for d in dst]


def check_assemble(case, guards=()):
    """every index inside its array, no two records on one output byte, no record on a guard byte (guards: (offset, length) pairs)"""
    n, n_src = len(case["out_off"]), len(case["sources"])
    assert len(case["layout"]) == n and len(case["src_item_off"]) == n_src * n
    taken = bytearray(case["out_size"])
    for at, length in guards:
        assert 0 <= at and at + length <= case["out_size"]
        taken[at:at + length] = b"\1" * length
    for i in range(n):
        l = case["layout"][i]
        assert 0 <= l < len(case["layout_off"]) - 1
        m0, m1 = case["layout_off"][l], case["layout_off"][l + 1]
        assert 0 <= m0 <= m1 <= len(case["map_words"])
        assert 0 <= case["out_off"][i] and case["out_off"][i] + (m1 - m0) <= case["out_size"]
        for b in range(m1 - m0):
            assert not taken[case["out_off"][i] + b], ("record %d lies on a guard or on another record" % i)
            taken[case["out_off"][i] + b] = 1
            v = case["map_words"][m0 + b]
            assert 0 <= v < 1 << 32
            if v >> 24 != 0xFF:
                assert v >> 24 < n_src
                assert 0 <= case["src_item_off"][(v >> 24) * n + i] + (v & 0xFFFFFF) < len(case["sources"][v >> 24])


def check_gather(case, guard=GUARD, overlap=False):
    """every index inside its array, every copy inside the blob and inside its destination less `guard` bytes at either end, no
    destination byte written by two parts (unless `overlap`: the inverse of an assemble case that reads a source byte twice)"""
    n, n_dst, n_parts = len(case["rec_off"]), len(case["dst_sizes"]), len(case["part_k"])
    assert len(case["layout"]) == n and len(case["dst_item_off"]) == n_dst * n
    assert len(case["part_src"]) == len(case["part_dst"]) == len(case["part_len"]) == n_parts
    taken = [bytearray(s) for s in case["dst_sizes"]]
    for i in range(n):
        l = case["layout"][i]
        assert 0 <= l < len(case["layout_off"]) - 1
        p0, p1 = case["layout_off"][l], case["layout_off"][l + 1]
        assert 0 <= p0 <= p1 <= n_parts
        for p in range(p0, p1):
            k, length = case["part_k"][p], case["part_len"][p]
            assert 0 <= k < n_dst and 0 <= length
            s, d = case["rec_off"][i] + case["part_src"][p], case["dst_item_off"][k * n + i] + case["part_dst"][p]
            assert 0 <= s and s + length <= len(case["blob"])
            assert guard <= d and d + length <= case["dst_sizes"][k] - guard
            assert overlap or not any(taken[k][d:d + length]), ("part %d of record %d lies on another part" % (p, i))
            taken[k][d:d + length] = b"\1" * length


def inverse_parts(case):
    """the gather that undoes an assemble case: one part per run of map words that walk one source upwards; the destinations are shaped
    like the sources.  Returns (the gather's keyword arguments less `blob`, the sources with every byte no record reads set to FILL)."""
    n = len(case["out_off"])
    part_src, part_dst, part_len, part_k, layout_off = [], [], [], [], [0]
    for l in range(len(case["layout_off"]) - 1):
        words = case["map_words"][case["layout_off"][l]:case["layout_off"][l + 1]]
        b = 0
        while b < len(words):
            e = b + 1
            if words[b] >> 24 != 0xFF:
                while e < len(words) and words[e] == words[e - 1] + 1 and words[e] >> 24 == words[b] >> 24:
                    e += 1
                part_src.append(b)
                part_dst.append(words[b] & 0xFFFFFF)
                part_len.append(e - b)
                part_k.append(words[b] >> 24)
            b = e
        layout_off.append(len(part_k))
    seen = [bytearray([FILL]) * len(s) for s in case["sources"]]
    for i in range(n):
        for p in range(layout_off[case["layout"][i]], layout_off[case["layout"][i] + 1]):
            at = case["src_item_off"][part_k[p] * n + i] + part_dst[p]
            seen[part_k[p]][at:at + part_len[p]] = case["sources"][part_k[p]][at:at + part_len[p]]
    back = dict(rec_off=case["out_off"], layout=case["layout"], layout_off=layout_off, part_src=part_src, part_dst=part_dst, part_len=part_len,
                part_k=part_k, dst_sizes=[len(s) for s in case["sources"]], dst_item_off=case["src_item_off"])
    return back, [bytes(s) for s in seen]


def _layout(rnd, length, part_sizes):
    """`length` map words: runs of literals and runs that walk a source, of 1 .. 300 bytes"""
    words = []
    while len(words) < length:
        run = min(length - len(words), rnd.choice([1, 2, 3, 31, 32, 64, 128, 300]))
        if rnd.random() < 0.4:
            words += [lit(rnd.randrange(256)) for _ in range(run)]
        else:
            k = rnd.randrange(len(part_sizes))
            run = min(run, part_sizes[k])
            o = rnd.randrange(part_sizes[k] - run + 1)
            words += [src(k, o + j) for j in range(run)]
    return words


def _pack(lengths, gaps_after=()):
    """records back to back from GUARD on, GUARD more bytes after every record named in gaps_after and after the last:
    (out_off, out_size, guards)"""
    at, out_off, guards = GUARD, [], [(0, GUARD)]
    for i, length in enumerate(lengths):
        out_off.append(at)
        at += length
        if i in gaps_after or i == len(lengths) - 1:
            guards.append((at, GUARD))
            at += GUARD
    return out_off, at, guards


def lengths_case():
    """records of 0, 1, 255, 256, 257, 511, 513 and 3000 bytes around the 256-thread stride: 20 items over eight layouts, four of them
    shared, not sorted by layout, packed back to back (most offsets are odd) with guards before, after item 9 and at the end"""
    rnd = random.Random(606)
    lengths = [0, 1, 255, 256, 257, 511, 513, 3000]
    part_sizes = [700, 64, 1500]
    layout = [6, 2, 7, 0, 3, 2, 5, 1, 3, 4, 2, 6, 0, 3, 6, 2, 3, 0, 6, 0]
    n = len(layout)
    assert set(layout) == set(range(8)) and sum(layout.count(l) > 1 for l in range(8)) == 4
    map_words, layout_off = [], [0]
    for length in lengths:
        map_words += _layout(rnd, length, part_sizes)
        layout_off.append(len(map_words))
    out_off, out_size, guards = _pack([lengths[l] for l in layout], gaps_after=(9,))
    assert sum(o % 2 for o in out_off) > n // 3
    sources = [bytes(rnd.randrange(256) for _ in range(n * p)) for p in part_sizes]
    src_item_off = [i * p for p in part_sizes for i in range(n)]
    return dict(out_size=out_size, out_off=out_off, layout=layout, layout_off=layout_off, map_words=map_words, sources=sources,
                src_item_off=src_item_off), guards


N_SRC_MAX = 254          # rhip_assemble_records: a larger n_src is RHIP_ERR_ARG, so 253 is the largest source a map word can name


def marker_case(n_src=N_SRC_MAX):
    """the literal marker 0xFF in a word's top byte next to the largest sources: a layout of literals alone (0xFF0000FF is the byte 0xFF,
    not a read) and one over sources 0, 1, n_src - 2 and n_src - 1; every other source is one shared one-byte dummy"""
    rnd = random.Random(255)
    n, part = 5, 300
    hi = n_src - 1
    dummy = b"\x5a"
    sources = [dummy] * n_src
    for k in (0, 1, hi - 1, hi):
        sources[k] = bytes(rnd.randrange(256) for _ in range(n * part))
    literals = [lit(v) for v in (0xFF, 0x00, 0xFE, 0xFF, 0x01, 0xFD, 0x80, 0xFF)]
    mixed = [src(hi, 0xFF), lit(0xFF), src(hi, 0), src(0, 0xFF), lit(0xFE), src(hi - 1, 0xFE), src(1, 1), lit(0x00), src(hi, 0xFE),
             src(hi - 1, 0xFF)] + [src(hi, 40 + j) for j in range(259)] + [lit(0xFF)]
    layout = [1, 0, 1, 1, 0]
    layout_off = [0, len(literals), len(literals) + len(mixed)]
    out_off, out_size, guards = _pack([layout_off[l + 1] - layout_off[l] for l in layout], gaps_after=(1,))
    src_item_off = [(i * part if len(sources[k]) > 1 else 0) for k in range(n_src) for i in range(n)]
    return dict(out_size=out_size, out_off=out_off, layout=layout, layout_off=layout_off, map_words=literals + mixed, sources=sources,
                src_item_off=src_item_off), guards


def offsets_case():
    """a source offset past 2^16 (byte 69 999 of a 70 000-byte part), per-item source offsets that are odd and go up and down, and two
    items (1 and 3) that read the same source bytes"""
    rnd = random.Random(70000)
    big = 70000
    sources = [bytes(rnd.randrange(256) for _ in range(3 * big + 5)), bytes(rnd.randrange(256) for _ in range(400))]
    item_off = [[2 * big + 3, 1, big + 2, 1], [301, 7, 150, 7]]
    n = 4
    words = [src(0, big - 1), src(0, 0), src(0, 65535), src(0, 65536), src(0, 65537), lit(0xFF), src(1, 98), src(0, big - 2)] + \
        [src(0, 65500 + j) for j in range(70)] + [src(1, j) for j in range(99)]
    layout, layout_off = [0, 0, 0, 0], [0, len(words)]
    out_off, out_size, guards = _pack([len(words)] * n)
    return dict(out_size=out_size, out_off=out_off, layout=layout, layout_off=layout_off, map_words=words, sources=sources,
                src_item_off=[o for per_src in item_off for o in per_src]), guards


ASSEMBLE_CASES = {"lengths": lengths_case, "marker": marker_case, "offsets": offsets_case}


def gather_case():
    """nine records at odd offsets over three layouts -- one without parts; parts of 0, 1, 255, 256, 257 and 1025 bytes; two parts that
    read overlapping record bytes into destinations 4 and 6; three parts of one record that lie adjacent in destination 4 -- into seven
    destinations with GUARD bytes at either end, the items of each in an order of its own; destination 5 receives nothing"""
    rnd = random.Random(77)
    parts = [[],
             [(10, 0, 0, 0), (5, 0, 1, 1), (6, 3, 255, 0), (261, 0, 256, 2), (517, 0, 257, 3), (3, 260, 1025, 2)],
             [(100, 0, 64, 4), (130, 0, 64, 6), (7, 64, 33, 4), (500, 97, 31, 4)]]
    layout = [1, 2, 0, 1, 2, 2, 0, 1, 1]
    n, rec_len = len(layout), 1101
    rec_off = [3 + i * rec_len for i in range(n)]
    blob = bytes(rnd.randrange(256) for _ in range(rec_off[-1] + rec_len + 5))
    stride = [259, 3, 1290, 263, 131, 16, 64]
    dst_sizes = [GUARD + n * s + GUARD for s in stride]
    dst_item_off = []
    for k, s in enumerate(stride):
        order = list(range(n))
        rnd.shuffle(order)
        dst_item_off += [GUARD + order[i] * s for i in range(n)]
    flat = [p for per_layout in parts for p in per_layout]
    layout_off = [0]
    for per_layout in parts:
        layout_off.append(layout_off[-1] + len(per_layout))
    return dict(blob=blob, rec_off=rec_off, layout=layout, layout_off=layout_off, part_src=[p[0] for p in flat], part_dst=[p[1] for p in flat],
                part_len=[p[2] for p in flat], part_k=[p[3] for p in flat], dst_sizes=dst_sizes, dst_item_off=dst_item_off)
