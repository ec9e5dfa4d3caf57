"""tests/set_edge_cases.py before a GPU sees it: every case reaches the condition it was built for, and tests/set_model.py
equals the oracle's regex reader on E(S) wherever the reader accepts the list (tests/test_gpu_set_edges.py takes XSG_MATCHES
from the model)."""
from pathlib import Path

import numpy as np
import pytest

import corpus
import packing
import set_cases as SC
import set_edge_cases as E
import set_model
import xsg
from gpu_util import oracle_rx_all_modes
from xs_oracle import RegexProgram, UnsupportedRegex

ROOT = Path(__file__).resolve().parents[1]
IC = xsg.FLAG_IGNORE_CASE
TILE = SC.TILE


def model_is_oracle(oracle, blocks, lits, icase=False):
    """-> the expected dict; asserts that the oracle's reader took the list and that the model says the same"""
    prog = RegexProgram(set_model.expression(lits), icase)
    want = oracle_rx_all_modes(oracle, list(blocks), prog)  # (what set_cases.expected returns for a list the reader takes)
    assert set_model.all_modes(list(blocks), lits, icase) == want
    return want


def match_starts(blocks, lits, icase=False):
    """-> per chunk, the chunk-local start of every match"""
    return [[s for s, _ in set_model.Occurrences(b, lits, icase).spans()] for b in blocks]


# ---- A. the grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [2048, 24, 8 * 304 + 1], ids=["256cu", "3cu", "odd"])
def test_grid_case_makes_every_workgroup_loop(oracle, grid):
    """(2048 = 8 x 256 compute units, an MI355X; the generator takes any grid, an odd one too)"""
    case = E.grid_case(grid)
    blocks = case.blocks
    tiles = E.tiles_of(blocks)
    assert all(1 <= b.size <= 40 or TILE + 1 <= b.size <= TILE + 17 for b in blocks)
    assert {int(b.size) - TILE for b in blocks if b.size > TILE} >= set(range(1, 6))  # chunks that own two tiles
    for icase in (False, True):
        starts = match_starts(blocks, E.GRID_LITS, icase)
        hit = [any(o <= s < o + TILE for s in starts[c]) for c, o in tiles]
        E.grid_conditions(case, grid, hit)  # tile count, hit as a function of the tile, alternation, chunk changes
        # tiles with candidates and no match: the emit pass has work there that the result does not show
        flags = IC if icase else 0
        idle = [t for t, (c, o) in enumerate(tiles)
                if not hit[t] and 8 <= blocks[c].size <= 40 and E.candidates(blocks[c], E.GRID_LITS, flags).size]
        assert len(idle) >= len(tiles) // 8
    want = model_is_oracle(oracle, blocks, E.GRID_LITS)
    assert model_is_oracle(oracle, blocks, E.GRID_LITS, True)["count_matches"] > want["count_matches"] > len(tiles) // 2


def test_grid_case_packed_tightly_is_hostile():
    """every chunk that ends inside an occurrence has the completing bytes right behind its end; stale matches in the pads"""
    case = E.grid_case(2048)
    packed = packing.pack_tight(case.blocks, E.grid_fill(case))
    cut = [c for c, l in enumerate(case.lack) if l and (-case.blocks[c].size) % 16 >= len(l)]  # (the pad holds what it lacks)
    assert len(cut) >= 300 and {b"le", b"e"} <= {case.lack[c] for c in cut}
    for c in cut[:60] + cut[-60:]:
        alone = set_model.Occurrences(case.blocks[c], E.GRID_LITS).spans()
        o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
        seen = set_model.Occurrences(packed.host[o:o + n + 8], E.GRID_LITS).spans()
        more = [s for s in seen if s[0] < n and s not in alone]
        assert len(more) == 1 and more[0][0] < n < more[0][0] + more[0][1], c
    pads = b"".join(packed.host[packed.base + int(o) + int(n):packed.base + int(o) + packing.round_up16(n)].tobytes()
                    for o, n in zip(packed.offsets, packed.lengths))
    assert pads.count(b"needle") > 100 and pads.count(b"kqzw") > 100


# ---- B. the walk ------------------------------------------------------------------------------------------------------------------
def heads_and_kept(cand, lens):
    """the walk the kernels resolve in parallel, done in order: -> (head, kept) per candidate of one chunk"""
    head, kept = np.zeros(cand.size, dtype=bool), np.zeros(cand.size, dtype=bool)
    run = last = 0
    for i, (p, n) in enumerate(zip(cand.tolist(), lens)):
        if n:
            head[i] = p >= run
            if p >= last:
                kept[i], last = True, p + n
            run = max(run, p + n)
    return head, kept


def verified(block, cand, lits):
    occ = set_model.Occurrences(block, lits)
    at = dict(zip(occ.pos, occ.len))
    return [at.get(int(p), 0) for p in cand]


def test_walk_periodic_reaches_the_second_scan_iteration(oracle):
    big, small = E.walk_periodic()
    cand = E.candidates(big, E.PERIODIC_LITS)
    assert cand.size > E.WALK_SCAN + E.WALK_BLOCK
    d = big.tobytes()
    kind = [d[p:p + 2] for p in cand.tolist()]
    assert set(kind) == {b"ab", b"bc", b"de"}
    lens = verified(big, cand, E.PERIODIC_LITS)
    assert all(lens)  # every candidate is an occurrence
    head, kept = heads_and_kept(cand, lens)
    by_kind = {k: {(bool(h), bool(x)) for kk, h, x in zip(kind[1:], head[1:], kept[1:]) if kk == k} for k in set(kind)}
    assert by_kind == {b"ab": {(True, True)}, b"bc": {(False, False)}, b"de": {(False, True)}}  # head, covered, kept non-head
    # candidate number 524 288, the first of the second iteration of k_rx_block_max_scan: a `bcd` covered by the `abc` before it
    assert kind[E.WALK_SCAN] == b"bc" and kind[E.WALK_SCAN - 1] == b"ab" and cand[E.WALK_SCAN - 1] + 3 > cand[E.WALK_SCAN]
    for step in (E.WALK_BLOCK, E.WALK_WAVE, E.WALK_ITEMS):  # every phase is the first candidate of a block, a wave, a thread
        assert {kind[i] for i in range(step, cand.size, step)} == {b"ab", b"bc", b"de"}, step
    # the second chunk: its candidates lie below the first chunk's last end, and are heads of their own
    assert E.candidates(small, E.PERIODIC_LITS)[0] == 0 and cand[-1] > small.size
    want = model_is_oracle(oracle, (big, small), E.PERIODIC_LITS)
    assert want["count_matches"] == int(kept.sum()) + 6 and want["match_byte_offsets"][-6:] == [big.size + x for x in (0, 3, 6, 9, 12, 17)]


def test_walk_long_cover_crosses_every_boundary(oracle):
    big, small = E.walk_long_cover()
    cand = E.candidates(big, E.COVER_LITS)
    assert cand.size > E.WALK_SCAN + E.WALK_BLOCK
    d = big.tobytes()
    at, i = [], d.find(E.COVER_X)
    while i >= 0:
        at.append(i)
        i = d.find(E.COVER_X, i + 1)
    index = [int(np.searchsorted(cand, p)) for p in at]
    assert tuple(index) == E.COVER_AT and all(cand[k] == p for k, p in zip(index, at))
    for k, (m, others) in zip(index, ((8, (512,)), (512, (2048,)), (2048, (E.WALK_SCAN,)), (E.WALK_SCAN, ()))):
        assert k % m == m - 1 and all(k % o != o - 1 for o in others)  # the last of a thread, a wave, a block, an iteration -- in turn
        assert cand[k + 127] < cand[k] + 255 <= cand[k + 128]  # the 127 candidates behind it are covered: they begin the next one
    lens = verified(big, cand, E.COVER_LITS)
    head, kept = heads_and_kept(cand, lens)
    for k in index:
        assert lens[k] == 255 and head[k] and not head[k + 1:k + 128].any() and not kept[k + 1:k + 128].any() and head[k + 128]
    assert E.candidates(small, E.COVER_LITS)[0] == 0
    want = model_is_oracle(oracle, (big, small), E.COVER_LITS)
    assert want["count_matches"] == int(kept.sum()) + 3 + 1 + 1 + 2


# ---- C. the fold ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,gi", E.FOLD_CASES, ids=["g%d-%s" % (g, E.FOLD_GROUPS[gi].name) for g, gi in E.FOLD_CASES])
def test_fold_case_places_every_byte_at_every_position(oracle, g, gi):
    case = E.fold_case(g, gi)
    group = case.group
    assert xsg.literals_info(xsg.literal_list(case.lits), IC)["gram"] == g == min(len(l) for l in case.lits)
    assert len(case.lits) <= xsg.MAX_LITERALS and len(xsg.literal_list(case.lits)) <= xsg.MAX_PATTERN
    text = b"".join(b.tobytes() for b in case.blocks)
    for b in group.values:  # b at every gram position and behind the gram, each at all 16 offsets of a unit
        for j in range(g + 1):
            lit = [l for l in case.lits if len(l) == (g + 1 if j == g else g) and l[j] == b and l[:j] == group.filler[:j]][0]
            for s in {lit, lit.swapcase()}:
                seen, i = set(), text.find(s)
                while i >= 0:
                    seen.add(i % 16)
                    i = text.find(s, i + 1)
                assert seen == set(range(16)), (b, j, s)
            assert E.false_partner(b) not in group.values
    if gi < 2:  # the ASCII half (NUL included): the oracle reads it
        want = model_is_oracle(oracle, case.blocks, case.lits, True)
        plain = model_is_oracle(oracle, case.blocks, case.lits, False)
    else:  # bytes >= 0x80 that are no UTF-8: the reader refuses, the model answers
        with pytest.raises(UnsupportedRegex):
            RegexProgram(set_model.expression(case.lits), True)
        want = SC.expected(oracle, list(case.blocks), case.lits, True)
        plain = SC.expected(oracle, list(case.blocks), case.lits, False)
        assert want == set_model.all_modes(list(case.blocks), case.lits, True)
    letters = any(65 <= b <= 90 or 97 <= b <= 122 for b in group.values)
    assert (want["count_matches"] > plain["count_matches"]) == letters and plain["count_matches"] >= 16 * len(case.lits) - 2
    # the false partners are in the text, 16 times each, and no match is one of them
    assert len(case.partners) >= (g + 1) * 2
    found = set(set_model.matches(list(case.blocks), case.lits, True)[0])
    for p in case.partners:
        assert text.count(p) >= 15 and p not in found and p not in case.lits


def test_fold_cases_cover_both_halves():
    groups = [E.FOLD_GROUPS[gi] for _, gi in E.FOLD_CASES]
    assert {b for gr in groups for b in gr.values} == set(range(256)) - {10}
    ascii_half = [gr for gr in E.FOLD_GROUPS if max(gr.values) < 0x80]
    high_half = [gr for gr in E.FOLD_GROUPS if min(gr.values) >= 0x80]
    assert ascii_half and high_half and len(ascii_half) + len(high_half) == len(E.FOLD_GROUPS)
    assert {g for g, _ in E.FOLD_CASES} == {1, 2, 3, 4} == {g for g, _ in E.FOLD_PLAIN}
    edges = (0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0xC1, 0xDA, 0xE1, 0xFA)
    assert all(any(b in gr.values for gr in E.FOLD_GROUPS) for b in edges)
    assert [E.false_partner(b) for b in (0x40, 0x60, 0x5B, 0x7B, 0xC1, 0xDA, 0xE1, 0xFA, 0x41, 0xC0, 0xDB)] == \
        [0x60, 0x40, 0x7B, 0x5B, 0xE1, 0xFA, 0xC1, 0xDA, None, None, None]


# ---- D. collisions and limits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [3, 4])
def test_collision_case_holds_false_positives_of_the_filter(oracle, g):
    lits, blocks, fakes = E.collision_case(g)
    d0, f0 = xsg.literals_info(xsg.literal_list(lits), 0, with_filter=True)
    assert d0["gram"] == g and d0["filter_bits_set"] == len(lits)
    grams = set()
    for gram, cs in E.colliding_grams(g).items():
        assert gram in {l[:g] for l in lits} and len(cs) >= 8 and gram not in cs
        assert tuple(cs[:8]) == E.COLLIDING_PINNED[gram]  # the strings of tests/cpp/set_selftest.cpp: collision_cases
        src = (ROOT / "tests" / "cpp" / "set_selftest.cpp").read_bytes()
        assert all(b'"' + c.replace(b"\\", b"\\\\").replace(b'"', b'\\"') + b'"' in src for c in cs[:8])
        for c in cs[:24]:
            # the Python hash is the product's: the filter image of [c + tail] has the single bit of [gram + tail]
            d1, f1 = xsg.literals_info(c + b"tail", 0, with_filter=True)
            d2, f2 = xsg.literals_info(gram + b"tail", 0, with_filter=True)
            assert d1["filter_bits_set"] == 1 and np.array_equal(f1, f2)
            assert xsg.literal_gram_hash(int.from_bytes(c, "little"), g) == xsg.literal_gram_hash(int.from_bytes(gram, "little"), g)
            grams.add(c)
    want = model_is_oracle(oracle, blocks, lits)
    starts = match_starts(blocks, lits)
    text = [b.tobytes() for b in blocks]
    in_text = set()
    for s in fakes:
        where = [(c, t.find(s)) for c, t in enumerate(text) if s in t]
        assert where, s
        for c, p in where:
            assert p in E.candidates(blocks[c], lits) and p not in starts[c]  # a candidate, and no match
        in_text.add(s[:g])
    assert in_text <= grams and len(in_text) >= 8
    # lane and tile edges: a colliding string and a real occurrence begin one byte in front of them
    assert not set(fakes) & set(set_model.matches(list(blocks), lits)[0])
    assert {31, 4095, TILE - 1} <= set(starts[0])
    assert text[0].startswith(fakes[0], 15) and text[0].startswith(fakes[3], 2 * TILE - 1) and text[1].endswith(fakes[0])
    assert want["count_matches"] == 4 * len(lits) + 3 + 1


def test_limit_lists_are_at_the_limits():
    shared, distinct = E.limit_shared(), E.limit_distinct()
    for lits, keys in ((shared, 1), (distinct, 4096), (E.LIMIT_LONG, 2), (E.LIMIT_SMALL, 2)):
        d = xsg.literals_info(xsg.literal_list(lits))
        assert d["gram"] == 4 and len({l[:4] for l in lits}) == keys and d["count"] == len(lits)
        assert keys - 140 <= d["filter_bits_set"] <= keys  # (4096 grams on 65 536 bits: ~125 share a bit)
    assert len(shared) == len(distinct) == xsg.MAX_LITERALS
    assert xsg.MAX_PATTERN - 3 <= len(xsg.literal_list(shared)) <= xsg.MAX_PATTERN
    assert len(xsg.literal_list(distinct)) == xsg.MAX_PATTERN - 1
    with pytest.raises(xsg.XsgError):  # one literal more is refused
        xsg.literals_info(xsg.literal_list(distinct + (b"abcdefg",)))
    assert [len(l) for l in E.LIMIT_LONG] == [xsg.MAX_LITERAL_BYTES, 4]
    filled = xsg.literals_info(xsg.literal_list(distinct))["filter_bits_set"] / 65536
    assert 0.055 < filled < 0.0626  # about 6 % of the filter


@pytest.mark.parametrize("name,lits", E.LIMIT_LISTS, ids=[n for n, _ in E.LIMIT_LISTS])
def test_limit_texts_hold_the_planted_literals(oracle, name, lits):
    lits = lits()
    case = E.limit_blocks()
    want = model_is_oracle(oracle, case.blocks, lits)  # (the reader compiles 4096 alternatives in a fraction of a second)
    found = set(set_model.matches(list(case.blocks), lits)[0])
    assert {lits[0], lits[len(lits) // 2 - 1], lits[-1]} <= found and want["count_matches"] >= 20
    if name == "shared":
        assert {E.ROOM_SHORT, lits[1234], lits[16]} <= found and b"abcdqaa" not in found
        assert len(found) > 40


def test_limit_room_case_is_hostile():
    """the chunk ends in `abcdb`; `abcdbaa`, listed 2744 places in front of `abcdb`, is completed by the bytes behind the
    end: a reader past the end reports 7 bytes, the chunk alone holds 5"""
    case = E.limit_blocks()
    lits = E.limit_shared()
    assert lits.index(E.ROOM_SHORT + b"aa") < lits.index(E.ROOM_SHORT) and [l for l in lits if len(l) != 7] == [E.ROOM_SHORT]
    packed = packing.pack_tight(case.blocks, E.limit_fill(case))
    c = case.lack.index(b"aa")
    n = int(packed.lengths[c])
    o = packed.base + int(packed.offsets[c])
    alone = set_model.Occurrences(case.blocks[c], lits).spans()
    naive = [s for s in set_model.Occurrences(packed.host[o:o + n + 255], lits).spans() if s[0] < n]
    assert alone[-1] == (n - 5, 5) and naive[-1] == (n - 5, 7) and alone[:-1] == naive[:-1]
    c = case.lack.index(b"d")  # `abc` + `d` behind the end, for the small list
    n, o = int(packed.lengths[c]), packed.base + int(packed.offsets[c])
    assert packed.host[o + n - 3:o + n + 1].tobytes() == b"abcd"
    assert (n - 3, 4) not in set_model.Occurrences(case.blocks[c], E.LIMIT_SMALL).spans()


# ---- E. NUL bytes ------------------------------------------------------------------------------------------------------------------
def upload_layout(blocks):
    """gpu_util.upload without a device: every chunk on a 256-byte boundary in zeroed memory"""
    off, ln, cap = corpus.chunk_table([int(b.size) for b in blocks])
    host = np.zeros(max(cap, 256), dtype=np.uint8)
    for o, b in zip(off, blocks):
        host[int(o):int(o) + b.size] = b
    return packing.Packed(host, 0, cap, np.asarray(off, dtype=np.uint64), np.asarray(ln, dtype=np.uint64))


@pytest.mark.parametrize("k", range(len(E.NUL_LISTS)))
def test_nul_layouts_are_hostile(oracle, k):
    """as test_set_host.py::test_the_chunk_end_layout_is_hostile: the zeros behind a chunk's end -- the pad, the chunk of
    NULs that follows, the zeroed memory of gpu_util.upload -- are the bytes that complete an occurrence cut at the end, or
    occurrences of their own that begin in the pad"""
    lits = E.NUL_LISTS[k]
    blocks = E.nul_blocks()
    assert sorted(int(b.size) for b in blocks if not b.any()) == sorted(E.NUL_RUNS)
    cut = E.nul_cut_chunks()
    assert sorted((int(blocks[c].size) % 16, int((blocks[c][-3:] == 0).sum())) for c in cut) == \
        sorted((r, n) for r in (13, 14, 15, 0) for n in (1, 2, 3))
    model_is_oracle(oracle, blocks, lits)
    zero = lambda i, n: np.zeros(n, dtype=np.uint8)
    for layout, packed in (("upload", upload_layout(blocks)), ("tight", packing.pack_tight(blocks, zero))):
        inside, in_pad = [], []
        for c in cut:
            alone = set_model.Occurrences(blocks[c], lits).spans()
            n = int(blocks[c].size)
            o = packed.base + int(packed.offsets[c])
            seen = set_model.Occurrences(packed.host[o:o + n + 255], lits).spans()
            if [s for s in seen if s[0] < n] != alone:
                inside.append(c)
            if any(n <= s[0] < packing.round_up16(n) for s in seen):
                in_pad.append(c)
        padded = [c for c in cut if blocks[c].size % 16]
        if k == 0:  # `\0`: nothing is cut, the pad holds occurrences of its own
            assert not inside and in_pad == padded
        elif k == 1:  # `\0\0` in front of `\0`: an odd run of NULs at the end grows by one, an even one is followed by more
            assert inside == [c for c in cut if int((blocks[c][-3:] == 0).sum()) != 2]
            assert set(inside) | set(in_pad) == set(cut) - {c for c in cut if c not in padded and c not in inside}
        else:  # `\0\0\0\0`: one to three NULs at the end, the rest behind it
            nuls = lambda c: int((blocks[c][-3:] == 0).sum()) + (-blocks[c].size) % 16  # (its own and the pad's)
            want = cut if layout == "upload" else [c for c in cut if nuls(c) >= 4 or blocks[c].size % 16 == 0]
            assert inside == want, layout
