"""xsg_set_max_count on the GPU (include/xsg.h): every tag, count and accessor of a limited search against tests/limit_model.py,
element for element.  The model cuts the oracle's (or invert_model's) per-chunk lists to their first N entries; context_model
widens what is left.

The binding is packed as tightly as the header allows (tests/packing.py: pack_tight, newline bytes in every pad and guard)
and holds, in this order: an empty chunk; a chunk without a hit; chunks with 1, 2 and 3 selected lines; a chunk of three
16 KiB tiles with hits in each (1, 2, 1: a cut at 2 or 3 falls inside the second tile); a chunk whose 2nd selected line is
its unterminated last one; a chunk that is one unterminated selected line; a chunk with 5 selected lines (the exact count).
Global offsets and line bases are disjoint and not in the chunks' order.  Every pattern kind selects the same number of
lines per chunk: a "unit" is a line every literal and expression matches, followed by a capitalised word alone on its line
for the anchored expression (that one and the literal with a newline select nothing in an unterminated last line: their
counts in those two chunks are one lower, and the model says so).

Without the feature every case fails: libxsg.so has no xsg_set_max_count."""
import ctypes as C

import numpy as np
import pytest

import all_of_model
import anchor_oracle
import context_model
import invert_model
import limit_model
import match_model
import packing as P
import set_model
import words_model
import xsg
from gpu_util import GpuSearch, oracle_all_modes, oracle_regex_all_modes

pytestmark = pytest.mark.gpu

IC, RX, INV = xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX, xsg.FLAG_INVERT
U64_MAX = (1 << 64) - 1
UNIT = b"Sherlock said that colour aaaaaaa is running\nHolmes\n"
LAST = b"Sherlock said that colour aaaaaaa is running"  # a selected line without its newline
PLAIN = b"plain words of no interest\n"

# (id, kind, pattern or literals, pattern flags, list flags)
PATTERNS = [
    ("literal", "lit", b"Sherlock", 0, 0),
    ("literal_icase", "lit", b"sherLOCK", IC, 0),
    ("aa_bordered", "lit", b"aa", 0, 0),
    ("literal_with_newline", "nl", b"running\nH", 0, 0),
    ("class_sequence", "rx", b"She[r ]lock", RX, 0),
    ("prefilter", "rx", b"colou?r", RX, 0),
    ("line_walk", "rx", b"\\w+ing", RX, 0),
    ("anchored", "anchor", b"(?m)^[A-Z][a-z]+$", RX, 0),
    ("any_of", "anyof", (b"Sherlock", b"colour", b"zebra"), 0, 0),
    ("whole_words", "words", (b"that", b"run"), 0, xsg.LIST_WHOLE_WORDS),
    ("all_of", "allof", (b"that", b"ing"), 0, xsg.LIST_ALL_OF),
]
# (id, invert, (before, after) or None)
FLAGS = [("none", False, None), ("invert", True, None), ("context_1_2", False, (1, 2)), ("invert_context_2_0", True, (2, 0))]
SELECTED = [0, 0, 1, 2, 3, 4, 2, 1, 5]  # lines every pattern selects, per chunk (asserted against the model)


def _tiles() -> bytes:
    """three 16 KiB tiles: a unit in the first, two in the second, one in the third"""
    out, at = bytearray(), {3_000: 1, 20_000: 1, 28_000: 1, 36_000: 1}
    marks = sorted(at)
    while len(out) < 40_000:
        if marks and len(out) >= marks[0]:
            out += UNIT
            marks.pop(0)
        else:
            out += PLAIN
    assert not marks and 2 * P.TILE < len(out) < 3 * P.TILE
    return bytes(out)


def make_blocks():
    blocks = [b"", PLAIN * 2, PLAIN + UNIT + PLAIN, UNIT * 2 + PLAIN, PLAIN + UNIT * 3, _tiles(), UNIT + PLAIN + LAST, LAST,
              UNIT * 5 + PLAIN]
    blocks = [P.u8(b) for b in blocks]
    for b in blocks:
        b.setflags(write=False)
    n = len(blocks)
    go = [((i * 5) % n) * 1_000_000 + 13 for i in range(n)]
    lb = [((i * 7) % n) * 10_000 + 7 for i in range(n)]
    return blocks, go, lb


def bind_tight(gs, blocks, go, lb):
    import torch
    pk = P.pack_tight(blocks, lambda i, n: np.full(n, 10, dtype=np.uint8))
    t = torch.from_numpy(pk.host).to("cuda:0")
    chunks = xsg.make_chunks(pk.offsets, pk.lengths, go, lb)
    if gs.shard is None:
        gs.shard = xsg.Shard(gs.ctx, t.data_ptr() + pk.base, pk.capacity, chunks)
    else:
        gs.shard.rebind(t.data_ptr() + pk.base, pk.capacity, chunks)
    gs.keep = t


@pytest.fixture(scope="module")
def bound():
    gs = GpuSearch()
    blocks, go, lb = make_blocks()
    bind_tight(gs, blocks, go, lb)
    return gs, blocks, go, lb


def set_pattern(ctx, kind, pat, pflags, lflags, extra=0):
    if kind in ("anyof", "words", "allof"):
        ctx.set_literals(b"\n".join(pat), pflags | extra, lflags)
    else:
        ctx.set_pattern(pat, pflags | extra)


def plain_of(oracle, kind, pat, pflags, invert, blocks, go, lb):
    """-> (the dict without a limit and without context bits, (strings, offsets) of XSG_MATCHES or None)"""
    icase = bool(pflags & IC)
    if kind in ("lit", "nl"):
        want = oracle_all_modes(oracle, blocks, pat, global_offsets=go, line_bases=lb, ignore_case=icase)
    elif kind == "rx":
        want, with_lines = oracle_regex_all_modes(oracle, blocks, pat, icase, go, lb)
        assert with_lines
    elif kind == "anchor":
        want = anchor_oracle.all_modes(blocks, pat, icase, go, lb)
    elif kind == "anyof":
        want = set_model.all_modes(blocks, list(pat), icase, go, lb)
    elif kind == "words":
        want = words_model.all_modes(blocks, list(pat), icase, go, lb)
    else:
        want = all_of_model.all_modes(blocks, list(pat), icase, False, invert, go, lb)
        return {k: v for k, v in want.items() if k not in ("count_matches", "match_byte_offsets")}, None
    if invert:
        return invert_model.invert_all_modes(want, blocks, go, lb), None
    if kind == "anyof":
        m = set_model.matches(blocks, list(pat), icase, go)
    elif kind == "words":
        m = words_model.matches(blocks, list(pat), icase, go)
    else:
        m = match_model.matches(oracle, blocks, pat, pflags, go)
    return want, (m[0], m[1])


def rows_of(values, ranges):
    return np.concatenate([[0], np.cumsum([len(i) for i in limit_model.split(values, ranges)])]).astype(np.int64).tolist()


def check_limited(s, want, ranges, blocks, context, where):
    """every tag, accessor and count the combination serves, against `want` (limit_model's dict, widened under context)"""
    nl_chunks = [int(np.count_nonzero(b == 10)) for b in blocks]
    for mode, key in ((xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices")):
        assert s.search_u64(mode).tolist() == want["lines_final"][key], (where, key)
        assert s.result_chunk_ptr().astype(np.int64).tolist() == rows_of(want["lines_final"]["line_byte_offsets"], ranges), (where, key, "rows")
        if context:
            e = s.context_edges()
            got = [(int(r["lines"]), int(r["first"]), int(r["last"]), int(r["open_before"]), int(r["open_after"])) for r in e]
            assert got == want["edges"], (where, key, "edges")
    ls, lo = s.search_lines()
    assert (ls, lo.tolist()) == (want["lines_final"]["lines"], want["lines_final"]["lines_offsets"]), (where, "lines")
    rows, byte_ptr = s.result_chunk_ptr(with_bytes=True)
    want_rows = rows_of(want["lines_final"]["lines_offsets"], ranges)
    cum = np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
    assert rows.astype(np.int64).tolist() == want_rows, (where, "lines", "rows")
    assert byte_ptr.astype(np.int64).tolist() == cum[want_rows].tolist(), (where, "lines", "byte_ptr")
    c = s.count(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
    assert (int(c[xsg.CTR_LINES]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])) == (want["count_lines"], sum(nl_chunks), sum(b.size for b in blocks)), (where, "count_lines")
    s.count_begin(xsg.COUNT_LINES)
    assert int(s.count_end()[xsg.CTR_LINES]) == want["count_lines"], (where, "count_begin / _end")
    counts, newlines, totals = s.count_chunks(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
    assert counts.tolist() == want["count_lines_chunks"] and newlines.tolist() == nl_chunks, (where, "count_chunks")
    assert int(totals[xsg.CTR_LINES]) == want["count_lines"] == int(counts.sum()) and int(totals[xsg.CTR_NEWLINES]) == sum(nl_chunks), (where, "totals")
    if "match_byte_offsets" not in want:
        return
    assert s.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist() == want["match_byte_offsets"], (where, "match_byte_offsets")
    m_rows = rows_of(want["match_byte_offsets"], ranges)
    assert s.result_chunk_ptr().astype(np.int64).tolist() == m_rows, (where, "match rows")
    ms, mo = s.search_matches()
    assert (ms, mo.tolist()) == (want["matches"], want["matches_offsets"]), (where, "matches")
    rows, byte_ptr = s.result_chunk_ptr(with_bytes=True)
    cum = np.concatenate([[0], np.cumsum([len(x) for x in ms])]).astype(np.int64)
    assert rows.astype(np.int64).tolist() == m_rows and byte_ptr.astype(np.int64).tolist() == cum[m_rows].tolist(), (where, "matches rows")
    assert int(s.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) == want["count_matches"], (where, "count_matches")
    counts, _, totals = s.count_chunks(xsg.COUNT_MATCHES)
    assert counts.tolist() == want["count_matches_chunks"] and int(totals[xsg.CTR_MATCHES]) == want["count_matches"], (where, "count_chunks matches")


@pytest.mark.parametrize("fid,invert,context", FLAGS, ids=[f[0] for f in FLAGS])
@pytest.mark.parametrize("pid,kind,pat,pflags,lflags", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_limited_results(bound, oracle, pid, kind, pat, pflags, lflags, fid, invert, context):
    gs, blocks, go, lb = bound
    s = gs.shard
    extra = (INV if invert else 0) | (xsg.flag_context(*context) if context else 0)
    if kind == "nl" and extra:  # a pattern that can match '\n' has no complement and no context: refused where it is set
        with pytest.raises(xsg.XsgError) as e:
            set_pattern(gs.ctx, kind, pat, pflags, lflags, extra)
        assert e.value.code == xsg.ENOTSUP
        return
    plain, matches = plain_of(oracle, kind, pat, pflags, invert, blocks, go, lb)
    ranges = limit_model._ranges(blocks, go)
    full = limit_model.limit_all_modes(plain, blocks, 0, go, lb)
    if not invert and kind not in ("nl", "anchor"):  # (those two select the line BEHIND the unit's first: none in LAST)
        assert full["count_lines_chunks"] == SELECTED, "the binding does not hold the chunks its docstring promises"
    exact = max(full["count_lines_chunks"])
    for n in (1, 2, 3, exact, (1 << 32) + 1, U64_MAX):
        want = limit_model.limit_all_modes(plain, blocks, n, go, lb, matches)
        want["lines_final"] = want
        if context:
            want["lines_final"] = context_model.context_all_modes(want, blocks, *context, go, lb)
            want["edges"] = context_model.edges(want, blocks, *context, go)
        if n >= exact:
            assert want["line_byte_offsets"] == full["line_byte_offsets"]
        set_pattern(gs.ctx, kind, pat, pflags, lflags, extra)
        gs.ctx.set_max_count(n)
        check_limited(s, want, ranges, blocks, context, (pid, fid, n))


def test_the_cut_falls_where_the_docstring_says(bound, oracle):
    """N - 1, N and N + 1 selected lines for N in 1..3, the cut inside the second tile, the unterminated Nth line"""
    gs, blocks, go, lb = bound
    for n in (1, 2, 3):
        assert {n - 1, n, n + 1} <= set(SELECTED)
    tiles = blocks[5]
    starts = [i for i in range(tiles.size - len(UNIT)) if tiles[i:i + 8].tobytes() == b"Sherlock"]
    assert [x // P.TILE for x in starts] == [0, 1, 1, 2]
    gs.ctx.set_pattern(b"Sherlock", 0)
    for n in (1, 2, 3):  # chunk 6: UNIT, PLAIN, LAST -- its 2nd selected line is cut in at n >= 2, then dropped by XSG_LINES
        gs.ctx.set_max_count(n)
        gs.shard.search_lines()
        rows = gs.shard.result_chunk_ptr().astype(np.int64)
        assert int(rows[7] - rows[6]) == 1, n
        assert int(rows[8] - rows[7]) == 0, "a chunk that is one unterminated selected line hands out nothing"
        assert gs.shard.count_chunks(xsg.COUNT_LINES)[0].tolist()[6:8] == [min(n, 2), 1]


def test_a_plain_literal_leaves_the_one_sync_route(bound):
    gs, blocks, go, lb = bound
    s = gs.shard
    gs.ctx.set_pattern(b"Sherlock", 0)
    assert "(max count)" not in s.scan_kernel_name(xsg.LINE_BYTE_OFFSETS)
    full = s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    gs.ctx.set_max_count(2)
    assert s.scan_kernel_name(xsg.LINE_BYTE_OFFSETS).endswith(" + xsg::k_limit_copy (max count)")
    assert s.scan_kernel_name(xsg.COUNT_LINES).endswith(" + xsg::k_limit_counts (max count)")
    cut = s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    rows = s.result_chunk_ptr().astype(np.int64)
    assert np.diff(rows).tolist() == [min(c, 2) for c in SELECTED] and set(cut) < set(full)
    gs.ctx.set_pattern(b"Sherlock", INV | xsg.flag_context(1, 2))
    gs.ctx.set_max_count(2)
    name = s.scan_kernel_name(xsg.LINES)
    assert name.index("(inverted)") < name.index("(max count)") < name.index("(context)"), name
    # the timing loop and the tuner ignore the limit
    assert s.time_scan_kernel(xsg.COUNT_MATCHES, 1) >= 0.0
    s.tune(xsg.COUNT_MATCHES)


def test_call_order(bound):
    gs, blocks, go, lb = bound
    s, ctx = gs.shard, gs.ctx
    ctx.set_pattern(b"that", 0)
    full = s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    full_count = int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES])
    ctx.set_max_count(1)
    first = s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    assert len(first) == sum(min(c, 1) for c in SELECTED) < len(full)
    assert s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == first, "two searches in a row"
    assert int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == len(first) == int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES])
    ctx.set_pattern(b"that", 0)  # the limit belongs to the pattern that was set before it
    assert s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == full and int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == full_count
    ctx.set_max_count(2)
    assert len(s.search_u64(xsg.LINE_BYTE_OFFSETS)) == sum(min(c, 2) for c in SELECTED)
    ctx.set_max_count(0)  # 0 after N: no limit
    assert s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == full and int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == full_count
    ctx.set_max_count(1)
    with pytest.raises(xsg.XsgError):  # a set call that fails clears it too -- and leaves no pattern
        ctx.set_pattern(b"", 0)
    ctx.set_pattern(b"that", 0)
    assert s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == full
    ctx.set_max_count(1)
    ctx.set_literals(b"that\nzebra", 0)
    assert s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == full, "xsg_set_literals clears the limit"


def test_refusals(bound):
    import torch
    gs, blocks, go, lb = bound
    s, ctx = gs.shard, gs.ctx
    fresh = xsg.Context(0)
    with pytest.raises(xsg.XsgError) as e:
        fresh.set_max_count(3)
    assert e.value.code == xsg.ESTATE
    fresh.close()
    n = len(blocks)
    d = torch.zeros(4 + 1 + 2 * n, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()
    ctx.set_pattern(b"Sherlock", 0)
    s.count_async(xsg.COUNT_MATCHES, 0, p)  # served without a limit
    s.count_chunks_async(xsg.COUNT_LINES, 0, p + 40, 0, n, p, p + 32)
    torch.cuda.synchronize()
    ctx.set_max_count(2)
    for call in (lambda: s.count_async(xsg.COUNT_MATCHES, 0, p), lambda: s.count_async(xsg.COUNT_LINES, 0, p),
                 lambda: s.count_async_status(xsg.COUNT_LINES, 0, p, p + 32),
                 lambda: s.count_chunks_async(xsg.COUNT_LINES, 0, p + 40, 0, n, p, p + 32)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "limit" in str(e.value)
    # an existing refusal keeps its precedence and its message
    ctx.set_pattern(b"Sherlock", INV)
    ctx.set_max_count(2)
    with pytest.raises(xsg.XsgError) as e:
        s.count_async(xsg.COUNT_MATCHES, 0, p)
    assert e.value.code == xsg.ENOTSUP and "limit" not in str(e.value)
    ctx.set_literals(b"Sherlock\ncolour", 0)
    s.count_literals()
    ctx.set_max_count(2)
    for call in (s.count_literals, s.count_literals_chunks, s.count_literals_csr, s.find_literals,
                 lambda: s.count_literals_async(0, p, 2), lambda: s.count_literals_chunks_async(0, p, 2 * n),
                 lambda: s.count_literals_csr_async(0, p, n + 1, p, p, 1, p), lambda: s.find_literals_async(0, p, n + 1, p, p, 1, p)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "limit" in str(e.value)
    ctx.set_max_count(0)
    assert s.count_literals().tolist() == [sum(SELECTED)] * 2
    torch.cuda.synchronize()


def test_seventy_thousand_one_line_chunks(oracle):
    """grid and scan edges of the stage: more chunks than one workgroup of the scan's top level handles in a trip, one
    line each; every 7th chunk has no hit, every 11th is empty"""
    n = 70_000
    hit, miss = P.u8(b"that and that\n"), P.u8(b"plain\n")
    empty = P.u8(b"")
    kinds = np.where(np.arange(n) % 11 == 0, 2, np.where(np.arange(n) % 7 == 0, 1, 0))
    blocks = [(hit, miss, empty)[k] for k in kinds]
    go = (np.arange(n, dtype=np.int64) * 32 + 5).tolist()
    gs = GpuSearch()
    bind_tight(gs, blocks, go, None)
    is_hit = kinds == 0
    starts = np.asarray(go, dtype=np.int64)[is_hit]
    sample = oracle_all_modes(oracle, blocks[:200], b"that", global_offsets=go[:200])
    k = int(is_hit[:200].sum())
    assert sample["match_byte_offsets"] == np.stack([starts[:k], starts[:k] + 9], axis=1).ravel().tolist()
    assert sample["line_byte_offsets"] == starts[:k].tolist()
    gs.ctx.set_pattern(b"that", 0)
    assert gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).size == 2 * starts.size
    gs.ctx.set_max_count(1)
    s = gs.shard
    assert np.array_equal(s.search_u64(xsg.MATCH_BYTE_OFFSETS).astype(np.int64), starts)
    rows = s.result_chunk_ptr().astype(np.int64)
    assert np.array_equal(np.diff(rows), is_hit.astype(np.int64))
    assert int(s.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) == starts.size
    counts, _, totals = s.count_chunks(xsg.COUNT_MATCHES)
    assert np.array_equal(counts.astype(np.int64), is_hit.astype(np.int64)) and int(totals[xsg.CTR_MATCHES]) == starts.size
    ls, lo = s.search_lines()
    assert len(ls) == starts.size and set(ls) == {b"that and that"} and np.array_equal(lo.astype(np.int64), starts)
    gs.ctx.set_pattern(b"that", INV)
    gs.ctx.set_max_count(1)
    assert np.array_equal(s.search_u64(xsg.LINE_BYTE_OFFSETS).astype(np.int64), np.asarray(go, dtype=np.int64)[kinds == 1])
    s.close()
