"""XSG_LIST_WHOLE_WORDS on the GPU (include/xsg.h: xsg_set_literals_opts, xsg_host_searcher_create_list_opts,
xsg_literal_counter_create_opts, xsg_job_start_list; xsgrep -F -w): every result against tests/words_model.py, which
tests/test_words_host.py pins to Python's re and to grep -w -F.  Invert and context come from invert_model and context_model
on top of the model's dict, as for every other pattern.  Shapes: a lane's unit is 16 B, a wave-load 1 KiB, a wave's span
4 KiB, a tile 16 KiB."""
import ctypes as C
import os
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import context_model
import corpus
import invert_model
import literal_counts_model as LM
import literal_csr_model as CM
import set_cases as SC
import set_model
import words_model as WM
import xsg
from gpu_util import GpuSearch
from set_gpu_util import bind_tight, check, list_all_modes

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
IC, WW = xsg.FLAG_IGNORE_CASE, xsg.LIST_WHOLE_WORDS
LINE_KEYS = ("count_lines", "line_byte_offsets", "line_indices", "lines", "lines_offsets")
UNIT, WAVE_LOAD, WAVE_SPAN, TILE = 16, 1024, 4096, 16384
u8 = SC.u8


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


class _WithListFlags:
    """a Context whose set_literals passes list_flags on: set_gpu_util.list_all_modes sets the pattern itself"""

    def __init__(self, ctx, list_flags):
        self.ctx, self.list_flags = ctx, list_flags

    def set_literals(self, lst, flags=0):
        self.ctx.set_literals(lst, flags, self.list_flags)


def words_all_modes(g, lits, flags=0, lines=True, matches=True, list_flags=WW):
    """every tag through every entry point and accessor (set_gpu_util.list_all_modes) for a list with list_flags"""
    return list_all_modes(SimpleNamespace(ctx=_WithListFlags(g.ctx, list_flags), shard=g.shard), lits, flags, lines, matches)


def check_matches(g, blocks, lits, flags, what):
    got, off = g.shard.search_matches()
    strings, offsets, _ = WM.matches(blocks, lits, bool(flags & IC))
    assert (got, off.tolist()) == (strings, offsets), (what, "matches")


def check_counts(g, blocks, lits, flags, what, rows=None):
    """count_literals, the matrix with chunks_with and the CSR form of the pattern in force, against the model (`rows`: the
    model's matrix where the caller has it already)"""
    icase = bool(flags & IC)
    rows = WM.matrix(blocks, lits, icase) if rows is None else rows
    assert g.shard.count_literals().tolist() == [sum(r[j] for r in rows) for j in range(len(lits))], (what, "count_literals")
    m, w = g.shard.count_literals_chunks(True)
    assert m.tolist() == rows and w.tolist() == WM.chunks_with(rows, len(lits)), (what, "count_literals_chunks")
    indptr, indices, data = g.shard.count_literals_csr()
    assert (indptr.tolist(), indices.tolist(), data.tolist()) == CM.from_rows(rows), (what, "count_literals_csr")


def check_everything(g, blocks, lits, flags, what):
    want = WM.all_modes(blocks, lits, bool(flags & IC))
    check(words_all_modes(g, lits, flags), want, what)
    check_matches(g, blocks, lits, flags, what)
    check_counts(g, blocks, lits, flags, what)
    assert g.shard.count_chunks(xsg.COUNT_MATCHES)[0].tolist() == [len(WM.Occurrences(b, lits, bool(flags & IC)).spans()) for b in blocks], (what, "count_chunks")
    return want


# ---- 1. neighbours ---------------------------------------------------------------------------------------------------------------------
NEIGHBOUR_LITS = {1: b"q", 2: b"Zq", 3: b"wOr", 4: b"wOrd"}


def neighbour_blocks(lit: bytes):
    """the literal (every other time with its case swapped) with each of the 256 byte values in front of it, behind it and on
    both sides, a blank on the other side; two chunks, so that a value also meets the chunk's first and last position"""
    rows = []
    for b in range(256):
        x, l = bytes([b]), lit if b & 1 else lit.swapcase()
        rows.append(b" " + x + l + b" ; " + l + x + b" ; " + x + l + x + b" ;")
    half = len(rows) // 2
    return [u8(lit + b"".join(rows[:half]) + lit), u8(b"".join(rows[half:]))]


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_neighbours(gs, g, icase):
    """all 256 values on each side: the 63 word bytes deny the occurrence, every other value -- '\\n', `@` `[` `` ` `` `{` next to
    the letters, 0xC1-0xDA (a letter + 0x80: fold4's edges) -- does not; ignore-case folds the literal, not the set"""
    lit, flags = NEIGHBOUR_LITS[g], IC if icase else 0
    assert xsg.literals_info(lit)["gram"] == g
    blocks = neighbour_blocks(lit)
    gs.bind(blocks)
    want = check_everything(gs, blocks, (lit,), flags, (g, icase))
    plain = set_model.all_modes(blocks, (lit,), icase)
    assert 0 < want["count_matches"] < plain["count_matches"]
    if g > 1:  # (a one-byte literal also meets itself as the neighbour: the model has counted) per value and side, folded or not
        per_side = (256 - 63) * (1 if icase else 0.5)
        assert want["count_matches"] >= 3 * per_side - 8, want["count_matches"]


# ---- 2. chunk edges on tightly packed chunks -----------------------------------------------------------------------------------------
def edge_blocks():
    """chunk by chunk (offsets are multiples of 16, so a chunk of 16 bytes touches the next one):
      0  begins with `word`; the guard in front of it ends in a word byte
      1  16 bytes that end in a word byte: the byte right in front of chunk 2
      2  `word` at offset 0, and `word` as its last bytes with a pad behind them that begins with a word byte
      3  32 bytes that end in `word`: chunk 4 begins right behind them with a word byte
      4  the same two with the word byte INSIDE the chunk: `sword`, `words` -- nothing counts
      5  one byte, `w` (a list with a one-byte literal finds it); 6: no byte at all; 7: `word` alone, the last chunk"""
    blocks = [b"word one", b"0123456 ends inx", b"word is in a word", b"a chunk of 32 bytes then a  word", b"sword and words xwordx _word",
              b"w", b"", b"word"]
    assert len(blocks[1]) == 16 and len(blocks[3]) == 32 and len(blocks[2]) % 16 != 0
    return [u8(b) for b in blocks]


def edge_fill(kind):
    """what the guards and the pads hold: word bytes that would finish `words` / `sword` (stale text), or zeros (the control)"""
    if kind == "zero":
        return lambda i, n: np.zeros(n, dtype=np.uint8)
    return lambda i, n: u8((b"swords_" * (n // 7 + 1))[:n])  # (4096 = 7 * 585 + 1: the front guard ends in `s` too)


@pytest.mark.parametrize("fill", ["stale", "zero"])
@pytest.mark.parametrize("lits", [(b"word",), (b"word", b"w"), (b"WORD", b"or")], ids=["g4", "g1", "g2-icase"])
def test_chunk_edges_on_tightly_packed_chunks(gs, lits, fill):
    flags = IC if lits[0] == b"WORD" else 0
    blocks = edge_blocks()
    f = edge_fill(fill)
    if fill == "stale":  # the layout is what the docstring says: a word byte in front of chunk 0 and behind every chunk's end
        assert chr(f(0, 4096)[-1]).isalnum() and all(chr(f(i, n)[0]).isalnum() for i in range(1, 9) for n in (1, 7, 15, 4096))
    bind_tight(gs, blocks, f)
    check_everything(gs, blocks, lits, flags, (lits, fill))
    rows = WM.matrix(blocks, lits, bool(flags))
    assert [r[0] for r in rows] == [1, 0, 2, 1, 0, 0, 0, 1]  # `word` per chunk: the edges count, the inside does not
    if b"w" in lits:
        assert rows[5][1] == 1 and rows[6] == [0, 0]  # a 1-byte chunk holding a 1-byte literal; a chunk of length 0


# ---- 3. geometry ---------------------------------------------------------------------------------------------------------------------------
EDGES = (UNIT, WAVE_LOAD, WAVE_SPAN, TILE)
GEO_LIT = b"needle"


def geometry_blocks():
    """chunks of 20 000 bytes; in each, `needle` near every edge E, placed so that
      at E        the byte in front of it is the last one before the edge,
      at E - 6    the byte behind it is the first one beyond the edge,
      at E - 3    it straddles the edge itself;
    one chunk per placement and per kind of the two neighbours (word byte or not, in front and behind): 12 chunks"""
    blocks = []
    for place in (0, -len(GEO_LIT), -3):
        for before, behind in ((b" ", b" "), (b"x", b" "), (b" ", b"_"), (b"9", b"Z")):
            d = bytearray((b"some text. " * 2000)[:20_000])
            d[999::1000] = b"\n" * 20
            for e in EDGES:
                p = e + place
                d[p - 2:p + len(GEO_LIT) + 2] = b"." + before + GEO_LIT + behind + b"."
            blocks.append(u8(bytes(d)))
    return blocks


@pytest.mark.parametrize("lits", [(GEO_LIT,), (GEO_LIT, b"dl"), (b"NEEDLE", b"e")], ids=["g4", "g2", "g1-icase"])
def test_geometry(gs, lits):
    """p - 1 and p + len on either side of a 16-byte unit, a 1 KiB wave-load, a 4 KiB wave span and a 16 KiB tile edge, each
    with both kinds of neighbour: the two extra reads leave the lane's own unit, its wave's span and its tile"""
    flags = IC if lits[0] == b"NEEDLE" else 0
    blocks = geometry_blocks()
    gs.bind(blocks)
    check_everything(gs, blocks, lits, flags, lits)
    rows = WM.matrix(blocks, lits, bool(flags))
    assert [r[0] for r in rows] == [4, 0, 0, 0] * 3  # only blanks on both sides leave the four occurrences standing
    bind_tight(gs, blocks, lambda i, n: np.full(n, ord("w"), dtype=np.uint8))  # 20 000 = 16 * 1250: the chunks touch
    check_everything(gs, blocks, lits, flags, (lits, "tight"))


# ---- 4. the walk --------------------------------------------------------------------------------------------------------------------------
WALK_TEXT = (b"abc ab abcd\nxab ab\nabcd abx\nab\n\nabc\nab-abc_ab ab.abc\nthe cat, the hat and The\nnothing here\nthen the\n"
             b"zab abz\ngo -abc ab. to , the end -abc\nlast ab")
WALK_CASES = [
    ("ab,abc", (b"ab", b"abc"), 0),
    ("abc,ab", (b"abc", b"ab"), 0),
    ("duplicates", (b"the", b"cat", b"the"), IC),
    ("second-listed", (b"abcd", b"ab", b"abc"), 0),  # at 0 of `abc ab`: abcd does not occur, ab is not admissible, abc is
    ("non-word edges", (b"-abc", b"ab.", b", the"), 0),
]


@pytest.mark.parametrize("name,lits,flags", WALK_CASES, ids=[c[0] for c in WALK_CASES])
def test_the_walk(gs, name, lits, flags):
    """at the leftmost position where a literal occurs ADMISSIBLY the first-listed one that does so is the match; all seven
    tags, XSG_MATCHES, XSG_FLAG_INVERT and XSG_FLAG_CONTEXT(2, 1)"""
    blocks = [u8(WALK_TEXT), u8(WALK_TEXT[5:70])]
    gs.bind(blocks)
    plain = check_everything(gs, blocks, lits, flags, name)
    assert 0 < plain["count_matches"] < set_model.all_modes(blocks, lits, bool(flags & IC))["count_matches"]
    if name in ("ab,abc", "abc,ab"):
        assert WM.matches(blocks[:1], lits)[0][:2] == [b"abc", b"ab"] and plain["match_byte_offsets"][:2] == [0, 4]
    inv = invert_model.invert_all_modes(plain, blocks)
    check(words_all_modes(gs, lits, flags | xsg.FLAG_INVERT, matches=False), inv, (name, "invert"), keys=LINE_KEYS)
    for base, extra in ((plain, 0), (inv, xsg.FLAG_INVERT)):
        want = context_model.context_all_modes(base, blocks, 2, 1)
        got = words_all_modes(gs, lits, flags | extra | xsg.flag_context(2, 1), matches=not extra)
        check(got, want, (name, "context", extra), keys=[k for k in want if k in got])
        gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS)
        assert [tuple(int(x) for x in e) for e in gs.shard.context_edges()] == context_model.edges(base, blocks, 2, 1)
        if not extra:
            check_matches(gs, blocks, lits, flags, (name, "matches under context"))  # XSG_MATCHES ignores the bits


# ---- 5. counts ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def count_case():
    """300 literals -- the lexicon's words, pieces of them that occur inside words only, literals cut from the text -- over
    240 chunks of 0.6 to 3 KB, each cut at a newline; the model's matrix of both foldings, computed once"""
    pieces = [w[i:i + n] for w in corpus.LEXICON for n in (2, 3) for i in (0, 1) if len(w) > i + n]
    lits = tuple((list(corpus.LEXICON) + pieces + list(SC.word_list(300)))[:300])
    assert len(lits) == 300 and len(set(lits)) < 300  # (duplicates among them)
    blocks = [corpus.text_block(41, i, 600 + (i * 977) % 2400, needle_rate=2e-3) for i in range(240)]
    assert all(b[-1] == 10 for b in blocks)
    return lits, blocks, {icase: WM.matrix(blocks, lits, icase) for icase in (False, True)}


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
def test_counts(gs, count_case, icase):
    import torch
    lits, blocks, matrices = count_case
    flags, k, n, rows = IC if icase else 0, len(lits), len(blocks), matrices[icase]
    gs.bind(blocks)
    gs.ctx.set_literals(xsg.literal_list(lits), flags, WW)
    counts = [sum(r[j] for r in rows) for j in range(k)]  # (column sums: what count_literals must equal)
    sub = LM.counts(blocks, lits, icase)
    assert all(a <= b for a, b in zip(counts, sub)) and 0 < sum(counts) < sum(sub) // 2
    assert all(counts[j] == counts[lits.index(l)] for j, l in enumerate(lits))  # duplicates get the same number each
    check_counts(gs, blocks, lits, flags, ("sync", icase), rows)
    # the stream-ordered forms, into buffers pre-filled with 0xFF
    stream = torch.cuda.Stream()
    nnz = sum(1 for r in rows for v in r if v)
    c = torch.full((k + 4,), -1, dtype=torch.int64, device="cuda:0")
    m = torch.full((n * k + 4,), -1, dtype=torch.int64, device="cuda:0")
    w = torch.full((k + 4,), -1, dtype=torch.int64, device="cuda:0")
    rp = torch.full((n + 1 + 4,), -1, dtype=torch.int64, device="cuda:0")
    cols = torch.full((nnz + 4,), -1, dtype=torch.int32, device="cuda:0")
    vals = torch.full((nnz + 4,), -1, dtype=torch.int64, device="cuda:0")
    status = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    s = stream.cuda_stream
    gs.shard.count_literals_async(s, c.data_ptr(), k)
    gs.shard.count_literals_chunks_async(s, m.data_ptr(), n * k, w.data_ptr(), k)
    gs.shard.count_literals_csr_async(s, rp.data_ptr(), n + 1, cols.data_ptr(), vals.data_ptr(), nnz, status.data_ptr())
    stream.synchronize()
    assert c.cpu().tolist() == counts + [-1] * 4
    assert m.cpu().numpy()[:n * k].reshape(n, k).tolist() == rows and m.cpu().tolist()[n * k:] == [-1] * 4
    assert w.cpu().tolist() == WM.chunks_with(rows, k) + [-1] * 4
    indptr, indices, data = CM.from_rows(rows)
    assert (rp.cpu().tolist(), cols.cpu().tolist(), vals.cpu().tolist()) == (indptr + [-1] * 4, indices + [-1] * 4, data + [-1] * 4)
    assert int(status.cpu()[0]) == xsg.STATUS_OK
    # a LiteralCounter fed the same chunks: every chunk's edges are word boundaries there too
    lc = xsg.LiteralCounter(0, xsg.literal_list(lits), flags, WW)
    try:
        for b in blocks:
            lc.add(b)
        got, nbytes = lc.get()
        assert got.tolist() == counts and nbytes == sum(int(b.size) for b in blocks)
    finally:
        lc.close()


# ---- 6. state -------------------------------------------------------------------------------------------------------------------------------
def test_the_option_belongs_to_the_pattern(gs, oracle):
    """set_literals_opts(WHOLE_WORDS), set_literals, set_pattern and a failed set call in turn on one binding: every result is
    that of the pattern then in force; list_flags = 0 is xsg_set_literals element for element"""
    import torch
    from gpu_util import oracle_all_modes
    blocks = [u8(WALK_TEXT), corpus.text_block(43, 0, 40_000, needle_rate=2e-3), u8(b"party art\nthe then\n")]
    lits = (b"art", b"he", b"the", b"ab", b"Sher", b"lock")
    gs.bind(blocks)
    words, plain = WM.all_modes(blocks, lits), set_model.all_modes(blocks, lits)
    assert words["count_matches"] < plain["count_matches"]
    lib, lst = xsg.load(), xsg.literal_list(lits)

    def in_force(want, counts, tag):
        assert int(gs.shard.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) == want["count_matches"], tag
        assert gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == want["line_byte_offsets"], tag
        assert gs.shard.count_literals().tolist() == counts, tag
        assert (" whole words" in gs.shard.scan_kernel_name(xsg.COUNT_LINES)) == (want is words), tag

    for turn in range(2):
        check(words_all_modes(gs, lits), words, ("words", turn))
        in_force(words, WM.counts(blocks, lits), ("words", turn))
        name = gs.shard.scan_kernel_name(xsg.COUNT_LINES)
        assert name.endswith(" whole words") and "k_set_scan" in name
        d = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.count_async(xsg.COUNT_MATCHES, 0, d.data_ptr())
        assert e.value.code == xsg.ENOTSUP
        # xsg_set_literals, the entry point itself: the option is gone
        assert lib.xsg_set_literals(gs.ctx.h, lst, len(lst), 0) == xsg.OK
        in_force(plain, LM.counts(blocks, lits), ("xsg_set_literals", turn))
        assert "whole words" not in gs.shard.scan_kernel_name(xsg.COUNT_LINES)
        # ... and list_flags = 0 is that call, element for element, on every tag and count
        old = list_all_modes(gs, lits)
        old_counts = (gs.shard.count_literals().tolist(), gs.shard.count_literals_chunks(True)[0].tolist(),
                      [a.tolist() for a in gs.shard.count_literals_csr()])
        new = words_all_modes(gs, lits, list_flags=0)
        assert new == old == plain
        assert (gs.shard.count_literals().tolist(), gs.shard.count_literals_chunks(True)[0].tolist(),
                [a.tolist() for a in gs.shard.count_literals_csr()]) == old_counts
        gs.ctx.set_literals(lst, 0, WW)
        gs.ctx.set_pattern(b"art")  # a single pattern: a substring search, as ever
        assert gs.all_modes(b"art") == oracle_all_modes(oracle, blocks, b"art")
        gs.ctx.set_literals(lst, 0, WW)
        for bad in (lambda: gs.ctx.set_literals(b"a\n\nb", 0, WW), lambda: gs.ctx.set_literals(lst, 0, 0x2),
                    lambda: gs.ctx.set_pattern(b"", 0)):
            gs.ctx.set_literals(lst, 0, WW)
            with pytest.raises(xsg.XsgError) as e:
                bad()
            assert e.value.code == xsg.EINVAL
        with pytest.raises(xsg.XsgError) as e:  # a failed xsg_set_literals_opts leaves no pattern behind
            gs.ctx.set_literals(lst, 0, 0x2)
        assert e.value.code == xsg.EINVAL
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.count(xsg.COUNT_MATCHES)
        assert e.value.code == xsg.ESTATE
        gs.ctx.set_literals(lst, 0)  # after the failure: no option left over
        in_force(plain, LM.counts(blocks, lits), ("after a failed call", turn))


# ---- 7. the file pipeline, the host seam, the command line ---------------------------------------------------------------------------
FILE_LITS = (b"lock", b"Sherlock", b"he", b"the", b"Watson said", b"art", b"she")


@pytest.fixture(scope="module")
def textfile(tmp_path_factory):
    d = tmp_path_factory.mktemp("words")
    raw = corpus.text_block(45, 0, 300_000, needle_rate=2e-3).tobytes()
    raw = raw[:777] + b"party art, she; the_lock (lock) Sherlock's\n" + raw[777:]
    (d / "text.txt").write_bytes(raw)
    (d / "words.txt").write_bytes(b"\n".join(FILE_LITS) + b"\n")
    return str(d / "text.txt"), str(d / "words.txt"), raw


def job_result(path, lits, mode, flags=0, list_flags=WW, pattern_is_list=False):
    j = xsg.Job(xsg.literal_list(lits), path, mode, chunk_bytes=32 << 10, flags=flags, num_threads=2, num_max_readers=2,
                pattern_is_list=pattern_is_list, list_flags=list_flags)
    try:
        r = j.result()
        return r.tolist() if isinstance(r, np.ndarray) else r
    finally:
        j.close()


def test_file_pipeline(textfile):
    """xsg_job_start_list on a file cut into chunks at newlines equals the model of the whole text; xsg_job_opts'
    pattern_is_list may say anything"""
    path, _, raw = textfile
    assert len(xsg.plan_chunks(path, 32 << 10)) >= 8
    for flags in (0, IC):
        want = WM.all_modes([raw], FILE_LITS, bool(flags))
        assert 0 < want["count_lines"] < set_model.all_modes([raw], FILE_LITS, bool(flags))["count_lines"]
        for mode, key in ((xsg.COUNT_MATCHES, "count_matches"), (xsg.COUNT_LINES, "count_lines"),
                          (xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"), (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"),
                          (xsg.LINE_INDICES, "line_indices"), (xsg.LINES, "lines")):
            assert job_result(path, FILE_LITS, mode, flags) == want[key], (flags, key)
        assert job_result(path, FILE_LITS, xsg.MATCHES, flags) == WM.matches([raw], FILE_LITS, bool(flags))[0]
    plain = WM.all_modes([raw], FILE_LITS)
    assert job_result(path, FILE_LITS, xsg.COUNT_LINES, pattern_is_list=True) == plain["count_lines"]
    arr = [np.frombuffer(raw, dtype=np.uint8)]
    assert job_result(path, FILE_LITS, xsg.LINES, xsg.FLAG_INVERT) == invert_model.invert_all_modes(plain, arr)["lines"]
    assert job_result(path, FILE_LITS, xsg.LINES, xsg.flag_context(1, 1)) == context_model.context_all_modes(plain, arr, 1, 1)["lines"]


def test_host_searcher_create_list_opts(textfile):
    _, _, raw = textfile
    lib, lst, hs = xsg.load(), xsg.literal_list(FILE_LITS), C.c_void_p()
    assert lib.xsg_host_searcher_create_list_opts(0, lst, len(lst), 0, WW, 2, C.byref(hs)) == xsg.OK, lib.xsg_last_error()
    try:
        for lo, hi in ((0, 100_000), (778, 800), (100_000, 100_003)):  # (778: the chunk begins inside `party`: its edge is a boundary)
            blk = np.frombuffer(raw[lo:hi], dtype=np.uint8).copy()
            want, n = WM.all_modes([blk], FILE_LITS), C.c_uint64(0)
            assert lib.xsg_host_count(hs, blk.ctypes.data, blk.size, 0, C.byref(n)) == xsg.OK and n.value == want["count_matches"]
            assert lib.xsg_host_count(hs, blk.ctypes.data, blk.size, 1, C.byref(n)) == xsg.OK and n.value == want["count_lines"]
            out = C.c_void_p()
            assert lib.xsg_host_offsets(hs, xsg.MATCH_BYTE_OFFSETS, blk.ctypes.data, blk.size, C.byref(out), C.byref(n)) == xsg.OK
            got = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
            lib.xsg_free(out)
            assert got == want["match_byte_offsets"], lo
    finally:
        lib.xsg_host_searcher_destroy(hs)


def xsgrep(*args, stdin=None, chunk_bytes=None):
    env = dict(os.environ)
    if chunk_bytes:
        env["XSGREP_CHUNK_BYTES"] = str(chunk_bytes)
    r = subprocess.run([str(XSGREP), *args], input=stdin, capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def text_of(lines):
    return b"".join(l + b"\n" for l in lines)


def count_table(model, raw):
    return b"".join(b"%d\t%s\n" % (c, l) for c, l in zip(model.counts([raw], FILE_LITS), FILE_LITS))


def test_xsgrep_w_on_a_file(textfile):
    path, words, raw = textfile
    arr = [np.frombuffer(raw, dtype=np.uint8)]
    plain, icase = WM.all_modes([raw], FILE_LITS), WM.all_modes([raw], FILE_LITS, True)
    assert icase["count_lines"] > plain["count_lines"] > 0
    assert xsgrep("-F", "-w", "-f", words, path) == text_of(plain["lines"])
    assert xsgrep("-Fwc", "-f", words, path) == b"%d\n" % plain["count_lines"]
    assert xsgrep("-F", "-w", "-i", "-f", words, path) == text_of(icase["lines"])
    assert xsgrep("-F", "-w", "-o", "-f", words, path) == text_of(WM.matches([raw], FILE_LITS)[0])
    assert xsgrep("-F", "--word-regexp", "-v", "-f", words, path) == text_of(invert_model.invert_all_modes(plain, arr)["lines"])
    assert xsgrep("-F", "-w", "-C", "1", "-f", words, path) == text_of(context_model.context_all_modes(plain, arr, 1, 1)["lines"])
    assert xsgrep("-F", "-w", "--count-each", "-f", words, path, chunk_bytes=40_000) == count_table(WM, raw) != count_table(LM, raw)
    # a single PATTERN goes as a list of one, positional or -e
    one = WM.all_modes([raw], (b"lock",))
    assert 0 < one["count_lines"] < set_model.all_modes([raw], (b"lock",))["count_lines"]
    assert xsgrep("-F", "-w", "lock", path) == xsgrep("-F", "-w", "-e", "lock", path) == text_of(one["lines"])
    r = subprocess.run([str(XSGREP), "-w", "lock", path], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"-F" in r.stderr and r.stdout == b""


def test_xsgrep_w_on_stdin(textfile):
    """read in newline-aligned chunks of about 40 KB: every cut is a word boundary, the output is the file's"""
    _, _, raw = textfile
    arr = [np.frombuffer(raw, dtype=np.uint8)]
    plain = WM.all_modes([raw], FILE_LITS)
    e = [x for l in FILE_LITS for x in ("-e", l.decode())]
    assert xsgrep("-F", "-w", *e, "-", stdin=raw, chunk_bytes=40_000) == text_of(plain["lines"])
    assert xsgrep("-F", "-w", "-c", *e, "-", stdin=raw, chunk_bytes=40_000) == b"%d\n" % plain["count_lines"]
    assert xsgrep("-F", "-w", "-o", *e, "-", stdin=raw, chunk_bytes=40_000) == text_of(WM.matches([raw], FILE_LITS)[0])
    assert xsgrep("-F", "-w", "-v", *e, "-", stdin=raw, chunk_bytes=40_000) == text_of(invert_model.invert_all_modes(plain, arr)["lines"])
    assert xsgrep("-F", "-w", "--count-each", *e, "-", stdin=raw, chunk_bytes=40_000) == count_table(WM, raw)
