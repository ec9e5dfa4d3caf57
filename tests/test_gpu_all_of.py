"""XSG_LIST_ALL_OF on the GPU (include/xsg.h; xsgrep -F --all-of): every result against tests/all_of_model.py, which
tests/test_all_of_host.py pins to the intersection of the lists of one and to Python's re.  Every case compares
xsg_count(COUNT_LINES), the three line lists and xsg_count_chunks with the model; `identity` also compares with the
intersection of k searches of lists of one on the same binding.  Invert is the model's own flag, context comes from
context_model on top of the model's dict.  Shapes: a wave of k_all_of_or holds 64 consecutive entries, a workgroup 256; a
lane's unit of the scan is 16 B, a wave's span 4 KiB, a tile 16 KiB."""
import ctypes as C
import os
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import all_of_model as AM
import context_model
import literal_counts_model as LM
import literal_find_model as FM
import set_cases as SC
import set_model
import words_model as WM
import xsg
from gpu_util import GpuSearch
from set_gpu_util import bind_tight, check, list_all_modes

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
IC, INV, WW, ALL = xsg.FLAG_IGNORE_CASE, xsg.FLAG_INVERT, xsg.LIST_WHOLE_WORDS, xsg.LIST_ALL_OF
LINE_KEYS = ("count_lines", "line_byte_offsets", "line_indices", "lines", "lines_offsets", "chunk_counts")
WAVE_SPAN, TILE = 4096, 16384
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


def all_of_modes(g, lits, flags=0, words=False):
    """the line tags through every entry point and accessor (set_gpu_util.list_all_modes) and the counts per chunk"""
    lf = ALL | (WW if words else 0)
    out = list_all_modes(SimpleNamespace(ctx=_WithListFlags(g.ctx, lf), shard=g.shard), lits, flags, lines=True, matches=False)
    counts, _, totals = g.shard.count_chunks(xsg.COUNT_LINES)
    out["chunk_counts"] = counts.tolist()
    assert int(totals[xsg.CTR_LINES]) == out["count_lines"], "xsg_count_chunks: the total differs from xsg_count"
    return out


def by_lists_of_one(g, lits, flags=0, words=False):
    """the header's identity on this binding: the lines every list of one reports"""
    sets = []
    for l in lits:
        g.ctx.set_literals(xsg.literal_list((l,)), flags & ~INV, WW if words else 0)
        sets.append(set(g.shard.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()))
    return sorted(set.intersection(*sets))


def run_case(g, blocks, lits, flags=0, words=False, identity=False, what=None, bind=True, **offsets):
    if bind:
        g.bind([u8(b) if isinstance(b, bytes) else b for b in blocks], **offsets)
    want = AM.all_modes(blocks, lits, bool(flags & IC), words, bool(flags & INV), offsets.get("global_offsets"), offsets.get("line_bases"))
    check(all_of_modes(g, lits, flags, words), want, what or (lits, flags, words), LINE_KEYS)
    if identity:
        assert not flags & INV
        assert by_lists_of_one(g, lits, flags, words) == want["line_byte_offsets"], (what, "identity")
    return want


# ---- 1. geometry of the entry column ------------------------------------------------------------------------------------------------
def column_blocks(n, where, filler):
    """`filler` lines of one `a` (an entry each), then ONE line of n times `a` and a `b` in front, behind or nowhere, then a
    line that holds both and one that holds only `b`: the heavy line's first entry sits at lane `filler` mod 64"""
    heavy = {"first": b"b" + b"a" * n, "last": b"a" * n + b"b", "absent": b"a" * n}[where]
    return [b"a\n" * filler + heavy + b"\nab\nb\n"]


@pytest.mark.parametrize("where", ["first", "last", "absent"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 255, 256, 257, 1000])
def test_a_line_of_n_entries(gs, n, where):
    for filler in (0, 1, 62, 63, 64, 200):  # the line opens a wave, ends one, straddles two, a workgroup's edge
        want = run_case(gs, column_blocks(n, where, filler), (b"a", b"b"), what=(n, where, filler))
        assert want["count_lines"] == (1 if where == "absent" else 2)


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_the_line_at_every_lane(gs, where):
    for filler in range(65):
        run_case(gs, column_blocks(65, where, filler), (b"a", b"b"), what=(where, filler))


@pytest.mark.parametrize("tail", [b"b\n", b"\n", b"", b"b"], ids=["b-last", "no-b", "no-newline", "b-no-newline"])
def test_one_heavy_line(gs, tail):
    """2^19 entries in one line: one atomic per wave, no lane walks the line"""
    blocks = [b"x b\n" + b"a" * (1 << 19) + tail]
    want = run_case(gs, blocks, (b"a", b"b"), identity=True, what=tail)
    assert want["count_lines"] == (1 if b"b" in tail else 0)
    run_case(gs, blocks, (b"a", b"b"), INV, what=(tail, "inverted"), bind=False)


# ---- 2. text geometry -----------------------------------------------------------------------------------------------------------------
def line_across(edge, before=b"alpha", behind=b"omega"):
    """one line whose first literal ends just in front of `edge` and whose second begins just behind it"""
    head = b"filler line\n" * 3
    pad = edge - len(head) - len(before) - 1
    assert pad > 0
    return head + b"." * pad + before + b" " + behind + b"\n"


@pytest.mark.parametrize("edge", [WAVE_SPAN, TILE, TILE + WAVE_SPAN, 3 * TILE], ids=["span", "tile", "tile+span", "3 tiles"])
def test_a_line_across_spans_and_tiles(gs, edge):
    text = line_across(edge) + b"alpha only\nomega only\n"
    assert text[edge - 1:edge] == b" " and text[edge:edge + 5] == b"omega"
    want = run_case(gs, [text, text[:edge]], (b"alpha", b"omega"), identity=True, what=edge)
    assert want["chunk_counts"] == [1, 0]  # (the second chunk ends in front of `omega`: no byte behind its end decides)
    # the literal itself straddles the edge
    text = line_across(edge + 2) + b"omega\n"
    run_case(gs, [text], (b"alpha", b"omega"), identity=True, what=(edge, "straddling"))


def test_a_line_that_gets_its_last_literal_three_tiles_later(gs):
    text = b"start\n" + b"one " + b"." * (3 * TILE + 100) + b" two" + b"." * 50 + b" three\n" + b"one two\nthree\n"
    want = run_case(gs, [text], (b"one", b"two", b"three"), identity=True)
    assert want["line_byte_offsets"] == [6]
    run_case(gs, [text], (b"one", b"two", b"three"), xsg.FLAG_INVERT, bind=False)


# ---- 3. chunk seams -------------------------------------------------------------------------------------------------------------------
SEAM = [b"b a\nxx a a", b"b b\na b\n", b"", b"a", b"", b"b\n", b"b a"]


def test_chunk_seams(gs):
    """chunk c ends without a newline in a line that holds only `a`, chunk c + 1 begins with a line that holds only `b`:
    neither is selected; empty chunks between"""
    want = run_case(gs, SEAM, (b"a", b"b"), identity=True)
    assert want["chunk_counts"] == [1, 1, 0, 0, 0, 0, 1]
    run_case(gs, SEAM, (b"a", b"b"), INV, bind=False)


@pytest.mark.parametrize("fill", ["ab", "nl"])
def test_chunk_seams_tightly_packed(gs, fill):
    """the same, packed as tests/packing.py packs: the pad behind a chunk holds the literal the chunk's last line lacks"""
    paint = (lambda i, n: u8((b"ab " * (n // 3 + 1))[:n])) if fill == "ab" else (lambda i, n: np.full(n, 10, dtype=np.uint8))
    blocks = [u8(b) for b in SEAM]
    bind_tight(gs, blocks, paint)
    run_case(gs, SEAM, (b"a", b"b"), identity=True, what=fill, bind=False)
    run_case(gs, SEAM, (b"a", b"b"), words=True, identity=True, what=(fill, "words"), bind=False)


def test_a_binding_of_no_chunks(gs):
    import torch
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    gs.shard.rebind(t.data_ptr(), 256, xsg.make_chunks([], []))
    gs.keep = t
    want = run_case(gs, [], (b"a", b"b"), bind=False)
    assert want["count_lines"] == 0 and want["chunk_counts"] == []
    run_case(gs, [], (b"a", b"b"), INV, bind=False)


# ---- 4. lists ---------------------------------------------------------------------------------------------------------------------------
LIST_TEXT = (b"abc\nab\naaa\naa\nERROR timeout db01\nerror Timeout DB01 x\nthe he\nthe\nhe\nxhe the\n"
             b"Sherlock Sherbet\nsherlock sherbet\nSherbet\nSherlock\na b c\nc b\n\nq\n")


@pytest.mark.parametrize("lits,flags,words", [
    ((b"ab",), 0, False), ((b"ab", b"abc"), 0, False), ((b"abc", b"ab"), 0, False), ((b"aa", b"aaa"), 0, False),
    ((b"a", b"b"), 0, False), ((b"a", b"b", b"a", b"b"), 0, False), ((b"a", b"b", b"c"), 0, False),
    ((b"Sherlock", b"Sherbet"), 0, False), ((b"sherlock", b"sherbet"), IC, False), ((b"Sher", b"Sherlock", b"Sherbet"), 0, False),
    ((b"error", b"db01", b"TIMEOUT"), IC, False), ((b"ERROR", b"timeout", b"db01"), 0, False),
    ((b"he", b"the"), 0, True), ((b"he", b"the"), 0, False), ((b"he",), 0, True), ((b"HE", b"The"), IC, True), ((b"q", b"q"), 0, True),
], ids=lambda v: None if isinstance(v, (int, bool)) else b"+".join(v).decode())
def test_lists(gs, lits, flags, words):
    want = run_case(gs, [LIST_TEXT, LIST_TEXT[:-2], b"he", b"the"], lits, flags, words, identity=True)
    assert want["count_lines"] > 0
    run_case(gs, [LIST_TEXT, LIST_TEXT[:-2], b"he", b"the"], lits, flags | INV, words, bind=False)


def test_a_list_of_one_is_the_plain_list(gs):
    gs.bind([u8(LIST_TEXT), u8(LIST_TEXT[:30])])
    for lit, flags, words in ((b"he", 0, False), (b"he", 0, True), (b"sher", IC, False)):
        model = (WM if words else set_model).all_modes([LIST_TEXT, LIST_TEXT[:30]], (lit,), bool(flags))
        check(all_of_modes(gs, (lit,), flags, words), model, lit, LINE_KEYS[:-1])


def words64():
    return [b"w%02dx" % j for j in range(64)]


def test_64_literals_with_the_64th_deciding(gs):
    lits = words64()
    full = b" ".join(lits)
    text = full + b"\n" + b" ".join(lits[:63]) + b"\n" + b" ".join(reversed(lits)) + b"\n" + lits[63] + b"\n" + b" ".join(lits[1:]) + b"\n"
    want = run_case(gs, [text, full], lits, identity=True)
    assert want["chunk_counts"] == [2, 1]
    run_case(gs, [text, full], lits, words=True, what="words", bind=False)
    run_case(gs, [text, full], lits, INV, what="inverted", bind=False)


def test_65_literals_are_refused_and_leave_no_pattern(gs):
    gs.bind([u8(LIST_TEXT)])
    lits = words64() + [b"w64x"]
    gs.ctx.set_literals(xsg.literal_list(lits[:64]), 0, ALL)
    for lf in (ALL, ALL | WW):
        with pytest.raises(xsg.XsgError) as e:
            gs.ctx.set_literals(xsg.literal_list(lits), 0, lf)
        assert e.value.code == xsg.EINVAL and "at most 64" in str(e.value)
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.count(xsg.COUNT_LINES)
        assert e.value.code == xsg.ESTATE
    gs.ctx.set_literals(xsg.literal_list(lits), 0, WW)  # without the bit the list is served as ever
    assert int(gs.shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == 0


# ---- 5. extremes ----------------------------------------------------------------------------------------------------------------------
def test_extremes(gs):
    every = [b"a b\n" * 3000, b"b a\n" * 500 + b"ab"]
    want = run_case(gs, every, (b"a", b"b"), identity=True, what="every line")
    assert want["chunk_counts"] == [3000, 501]
    assert run_case(gs, every, (b"a", b"b"), INV, what="every line, inverted", bind=False)["count_lines"] == 0
    nothing = [b"x y z\n" * 3000, b"zzz"]
    assert run_case(gs, nothing, (b"a", b"b"), identity=True, what="no candidates")["count_lines"] == 0
    assert run_case(gs, nothing, (b"a", b"b"), INV, what="no candidates, inverted", bind=False)["count_lines"] == 3001
    apart = [b"a\nb\n" * 3000 + b"a", b"b\n" + b"a\n" * 20_000 + b"b"]  # (kept entries are rare: 26 000 lines, none selected)
    assert run_case(gs, apart, (b"a", b"b"), identity=True, what="never together")["count_lines"] == 0
    run_case(gs, apart, (b"a", b"b"), INV, what="never together, inverted", bind=False)


# ---- 6. composition -------------------------------------------------------------------------------------------------------------------
def composition_blocks():
    rng = np.random.Generator(np.random.PCG64(7))
    words = [b"red", b"green", b"blue", b"grey", b"x", b"yy"]
    out = []
    for n in (300, 1, 250):
        lines = [b" ".join(words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(0, 7)))) for _ in range(n)]
        out.append(b"\n".join(lines) + (b"\n" if n != 250 else b""))
    return out


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
def test_context_and_edges(gs, invert):
    blocks, lits = composition_blocks(), (b"red", b"blue")
    arr = [u8(b) for b in blocks]
    gs.bind(arr)
    plain = AM.all_modes(blocks, lits, invert=invert)
    assert 0 < plain["count_lines"] < sum(len(AM.chunk_lines(b)) for b in blocks)
    want = context_model.context_all_modes(plain, arr, 2, 1)
    flags = xsg.flag_context(2, 1) | (INV if invert else 0)
    got = all_of_modes(gs, lits, flags)
    check(got, want, invert, ("count_lines", "line_byte_offsets", "line_indices", "lines", "lines_offsets"))
    gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS)
    assert [tuple(int(x) for x in e) for e in gs.shard.context_edges()] == context_model.edges(plain, arr, 2, 1)


def test_line_indices_with_line_bases(gs):
    blocks = composition_blocks()
    go, lb = [1000, 50_000, 900_000], [10, 5000, 70_000]
    run_case(gs, blocks, (b"red", b"blue"), identity=True, global_offsets=go, line_bases=lb)
    run_case(gs, blocks, (b"red", b"blue", b"green"), INV, global_offsets=go, line_bases=lb)


# ---- 7. refusals and state ------------------------------------------------------------------------------------------------------------
def test_refusals_and_state(gs, tmp_path):
    import torch
    blocks, lits = [LIST_TEXT, LIST_TEXT[:40]], (b"he", b"the", b"he")
    gs.bind([u8(b) for b in blocks])
    lst, lib = xsg.literal_list(lits), xsg.load()
    for words in (False, True):
        lf = ALL | (WW if words else 0)
        gs.ctx.set_literals(lst, 0, lf)
        name = gs.shard.scan_kernel_name(xsg.COUNT_LINES)
        assert name.endswith(" whole words all of" if words else " all of") and "k_set_scan" in name, name
        for call in (lambda: gs.shard.count(xsg.COUNT_MATCHES), lambda: gs.shard.count_chunks(xsg.COUNT_MATCHES),
                     lambda: gs.shard.count_begin(xsg.COUNT_MATCHES), lambda: gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS),
                     lambda: gs.shard.search_matches()):
            with pytest.raises(xsg.XsgError) as e:
                call()
            assert e.value.code == xsg.ENOTSUP and "XSG_LIST_ALL_OF" in str(e.value)
        d = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")
        with pytest.raises(xsg.XsgError) as e:  # as for every list
            gs.shard.count_async(xsg.COUNT_LINES, 0, d.data_ptr())
        assert e.value.code == xsg.ENOTSUP
        # the counts per literal do not know the bit
        model = WM if words else LM
        assert gs.shard.count_literals().tolist() == model.counts(blocks, lits)
        hits = tuple(x.tolist() for x in gs.shard.find_literals())
        gs.ctx.set_literals(lst, 0, lf & ~ALL)
        assert gs.shard.count_literals().tolist() == model.counts(blocks, lits)
        assert tuple(x.tolist() for x in gs.shard.find_literals()) == hits
        if not words:
            assert hits == FM.find(blocks, lits)
        # a later set call clears the option: the plain list's answers, match tags included
        gs.ctx.set_literals(lst, 0, lf)
        assert lib.xsg_set_literals(gs.ctx.h, lst, len(lst), 0) == xsg.OK
        plain = set_model.all_modes(blocks, lits)
        assert "all of" not in gs.shard.scan_kernel_name(xsg.COUNT_LINES)
        assert int(gs.shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == plain["count_lines"] > AM.all_modes(blocks, lits)["count_lines"]
        assert gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist() == plain["match_byte_offsets"]
    for make in (xsg.LiteralCounter, xsg.LiteralFinder):
        for lf in (ALL, ALL | WW):
            with pytest.raises(xsg.XsgError) as e:
                make(0, lst, 0, lf)
            assert e.value.code == xsg.EINVAL
    # the host searcher: the line calls answer, the match calls are XSG_ENOTSUP
    hs, n, out, o2 = C.c_void_p(), C.c_uint64(0), C.c_void_p(), C.c_void_p()
    assert lib.xsg_host_searcher_create_list_opts(0, lst, len(lst), 0, ALL, 1, C.byref(hs)) == xsg.OK, lib.xsg_last_error()
    try:
        blk = u8(LIST_TEXT)
        want = AM.all_modes([LIST_TEXT], lits)
        assert lib.xsg_host_count(hs, blk.ctypes.data, blk.size, 1, C.byref(n)) == xsg.OK and n.value == want["count_lines"]
        assert lib.xsg_host_count(hs, blk.ctypes.data, blk.size, 0, C.byref(n)) == xsg.ENOTSUP
        for mode, key in ((xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices")):
            assert lib.xsg_host_offsets(hs, mode, blk.ctypes.data, blk.size, C.byref(out), C.byref(n)) == xsg.OK
            got = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
            lib.xsg_free(out)
            assert got == want[key], key
        assert lib.xsg_host_offsets(hs, xsg.MATCH_BYTE_OFFSETS, blk.ctypes.data, blk.size, C.byref(out), C.byref(n)) == xsg.ENOTSUP
        nb = C.c_uint64(0)
        assert lib.xsg_host_matches(hs, blk.ctypes.data, blk.size, C.byref(out), C.byref(o2), C.byref(n), C.byref(nb)) == xsg.ENOTSUP
        assert lib.xsg_host_lines(hs, blk.ctypes.data, blk.size, C.byref(out), C.byref(o2), C.byref(n), C.byref(nb)) == xsg.OK
        lens = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
        raw = C.string_at(o2, nb.value)
        lib.xsg_free(out)
        lib.xsg_free(o2)
        ends = np.cumsum([0] + lens).tolist()
        assert [raw[a:b] for a, b in zip(ends, ends[1:])] == want["lines"]
    finally:
        lib.xsg_host_searcher_destroy(hs)
    # a job refuses the match tags when it is started
    (tmp_path / "t.txt").write_bytes(LIST_TEXT)
    for mode in (xsg.COUNT_MATCHES, xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES):
        with pytest.raises(xsg.XsgError) as e:
            xsg.Job(lst, str(tmp_path / "t.txt"), mode, list_flags=ALL)
        assert e.value.code == xsg.ENOTSUP


# ---- 8. identity on a random text -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_text():
    rng = np.random.Generator(np.random.PCG64(2026))
    vocab = [b"alpha", b"beta", b"gamma", b"delta", b"alphabet", b"be", b"x", b"-", b"_", b"Gamma", b"et"]
    picks = rng.integers(0, len(vocab), 80_000)
    seps = rng.integers(0, 10, 80_000)
    raw = b"".join(vocab[int(p)] + (b"\n" if s < 2 else b"" if s < 4 else b" ") for p, s in zip(picks, seps))[:256 << 10]
    cuts = [0, 50_001, 50_001, 120_000, 200_017, len(raw)]  # five chunks, one of them empty, cut anywhere
    return [raw[a:b] for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("words", [False, True], ids=["substrings", "words"])
@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
def test_identity_on_a_random_text(gs, random_text, icase, words):
    gs.bind([u8(b) for b in random_text])
    for lits in ((b"alpha", b"beta"), (b"gamma", b"be", b"et"), (b"alpha", b"alphabet", b"delta", b"x", b"gamma")):
        want = run_case(gs, random_text, lits, IC if icase else 0, words, identity=True, what=lits, bind=False)
        assert 0 < want["count_lines"] < sum(len(AM.chunk_lines(b)) for b in random_text)


# ---- 9. the file job and the command line ---------------------------------------------------------------------------------------------
FILE_LITS = (b"alpha", b"be", b"gamma")


@pytest.fixture(scope="module")
def textfile(tmp_path_factory, random_text):
    d = tmp_path_factory.mktemp("all_of")
    raw = b"".join(random_text)[:200_000]
    raw = raw[:raw.rfind(b"\n") + 1] + b"gamma be alpha"  # (an unterminated last line that is selected)
    (d / "text.txt").write_bytes(raw)
    (d / "lits.txt").write_bytes(b"\n".join(FILE_LITS) + b"\n")
    return str(d / "text.txt"), str(d / "lits.txt"), raw


def job_result(path, lits, mode, flags=0, list_flags=ALL):
    j = xsg.Job(xsg.literal_list(lits), path, mode, chunk_bytes=16 << 10, flags=flags, num_threads=2, num_max_readers=2,
                list_flags=list_flags)
    try:
        r = j.result()
        return r.tolist() if isinstance(r, np.ndarray) else r
    finally:
        j.close()


def test_file_job(textfile):
    """xsg_job_start_list on a file cut into many chunks at newlines equals the model of the whole text"""
    path, _, raw = textfile
    assert len(xsg.plan_chunks(path, 16 << 10)) >= 8
    arr = [np.frombuffer(raw, dtype=np.uint8)]
    for flags, words in ((0, False), (IC, False), (0, True)):
        want = AM.all_modes([raw], FILE_LITS, bool(flags), words)
        assert 0 < want["count_lines"]
        for mode, key in ((xsg.COUNT_LINES, "count_lines"), (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"),
                          (xsg.LINE_INDICES, "line_indices"), (xsg.LINES, "lines")):
            assert job_result(path, FILE_LITS, mode, flags, ALL | (WW if words else 0)) == want[key], (flags, words, key)
    plain = AM.all_modes([raw], FILE_LITS)
    assert job_result(path, FILE_LITS, xsg.LINES, INV) == AM.all_modes([raw], FILE_LITS, invert=True)["lines"]
    assert job_result(path, FILE_LITS, xsg.LINES, xsg.flag_context(1, 1)) == context_model.context_all_modes(plain, arr, 1, 1)["lines"]


def xsgrep(*args, stdin=None, chunk_bytes=None, status=0):
    env = dict(os.environ)
    if chunk_bytes:
        env["XSGREP_CHUNK_BYTES"] = str(chunk_bytes)
    r = subprocess.run([str(XSGREP), *args], input=stdin, capture_output=True, timeout=120, env=env)
    assert r.returncode == status, r.stderr.decode()
    return r.stdout


def text_of(lines):
    return b"".join(l + b"\n" for l in lines)


def test_xsgrep_all_of(textfile):
    path, lits, raw = textfile
    arr = [np.frombuffer(raw, dtype=np.uint8)]
    plain, words = AM.all_modes([raw], FILE_LITS), AM.all_modes([raw], FILE_LITS, words=True)
    assert plain["count_lines"] > words["count_lines"] > 0
    assert xsgrep("-F", "--all-of", "-f", lits, path) == text_of(plain["lines"])
    assert xsgrep("-F", "--all-of", "-c", "-f", lits, path) == b"%d\n" % plain["count_lines"]
    assert xsgrep("-F", "--all-of", "-w", "-f", lits, path) == text_of(words["lines"])
    assert xsgrep("-F", "--all-of", "-v", "-f", lits, path) == text_of(AM.all_modes([raw], FILE_LITS, invert=True)["lines"])
    assert xsgrep("-F", "--all-of", "-C", "1", "-f", lits, path) == text_of(context_model.context_all_modes(plain, arr, 1, 1)["lines"])
    assert xsgrep("-F", "--all-of", "-i", "-e", "ALPHA", "-e", "Be", path) == text_of(AM.all_modes([raw], (b"alpha", b"be"), True)["lines"])
    one = set_model.all_modes([raw], (b"gamma",))  # a single PATTERN: a list of one, the plain search
    assert xsgrep("-F", "--all-of", "gamma", path) == xsgrep("-F", "gamma", path) == text_of(one["lines"])
    # stdin in newline-aligned chunks of about 20 KB (there the unterminated last line is printed by no search)
    e = [x for l in FILE_LITS for x in ("-e", l.decode())]
    assert xsgrep("-F", "--all-of", *e, "-", stdin=raw, chunk_bytes=20_000) == text_of(plain["lines"])
    assert xsgrep("-F", "--all-of", "-c", *e, "-", stdin=raw, chunk_bytes=20_000) == b"%d\n" % plain["count_lines"]
    assert xsgrep("-F", "--all-of", "-w", "-v", *e, "-", stdin=raw, chunk_bytes=20_000) == text_of(
        AM.all_modes([raw], FILE_LITS, words=True, invert=True)["lines"])
    for bad in (["--all-of", "-f", lits, path], ["-F", "--all-of", "-o", "-f", lits, path], ["-F", "--all-of", "-x", "gamma", path],
                ["-F", "--all-of", "--count-each", "-f", lits, path], ["-F", "--all-of", "--find-each", "-f", lits, path]):
        assert xsgrep(*bad, status=2) == b""
