"""xsg_find_literals / xsg_result_literal_hits / xsg_find_literals_async, LiteralFinder and xsgrep --find-each: every
occurrence of every literal of a list as (chunk_ptr, pos, lit), sorted by (chunk, position, listing index).

Expected values are tests/literal_find_model.py's: exact equality of the whole arrays everywhere.  Chunks are bound with
set_gpu_util.bind_tight, so hostile bytes -- stale occurrences, and what a literal cut by a chunk's end lacks -- follow
every chunk end.  Every case runs the synchronous form and the stream-ordered form on a side stream into buffers
pre-filled with 0xFF that are 8 entries longer than needed.  On every case the bincount of lit equals
Shard.count_literals(), the per-chunk bincount Shard.count_literals_chunks(), pos ascends within a chunk and lit ascends
strictly at equal pos."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import literal_find_model as FM
import packing as P
import set_cases as SC
import set_edge_cases as SE
import xsg
from gpu_util import GpuSearch
from set_gpu_util import IC, bind_tight

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
TILE = SC.TILE
SPARE = 8
WW = xsg.LIST_WHOLE_WORDS
STALE = b" needle kqzw art aa ab abc a "  # what the pads and guards hold besides what a cut literal lacks


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


class Side:
    """a side stream for the stream-ordered form; the buffers are made per call, SPARE words longer than asked for"""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()

    def run(self, shard, n, cap_entries):
        """-> (chunk_ptr[n + 1], pos[:cap_entries], lit[:cap_entries], status); asserts that nothing behind them was written"""
        torch = self.torch
        cp = torch.full((n + 1 + SPARE,), -1, dtype=torch.int64, device="cuda:0")  # every byte 0xFF
        pos = torch.full((cap_entries + SPARE,), -1, dtype=torch.int64, device="cuda:0")
        lit = torch.full((cap_entries + SPARE,), -1, dtype=torch.int32, device="cuda:0")
        status = torch.full((1 + SPARE,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        shard.find_literals_async(self.stream.cuda_stream, cp.data_ptr(), n + 1, pos.data_ptr(), lit.data_ptr(), cap_entries, status.data_ptr())
        self.stream.synchronize()
        gcp, gp, gl, gst = cp.cpu().numpy(), pos.cpu().numpy(), lit.cpu().numpy(), status.cpu().numpy()
        assert (gcp[n + 1:] == -1).all(), "words behind chunk_ptr were written"
        assert (gp[cap_entries:] == -1).all() and (gl[cap_entries:] == -1).all(), "entries at or behind cap_entries were written"
        assert (gst[1:] == -1).all(), "words behind the status were written"
        return gcp[:n + 1].view(np.uint64).tolist(), gp[:cap_entries].view(np.uint64).tolist(), gl[:cap_entries].view(np.uint32).tolist(), int(gst[0])


@pytest.fixture(scope="module")
def side():
    return Side()


def with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sync(gs):
    cp, pos, lit = gs.shard.find_literals()
    assert cp.dtype == np.uint64 and pos.dtype == np.uint64 and lit.dtype == np.uint32
    return cp.tolist(), pos.tolist(), lit.tolist()


def stale_fill(plan):
    """fill(i, n): the gap in FRONT of chunk i -- what chunk i - 1 lacks of a literal its end cuts, then stale occurrences"""
    def fill(i, n):
        head = plan[i - 1][1] if 0 < i <= len(plan) else b""
        return SC.u8((head + STALE * (n // len(STALE) + 2))[:n])
    return fill


def bind_plan(gs, plan, global_offsets=None):
    """plan: ((chunk, what the bytes behind it must hold to complete a cut literal), ...), packed tightly"""
    blocks = [b for b, _ in plan]
    if global_offsets is None:
        bind_tight(gs, blocks, stale_fill(plan))
        return blocks
    import torch
    pk = P.pack_tight(blocks, stale_fill(plan))
    t = torch.from_numpy(pk.host).to("cuda:0")
    chunks = xsg.make_chunks(pk.offsets, pk.lengths, global_offsets)
    if gs.shard is None:
        gs.shard = xsg.Shard(gs.ctx, t.data_ptr() + pk.base, pk.capacity, chunks)
    else:
        gs.shard.rebind(t.data_ptr() + pk.base, pk.capacity, chunks)
    gs.keep = t
    return blocks


def check(gs, side, blocks, lits, flags=0, list_flags=0, what="", go=None, want=None):
    """both forms against the model, the form of the result, and the counts of the same binding -> the expected arrays"""
    n, k = len(blocks), len(lits)
    if want is None:
        want = FM.find(blocks, lits, bool(flags & IC), bool(list_flags & WW), go)
    gs.ctx.set_literals(xsg.literal_list(lits), flags, list_flags)
    got = {"synchronous": sync(gs)}
    cp, pos, lit, status = side.run(gs.shard, n, len(want[1]))
    assert status == xsg.STATUS_OK, (what, "stream-ordered: status")
    got["stream-ordered"] = (cp, pos, lit)
    print(what, "n", n, "k", k, "total", len(want[1]), "chunk_ptr", want[0][:6], "got", got["synchronous"][0][:6])
    counts = gs.shard.count_literals().tolist()
    rows = gs.shard.count_literals_chunks(False)[0].tolist()
    for name, g in got.items():
        assert g[0] == want[0], (what, name, "chunk_ptr")
        assert g[1] == want[1], (what, name, "pos")
        assert g[2] == want[2], (what, name, "lit")
        assert FM.well_formed(*g, k), (what, name, "form")
        assert FM.bincount(g[2], k) == counts, (what, name, "bincount against count_literals")
        assert FM.rows(g[0], g[2], k) == rows, (what, name, "per-chunk bincount against count_literals_chunks")
    return want


def plain(texts):
    return [(SC.u8(t), b"") for t in texts]


# ---- 1. definitions ------------------------------------------------------------------------------------------------------------
def test_overlapping_covered_and_duplicate_occurrences(gs, side):
    blocks = bind_plan(gs, plain([b"aaaa"]))
    assert check(gs, side, blocks, (b"aa",), what="aa in aaaa") == ([0, 3], [0, 1, 2], [0, 0, 0])
    blocks = bind_plan(gs, plain([b"abc"]))
    assert check(gs, side, blocks, (b"ab", b"abc"), what="ab, abc on abc") == ([0, 2], [0, 0], [0, 1])
    blocks = bind_plan(gs, plain([b"xabab", b"", b"ab", b"b"]))
    want = check(gs, side, blocks, (b"ab", b"b", b"ab", b"zz"), what="a duplicate")
    assert want == ([0, 6, 6, 9, 10], [1, 1, 2, 3, 3, 4, 5, 5, 6, 7], [0, 2, 1, 0, 2, 1, 0, 2, 1, 1])
    blocks = bind_plan(gs, plain([b"xa", b"b"]))
    assert check(gs, side, blocks, (b"ab",), what="no occurrence straddles two chunks") == ([0, 0, 0], [], [])


def test_ignore_case_and_global_offsets(gs, side):
    blocks = bind_plan(gs, plain([b"AbaB caf\xc9", b"Ab"]))
    assert check(gs, side, blocks, (b"aB", b"caf\xe9", b"CAF\xc9"), IC, what="icase") == ([0, 3, 4], [0, 2, 5, 9], [0, 0, 2, 0])
    assert check(gs, side, blocks, (b"aB", b"Ab"), 0, what="the same, case-sensitive") == ([0, 2, 3], [0, 2, 9], [1, 0, 1])
    go = [(1 << 40) + 7, 3]
    blocks = bind_plan(gs, plain([b"xab", b"ab ab"]), go)
    assert check(gs, side, blocks, (b"ab",), what="global offsets", go=go) == ([0, 1, 3], [(1 << 40) + 8, 3, 6], [0, 0, 0])


def test_whole_words(gs, side):
    # `art` not in `party`; the edges of a chunk are boundaries whatever lies around it (`xart|` + `art` + `_`)
    plan = [(SC.u8(b"art party art"), b""), (SC.u8(b"xart"), b""), (SC.u8(b"art"), b"_art"), (SC.u8(b"ART-art_ art"), b"s")]
    blocks = bind_plan(gs, plan)
    assert check(gs, side, blocks, (b"art", b"party"), 0, WW, "whole words") == ([0, 3, 3, 4, 5], [0, 4, 10, 17, 29], [0, 1, 0, 0, 0])
    assert check(gs, side, blocks, (b"art",), IC, WW, "whole words, icase")[0] == [0, 2, 2, 3, 5]
    assert check(gs, side, blocks, (b"art",), 0, 0, "the same list without the option")[0] == [0, 3, 4, 5, 7]


# ---- 2. the edges of the partition ---------------------------------------------------------------------------------------------
EDGES = (15, 16, 17, 1023, 1024, 4095, 4096, 16383, 16384)  # unit, wave-load, wave span and tile edges


def edge_plan(g):
    """the shortest literal (g bytes) and `needle`, each starting at every edge position (three groups, so that no two
    overlap), in chunks of a tile and 23 bytes; then each ending exactly at a chunk's end and each cut by it, the bytes
    behind the end completing it"""
    short, long_ = SC.END_LITS[g]
    plan, groups = [], []  # groups: (chunk, index of the literal in (long_, short), the positions it starts at)
    for j, lit in ((1, short), (0, long_)):
        for group in (EDGES[0::3], EDGES[1::3], EDGES[2::3]):
            body = bytearray(b"." * (TILE + 23))
            for p in group:
                body[p:p + len(lit)] = lit
            groups.append((len(plan), j, list(group)))
            plan.append((SC.u8(body), b""))
        for n in (5003, 2 * TILE + 5, TILE + len(lit), len(lit)):
            groups.append((len(plan), j, [n - len(lit)]))
            plan.append((SC.u8(b"." * (n - len(lit)) + lit), b""))  # ends exactly at L
            if len(lit) > 1 and n > len(lit):
                groups.append((len(plan), j, []))
                plan.append((SC.u8(b"." * (n - len(lit)) + lit[:-1]), lit[-1:]))  # cut by L: not reported
    return plan, groups


@pytest.mark.parametrize("flags", [0, IC], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_edges_of_the_partition(gs, side, g, flags):
    plan, groups = edge_plan(g)
    short, long_ = SC.END_LITS[g]
    assert all(b.size % 16 for b, lack in plan if lack)  # a pad behind every cut end: the bytes there complete the literal
    assert sum(1 for _, lack in plan if lack) >= 3 and any(b.size % 16 for b, _ in plan)
    blocks = bind_plan(gs, plan)
    want = check(gs, side, blocks, (long_, short), flags, what=("edges", g, flags))
    # (the model, spelled out: every planted literal at its position and nothing else -- a cut one is not reported)
    starts = [0] + np.cumsum([b.size for b in blocks]).tolist()
    for c, j, at in groups:
        lo, hi = want[0][c], want[0][c + 1]
        assert [p - starts[c] for p in want[1][lo:hi]] == at and want[2][lo:hi] == [j] * len(at), ("edges", g, "chunk", c)


# ---- 3. queue rounds and ranks ---------------------------------------------------------------------------------------------------
def test_every_position_a_candidate_with_three_hits(gs, side):
    n = TILE + 5
    plan = [(SC.u8(b"a" * n), b"")]
    blocks = bind_plan(gs, plan)  # (behind the end: ` needle ...`, no `a` at once)
    want = check(gs, side, blocks, (b"a", b"aa", b"a"), what="rounds and ranks")
    assert len(want[1]) == 3 * n - 1 and want[1][:6] == [0, 0, 0, 1, 1, 1] and want[2][:6] == [0, 1, 2, 0, 1, 2]
    assert want[1][-2:] == [n - 1, n - 1] and want[2][-2:] == [0, 2]


# ---- 4. many chunks ----------------------------------------------------------------------------------------------------------------
def many_chunks():
    rng = np.random.Generator(np.random.PCG64(300))
    short, long_ = SC.END_LITS[3]
    plan = []
    for i in range(300):
        n = 0 if i % 19 == 4 else int(rng.integers(1, 3 * TILE + 1))
        body = bytearray(SC._ending_in(b"", n).tobytes()) if n else bytearray()
        hits = 0 if i % 7 == 3 else int(rng.integers(1, 6))  # every seventh holds none
        for _ in range(hits):
            lit = (short, long_)[int(rng.integers(0, 2))]
            if n > len(lit):
                at = int(rng.integers(0, n - len(lit) + 1))
                body[at:at + len(lit)] = lit
        lack = b""
        if i % 5 == 1 and n > 8 and n % 16:  # cut by the end; the pad completes it
            body[n - len(long_) + 1:] = long_[:-1]
            lack = long_[-1:]
        plan.append((SC.u8(body), lack))
    return plan


def test_many_chunks_and_grids(gs, side):
    plan = many_chunks()
    lits = SC.END_LITS[3]
    blocks = bind_plan(gs, plan)
    assert sum(1 for b in blocks if b.size == 0) >= 10 and sum(1 for _, lack in plan if lack) >= 30
    want = check(gs, side, blocks, lits, what="many chunks")
    empty = sum(1 for c in range(len(blocks)) if blocks[c].size and want[0][c] == want[0][c + 1])
    assert empty >= 20 and len(want[1]) > 300
    assert all(want[0][c] == want[0][c + 1] for c, b in enumerate(blocks) if b.size == 0)
    for grid in ("1", "3", None):
        for _ in range(2):  # bit-identical across grids and from call to call
            assert with_env({"XSG_LITFIND_GRID": grid}, lambda: sync(gs)) == want, ("many chunks", "grid", grid)
    rerun = with_env({"XSG_LITFIND_GRID": "3"}, lambda: side.run(gs.shard, len(blocks), len(want[1])))
    assert rerun == (*want, xsg.STATUS_OK)


# ---- 5. the longest list -----------------------------------------------------------------------------------------------------------
def test_4096_distinct_literals_on_one_tile(gs, side):
    lits = SE.limit_distinct()
    assert len(lits) == xsg.MAX_LITERALS
    rng = np.random.Generator(np.random.PCG64(4096))
    body = bytearray(bytes(b"abcdefgh"[int(x)] for x in rng.integers(0, 8, size=TILE - 3)))
    for at, j in ((0, 0), (1017, 4095), (4090, 2048), (TILE - 3 - 7, 1)):  # the first, the last, across a span edge, at the end
        body[at:at + 7] = lits[j]
    plan = [(SC.u8(body), b"")]
    blocks = bind_plan(gs, plan)
    want = check(gs, side, blocks, lits, what="4096 literals")
    assert len(want[1]) >= 4 and {0, 4095, 2048, 1} <= set(want[2])


# ---- 6. capacity ---------------------------------------------------------------------------------------------------------------------
def test_capacity_of_the_stream_ordered_form(gs, side):
    import corpus
    blocks = [corpus.text_block(11, i, 40_000 + 13 * i, needle_rate=2e-3) for i in range(3)]
    lits = SC.word_list(9)
    n = len(blocks)
    bind_plan(gs, [(b, b"") for b in blocks])
    want = check(gs, side, blocks, lits, what="capacity")
    total = len(want[1])
    first = want[0][1]
    assert 1 < first < total - 1
    for cap in (total, total - 1, first, 0):
        cp, pos, lit, status = side.run(gs.shard, n, cap)  # (asserts that the 0xFF words at and behind cap are untouched)
        assert status == (xsg.STATUS_OK if cap >= total else xsg.STATUS_OVERFLOW), ("capacity", cap)
        assert cp == want[0], ("capacity", cap, "chunk_ptr is complete")
        assert pos == want[1][:cap] and lit == want[2][:cap], ("capacity", cap, "the entries below it")
        cp2, pos2, lit2, status2 = side.run(gs.shard, n, cp[n])  # come back with chunk_ptr[n]
        assert status2 == xsg.STATUS_OK and (cp2, pos2, lit2) == want, ("capacity", cap, "the second call")


# ---- 7. refusals and the kept result -------------------------------------------------------------------------------------------------
def test_refusals_and_the_kept_result(gs, side):
    import torch
    blocks = SC.raw_blocks()
    lits = SC.RAW_LIST
    n = len(blocks)
    want = FM.find(blocks, lits)
    total = len(want[1])
    assert total >= 2

    def result(lib, h, rows=n + 1, entries=total, with_pos=True, with_lit=True):
        cp = np.full(n + 3, 7, dtype=np.uint64)
        pos = np.full(total + 2, 7, dtype=np.uint64)
        lit = np.full(total + 2, 7, dtype=np.uint32)
        rc = lib.xsg_result_literal_hits(h, C.c_void_p(cp.ctypes.data), rows, C.c_void_p(pos.ctypes.data) if with_pos else None,
                                         C.c_void_p(lit.ctypes.data) if with_lit else None, entries)
        return rc, cp.tolist(), pos.tolist(), lit.tolist()

    untouched = ([7] * (n + 3), [7] * (total + 2), [7] * (total + 2))
    kept = (xsg.OK, want[0] + [7, 7], want[1] + [7, 7], want[2] + [7, 7])
    fresh = GpuSearch()
    fresh.bind(blocks)
    with pytest.raises(xsg.XsgError) as e:  # the context holds no pattern
        fresh.shard.find_literals()
    assert e.value.code == xsg.ESTATE
    fresh.ctx.set_literals(xsg.literal_list(lits), 0)
    assert result(fresh.shard._lib, fresh.shard.h) == (xsg.ESTATE,) + untouched  # before any find
    fresh.ctx.close()

    gs.bind(blocks)
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    lib, h = gs.shard._lib, gs.shard.h
    assert sync(gs) == want
    # the kept result: copied out again and again, with room to spare, chunk_ptr alone
    assert result(lib, h) == kept
    assert result(lib, h, rows=n + 3, entries=total + 2) == kept
    assert result(lib, h, entries=0, with_pos=False, with_lit=False) == (xsg.OK, want[0] + [7, 7]) + untouched[1:]
    for kw in ({"rows": n}, {"entries": total - 1}, {"with_pos": False}, {"with_lit": False}):
        assert result(lib, h, **kw) == (xsg.EINVAL,) + untouched, kw
    assert lib.xsg_result_literal_hits(h, None, n + 1, None, None, 0) == xsg.EINVAL  # chunk_ptr is null
    assert lib.xsg_find_literals(h, None) == xsg.EINVAL  # total is null
    # ... and it survives other entry points in between: a count, a search, the other counts per literal, the other form
    assert int(gs.shard.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) > 0
    assert gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).size > 0
    assert gs.shard.count_literals().tolist() == FM.bincount(want[2], len(lits))
    gs.shard.count_literals_csr()
    assert side.run(gs.shard, n, total)[:3] == want
    assert result(lib, h) == kept
    # the stream-ordered form's own refusals: a null output, one row short
    dev = torch.zeros(n + 2 * total + 8, dtype=torch.int64, device="cuda:0")
    p = C.c_void_p(dev.data_ptr())
    for args in ((None, n + 1, p, p, total, p), (p, n + 1, None, p, total, p), (p, n + 1, p, None, total, p), (p, n + 1, p, p, total, None),
                 (p, n, p, p, total, p)):
        assert lib.xsg_find_literals_async(h, None, *args) == xsg.EINVAL, args
    assert not dev.any().item()  # a refusal writes nothing
    # a pattern that is no list, an inverted list
    total_out = C.c_uint64(0)
    gs.ctx.set_pattern(b"caf", 0)
    for call in (lambda: gs.shard.find_literals(), lambda: side.run(gs.shard, n, total)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "xsg_set_literals" in str(e.value)
    gs.ctx.set_literals(xsg.literal_list(lits), xsg.FLAG_INVERT)
    for call in (lambda: gs.shard.find_literals(), lambda: side.run(gs.shard, n, total)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "XSG_FLAG_INVERT" in str(e.value)
    assert lib.xsg_find_literals(h, C.byref(total_out)) == xsg.ENOTSUP
    assert result(lib, h)[0] == xsg.OK  # (a refused call ran no pass: the result of the last one that did is still kept)
    # the CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and change nothing
    for flags in (xsg.FLAG_EXACT_TAIL, xsg.flag_context(2, 3), xsg.FLAG_EXACT_TAIL | xsg.flag_context(4095, 1)):
        gs.ctx.set_literals(xsg.literal_list(lits), flags)
        assert sync(gs) == want
    # a list of one literal without a border: pos is the XSG_MATCH_BYTE_OFFSETS list under XSG_FLAG_EXACT_TAIL
    gs.ctx.set_literals(xsg.literal_list(lits[1:2]), xsg.FLAG_EXACT_TAIL)
    one = sync(gs)
    assert len(one[1]) > 0 and one[1] == gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist()
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    assert sync(gs) == want
    # an invalidate and a rebind drop the kept result
    gs.shard.invalidate()
    assert result(lib, h) == (xsg.ESTATE,) + untouched
    assert sync(gs) == want and result(lib, h)[0] == xsg.OK
    gs.bind(blocks)
    assert result(gs.shard._lib, gs.shard.h) == (xsg.ESTATE,) + untouched
    assert sync(gs) == want


def test_a_binding_of_2_24_chunks_is_refused():
    import torch
    n = 1 << 24
    g = GpuSearch()
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    g.shard = xsg.Shard(g.ctx, t.data_ptr(), 256, np.zeros(n, dtype=xsg.CHUNK_DTYPE))  # chunks of length 0: no tile, no text
    g.ctx.set_literals(b"ab", 0)
    lib, h = g.shard._lib, g.shard.h
    total = C.c_uint64(7)
    assert lib.xsg_find_literals(h, C.byref(total)) == xsg.ENOTSUP and b"2^24" in lib.xsg_last_error() and total.value == 7
    p = C.c_void_p(t.data_ptr())  # (refused before an output is looked at)
    assert lib.xsg_find_literals_async(h, None, p, n + 1, p, p, 0, p) == xsg.ENOTSUP and b"2^24" in lib.xsg_last_error()
    assert not t.any().item()
    g.ctx.close()


def test_no_chunks(gs, side):
    import torch
    gs.bind([SC.u8(b"ab")])
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    gs.shard.rebind(t.data_ptr(), 256, xsg.make_chunks([], []))
    gs.keep = t
    assert check(gs, side, [], (b"ab", b"b"), what="no chunks") == ([0], [], [])


# ---- 8. chunks in host memory: LiteralFinder and xsgrep --find-each ------------------------------------------------------------------
FILE_LITS = (b"Sherlock", b"She", b"lock", b"e", b"Holmes", b"She", b"zzzq")


@pytest.fixture(scope="module")
def text_file(tmp_path_factory):
    """about 100 KB of lines; with XSGREP_CHUNK_BYTES = 40 000 it is read in three newline-aligned chunks"""
    import corpus
    t = corpus.text_block(21, 0, 100_000, needle_rate=2e-3).tobytes()
    t = t[:1000] + b"SHERLOCK hOLMES sherlocks\n" + t[1000:] + b"Holmes"  # (an open last line)
    p = tmp_path_factory.mktemp("find_each") / "text.txt"
    p.write_bytes(t)
    return p, t


@pytest.mark.parametrize("flags,list_flags", [(0, 0), (IC, 0), (0, WW), (IC, WW)], ids=["plain", "icase", "words", "icase-words"])
def test_literal_finder_on_three_chunks(text_file, flags, list_flags):
    _, t = text_file
    cuts = [0, t.rfind(b"\n", 0, 40_000) + 1, t.rfind(b"\n", 0, 80_000) + 1, len(t)]
    blocks = [SC.u8(t[a:b]) for a, b in zip(cuts, cuts[1:])]
    assert len(blocks) == 3 and all(b.size > TILE for b in blocks)
    want = FM.find(blocks, FILE_LITS, bool(flags & IC), bool(list_flags & WW))
    lf = xsg.LiteralFinder(0, xsg.literal_list(FILE_LITS), flags, list_flags)
    pos, lit = [], []
    for c, b in enumerate(blocks):
        p, l = lf.find(b if c else b.tobytes(), cuts[c])  # (bytes and arrays alike)
        assert p.dtype == np.uint64 and l.dtype == np.uint32
        assert (p.tolist(), l.tolist()) == (want[1][want[0][c]:want[0][c + 1]], want[2][want[0][c]:want[0][c + 1]]), ("finder", c)
        pos += p.tolist()
        lit += l.tolist()
    assert len(pos) > 1000 and (pos, lit) == (want[1], want[2])
    p, l = lf.find(b"", 5)
    assert p.size == 0 and l.size == 0
    p, l = lf.find(b"xShe She", 1 << 40)  # the finder goes on after an empty chunk; `base` is added
    small = FM.find([SC.u8(b"xShe She")], FILE_LITS, bool(flags & IC), bool(list_flags & WW), [1 << 40])
    assert (p.tolist(), l.tolist()) == (small[1], small[2]) and p.size >= 2
    lf.close()


def run_xsgrep(args, stdin=None, chunk_bytes=None):
    env = dict(os.environ)
    if chunk_bytes:
        env["XSGREP_CHUNK_BYTES"] = str(chunk_bytes)
    return subprocess.run([str(XSGREP)] + [os.fsencode(a) if isinstance(a, str) else a for a in args], input=stdin, capture_output=True,
                          timeout=300, env=env)


def printed(want, lits):
    return b"".join(b"%d:%s\n" % (p, lits[j]) for p, j in zip(want[1], want[2]))


@pytest.mark.parametrize("opts,icase,words", [([], False, False), (["-i"], True, False), (["-w"], False, True), (["-i", "-w"], True, True)],
                         ids=["plain", "icase", "words", "icase-words"])
def test_xsgrep_find_each_on_a_file_in_three_chunks(text_file, tmp_path, opts, icase, words):
    path, t = text_file
    pf = tmp_path / "patterns.txt"
    pf.write_bytes(b"\n".join(FILE_LITS[2:5]) + b"\n")
    args = ["-F"] + opts + ["--find-each", "-e", FILE_LITS[0], "-e", FILE_LITS[1], "-f", str(pf), "-e", FILE_LITS[5], "-e", FILE_LITS[6]]
    # (a newline is no word byte and a literal holds none: the cuts change nothing, the input's end is the last chunk's)
    want = FM.find([SC.u8(t)], FILE_LITS, icase, words)
    assert len(want[1]) > 1000
    r = run_xsgrep(args + [str(path)], chunk_bytes=40_000)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == printed(want, FILE_LITS)  # the literal as listed, not the text's case
    one = run_xsgrep(args + [str(path)])  # one chunk holds it all: the same lines
    assert one.returncode == 0 and one.stdout == r.stdout


def test_xsgrep_find_each_on_stdin_and_a_single_pattern(text_file):
    path, t = text_file
    r = run_xsgrep(["-F", "--find-each", "-e", "lock", "-e", "She", "-"], stdin=t, chunk_bytes=30_000)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == printed(FM.find([SC.u8(t)], (b"lock", b"She")), (b"lock", b"She"))
    r = run_xsgrep(["-F", "--find-each", "Holmes", str(path)])  # a list of one
    assert r.returncode == 0 and r.stdout == printed(FM.find([SC.u8(t)], (b"Holmes",)), (b"Holmes",))
    r = run_xsgrep(["-Fi", "--find-each", "-e", "aa", "-e", "A", "-"], stdin=b"aAa\naa")
    assert r.returncode == 0 and r.stdout == b"0:aa\n0:A\n1:aa\n1:A\n2:A\n4:aa\n4:A\n5:A\n"
    r = run_xsgrep(["-F", "--find-each", "-e", "x", "-"], stdin=b"")
    assert r.returncode == 0 and r.stdout == b""
