"""xsg_count_chunks / xsg_count_chunks_async: one count per bound chunk in one pass.

For chunk c the expected value is the oracle run on that chunk's bytes alone (the per-chunk loop bodies of
tests/gpu_util.py: oracle_all_modes and its regex siblings; set_model for a literal list).  Every case also checks
sum(counts) == totals[...], totals == shard.count(mode), and that a plain count right behind the call finds the per-tile
arrays as it expects (same numbers as before the call, with and without XSG_WITH_NEWLINES).

Tiles are 16 KiB and are counted per chunk: a chunk of k tiles is a chunk of (k - 1) * 16 KiB + 1 .. k * 16 KiB bytes.
"""
import os

import numpy as np
import pytest

import anchor_oracle
import corpus
import set_model
import xsg
from gpu_util import GpuSearch, oracle_all_modes, oracle_regex_all_modes

pytestmark = pytest.mark.gpu
TILE = xsg.TILE
NEEDLE = b"Sherlock"
M, L, NL = xsg.COUNT_MATCHES, xsg.COUNT_LINES, xsg.WITH_NEWLINES
TAILS = ((0, "lossy"), (xsg.FLAG_EXACT_TAIL, "exact"))


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


@pytest.fixture(scope="module")
def base_text():
    """8 MiB of lower-case text without the needle; chunks are slices of it"""
    t = corpus.text_block(77, 0, 8 << 20, needle_rate=0.0)
    assert NEEDLE not in t.tobytes()
    t.setflags(write=False)
    return t


def put(b, pat, *offs):
    for o in offs:
        if 0 <= o <= b.size - len(pat):
            b[o:o + len(pat)] = np.frombuffer(pat, dtype=np.uint8)


def bind_raw(gs, t, capacity, chunks):
    """bind a tensor that is already laid out (gpu_util.upload packs at 256-byte offsets)"""
    if gs.shard is None:
        gs.shard = xsg.Shard(gs.ctx, t.data_ptr(), capacity, chunks)
    else:
        gs.shard.rebind(t.data_ptr(), capacity, chunks)
    gs.keep = t


def chunk_newlines(blocks):
    return [int(np.count_nonzero(b == 10)) for b in blocks]


def chunk_lines(blocks):
    """lines of a chunk as include/xsg.h defines them under XSG_FLAG_INVERT"""
    return [int(np.count_nonzero(b == 10)) + (1 if b.size and b[-1] != 10 else 0) for b in blocks]


def literal_want(oracle, blocks, pat, lines, exact=False, icase=False):
    """the body of oracle_all_modes' loop, count tags only"""
    if icase:
        blocks = [oracle.lower(b) for b in blocks]
        pat = oracle.lower(pat).tobytes()
    oracle.set_exact(bool(exact))
    try:
        return [oracle.count(b, pat, lines) for b in blocks]
    finally:
        oracle.set_exact(False)


def check(gs, mode, want, want_nl, where):
    s = gs.shard
    key = xsg.CTR_MATCHES if mode == M else xsg.CTR_LINES
    before = s.count(mode).tolist()
    before_nl = s.count(mode | NL).tolist()
    counts, nls, totals = s.count_chunks(mode)
    print(where, "counts", counts.tolist()[:16], "want", want[:16], "totals", totals.tolist())
    assert nls is None
    assert counts.tolist() == want, where
    assert int(counts.sum()) == int(totals[key]), where
    assert totals.tolist() == before, where
    counts, nls, totals = s.count_chunks(mode | NL)
    assert counts.tolist() == want, (where, "with newlines")
    assert nls.tolist() == want_nl, (where, "newlines")
    assert int(counts.sum()) == int(totals[key]) and int(nls.sum()) == int(totals[xsg.CTR_NEWLINES]), where
    assert totals.tolist() == before_nl, where
    assert s.count(mode).tolist() == before, (where, "a plain count behind the call")
    assert s.count(mode | NL).tolist() == before_nl, (where, "a plain count with newlines behind the call")


def check_literal(gs, oracle, blocks, pat, where, flags=0):
    gs.ctx.set_pattern(pat, flags)
    exact, icase = bool(flags & xsg.FLAG_EXACT_TAIL), bool(flags & xsg.FLAG_IGNORE_CASE)
    nl = chunk_newlines(blocks)
    for mode, lines in ((M, False), (L, True)):
        check(gs, mode, literal_want(oracle, blocks, pat, lines, exact, icase), nl, (where, "lines" if lines else "matches"))


# ---- cut shapes -----------------------------------------------------------------------------------------------------------
def cut(base_text, rng, tiles):
    """chunks of the given sizes in tiles (0: a chunk of length 0), the needle at known places: inside, across a tile
    border, and in the last bytes of every third chunk"""
    blocks, pos = [], 0
    for i, k in enumerate(tiles):
        n = 0 if k == 0 else (k - 1) * TILE + int(rng.integers(1, TILE + 1))
        if k and i % 4 == 1:
            n = k * TILE  # a chunk that fills its last tile
        pos = (pos + 4099) % (base_text.size - n - 1)
        b = base_text[pos:pos + n].copy()
        if n >= 64:
            put(b, NEEDLE, *[int(x) for x in rng.integers(0, n - 8, size=min(3, 1 + k // 16))])
            for t in range(1, k, 7):
                put(b, NEEDLE, t * TILE - 3, t * TILE)  # across a tile border, and at a tile's first byte
            if i % 3 == 0:
                put(b, NEEDLE, n - 8 - int(rng.integers(0, 30)))  # in the end-of-chunk zone
        blocks.append(b)
    return blocks


SHAPES = {
    "1x1": [1],
    "1x64": [64],
    "1x65": [65],
    "1x200": [200],
    "1x300": [300],  # a wave takes a second block of 64 tiles: the run it holds pending continues there
    "pending_runs_end": [130, 130, 40, 1, 70],  # ... and ends there, in the block's first lanes or further in
    "65x1": [1] * 65,
    "lanes_0_1_63_and_aligned": [1, 62, 1, 1, 63, 64, 2],
    "empty_chunks": [0, 3, 0, 0, 2, 1, 0],
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cut_shapes(gs, oracle, base_text, shape):
    rng = np.random.default_rng(6100 + len(shape))
    blocks = cut(base_text, rng, SHAPES[shape])
    if shape == "65x1":
        blocks[0] = np.frombuffer(b"a Sherlock here\n", dtype=np.uint8).copy()  # a 16-byte chunk is one tile
    gs.bind(blocks)
    for flags, name in TAILS:
        check_literal(gs, oracle, blocks, NEEDLE, (shape, name), flags)


def test_more_chunks_than_the_finish_grid_has_waves(gs, oracle, base_text):
    rng = np.random.default_rng(6200)
    n = 8200  # > 2048 workgroups x 4 waves: the chunk loop strides
    blocks = [base_text[48 * i:48 * i + 48].copy() for i in range(n)]
    for i in rng.integers(0, n, size=600):
        put(blocks[int(i)], NEEDLE, int(rng.integers(0, 41)))
    put(blocks[n - 1], NEEDLE, 40)
    put(blocks[8192], NEEDLE, 0, 20)
    gs.bind(blocks)
    for flags, name in TAILS:
        check_literal(gs, oracle, blocks, NEEDLE, ("8200x48", name), flags)


# ---- places relative to a chunk's end -------------------------------------------------------------------------------------
def test_needle_only_in_the_end_of_chunk_zone(gs, oracle, base_text):
    """the last plen + 31 bytes are decided by the replayed walk: decoys in front of the needle make the lossy count differ
    from the exact one, chunk by chunk"""
    tails = (b"Sherlock", b"SSherlock", b" SheSherlock", b"SherSherlock\n", b"Sherlock Sherlock", b"SheSherlockSherlock\n", b"xx\n")
    blocks = []
    for i in range(40):
        n = 3 * TILE + 17 * i
        b = base_text[1000 * i:1000 * i + n].copy()
        t = tails[i % len(tails)]
        if i % 5 != 4:  # every fifth chunk holds nothing
            put(b, t, n - len(t) - (i % 3) * 4)
        blocks.append(b)
    gs.bind(blocks)
    want = {}
    for flags, name in TAILS:
        want[name] = literal_want(oracle, blocks, NEEDLE, False, bool(flags))
        check_literal(gs, oracle, blocks, NEEDLE, ("zone", name), flags)
    assert want["lossy"] != want["exact"]  # the cases do tell the two tails apart


def test_needle_cut_by_a_chunk_end_counts_in_neither_chunk(gs, oracle, base_text):
    """16-byte packing: chunk k + 1 starts where chunk k ends, and holds the rest of the needle chunk k's end cut off"""
    import torch
    lengths = [TILE + 32, 48, 16, 5 * TILE, 64, 2 * TILE + 16]
    blocks = [base_text[7000 * i:7000 * i + n].copy() for i, n in enumerate(lengths)]
    for k in range(len(blocks) - 1):
        cutat = 1 + k % 7
        put(blocks[k], NEEDLE[:cutat], blocks[k].size - cutat)
        put(blocks[k + 1], NEEDLE[cutat:], 0)
    put(blocks[3], NEEDLE, 100, 3 * TILE - 4)
    host = np.concatenate(blocks)
    assert host.tobytes().count(NEEDLE) == 2 + len(blocks) - 1  # a reader that looks past a chunk's end sees them all
    off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    t = torch.from_numpy(np.concatenate([host, np.zeros(256, dtype=np.uint8)])).to("cuda:0")
    bind_raw(gs, t, int(host.size), xsg.make_chunks(off, lengths))
    for flags, name in TAILS:
        gs.ctx.set_pattern(NEEDLE, flags)
        want = literal_want(oracle, blocks, NEEDLE, False, bool(flags))
        assert sum(want) == 2
        check(gs, M, want, chunk_newlines(blocks), ("packed", name))
        check(gs, L, literal_want(oracle, blocks, NEEDLE, True, bool(flags)), chunk_newlines(blocks), ("packed lines", name))


def test_open_last_line_and_one_long_line(gs, oracle, base_text):
    a = base_text[:2 * TILE + 100].copy()
    a[-1] = ord("k")  # does not end in '\n'
    put(a, NEEDLE, 50, a.size - 8)
    one = base_text[50000:50000 + 3 * TILE + 5].copy()
    one[one == 10] = 32  # one long line, no '\n' at all
    put(one, NEEDLE, 10, TILE - 4, 2 * TILE + 9, one.size - 20)
    c = base_text[90000:90000 + TILE].copy()
    blocks = [a, one, c]
    gs.bind(blocks)
    for flags, name in TAILS:
        check_literal(gs, oracle, blocks, NEEDLE, ("lines", name), flags)
    assert literal_want(oracle, blocks, NEEDLE, True)[1] == 1
    # the inverted count: lines(c) - matching lines(c), by the definition of a chunk's lines under XSG_FLAG_INVERT
    gs.ctx.set_pattern(NEEDLE, xsg.FLAG_INVERT)
    want = [n - m for n, m in zip(chunk_lines(blocks), literal_want(oracle, blocks, NEEDLE, True))]
    check(gs, L, want, chunk_newlines(blocks), "inverted")


# ---- pattern kinds -----------------------------------------------------------------------------------------------------------
LONG = {n: bytes(np.random.default_rng(7000 + n).integers(65, 91, size=n, dtype=np.uint8)) for n in (20, 40, 2000)}
EXTRA = (b"ERROR one\nthe colour of color that that\naaaa aa aaaaa a\nabababab abab\nfoo\nwoo o\nw\nwalking singing\n",
         b"no ERROR here\nERROR two\nERRORS\ncolor colr\naaa\nababab\nthat\n",
         b"xERROR\nwing\nbringing it\nfoo\n\nwoo\n")


@pytest.fixture(scope="module")
def six(gs):
    """six chunks, about 1 MiB, the needles of every kind below in them; the last chunk's last line is open"""
    blocks = []
    for i in range(6):
        b = corpus.text_block(91, i, 170_000 + 777 * i, needle_rate=5e-4)
        for n, pat in LONG.items():
            if (i + n) % 3 == 0:
                put(b, pat, 5000 + n, b.size - n - 200 * (i % 2))
        put(b, LONG[20], b.size - 20 - 7)  # in the end-of-chunk zone
        blocks.append(np.concatenate([b, np.frombuffer(EXTRA[i % 3], dtype=np.uint8)]))
    blocks[5] = np.concatenate([blocks[5], np.frombuffer(b" SheSherlock", dtype=np.uint8)])
    assert all(b"thathat" not in b.tobytes() for b in blocks)
    return blocks


def bind_six(gs, six):
    gs.bind(six)
    return six


@pytest.mark.parametrize("plen", (1, 3, 4, 6, 8, 20, 40, 2000))
def test_literals_of_every_length_class(gs, oracle, six, plen):
    blocks = bind_six(gs, six)
    pat = LONG[plen] if plen in LONG else (b"e", b"She", b"Sher", b"Sherlo", b"Sherlock")[(1, 3, 4, 6, 8).index(plen)]
    for flags, name in TAILS:
        check_literal(gs, oracle, blocks, pat, (plen, name), flags)


def test_ignore_case_literal(gs, oracle, six):
    blocks = bind_six(gs, six)
    check_literal(gs, oracle, blocks, b"sHERlock", "icase", xsg.FLAG_IGNORE_CASE)
    # literal_want is oracle_all_modes' loop body: the same numbers as the function itself, chunk by chunk
    per = [oracle_all_modes(oracle, [b], b"sHERlock", ignore_case=True) for b in blocks]
    assert [p["count_matches"] for p in per] == literal_want(oracle, blocks, b"sHERlock", False, icase=True)
    assert [p["count_lines"] for p in per] == literal_want(oracle, blocks, b"sHERlock", True, icase=True)


def regex_want(oracle, blocks, expr):
    per = [oracle_regex_all_modes(oracle, [b], expr, False)[0] for b in blocks]
    return [p["count_matches"] for p in per], [p["count_lines"] for p in per]


@pytest.mark.parametrize("expr", (b"She[r ]lock", b"colou?r", b"\\w+ing", b"[a-z]+ [a-z]+"))
def test_expressions(gs, oracle, six, expr):
    blocks = bind_six(gs, six)
    wm, wl = regex_want(oracle, blocks, expr)
    assert sum(wm) > 0
    gs.ctx.set_pattern(expr, xsg.FLAG_REGEX)
    check(gs, M, wm, chunk_newlines(blocks), (expr, "matches"))
    check(gs, L, wl, chunk_newlines(blocks), (expr, "lines"))


def test_line_anchor(gs, six):
    blocks = bind_six(gs, six)
    per = [anchor_oracle.all_modes([b], b"(?m)^ERROR") for b in blocks]
    assert sum(p["count_matches"] for p in per) >= 6
    gs.ctx.set_pattern(b"(?m)^ERROR", xsg.FLAG_REGEX)
    check(gs, M, [p["count_matches"] for p in per], chunk_newlines(blocks), "anchor matches")
    check(gs, L, [p["count_lines"] for p in per], chunk_newlines(blocks), "anchor lines")


LIST = (b"Sherlock", b"She", b"lock", b"colour", b"ERROR")


def test_literal_list(gs, six):
    blocks = bind_six(gs, six)
    per = [set_model.all_modes([b], LIST) for b in blocks]
    gs.ctx.set_literals(xsg.literal_list(LIST), 0)
    check(gs, M, [p["count_matches"] for p in per], chunk_newlines(blocks), "list matches")
    check(gs, L, [p["count_lines"] for p in per], chunk_newlines(blocks), "list lines")


@pytest.mark.parametrize("pat", (b"aa", b"abab"))
def test_bordered_literals_that_overlap_take_the_list_fallback(gs, oracle, six, pat):
    blocks = bind_six(gs, six)
    assert any((pat + pat[-len(pat) // 2:]) in b.tobytes() for b in blocks)  # `aaa` / `ababab`: occurrences do overlap here
    check_literal(gs, oracle, blocks, pat, pat)


def test_bordered_literal_that_is_overlap_free_takes_scan_and_finish(gs, oracle, six):
    blocks = bind_six(gs, six)
    check_literal(gs, oracle, blocks, b"that", "that")
    assert sum(literal_want(oracle, blocks, b"that", False)) >= 6


def test_count_lines_of_a_literal_with_a_newline(gs, oracle, six):
    blocks = bind_six(gs, six)
    gs.ctx.set_pattern(b"o\nw", 0)
    want = literal_want(oracle, blocks, b"o\nw", True)
    assert sum(want) >= 4
    check(gs, L, want, chunk_newlines(blocks), "o\\nw lines")


@pytest.mark.parametrize("kind", ("literal", "prefilter", "list"))
def test_inverted_line_counts(gs, oracle, six, kind):
    blocks = bind_six(gs, six)
    if kind == "literal":
        plain = literal_want(oracle, blocks, NEEDLE, True)
        gs.ctx.set_pattern(NEEDLE, xsg.FLAG_INVERT)
    elif kind == "prefilter":
        plain = regex_want(oracle, blocks, b"colou?r")[1]
        gs.ctx.set_pattern(b"colou?r", xsg.FLAG_REGEX | xsg.FLAG_INVERT)
    else:
        plain = [set_model.all_modes([b], LIST)["count_lines"] for b in blocks]
        gs.ctx.set_literals(xsg.literal_list(LIST), xsg.FLAG_INVERT)
    want = [n - m for n, m in zip(chunk_lines(blocks), plain)]
    check(gs, L, want, chunk_newlines(blocks), ("inverted", kind))
    with pytest.raises(xsg.XsgError) as e:
        gs.shard.count_chunks(M)
    assert e.value.code == xsg.ENOTSUP


# ---- behind the sketch gate --------------------------------------------------------------------------------------------------
def test_sketch_gate_keeps_its_storing_form_and_the_plain_count_its_one_launch(oracle):
    saved = os.environ.get("XSG_SKETCH")
    os.environ["XSG_SKETCH"] = "1"  # a synchronous call builds the sketch before its first eligible pass
    try:
        g = GpuSearch()
        one = corpus.text_block(93, 0, 1 << 20, needle_rate=0.0)
        blocks = []
        for i in range(64):  # 64 MiB: the smallest binding that gets a sketch
            b = one.copy()
            if i % 5 == 0:
                put(b, NEEDLE, 1000 + 37 * i, 40 * TILE - 3, b.size - 8 - (i % 30))
            blocks.append(b)
        g.bind(blocks)
        g.ctx.set_pattern(NEEDLE, 0)
        # (the chunks without a planted needle are copies of one text that holds none)
        want = [literal_want(oracle, [b], NEEDLE, False)[0] if i % 5 == 0 else 0 for i, b in enumerate(blocks)]
        assert sum(want) >= 26
        counts, _, totals = g.shard.count_chunks(M)
        assert counts.tolist() == want
        assert " finishing" in g.shard.scan_kernel_name(M)  # the plain count is still the one-launch form
        assert int(counts.sum()) == int(totals[xsg.CTR_MATCHES])
        assert g.shard.count(M).tolist() == totals.tolist()
        counts2, _, _ = g.shard.count_chunks(M)  # behind the finishing form, which writes no per-tile words
        assert counts2.tolist() == want
        assert " finishing" in g.shard.scan_kernel_name(M)
    finally:
        os.environ.pop("XSG_SKETCH", None)
        if saved is not None:
            os.environ["XSG_SKETCH"] = saved


# ---- the stream-ordered form ---------------------------------------------------------------------------------------------------
class Async:
    def __init__(self, gs, n):
        import torch
        self.torch, self.gs = torch, gs
        self.stream = torch.cuda.Stream()
        z = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda:0")
        self.counts, self.nls, self.counters, self.status = z(n), z(n), z(xsg.NUM_COUNTERS), z(1)

    def run(self, mode, with_nl):
        for t in (self.counts, self.nls, self.counters, self.status):
            t.fill_(-1)
        self.torch.cuda.synchronize()
        self.gs.shard.count_chunks_async(mode | (NL if with_nl else 0), self.stream.cuda_stream, self.counts.data_ptr(),
                                         self.nls.data_ptr() if with_nl else 0, self.counts.numel(), self.counters.data_ptr(),
                                         self.status.data_ptr())
        self.stream.synchronize()
        return self.counts.tolist(), self.nls.tolist(), self.counters.tolist(), int(self.status.item())


@pytest.mark.parametrize("case", ("literal", "literal_exact", "class_sequence", "prefilter_expr", "inverted", "overlap_free"))
def test_async_form_equals_the_synchronous_one(gs, six, case):
    blocks = bind_six(gs, six)
    pat, flags = {"literal": (NEEDLE, 0), "literal_exact": (LONG[40], xsg.FLAG_EXACT_TAIL), "class_sequence": (b"She[r ]lock", xsg.FLAG_REGEX),
                  "prefilter_expr": (b"colou?r", xsg.FLAG_REGEX), "inverted": (NEEDLE, xsg.FLAG_INVERT),
                  "overlap_free": (b"that", 0)}[case]
    gs.ctx.set_pattern(pat, flags)
    a = Async(gs, len(blocks))
    for mode in ((L,) if case == "inverted" else (M, L)):
        sc, sn, st = gs.shard.count_chunks(mode | NL)  # (establishes `that` as overlap-free on this binding as well)
        for with_nl in (False, True):
            counts, nls, counters, status = a.run(mode, with_nl)
            assert status == 0
            assert counts == sc.tolist(), (case, mode, with_nl)
            want_tot = st.tolist() if with_nl else gs.shard.count(mode).tolist()
            assert counters == want_tot, (case, mode, with_nl)
            assert nls == (sn.tolist() if with_nl else [-1] * len(blocks))  # nothing is written without the flag
        assert gs.shard.count(mode | NL).tolist() == st.tolist()


def test_async_refusal_of_non_ascii_data_zeroes_everything(gs, oracle, six):
    blocks = [b.copy() for b in six]
    blocks[3][1234] = 0xC3
    gs.bind(blocks)
    gs.ctx.set_pattern(b"S.erlock", xsg.FLAG_REGEX)  # '.' is exact on ASCII data only
    a = Async(gs, len(blocks))
    for mode in (M, L):
        counts, nls, counters, status = a.run(mode, True)
        assert status == xsg.STATUS_NONASCII
        assert counts == [0] * 6 and nls == [0] * 6 and counters == [0] * 4
        with pytest.raises(xsg.XsgError) as e:  # the synchronous call refuses the whole binding, never per chunk
            gs.shard.count_chunks(mode)
        assert e.value.code == xsg.ENOTSUP
    blocks[3][1234] = ord("x")
    gs.bind(blocks)
    wm = [oracle_regex_all_modes(oracle, [b], b"S.erlock", False)[0]["count_matches"] for b in blocks]
    assert sum(wm) > 0
    assert a.run(M, False)[0] == wm and a.run(M, False)[3] == 0  # the flag word was left at rest


def test_async_refuses_what_needs_a_list(gs, six):
    blocks = bind_six(gs, six)
    a = Async(gs, len(blocks))

    def refused(mode):
        with pytest.raises(xsg.XsgError) as e:
            a.run(mode, False)
        assert e.value.code == xsg.ENOTSUP
        assert "xsg_count_chunks" in str(e.value)

    gs.ctx.set_literals(xsg.literal_list(LIST), 0)
    refused(M)
    refused(L)
    gs.ctx.set_pattern(b"aa", 0)  # bordered, and nothing known about this binding yet
    refused(M)
    gs.ctx.set_pattern(b"o\nw", 0)
    refused(L)


# ---- arguments --------------------------------------------------------------------------------------------------------------
def test_argument_errors(gs, six):
    import ctypes as C
    blocks = bind_six(gs, six)
    gs.ctx.set_pattern(NEEDLE, 0)
    lib, h = gs.shard._lib, gs.shard.h
    n = len(blocks)
    counts = np.zeros(n, dtype=np.uint64)
    nls = np.zeros(n, dtype=np.uint64)
    tot = np.zeros(4, dtype=np.uint64)
    cp, npn, tp = C.c_void_p(counts.ctypes.data), C.c_void_p(nls.ctypes.data), C.c_void_p(tot.ctypes.data)
    assert lib.xsg_count_chunks(h, M, cp, None, n - 1, tp) == xsg.EINVAL              # cap_chunks < nchunks
    assert lib.xsg_count_chunks(h, M, None, None, n, tp) == xsg.EINVAL               # counts null
    assert lib.xsg_count_chunks(h, xsg.MATCH_BYTE_OFFSETS, cp, None, n, tp) == xsg.EINVAL  # a list mode
    assert lib.xsg_count_chunks(h, M | 0x200, cp, None, n, tp) == xsg.EINVAL         # unknown mode bits
    assert lib.xsg_count_chunks(h, M, cp, npn, n, tp) == xsg.EINVAL                  # newlines without XSG_WITH_NEWLINES
    assert lib.xsg_count_chunks(h, M, cp, None, n + 5, None) == xsg.OK               # room to spare, no totals
    a = Async(gs, n)
    for bad in (dict(d_counts=0), dict(d_counters=0), dict(d_status=0), dict(cap=n - 1), dict(mode=xsg.LINES), dict(mode=M | 0x400)):
        kw = dict(mode=M, stream=a.stream.cuda_stream, d_counts=a.counts.data_ptr(), d_newlines=0, cap=n,
                  d_counters=a.counters.data_ptr(), d_status=a.status.data_ptr())
        kw.update(bad)
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.count_chunks_async(**kw)
        assert e.value.code == xsg.EINVAL, bad
    gs.ctx.set_pattern(NEEDLE, xsg.FLAG_INVERT)
    assert lib.xsg_count_chunks(h, M, cp, None, n, tp) == xsg.ENOTSUP                # match count under XSG_FLAG_INVERT
    with pytest.raises(xsg.XsgError) as e:
        a.run(M, False)
    assert e.value.code == xsg.ENOTSUP


def test_a_binding_of_no_chunks(gs):
    import torch
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    gs.ctx.set_pattern(NEEDLE, 0)
    bind_raw(gs, t, 256, xsg.make_chunks([], []))
    counts, nls, totals = gs.shard.count_chunks(M | NL)
    assert counts.size == 0 and nls.size == 0
    assert totals.tolist() == gs.shard.count(M | NL).tolist() == [0, 0, 0, 0]


# ---- call order --------------------------------------------------------------------------------------------------------------
def test_behind_a_list_search_and_across_rebinds(gs, oracle, six, base_text):
    blocks = bind_six(gs, six)
    gs.ctx.set_pattern(NEEDLE, 0)
    gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS)  # leaves the tile counts dirty
    gs.shard.search_u64(xsg.LINE_INDICES)
    check_literal(gs, oracle, blocks, NEEDLE, "behind a list search")
    small = [b[:TILE + 5].copy() for b in blocks[:2]]  # a smaller table
    gs.bind(small)
    check_literal(gs, oracle, small, NEEDLE, "smaller table")
    rng = np.random.default_rng(6300)
    large = cut(base_text, rng, [3, 1, 9, 2, 1, 1, 30, 4, 2])  # a larger one
    put(large[2], b"colour", 100, 8 * TILE + 50)
    put(large[6], b"color", 5 * TILE - 2, large[6].size - 6)
    gs.bind(large)
    gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS)
    check_literal(gs, oracle, large, NEEDLE, "larger table")
    gs.ctx.set_pattern(b"colou?r", xsg.FLAG_REGEX)  # the list fallback on the same binding, then scan + finish again
    wm, wl = regex_want(oracle, large, b"colou?r")
    assert sum(wl) >= 3
    check(gs, L, wl, chunk_newlines(large), "fallback behind a rebind")
    check_literal(gs, oracle, large, NEEDLE, "again")
