"""XSG_FLAG_CONTEXT on the GPU: the three line-list tags and xsg_result_context_edges, element by element against
tests/context_model.py (the plain oracle results plus interval arithmetic over the line starts), for every pattern kind, on
bindings with awkward chunks; what ignores the bits; call orders and routes; the refusals; the file pipeline with its seam
stitcher, the host-searcher seam, the C++ surface and xsgrep -A/-B/-C.

Without the feature every case fails at set_pattern ("unknown pattern flags")."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import anchor_oracle
import context_model
import corpus
import invert_model
import xsg
from gpu_util import GpuSearch, oracle_all_modes, oracle_regex_all_modes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TILE = 16384
KEYS = ("line_byte_offsets", "line_indices", "lines", "lines_offsets")
PAIRS = [(1, 0), (0, 1), (2, 3), (4095, 4095)]
X = xsg.FLAG_EXACT_TAIL
RX = xsg.FLAG_REGEX

# one pattern per kind: a dense 1-byte literal, a bordered one, a long-window one, a class sequence, an expression with a
# selective start (the prefilter route's kind), a line-walking one, a (?m) anchored one, ignore-case
KINDS = [(b"e", 0), (b"e", X), (b"that", 0), (b"that", X), (b"Sherlock", 0), (b"Sherlock", X), (b"She[r ]lock", RX),
         (b"colou?r", RX), (b"\\w+ing", RX), (b"(?m)^She", RX), (b"(?m)locked$", RX), (b"sHERLOCK", xsg.FLAG_IGNORE_CASE),
         (b"THAT", xsg.FLAG_IGNORE_CASE | X)]

TALLY = {"cases": 0, "widened": 0}


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


def text_blocks(seed, n=3, size=50_000):
    out = []
    for i in range(n):
        needle = (b"Sherlock", b"colour", b"locking", b"color")[i % 4]
        out.append(corpus.text_block(seed, i, size + 977 * i, needle=needle, needle_rate=2e-2))
    return out


def awkward_blocks():
    """the awkward chunks of the invert suite: empty, one byte, "\\n", 5 000 bare newlines (thousands of starts in one
    tile), an unterminated last line, a line longer than two tiles (select across tiles that hold no newline), starts at
    the last byte of a tile and at the first of the next, a chunk that ends exactly on a tile"""
    long_line = _u8(b"Sherlock " + b"x" * (2 * TILE + 100) + b" the end\nshort that\n\nlast line without newline")
    edge = _u8(b"y" * (TILE - 2) + b"\n" + b"\n" + b"\nthat line starts a tile\n" + b"e" * 40 + b"\n")  # starts at TILE - 1 and TILE
    exact_tile = corpus.text_block(5, 9, 2 * TILE)
    bare = _u8(b"\n" * 5000)
    bare[[0, 2499, 4999]] = ord("e")  # (three lines of it hold a needle; one byte each, so the newline count stays)
    return [corpus.text_block(5, 0, 40_000, needle_rate=2e-2), _u8(b""), _u8(b"x"), _u8(b"\n"), _u8(b"\n" * 5000), bare,
            corpus.text_block(5, 1, 33_333, needle_rate=2e-2)[:-1], long_line, edge, exact_tile, _u8(b"e"), _u8(b"aa\naa")]


def plain_model(oracle, blocks, pat, flags, go=None, lb=None):
    """the oracle's dict without the context bits (and, under XSG_FLAG_INVERT, its complement)"""
    icase = bool(flags & xsg.FLAG_IGNORE_CASE)
    if not flags & RX:
        want = oracle_all_modes(oracle, blocks, pat, exact=bool(flags & X), global_offsets=go, line_bases=lb, ignore_case=icase)
    elif pat.startswith(b"(?m)"):
        want = anchor_oracle.all_modes(blocks, pat, icase, global_offsets=go, line_bases=lb)
    else:
        want, with_lines = oracle_regex_all_modes(oracle, blocks, pat, icase, global_offsets=go, line_bases=lb)
        assert with_lines
    if flags & xsg.FLAG_INVERT:
        want = invert_model.invert_all_modes(want, blocks, go, lb)
    return want


def context_modes(gs, pat, flags, before, after, edges=True):
    """the three line lists of the bound shard under flag_context(before, after) -> dict like the model's (+ "edges")"""
    gs.ctx.set_pattern(pat, flags | xsg.flag_context(before, after))
    s = gs.shard
    out = {"line_byte_offsets": s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()}
    on = before or after
    if on and edges:
        out["edges"] = [tuple(int(x) for x in e) for e in s.context_edges()]
    out["line_indices"] = s.search_u64(xsg.LINE_INDICES).tolist()
    if on and edges:
        assert [tuple(int(x) for x in e) for e in s.context_edges()] == out["edges"], "edges after XSG_LINE_INDICES differ"
    ls, lo = s.search_lines()
    out["lines"], out["lines_offsets"] = ls, lo.tolist()
    if on and edges:
        assert [tuple(int(x) for x in e) for e in s.context_edges()] == out["edges"], "edges after XSG_LINES differ"
    return out


def compare(got, want, ctx, keys=KEYS):
    for k in keys:
        g, w = got[k], want[k]
        if g == w:
            continue
        n = min(len(g), len(w))
        first = next((i for i in range(n) if g[i] != w[i]), n)
        pytest.fail(f"{ctx}: {k}: {len(g)} entries, want {len(w)}; first difference at [{first}]: "
                    f"got {g[first] if first < len(g) else None!r} want {w[first] if first < len(w) else None!r}")


def check(gs, oracle, blocks, pat, flags, before, after, go=None, lb=None, ctx="", plain=None):
    plain = plain if plain is not None else plain_model(oracle, blocks, pat, flags, go, lb)
    want = context_model.context_all_modes(plain, blocks, before, after, go, lb)
    got = context_modes(gs, pat, flags, before, after)
    where = f"{ctx} pattern={pat!r} flags={flags:#x} (B, A)=({before}, {after})"
    compare(got, want, where)
    if before or after:
        want_edges = context_model.edges(plain, blocks, before, after, go)
        assert got["edges"] == want_edges, (where, [(i, g, w) for i, (g, w) in enumerate(zip(got["edges"], want_edges)) if g != w][:3])
    TALLY["cases"] += 1
    TALLY["widened"] += len(want["line_byte_offsets"]) > len(plain["line_byte_offsets"])
    return plain, want


def test_known_answers(gs, oracle):
    text = b"".join(b"l%d\n" % i for i in range(10)).replace(b"l5", b"that")
    blocks = [_u8(text)]
    gs.bind(blocks)
    for (before, after), idx in (((1, 2), [4, 5, 6, 7]), ((0, 0), [5]), ((4095, 0), [0, 1, 2, 3, 4, 5]), ((0, 4095), [5, 6, 7, 8, 9])):
        _, want = check(gs, oracle, blocks, b"that", X, before, after, ctx="known")
        assert want["line_indices"] == idx
    gs.ctx.set_pattern(b"that", X | xsg.flag_context(1, 2))
    assert gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == [12, 15, 20, 23]
    assert [tuple(int(x) for x in e) for e in gs.shard.context_edges()] == [(10, 4, 7, 0, 0)]
    assert gs.shard.search_lines()[0] == [b"l4", b"that", b"l6", b"l7"]


def test_every_pattern_kind_on_text(gs, oracle):
    blocks = text_blocks(31)
    gs.bind(blocks)
    for pat, flags in KINDS:
        plain = plain_model(oracle, blocks, pat, flags)
        assert plain["line_byte_offsets"], pat
        for before, after in PAIRS:
            check(gs, oracle, blocks, pat, flags, before, after, ctx="text", plain=plain)
        got = context_modes(gs, pat, flags, 0, 0)  # (0, 0) is the plain search
        compare(got, plain, f"(0, 0) pattern={pat!r}")


def test_the_forced_prefilter_and_factor_routes(gs, oracle, monkeypatch):
    blocks = text_blocks(32)
    gs.bind(blocks)
    for pre, fac in (("1", "1"), ("0", "0")):
        monkeypatch.setenv("XSG_RX_PRE", pre)
        monkeypatch.setenv("XSG_RX_FAC", fac)
        for expr in (b"colou?r", b"lock(ed|s)?", b"\\w+ing", b"(?m)^Sher.*street$"):
            check(gs, oracle, blocks, expr, RX, 2, 3, ctx=f"pre={pre} fac={fac}")


def test_awkward_chunks(gs, oracle):
    blocks = awkward_blocks()
    gs.bind(blocks)
    for pat, flags in ((b"that", 0), (b"e", 0), (b"e", X), (b"Sherlock", X), (b"x", 0), (b"She[r ]lock", RX), (b"(?m)^that", RX)):
        plain = plain_model(oracle, blocks, pat, flags)
        for before, after in PAIRS[:3] if pat != b"e" else PAIRS:
            check(gs, oracle, blocks, pat, flags, before, after, ctx="awkward", plain=plain)


def test_awkward_chunks_with_offsets_and_line_bases(gs, oracle):
    blocks = awkward_blocks()
    n = len(blocks)
    go = [10_000_000 * (n - i) + 13 for i in range(n)]  # disjoint, descending, not aligned
    lb = [1000 * i + 7 for i in range(n)]
    gs.bind(blocks, go, lb)
    for pat, flags in ((b"that", 0), (b"e", X), (b"She[r ]lock", RX), (b"(?m)^e+$", RX)):
        plain = plain_model(oracle, blocks, pat, flags, go, lb)
        for before, after in ((2, 3), (4095, 4095)) if pat == b"that" else ((2, 3),):
            check(gs, oracle, blocks, pat, flags, before, after, go, lb, ctx="awkward go lb", plain=plain)
    gs.bind(blocks, go, None)
    gs.shard.set_line_base(5000)  # the shard's base under XSG_LINE_BASE_AUTO
    want = context_model.context_all_modes(oracle_all_modes(oracle, blocks, b"that", global_offsets=go), blocks, 2, 1, go)
    gs.ctx.set_pattern(b"that", xsg.flag_context(2, 1))
    assert gs.shard.search_u64(xsg.LINE_INDICES).tolist() == [5000 + x for x in want["line_indices"]]
    nl = C.c_uint64(0)
    assert gs.shard._lib.xsg_result_newlines(gs.shard.h, C.byref(nl)) == xsg.OK and nl.value == sum(int((b == 10).sum()) for b in blocks)
    gs.shard.set_line_base(0)


def test_single_chunks_at_tile_edges(gs, oracle):
    for n in (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):
        for fill in (b"e\nab\n\n", b"\nab e\nab", b"abe\n\n\n", b"xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxe\n"):
            blocks = [_u8((fill * (n // len(fill) + 1))[:n])]
            gs.bind(blocks)
            check(gs, oracle, blocks, b"e", 0, 1, 1, ctx=f"edge n={n} fill={fill!r}")
            check(gs, oracle, blocks, b"ab", X, 2, 0, ctx=f"edge n={n} fill={fill!r}")


def test_first_and_last_lines_and_the_spacing_of_matches(gs, oracle):
    """matches in the first and the last line of a chunk (clipping; the edges say what was cut), and matches exactly
    A + B, A + B + 1 and A + B + 2 lines apart: merge, touch, gap.  Rows are 40 bytes, so a tile holds ~400 of them."""
    def rows(n, hits):
        return _u8(b"".join((b"that" if i in hits else b"row ") + b" %034d\n" % i for i in range(n)))
    for before, after in PAIRS[:3] + [(3, 3)]:
        d = before + after
        hits = {0, 1999}
        at = 100
        for gap in (d, d + 1, d + 2, d, d + 2, d + 1):
            hits.update((at, at + max(gap, 1)))
            at += 500  # (pairs in different tiles, and one pair around the end of a tile)
        hits.update((TILE // 40 - 1, TILE // 40 - 1 + max(d + 1, 1)))
        blocks = [rows(2000, hits), rows(1, {0}), rows(3, {2}), rows(900, {0, 899})[:-1]]
        gs.bind(blocks)
        plain, want = check(gs, oracle, blocks, b"that", X, before, after, ctx="spacing")
        e = context_model.edges(plain, blocks, before, after)
        assert e[0][3:] == (before, after) and e[1][3:] == (before, after) and e[2][3:] == (max(0, before - 2), after)
    every = [rows(1500, set(range(1500))), rows(700, set(range(700)))[:-1]]  # every line matches
    gs.bind(every)
    for before, after in PAIRS:
        check(gs, oracle, every, b"that", 0, before, after, ctx="every line")


def test_combined_with_invert(gs, oracle):
    blocks = text_blocks(33)
    gs.bind(blocks)
    for pat, flags in ((b"e", 0), (b"that", X), (b"Sherlock", 0), (b"She[r ]lock", RX), (b"\\w+ing", RX), (b"(?m)^She", RX)):
        for before, after in ((1, 0), (2, 3)):
            check(gs, oracle, blocks, pat, flags | xsg.FLAG_INVERT, before, after, ctx="invert")
    awkward = awkward_blocks()
    gs.bind(awkward)
    for pat, flags in ((b"e", X), (b"that", 0)):
        check(gs, oracle, awkward, pat, flags | xsg.FLAG_INVERT, 2, 3, ctx="invert awkward")


def counts_everywhere(gs, mode):
    """a count mode through the four count entry points -> list of counter lists"""
    import torch
    s = gs.shard
    out = [[int(x) for x in s.count(mode)]]
    s.count_begin(mode)
    out.append([int(x) for x in s.count_end()])
    buf = torch.full((xsg.NUM_COUNTERS + 1,), 77, dtype=torch.int64, device="cuda:0")
    s.count_async(mode, 0, buf.data_ptr())
    torch.cuda.synchronize()
    out.append(buf.cpu().tolist()[:xsg.NUM_COUNTERS])
    st = torch.cuda.Stream()
    s.count_async_status(mode, st.cuda_stream, buf.data_ptr(), buf.data_ptr() + 8 * xsg.NUM_COUNTERS)
    st.synchronize()
    c = buf.cpu().tolist()
    assert c[xsg.NUM_COUNTERS] == xsg.STATUS_OK
    out.append(c[:xsg.NUM_COUNTERS])
    return out


def test_every_other_tag_ignores_the_bits(gs, oracle):
    blocks = text_blocks(34)
    gs.bind(blocks)
    for pat, flags in ((b"e", 0), (b"Sherlock", X), (b"She[r ]lock", RX), (b"colou?r", RX)):
        plain = plain_model(oracle, blocks, pat, flags)
        res = []
        for bits in (0, xsg.flag_context(2, 3)):
            gs.ctx.set_pattern(pat, flags | bits)
            r = [counts_everywhere(gs, m) for m in (xsg.COUNT_MATCHES, xsg.COUNT_LINES, xsg.COUNT_LINES | xsg.WITH_NEWLINES)]
            r.append(gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist())
            ms, mo = gs.shard.search_matches()
            r.append((ms, mo.tolist()))
            res.append(r)
        assert res[0] == res[1], pat
        assert res[1][3] == plain["match_byte_offsets"] and all(c[xsg.CTR_MATCHES] == plain["count_matches"] for c in res[1][0])
        assert all(c[xsg.CTR_LINES] == plain["count_lines"] for c in res[1][1])


STATE = ("epoch", "cnt_clean", "sum_clean", "last_valid", "nl_cached", "table_pending", "fast_result", "fast_dense")


def shard_state(shard):
    """the host-side bookkeeping of a shard (xsg_test_shard_state, XSG_TEST_HOOKS=1: as tests/test_gpu_call_sequences.py)"""
    fn = shard._lib.xsg_test_shard_state
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]
    out = (C.c_uint64 * len(STATE))()
    assert fn(shard.h, out, len(STATE)) == xsg.OK, shard._lib.xsg_last_error()
    return dict(zip(STATE, [int(x) for x in out]))


def test_call_order_on_one_binding(gs, oracle):
    """context, plain, context, rebind, context: the plain call in between is exact and still on the one-sync route"""
    blocks = text_blocks(35)
    gs.bind(blocks)
    plain = plain_model(oracle, blocks, b"Sherlock", 0)
    first = check(gs, oracle, blocks, b"Sherlock", 0, 2, 3, ctx="first", plain=plain)[1]
    assert "k_context_tile" in gs.shard.scan_kernel_name(xsg.LINES)
    assert "k_context_tile" not in gs.shard.scan_kernel_name(xsg.MATCH_BYTE_OFFSETS)
    gs.ctx.set_pattern(b"Sherlock", xsg.flag_context(2, 3))
    gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS)
    assert not shard_state(gs.shard)["fast_result"], "a context list was served by the one-sync route"
    gs.ctx.set_pattern(b"Sherlock", 0)
    assert "k_context_tile" not in gs.shard.scan_kernel_name(xsg.LINES)
    assert gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == plain["line_byte_offsets"]
    st = shard_state(gs.shard)
    assert st["fast_result"] and not st["fast_dense"], ("the plain call left the one-sync route", st)
    with pytest.raises(xsg.XsgError) as e:
        gs.shard.context_edges()
    assert e.value.code == xsg.ESTATE
    got = gs.all_modes(b"Sherlock", 0)
    for k, v in plain.items():
        assert got[k] == v, k
    compare(context_modes(gs, b"Sherlock", 0, 2, 3), first, "context again")
    other = text_blocks(36, n=2, size=70_000)
    gs.bind(other)  # a rebind: nothing of the old binding's ranks may survive
    check(gs, oracle, other, b"Sherlock", 0, 2, 3, ctx="rebound")
    check(gs, oracle, other, b"colou?r", RX, 1, 0, ctx="rebound")


def _refused(fn, *args):
    with pytest.raises(xsg.XsgError) as e:
        fn(*args)
    return e.value


def test_refusals(gs, oracle):
    blocks = text_blocks(37, n=1)
    gs.bind(blocks)
    s = gs.shard
    for pat, flags in ((b"a\nb", 0), (b"\n", X), (b"She\\s+lock", RX), (b"a[\\n ]b", RX), (b"a\\nb", RX)):
        for bits in (xsg.flag_context(1, 0), xsg.flag_context(0, 1), xsg.flag_context(0, 1) | xsg.FLAG_INVERT):
            gs.ctx.set_pattern(b"that", 0)
            e = _refused(gs.ctx.set_pattern, pat, flags | bits)
            assert e.code == xsg.ENOTSUP and "'\\n'" in str(e), pat
            assert _refused(s.count, xsg.COUNT_LINES).code == xsg.ESTATE  # the context holds no pattern
        gs.ctx.set_pattern(pat, flags)  # (without context the match tags serve it)
    for bad in (0x10, 0x20, 0x40, 0x80):  # bits 4-7 stay unknown flags
        assert _refused(gs.ctx.set_pattern, b"that", xsg.flag_context(1, 1) | bad).code == xsg.EINVAL
    gs.ctx.set_pattern(b"that", xsg.flag_context(1, 1))
    assert _refused(s.context_edges).code == xsg.ESTATE  # nothing searched yet
    s.search_u64(xsg.MATCH_BYTE_OFFSETS)
    assert _refused(s.context_edges).code == xsg.ESTATE  # a match tag ignores the bits
    s.search_u64(xsg.LINE_BYTE_OFFSETS)
    assert len(s.context_edges()) == 1
    out = np.zeros(1, dtype=xsg.CONTEXT_EDGE_DTYPE)
    assert s._lib.xsg_result_context_edges(s.h, out.ctypes.data, 0) == xsg.EINVAL
    gs.ctx.set_pattern(b"that", 0)
    s.search_u64(xsg.LINE_BYTE_OFFSETS)
    assert _refused(s.context_edges).code == xsg.ESTATE  # a plain search
    dirty = [np.concatenate([blocks[0], _u8("grüße the\n".encode())])]  # non-ASCII data under '.': still refused
    gs.bind(dirty)
    gs.ctx.set_pattern(b"t.e", RX | xsg.flag_context(1, 1))
    for mode in (xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES):
        assert _refused(s.search_u64, mode).code == xsg.ENOTSUP
    gs.bind(blocks)
    check(gs, oracle, blocks, b"t.e", RX, 1, 1, ctx="clean again")


CHUNK = 16 << 10


@pytest.fixture(scope="module")
def textfile(tmp_path_factory):
    d = tmp_path_factory.mktemp("xscontext")
    data = np.concatenate(text_blocks(38, n=3, size=120_000))
    data = np.concatenate([_u8(b"Sherlock opens the file that\n"), data[:-1], _u8(b" SheSherlock")])  # first line; a tail decoy, no final newline
    p = d / "t.txt"
    data.tofile(p)
    plan = xsg.plan_chunks(str(p), CHUNK)
    chunks = [data[int(c["original_offset"]):int(c["original_offset"] + c["original_size"])] for c in plan]
    assert len(chunks) > 10
    meta, packed = d / "t.xslz4.meta", d / "t.xslz4"
    xsg.meta_write(str(p), str(meta), str(packed), xsg.COMPRESSION_LZ4, CHUNK, 500)
    return {"path": str(p), "chunks": chunks, "lz4": (str(packed), str(meta))}


TAGS = {"line_byte_offsets": xsg.LINE_BYTE_OFFSETS, "line_indices": xsg.LINE_INDICES, "lines": xsg.LINES}


def _job(pat, path, mode, flags, threads=1, meta=None, live=False, chunk=CHUNK):
    j = xsg.Job(pat, path, mode, meta_path=meta, num_threads=threads, num_max_readers=threads, chunk_bytes=chunk, flags=flags)
    try:
        r = list(j) if live else j.result()
        if live:
            j.join()
        return list(r) if mode == xsg.LINES else [int(x) for x in r]
    finally:
        j.close()


def test_jobs_equal_whole_file_context(textfile, oracle):
    path, chunks = textfile["path"], textfile["chunks"]
    for pat, flags in ((b"Sherlock", 0), (b"that", X), (b"colou?r", RX), (b"the", xsg.FLAG_INVERT)):
        plain = plain_model(oracle, chunks, pat, flags)
        for before, after in ((1, 0), (0, 1), (2, 3), (40, 40)):
            assert not context_model.job_refuses(plain, chunks, before, after)
            want = context_model.whole_file(plain, chunks, before, after)
            for threads in (1, 2, 3) if (before, after) == (2, 3) else (2,):
                for key, mode in TAGS.items():
                    got = _job(pat, path, mode, flags | xsg.flag_context(before, after), threads)
                    compare({**want, key: got}, want, f"job {key} threads={threads} pattern={pat!r} ({before}, {after})", keys=(key,))
        TALLY["cases"] += 1
    plain = plain_model(oracle, chunks, b"Sherlock", 0)
    want = context_model.whole_file(plain, chunks, 2, 3)
    assert _job(b"Sherlock", path, xsg.LINES, xsg.flag_context(2, 3), 2, live=True) == want["lines"]  # a live reader
    packed, meta = textfile["lz4"]
    for key, mode in TAGS.items():  # an LZ4 metafile job: the same chunks, line bases from the metafile
        assert _job(b"Sherlock", packed, mode, xsg.flag_context(2, 3), 2, meta=meta) == want[key], key
    # a chunk range is searched on its own: context is clipped at its ends
    sub = chunks[3:7]
    sub_plain = oracle_all_modes(oracle, sub, b"Sherlock")
    clipped = context_model.whole_file(sub_plain, sub, 150, 150)
    assert not context_model.job_refuses(sub_plain, sub, 150, 150)
    assert clipped["line_indices"][0] == 0 and len(clipped["lines"]) < len(context_model.whole_file(plain, chunks, 150, 150)["lines"])
    j = xsg.Job(b"Sherlock", path, xsg.LINES, num_threads=2, chunk_bytes=CHUNK, flags=xsg.flag_context(150, 150), chunk_range=(3, 7))
    assert j.result() == clipped["lines"]
    j.close()
    j = xsg.Job(b"Sherlock", path, xsg.LINES, num_threads=2, chunk_bytes=CHUNK, flags=xsg.flag_context(4095, 4095), chunk_range=(3, 7))
    assert _refused(j.join).code == xsg.ENOTSUP  # (4095 lines reach across whole chunks of this size)
    j.close()
    # the counts and the match tags of a job ignore the bits
    for mode, key in ((xsg.COUNT_LINES, "count_lines"), (xsg.COUNT_MATCHES, "count_matches")):
        j = xsg.Job(b"Sherlock", path, mode, chunk_bytes=CHUNK, flags=xsg.flag_context(2, 3))
        assert j.result() == plain[key]
        j.close()
    assert _job(b"Sherlock", path, xsg.MATCH_BYTE_OFFSETS, xsg.flag_context(2, 3)) == plain["match_byte_offsets"]
    e = _refused(lambda: xsg.Job(b"a\nb", path, xsg.LINES, flags=xsg.flag_context(1, 0)))
    assert e.code == xsg.ENOTSUP


def test_job_refuses_context_across_a_whole_chunk(tmp_path, oracle):
    """a file whose middle chunks hold one line each: B = 2 from the chunk behind them reaches across one -- refused at
    join, never approximated; (0, 0) and (1, 1) are served"""
    small = 4096
    text = b"head row\n" * 456 + b"".join(b"%d " % i + b"x" * 5000 + b"\n" for i in range(3)) + b"that row\n" + b"tail row\n" * 600
    p = tmp_path / "one_line_chunks.txt"
    p.write_bytes(text)
    plan = xsg.plan_chunks(str(p), small)
    chunks = [_u8(text[int(c["original_offset"]):int(c["original_offset"] + c["original_size"])]) for c in plan]
    assert [len(invert_model.lines(c)) for c in chunks[1:4]] == [1, 1, 1]
    plain = oracle_all_modes(oracle, chunks, b"that", exact=True)
    assert context_model.job_refuses(plain, chunks, 2, 0) and not context_model.job_refuses(plain, chunks, 1, 1)
    for mode in TAGS.values():
        j = xsg.Job(b"that", str(p), mode, num_threads=2, chunk_bytes=small, flags=X | xsg.flag_context(2, 0))
        e = _refused(j.join)
        assert e.code == xsg.ENOTSUP and "chunk_bytes" in str(e), str(e)
        j.close()
    for before, after in ((0, 0), (1, 1)):
        want = context_model.whole_file(plain, chunks, before, after)
        for key, mode in TAGS.items():
            assert _job(b"that", str(p), mode, X | xsg.flag_context(before, after), 2, chunk=small) == want[key], (key, before, after)


def test_host_searcher_seam_is_chunk_local(textfile, oracle):
    """xsg_host_*: what the Gpu*Searcher functors call with their `flags`; context is clipped at the chunk handed in"""
    chunks = textfile["chunks"]
    lib = xsg.load()
    hs = C.c_void_p()
    assert lib.xsg_host_searcher_create(0, b"Sherlock", 8, xsg.flag_context(3, 2), 2, C.byref(hs)) == xsg.OK
    try:
        for i, b in enumerate(chunks[:3] + [chunks[-1], _u8(b"")]):
            plain = oracle_all_modes(oracle, [b], b"Sherlock")
            want = context_model.context_all_modes(plain, [b], 3, 2)
            data = np.ascontiguousarray(b)
            n = C.c_uint64(0)
            assert lib.xsg_host_count(hs, data.ctypes.data, data.size, 1, C.byref(n)) == xsg.OK and n.value == plain["count_lines"]
            for mode, key in ((xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices"), (xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets")):
                out = C.c_void_p()
                assert lib.xsg_host_offsets(hs, mode, data.ctypes.data, data.size, C.byref(out), C.byref(n)) == xsg.OK
                got = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
                lib.xsg_free(out)
                assert got == want[key], (i, key)
            lens, raw, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
            assert lib.xsg_host_lines(hs, data.ctypes.data, data.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == xsg.OK
            ll = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
            blob = C.string_at(raw, nb.value)
            lib.xsg_free(lens)
            lib.xsg_free(raw)
            ends = np.cumsum(ll).tolist()
            assert [blob[e - k:e] for e, k in zip(ends, ll)] == want["lines"], i
    finally:
        lib.xsg_host_searcher_destroy(hs)


def test_cpp_extern_search(textfile, oracle):
    """xs::extern_search with XS_CONTEXT_BEFORE / XS_CONTEXT_AFTER"""
    cli = ROOT / "tests" / "cpp" / "build" / "extern_search_cli"
    if not cli.exists():
        pytest.fail(f"{cli} not built (make -C tests/cpp)")
    path, chunks = textfile["path"], textfile["chunks"]
    plain = oracle_all_modes(oracle, chunks, b"Sherlock")
    want = context_model.whole_file(plain, chunks, 2, 1)
    env = dict(os.environ, XS_CHUNK_BYTES=str(CHUNK), XS_CONTEXT_BEFORE="2", XS_CONTEXT_AFTER="1")

    def run(tag, how="join", **more):
        return subprocess.run([str(cli), tag, how, "Sherlock", path, "-", "2"], capture_output=True, env=dict(env, **more), timeout=300)
    r = run("lines")
    assert r.returncode == 0 and r.stdout.split(b"\n")[:-1] == want["lines"], r.stderr.decode()
    r = run("line_indices", "live")
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == want["line_indices"], r.stderr.decode()
    r = run("line_byte_offsets")
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == want["line_byte_offsets"], r.stderr.decode()
    r = run("count_lines")  # the other tags ignore the variables
    assert r.returncode == 0 and int(r.stdout) == plain["count_lines"], r.stderr.decode()
    r = run("match_byte_offsets")
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == plain["match_byte_offsets"], r.stderr.decode()
    for more in ({"XS_CONTEXT_BEFORE": "4096"}, {"XS_CONTEXT_AFTER": "4096"}):
        r = run("lines", **more)
        assert r.returncode != 0 and b"4095" in r.stderr, more
    r = run("lines", XS_DEVICES="0,0")  # several devices: the seams between their ranges are not stitched
    assert r.returncode != 0 and b"one device" in r.stderr.lower().replace(b"\n", b" "), r.stderr.decode()


def test_xsgrep_context(textfile, oracle, tmp_path):
    """xsgrep -A / -B / -C against the model (exact and default semantics agree here: the file ends in rows without a needle)"""
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    data = np.concatenate(text_blocks(39, n=3, size=100_000) + [_u8(b"a plain closing row of words, none of which is searched for below\n" * 2)])
    p = tmp_path / "g.txt"
    data.tofile(p)
    env = dict(os.environ, XS_CHUNK_BYTES=str(CHUNK), LC_ALL="C")
    plan = xsg.plan_chunks(str(p), CHUNK)
    chunks = [data[int(c["original_offset"]):int(c["original_offset"] + c["original_size"])] for c in plan]
    for pat, flags, args in ((b"Sherlock", 0, ["-F", "Sherlock"]), (b"sherlock", xsg.FLAG_IGNORE_CASE, ["-i", "-F", "sherlock"]),
                             (b"colou?r", RX, ["-E", "colou?r"]), (b"the", xsg.FLAG_INVERT, ["-v", "-F", "the"])):
        plain = plain_model(oracle, chunks, pat, flags)
        sets = ((["-A", "2"], (0, 2)), (["-B", "3"], (3, 0)), (["-C", "1"], (1, 1)), (["-C", "9", "-A", "0"], (9, 0)))
        for cargs, (before, after) in sets if pat == b"Sherlock" else sets[2:3]:
            want = context_model.whole_file(plain, chunks, before, after)["lines"]
            got = subprocess.run([str(exe), "-j", "2", *cargs, *args, str(p)], capture_output=True, env=env, timeout=120)
            assert got.returncode == 0, got.stderr.decode()
            assert got.stdout.split(b"\n")[:-1] == want and want, (args, cargs)
        for extra, key in ((["-c"], "count_lines"),):  # with -c the numbers change nothing
            got = subprocess.run([str(exe), *extra, "-C", "3", *args, str(p)], capture_output=True, env=env, timeout=120)
            assert got.returncode == 0 and int(got.stdout) == plain[key], (args, got.stderr.decode())
    a = subprocess.run([str(exe), "-o", "-C", "3", "Sherlock", str(p)], capture_output=True, env=env, timeout=120)
    b = subprocess.run([str(exe), "-o", "Sherlock", str(p)], capture_output=True, env=env, timeout=120)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stdout
    with open(p, "rb") as f:
        r = subprocess.run([str(exe), "-C", "3", "Sherlock", "-"], stdin=f, capture_output=True, env=env, timeout=120)
    assert r.returncode == 2 and b"stdin" in r.stderr


def test_zz_enough_cases_widen_the_list():
    """test honesty: in most of the generated cases above context adds lines to the plain result"""
    assert TALLY["cases"] >= 120, TALLY
    assert 2 * TALLY["widened"] >= TALLY["cases"], TALLY
