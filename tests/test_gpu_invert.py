"""XSG_FLAG_INVERT on the GPU: the four line tags and every count entry point, element by element against
tests/invert_model.py (the plain oracle results plus one set difference), for every pattern kind, on bindings with awkward
chunks; the refusals; the file pipeline, the host-searcher seam, the C++ surface and xsgrep -v.

Without the feature every case fails at set_pattern ("unknown pattern flags")."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import anchor_oracle
import corpus
import invert_model
import xsg
from gpu_util import GpuSearch, oracle_all_modes, oracle_regex_all_modes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TILE = 16384
KEYS = ("count_lines", "line_byte_offsets", "line_indices", "lines", "lines_offsets")

# kMask1 (1-3 bytes), kOne (4, `that` has a border), kMask2 (5-7), kTwo (8), kLong (> 8)
LITERALS = [b"e", b" ", b"aa", b"the", b"that", b"lock", b"Holmes", b"Sherlock", b"detective street"]
REGEXES = [b"She[r ]lock", b"colou?r", b"\\w+ing", b"lock(ed|s)?"]
ANCHORED = [b"(?m)^She", b"(?m)locked$", b"(?m)^[a-z]+$", b"(?m)^Sher.*street$"]

TALLY = {"cases": 0, "both": 0}


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


def text_blocks(seed, n=3, size=50_000):
    """text with every needle of this file in some lines and not in others"""
    out = []
    for i in range(n):
        needle = (b"Sherlock", b"colour", b"locking", b"color")[i % 4]
        out.append(corpus.text_block(seed, i, size + 977 * i, needle=needle, needle_rate=2e-2))
    return out


def awkward_blocks():
    """empty, one byte, unterminated, all newlines, one line longer than a tile, line starts at byte 0 and at the last
    byte of a tile, a chunk that ends exactly on a tile"""
    long_line = _u8(b"Sherlock " + b"x" * (2 * TILE + 100) + b" the end\nshort that\n\nlast line without newline")
    edge = _u8(b"y" * (TILE - 2) + b"\n" + b"\n" + b"\nthat line starts a tile\n" + b"e" * 40 + b"\n")  # starts at TILE - 1 and TILE
    exact_tile = corpus.text_block(5, 9, 2 * TILE)
    return [corpus.text_block(5, 0, 40_000, needle_rate=2e-2), _u8(b""), _u8(b"x"), _u8(b"\n"), _u8(b"\n" * 5000),
            corpus.text_block(5, 1, 33_333, needle_rate=2e-2)[:-1], long_line, edge, exact_tile, _u8(b"e"), _u8(b"aa\naa")]


def plain_model(oracle, blocks, pat, flags, go=None, lb=None):
    icase = bool(flags & xsg.FLAG_IGNORE_CASE)
    if not flags & xsg.FLAG_REGEX:
        return oracle_all_modes(oracle, blocks, pat, exact=bool(flags & xsg.FLAG_EXACT_TAIL), global_offsets=go, line_bases=lb,
                                ignore_case=icase)
    if pat.startswith(b"(?m)"):
        return anchor_oracle.all_modes(blocks, pat, icase, global_offsets=go, line_bases=lb)
    want, with_lines = oracle_regex_all_modes(oracle, blocks, pat, icase, global_offsets=go, line_bases=lb)
    assert with_lines
    return want


def counts_everywhere(gs, want_nl):
    """XSG_COUNT_LINES through the four count entry points -> list of (name, lines, newlines, bytes)"""
    import torch
    s = gs.shard
    mode = xsg.COUNT_LINES | (xsg.WITH_NEWLINES if want_nl else 0)
    out = []
    c = s.count(mode)
    out.append(("xsg_count", int(c[xsg.CTR_LINES]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])))
    s.count_begin(mode)
    c = s.count_end()
    out.append(("xsg_count_begin/_end", int(c[xsg.CTR_LINES]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])))
    buf = torch.full((xsg.NUM_COUNTERS + 1,), 77, dtype=torch.int64, device="cuda:0")
    s.count_async(mode, 0, buf.data_ptr())
    torch.cuda.synchronize()
    c = buf.cpu().tolist()
    out.append(("xsg_count_async", c[xsg.CTR_LINES], c[xsg.CTR_NEWLINES], c[xsg.CTR_BYTES]))
    st = torch.cuda.Stream()
    s.count_async_status(mode, st.cuda_stream, buf.data_ptr(), buf.data_ptr() + 8 * xsg.NUM_COUNTERS)
    st.synchronize()
    c = buf.cpu().tolist()
    assert c[xsg.NUM_COUNTERS] == xsg.STATUS_OK
    out.append(("xsg_count_async_status", c[xsg.CTR_LINES], c[xsg.CTR_NEWLINES], c[xsg.CTR_BYTES]))
    return out


def inverted_modes(gs, pat, flags, entry_points=True):
    """every inverted result of the bound shard -> dict like the model's"""
    gs.ctx.set_pattern(pat, flags | xsg.FLAG_INVERT)
    s = gs.shard
    out = {}
    c = s.count(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
    out["count_lines"], out["newlines"], out["bytes"] = int(c[xsg.CTR_LINES]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])
    assert int(c[xsg.CTR_MATCHES]) == 0, "|I| leaked into XSG_CTR_MATCHES"
    if entry_points:
        for name, nlines, nl, nbytes in counts_everywhere(gs, True):
            assert (nlines, nl, nbytes) == (out["count_lines"], out["newlines"], out["bytes"]), (name, pat)
        for name, nlines, nl, nbytes in counts_everywhere(gs, False):
            assert (nlines, nl, nbytes) == (out["count_lines"], 0, out["bytes"]), (name, pat)
    out["line_byte_offsets"] = s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    out["line_indices"] = s.search_u64(xsg.LINE_INDICES).tolist()
    nl = C.c_uint64(0)
    assert s._lib.xsg_result_newlines(s.h, C.byref(nl)) == xsg.OK and nl.value == out["newlines"], "xsg_result_newlines"
    ls, lo = s.search_lines()
    out["lines"], out["lines_offsets"] = ls, lo.tolist()
    vl, vb, vo = s.search_lines_view()
    ends = np.cumsum(vl.astype(np.int64)) if vl.size else np.zeros(0, dtype=np.int64)
    raw = vb.tobytes()
    assert [raw[int(e) - int(n):int(e)] for e, n in zip(ends, vl)] == ls, "xsg_result_lines_view: lines differ"
    assert vo.tolist() == out["lines_offsets"], "xsg_result_lines_view: offsets differ"
    assert s.search_u64_view(xsg.LINE_BYTE_OFFSETS).tolist() == out["line_byte_offsets"], "xsg_result_u64_view"
    return out


def compare(got, want, ctx):
    for k in KEYS + ("newlines", "bytes"):
        g, w = got[k], want[k]
        if g == w:
            continue
        if isinstance(w, list):
            n = min(len(g), len(w))
            first = next((i for i in range(n) if g[i] != w[i]), n)
            pytest.fail(f"{ctx}: {k}: {len(g)} entries, want {len(w)}; first difference at [{first}]: "
                        f"got {g[first] if first < len(g) else None!r} want {w[first] if first < len(w) else None!r}")
        pytest.fail(f"{ctx}: {k}: got {g} want {w}")


def check(gs, oracle, blocks, pat, flags=0, go=None, lb=None, ctx="", entry_points=True):
    plain = plain_model(oracle, blocks, pat, flags, go, lb)
    invert_model.properties(plain, blocks, go)
    want = invert_model.invert_all_modes(plain, blocks, go, lb)
    got = inverted_modes(gs, pat, flags, entry_points)
    compare(got, want, f"{ctx} pattern={pat!r} flags={flags:#x}")
    TALLY["cases"] += 1
    TALLY["both"] += bool(plain["count_lines"]) and bool(want["count_lines"])
    return plain, want


def test_known_answers(gs, oracle):
    for chunk, pat, offs in ((b"a\nb", b"a", [2]), (b"a\n", b"b", [0]), (b"a\n\n", b"a", [2]), (b"ab\ncd\nab", b"ab", [3]),
                             (b"\n\n\n", b"x", [0, 1, 2]), (b"x", b"x", []), (b"x", b"y", [0])):
        blocks = [_u8(chunk)]
        gs.bind(blocks)
        _, want = check(gs, oracle, blocks, pat, xsg.FLAG_EXACT_TAIL, ctx=f"known {chunk!r}")
        assert want["line_byte_offsets"] == offs


def test_literals_of_every_kind_both_tail_modes(gs, oracle):
    blocks = text_blocks(21)
    gs.bind(blocks)
    for pat in LITERALS:
        for flags in (0, xsg.FLAG_EXACT_TAIL):
            check(gs, oracle, blocks, pat, flags, ctx="text")
    for pat, flags in ((b"sHERLOCK", xsg.FLAG_IGNORE_CASE), (b"THAT", xsg.FLAG_IGNORE_CASE | xsg.FLAG_EXACT_TAIL), (b"E", xsg.FLAG_IGNORE_CASE)):
        check(gs, oracle, blocks, pat, flags, ctx="text -i")
    for seed in range(4):  # dense overlaps and many newlines; the lossy tail zone covers much of such small chunks
        small = [corpus.small_alphabet(seed * 11 + i, n) for i, n in enumerate((300, 1, 0, 2, 777, TILE + 5))]
        gs.bind(small)
        for pat in (b"a", b"ab", b"aa", b"aba", b"b"):
            for flags in (0, xsg.FLAG_EXACT_TAIL):
                check(gs, oracle, small, pat, flags, ctx=f"small{seed}", entry_points=seed == 0)


def test_regex_routes(gs, oracle, monkeypatch):
    blocks = text_blocks(22)
    gs.bind(blocks)
    for expr in REGEXES:
        check(gs, oracle, blocks, expr, xsg.FLAG_REGEX, ctx="regex")
    check(gs, oracle, blocks, b"she[r ]LOCK", xsg.FLAG_REGEX | xsg.FLAG_IGNORE_CASE, ctx="regex -i")
    for expr in ANCHORED:
        check(gs, oracle, blocks, expr, xsg.FLAG_REGEX, ctx="anchored")
    # the prefilter and factor-mask variants of the automaton route, forced on this small shard, and both switched off
    for pre, fac in (("1", "1"), ("0", "0")):
        monkeypatch.setenv("XSG_RX_PRE", pre)
        monkeypatch.setenv("XSG_RX_FAC", fac)
        for expr in (b"colou?r", b"lock(ed|s)?", b"\\w+ing", b"(?m)^Sher.*street$"):
            check(gs, oracle, blocks, expr, xsg.FLAG_REGEX, ctx=f"regex pre={pre} fac={fac}")


def test_awkward_chunks_with_offsets_and_line_bases(gs, oracle):
    blocks = awkward_blocks()
    n = len(blocks)
    go = [10_000_000 * (n - i) + 13 for i in range(n)]  # disjoint, descending, not aligned
    lb = [1000 * i + 7 for i in range(n)]
    for offsets, bases in ((go, lb), (None, None), (go, None)):
        gs.bind(blocks, offsets, bases)
        for pat, flags in ((b"that", 0), (b"e", 0), (b"e", xsg.FLAG_EXACT_TAIL), (b"aa", 0), (b"Sherlock", xsg.FLAG_EXACT_TAIL),
                           (b"x", 0), (b"She[r ]lock", xsg.FLAG_REGEX), (b"\\w+ing", xsg.FLAG_REGEX),
                           (b"(?m)^that", xsg.FLAG_REGEX), (b"(?m)^e+$", xsg.FLAG_REGEX)):
            check(gs, oracle, blocks, pat, flags, offsets, bases, ctx=f"awkward go={offsets is not None} lb={bases is not None}",
                  entry_points=offsets is None)
    gs.shard.set_line_base(5000)  # the shard's base under XSG_LINE_BASE_AUTO
    gs.bind(blocks, go, None)
    gs.shard.set_line_base(5000)
    plain = oracle_all_modes(oracle, blocks, b"that", global_offsets=go)
    want = invert_model.invert_all_modes(plain, blocks, go)
    gs.ctx.set_pattern(b"that", xsg.FLAG_INVERT)
    assert gs.shard.search_u64(xsg.LINE_INDICES).tolist() == [5000 + x for x in want["line_indices"]]
    gs.shard.set_line_base(0)


def test_single_chunks_at_tile_edges(gs, oracle):
    for n in (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):
        for fill in (b"e\nab\n\n", b"\nab e\nab", b"abe\n\n\n"):
            blocks = [_u8((fill * (n // len(fill) + 1))[:n])]
            gs.bind(blocks)
            check(gs, oracle, blocks, b"e", 0, ctx=f"edge n={n} fill={fill!r}", entry_points=False)
            check(gs, oracle, blocks, b"ab", xsg.FLAG_EXACT_TAIL, ctx=f"edge n={n} fill={fill!r}", entry_points=False)


def test_lines_on_demand_rebind_and_second_search(gs, oracle, monkeypatch):
    blocks = text_blocks(23)
    gs.bind(blocks)
    first = check(gs, oracle, blocks, b"the", 0, ctx="first")[1]
    again = inverted_modes(gs, b"the", 0)  # a second search on the same binding
    compare(again, first, "second search")
    monkeypatch.setenv("XSG_LINES_EAGER", "0")  # the accessors copy on demand
    check(gs, oracle, blocks, b"the", 0, ctx="on demand")
    check(gs, oracle, blocks, b"Sherlock", xsg.FLAG_EXACT_TAIL, ctx="on demand")
    monkeypatch.delenv("XSG_LINES_EAGER")
    other = text_blocks(24, n=2, size=70_000)
    gs.bind(other)  # a rebind: nothing of the old binding's line starts may survive
    check(gs, oracle, other, b"the", 0, ctx="rebound")
    check(gs, oracle, other, b"colou?r", xsg.FLAG_REGEX, ctx="rebound")


def test_the_flag_does_not_stick(gs, oracle):
    blocks = text_blocks(25)
    gs.bind(blocks)
    for pat, flags in ((b"that", 0), (b"Sherlock", xsg.FLAG_EXACT_TAIL), (b"She[r ]lock", xsg.FLAG_REGEX), (b"\\w+ing", xsg.FLAG_REGEX)):
        check(gs, oracle, blocks, pat, flags, ctx="before", entry_points=False)
        want = plain_model(oracle, blocks, pat, flags)
        got = gs.all_modes(pat, flags)  # the same pattern without the flag: every tag, the match tags included
        for k, v in want.items():
            assert got[k] == v, (pat, k)
        assert "invert" not in gs.shard.scan_kernel_name(xsg.LINE_BYTE_OFFSETS)
        gs.ctx.set_pattern(pat, flags | xsg.FLAG_INVERT)
        assert "k_invert_tile" in gs.shard.scan_kernel_name(xsg.LINE_BYTE_OFFSETS)
        assert "k_invert_count_lines" in gs.shard.scan_kernel_name(xsg.COUNT_LINES)


def _refused(fn, *args):
    with pytest.raises(xsg.XsgError) as e:
        fn(*args)
    return e.value


def test_refusals(gs, oracle):
    import torch
    blocks = text_blocks(26, n=1)
    gs.bind(blocks)
    gs.ctx.set_pattern(b"that", xsg.FLAG_INVERT)
    s = gs.shard
    buf = torch.zeros(xsg.NUM_COUNTERS + 1, dtype=torch.int64, device="cuda:0")
    for fn, args in ((s.count, (xsg.COUNT_MATCHES,)), (s.count, (xsg.COUNT_MATCHES | xsg.WITH_NEWLINES,)), (s.count_begin, (xsg.COUNT_MATCHES,)),
                     (s.count_async, (xsg.COUNT_MATCHES, 0, buf.data_ptr())),
                     (s.count_async_status, (xsg.COUNT_MATCHES, 0, buf.data_ptr(), buf.data_ptr() + 32)),
                     (s.search_u64, (xsg.MATCH_BYTE_OFFSETS,))):
        e = _refused(fn, *args)
        assert e.code == xsg.ENOTSUP and "invert" in str(e).lower(), (fn.__name__, args)
    # a pattern that can match '\n': refused by set_pattern, and no pattern is set afterwards
    for pat, flags in ((b"a\nb", 0), (b"\n", xsg.FLAG_EXACT_TAIL), (b"She\\s+lock", xsg.FLAG_REGEX), (b"a[\\n ]b", xsg.FLAG_REGEX),
                       (b"a\\nb", xsg.FLAG_REGEX)):
        gs.ctx.set_pattern(b"that", 0)
        e = _refused(gs.ctx.set_pattern, pat, flags | xsg.FLAG_INVERT)
        assert e.code == xsg.ENOTSUP and "invert" in str(e).lower(), pat
        assert _refused(s.count, xsg.COUNT_LINES).code == xsg.ESTATE
    assert _refused(gs.ctx.set_pattern, b"that", xsg.FLAG_INVERT | 0x10).code == xsg.EINVAL
    # non-ASCII data under an ascii_only expression: still refused, by every route
    dirty = [np.concatenate([blocks[0], _u8("grüße the\n".encode())])]
    gs.bind(dirty)
    for expr in (b"t.e", b"Sher.*k"):
        gs.ctx.set_pattern(expr, xsg.FLAG_REGEX | xsg.FLAG_INVERT)
        assert _refused(s.count, xsg.COUNT_LINES).code == xsg.ENOTSUP
        for mode in (xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES):
            assert _refused(s.search_u64, mode).code == xsg.ENOTSUP
        s.count_async(xsg.COUNT_LINES, 0, buf.data_ptr())
        torch.cuda.synchronize()
        assert all(int(x) == -1 for x in buf.cpu()[:xsg.NUM_COUNTERS]), expr
        s.count_async_status(xsg.COUNT_LINES | xsg.WITH_NEWLINES, 0, buf.data_ptr(), buf.data_ptr() + 8 * xsg.NUM_COUNTERS)
        torch.cuda.synchronize()
        got = buf.cpu().tolist()
        assert got[xsg.NUM_COUNTERS] == xsg.STATUS_NONASCII and got[:xsg.NUM_COUNTERS] == [0] * xsg.NUM_COUNTERS, expr
    gs.bind(blocks)
    check(gs, oracle, blocks, b"t.e", xsg.FLAG_REGEX, ctx="clean again")


CHUNK = 64 << 10


@pytest.fixture(scope="module")
def textfile(tmp_path_factory):
    d = tmp_path_factory.mktemp("xsinvert")
    data = np.concatenate(text_blocks(27, n=4, size=300_000))
    data = np.concatenate([data[:-1], _u8(b" SheSherlock")])  # a decoy in the tail zone, no final newline
    p = d / "t.txt"
    data.tofile(p)
    plan = xsg.plan_chunks(str(p), CHUNK)
    chunks = [data[int(c["original_offset"]):int(c["original_offset"] + c["original_size"])] for c in plan]
    assert len(chunks) > 10
    return str(p), chunks


def test_job_over_a_file(textfile, oracle):
    path, chunks = textfile
    tags = {"count_lines": xsg.COUNT_LINES, "line_byte_offsets": xsg.LINE_BYTE_OFFSETS, "line_indices": xsg.LINE_INDICES,
            "lines": xsg.LINES}
    for pat, flags in ((b"Sherlock", 0), (b"the", 0), (b"that", xsg.FLAG_EXACT_TAIL), (b"colou?r", xsg.FLAG_REGEX)):
        plain = plain_model(oracle, chunks, pat, flags)
        want = invert_model.invert_all_modes(plain, chunks)
        for threads in (1, 3):
            for key, mode in tags.items():
                j = xsg.Job(pat, path, mode, num_threads=threads, num_max_readers=threads, chunk_bytes=CHUNK, flags=flags | xsg.FLAG_INVERT)
                r = j.result()
                got = int(r) if key == "count_lines" else list(r) if key == "lines" else [int(x) for x in r]
                j.close()
                compare({**want, key: got}, want, f"job {key} threads={threads} pattern={pat!r}")
        TALLY["cases"] += 1
        TALLY["both"] += bool(plain["count_lines"]) and bool(want["count_lines"])
    for mode in (xsg.COUNT_MATCHES, xsg.MATCH_BYTE_OFFSETS):
        e = _refused(lambda: xsg.Job(b"the", path, mode, flags=xsg.FLAG_INVERT))
        assert e.code == xsg.ENOTSUP and "invert" in str(e).lower()


def test_host_searcher_seam(textfile, oracle):
    """xsg_host_*: what the Gpu*Searcher functors of include/xsearch/tasks/gpu_searchers.h call with their `flags`"""
    _, chunks = textfile
    lib = xsg.load()
    for pat, flags in ((b"the", 0), (b"Sherlock", xsg.FLAG_EXACT_TAIL)):
        hs = C.c_void_p()
        assert lib.xsg_host_searcher_create(0, pat, len(pat), flags | xsg.FLAG_INVERT, 2, C.byref(hs)) == xsg.OK
        try:
            for i, b in enumerate(chunks[:4] + [chunks[-1], _u8(b"")]):
                want = invert_model.invert_all_modes(plain_model(oracle, [b], pat, flags), [b])
                data = np.ascontiguousarray(b)
                n = C.c_uint64(0)
                assert lib.xsg_host_count(hs, data.ctypes.data, data.size, 1, C.byref(n)) == xsg.OK
                assert n.value == want["count_lines"], (pat, i)
                assert lib.xsg_host_count(hs, data.ctypes.data, data.size, 0, C.byref(n)) == xsg.ENOTSUP
                assert "invert" in lib.xsg_last_error().decode().lower()
                for mode, key in ((xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices")):
                    out = C.c_void_p()
                    assert lib.xsg_host_offsets(hs, mode, data.ctypes.data, data.size, C.byref(out), C.byref(n)) == xsg.OK
                    got = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
                    lib.xsg_free(out)
                    assert got == want[key], (pat, i, key)
                out = C.c_void_p()
                assert lib.xsg_host_offsets(hs, xsg.MATCH_BYTE_OFFSETS, data.ctypes.data, data.size, C.byref(out), C.byref(n)) == xsg.ENOTSUP
                lens, raw, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
                assert lib.xsg_host_lines(hs, data.ctypes.data, data.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == xsg.OK
                ll = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
                blob = C.string_at(raw, nb.value)
                lib.xsg_free(lens)
                lib.xsg_free(raw)
                ends = np.cumsum(ll).tolist()
                assert [blob[e - k:e] for e, k in zip(ends, ll)] == want["lines"], (pat, i)
        finally:
            lib.xsg_host_searcher_destroy(hs)


def test_cpp_extern_search(textfile, oracle):
    """xs::extern_search with XS_INVERT_MATCH=1: the line tags are served, the match tags throw"""
    cli = ROOT / "tests" / "cpp" / "build" / "extern_search_cli"
    if not cli.exists():
        pytest.fail(f"{cli} not built (make -C tests/cpp)")
    path, chunks = textfile
    want = invert_model.invert_all_modes(plain_model(oracle, chunks, b"the", 0), chunks)
    env = dict(os.environ, XS_CHUNK_BYTES=str(CHUNK), XS_INVERT_MATCH="1")

    def run(tag):
        return subprocess.run([str(cli), tag, "join", "the", path, "-", "2"], capture_output=True, env=env, timeout=300)
    r = run("count_lines")
    assert r.returncode == 0 and int(r.stdout) == want["count_lines"], r.stderr.decode()
    r = run("lines")
    assert r.returncode == 0 and r.stdout.split(b"\n")[:-1] == want["lines"], r.stderr.decode()
    r = run("line_indices")
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == want["line_indices"], r.stderr.decode()
    for tag in ("count", "match_byte_offsets"):
        r = run(tag)
        assert r.returncode != 0 and b"invert" in r.stderr.lower(), tag


def test_xsgrep_invert_equals_gnu_grep(tmp_path):
    """xsgrep -v / -vc against grep -v on a terminated ASCII file searched as one chunk.  The file ends in lines without
    any needle, so nothing sits in the reference's lossy end-of-chunk zone and exact and default semantics agree."""
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    if not shutil.which("grep"):
        pytest.skip("no GNU grep on this host")
    data = np.concatenate(text_blocks(28, n=4, size=2_000_000))
    data = np.concatenate([data, _u8(b"a plain closing row of words, none of which is searched for below\n" * 2)])
    p = tmp_path / "g.txt"
    data.tofile(p)
    env = dict(os.environ, XS_CHUNK_BYTES=str(1 << 30), LC_ALL="C")
    for gflag, args in (("-F", ["Sherlock"]), ("-F", ["-i", "sherlock"]), ("-F", ["that"]), ("-F", ["-F", "colo.r"]), ("-E", ["colou?r"]),
                        ("-E", ["-E", "lock(ed|s)? "]), ("-F", ["-x", "-F", "that"]), ("-E", ["-x", "[a-z ]+"])):
        want = subprocess.run(["grep", gflag, "-v", *args, str(p)], capture_output=True, env=env).stdout
        got = subprocess.run([str(exe), "-v", "-j", "2", *args, str(p)], capture_output=True, env=env, timeout=120)
        assert got.returncode == 0, got.stderr.decode()
        assert got.stdout == want and len(want) > 0, args
        wc = subprocess.run(["grep", gflag, "-v", "-c", *args, str(p)], capture_output=True, env=env).stdout
        for bundle in (["-vc"], ["-c", "--invert-match"]):
            gc = subprocess.run([str(exe), *bundle, *args, str(p)], capture_output=True, env=env, timeout=120)
            assert gc.returncode == 0 and gc.stdout == wc, (args, bundle, gc.stderr.decode())
        with open(p, "rb") as f:  # stdin: newline-aligned chunks through the functor seam
            gs_ = subprocess.run([str(exe), "-vc", *args, "-"], stdin=f, capture_output=True, env=env, timeout=120)
        assert gs_.returncode == 0 and gs_.stdout == wc, (args, gs_.stderr.decode())
    with open(p, "rb") as f:
        got = subprocess.run([str(exe), "-v", "Sherlock", "-"], stdin=f, capture_output=True, env=env, timeout=120)
    assert got.stdout == subprocess.run(["grep", "-F", "-v", "Sherlock", str(p)], capture_output=True, env=env).stdout


def test_zz_enough_cases_have_both_sides():
    """test honesty: in at least half of the generated cases above both R and I are non-empty"""
    assert TALLY["cases"] >= 150, TALLY
    assert 2 * TALLY["both"] >= TALLY["cases"], TALLY
