"""xsg_result_chunk_ptr: the rows of a list result, one per bound chunk, against the CPU oracle run chunk by chunk.

For chunk c the expected entries are what the oracle (tests/per_chunk_model.py: gpu_util.oracle_*_all_modes, anchor_oracle,
set_model, all_of_model, match_model; invert_model and context_model on top of them) reports for a binding that holds chunk c alone, with that
chunk's global_offset and line_base.  Every case checks
  * diff(chunk_ptr) == the per-chunk lengths of those lists, chunk_ptr[0] == 0, chunk_ptr[n] == *n_results,
  * the flat result cut at the rows == the per-chunk lists (the flat result equals their concatenation and the cuts fall
    at their lengths: the same statement),
  * byte_ptr == the cumulative lengths of the entries in front of every row (XSG_LINES, XSG_MATCHES),
  * the other accessors hand out the same result before and after the call, and a second call the same rows,
  * without context bits: diff(chunk_ptr) == Shard.count_chunks (COUNT_MATCHES for the match offsets, COUNT_LINES for the
    two uint64 line tags).
The chunks are bound with non-monotone global offsets and line bases, so no row can be derived from a reported value.

Without the feature every case fails: libxsg.so has no xsg_result_chunk_ptr."""
import ctypes as C

import numpy as np
import pytest

import context_model
import xsg
from gpu_util import GpuSearch
from per_chunk_model import CTX, IC, INV, RX, X, chunk_matches, chunk_plain

pytestmark = pytest.mark.gpu

FLAGS = [(0, "none"), (IC, "icase"), (X, "exact"), (INV, "invert"), (CTX, "context"), (INV | CTX, "invert+context")]
ROUTES = [(None, "default"), (("XSG_LIST_FAST", "0"), "exact route"), (("XSG_LIST_CAP", "3"), "capacity 3")]
U64_MODES = {xsg.MATCH_BYTE_OFFSETS: "match_byte_offsets", xsg.LINE_BYTE_OFFSETS: "line_byte_offsets",
             xsg.LINE_INDICES: "line_indices"}

# (id, kind, pattern or literals, pattern flags)
PATTERNS = [
    ("literal", "lit", b"that", 0),
    ("aa_overlapping", "lit", b"aa", 0),
    ("literal_with_newline", "nl", b"g\nx", 0),
    ("class_sequence", "rx", b"th[ae]t", RX),
    ("prefilter", "rx", b"colou?r", RX),
    ("line_walk", "rx", b"\\w+ing", RX),
    ("anchored", "anchor", b"(?m)^x", RX),
    ("any_of", "anyof", (b"that", b"colour", b"zebra"), 0),
    ("all_of", "allof", (b"that", b"ing"), 0),
]
BINDINGS = ["0", "1", "2", "257", "513", "257_all_in_the_last"]

WORDS = [b"that", b"That", b"colour", b"color", b"COLOUR", b"running", b"going", b"x", b"xy", b"aa", b"aaa", b"aaaaa", b"AA",
         b"plain", b"words", b"zebra", b"the", b"bat", b"thet", b"g", b"sing", b"THAT"]
EVERY_LINE = b"x that colour aaaa running\n" * 3   # every line holds a match of every pattern above
NO_MATCH = b"plain words\nplain\n"                 # none does


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


def words_text(rng, nbytes: int, terminated: bool):
    out, size = [], 0
    while size < nbytes:
        w = WORDS[int(rng.integers(0, len(WORDS)))] + (b"\n" if rng.random() < 0.3 else b" ")
        out.append(w)
        size += len(w)
    b = _u8(b"".join(out)[:nbytes])
    if terminated:
        b[-1] = 10
    return b


def make_blocks(name: str):
    """most chunks at most 64 bytes, a few of 33-40 KiB (they span 16 KiB tiles); empty chunks first, last and in runs; one
    chunk whose every line matches, one without a match; a matching last line without its newline (XSG_LINES drops it)"""
    rng = np.random.default_rng(9000 + len(name) + sum(name.encode()))
    if name == "0":
        return []
    if name == "1":
        return [np.concatenate([words_text(rng, 35_000, True), _u8(b"that colour running x")])]
    if name == "2":
        return [_u8(b"plain\nx that going colour aa"), words_text(rng, 33_333, False)]
    if name == "257_all_in_the_last":
        rich = np.concatenate([_u8(EVERY_LINE), words_text(rng, 34_000, True), _u8(b"x that colour running")])
        return [_u8(NO_MATCH) if i % 3 else _u8(b"") for i in range(256)] + [rich]
    n = int(name)
    blocks = [words_text(rng, int(rng.integers(1, 65)), bool(rng.random() < 0.5)) for _ in range(n)]
    for i in (0, 1, 100, 101, 102, 103, 104, n - 1):
        blocks[i] = _u8(b"")
    blocks[2] = _u8(EVERY_LINE)
    blocks[3] = _u8(NO_MATCH)
    blocks[4] = _u8(b"plain\nx that colour running")       # the matching last line lacks its newline
    blocks[n - 2] = _u8(b"going aa\nthat colour sing")       # ... in the last chunk that holds a byte
    for k, i in enumerate((5, 130, n - 3)):
        blocks[i] = words_text(rng, 33_000 + 3_491 * k, k != 1)
    assert sum(b.size for b in blocks) + 512 * n < (1 << 20)
    return blocks


def offsets_and_bases(n: int):
    """disjoint global ranges and line bases in an order that is not the chunks' (7919 and 31 are coprime to 257 and 513)"""
    go = [((i * 7919) % max(n, 1)) * 1_000_000 + 13 for i in range(n)]
    lb = [((i * 31) % max(n, 1)) * 1_000 + 7 for i in range(n)]
    return go, lb


def expected(oracle, kind, pat, pflags, flags, blocks, go, lb):
    """-> {key: per-chunk lists}: the u64 tags by their names, "lines" as (bytes, offset) pairs, "matches" likewise"""
    want = {k: [] for k in ("match_byte_offsets", "line_byte_offsets", "line_indices", "lines", "matches")}
    for i, b in enumerate(blocks):
        w = chunk_plain(oracle, kind, pat, pflags, flags, b, go[i], lb[i])
        if flags & CTX:  # (the match tags ignore the bits)
            cw = context_model.context_all_modes(w, [b], 1, 2, [go[i]], [lb[i]])
            w = {**w, **{k: cw[k] for k in ("line_byte_offsets", "line_indices", "lines", "lines_offsets")}}
        for k in ("line_byte_offsets", "line_indices"):
            want[k].append([int(x) for x in w[k]])
        want["lines"].append(list(zip(w["lines"], [int(x) for x in w["lines_offsets"]])))
        if kind != "allof" and not flags & INV:
            want["match_byte_offsets"].append([int(x) for x in w["match_byte_offsets"]])
            s, o = chunk_matches(oracle, kind, pat, pflags, flags, b, go[i])
            want["matches"].append(list(zip(s, [int(x) for x in o])))
    return want


# ---- the accessors, without a search of their own ------------------------------------------------------------------------
def run_search(s, mode) -> int:
    n = C.c_uint64(0)
    xsg._check(s._lib.xsg_search(s.h, mode, C.byref(n)))
    return int(n.value)


def get_u64(s, n):
    out = np.zeros(max(n, 1), dtype=np.uint64)
    xsg._check(s._lib.xsg_result_u64(s.h, out.ctypes.data_as(xsg._u64p), n))
    return out[:n].tolist()


def get_packed(s):
    """-> (lengths, [(bytes, offset)]) through xsg_result_lines_size / xsg_result_lines"""
    nl, nb = C.c_uint64(0), C.c_uint64(0)
    xsg._check(s._lib.xsg_result_lines_size(s.h, C.byref(nl), C.byref(nb)))
    lens = np.zeros(max(nl.value, 1), dtype=np.uint64)
    offs = np.zeros(max(nl.value, 1), dtype=np.uint64)
    buf = np.zeros(max(nb.value, 1), dtype=np.uint8)
    xsg._check(s._lib.xsg_result_lines(s.h, lens.ctypes.data_as(xsg._u64p), buf.ctypes.data, nb.value, offs.ctypes.data_as(xsg._u64p)))
    lens, offs, raw = lens[:nl.value].tolist(), offs[:nl.value].tolist(), buf.tobytes()
    ends = np.cumsum(np.asarray(lens, dtype=np.int64)).tolist()
    return lens, [(raw[e - n:e], o) for e, n, o in zip(ends, lens, offs)], int(nb.value)


def get_packed_view(s):
    lens, offs, nl, nb = xsg._u64p(), xsg._u64p(), C.c_uint64(0), C.c_uint64(0)
    data = C.c_void_p()
    xsg._check(s._lib.xsg_result_lines_view(s.h, C.byref(lens), C.cast(C.byref(data), C.POINTER(C.c_char_p)), C.byref(offs),
                                            C.byref(nl), C.byref(nb)))
    n = int(nl.value)
    raw = C.string_at(data, nb.value) if nb.value else b""
    ln = [int(lens[i]) for i in range(n)]
    ends = np.cumsum(np.asarray(ln, dtype=np.int64)).tolist()
    return ln, [(raw[e - k:e], int(offs[i])) for i, (e, k) in enumerate(zip(ends, ln))]


def check_rows(rows, got, want_chunks, where):
    n = len(want_chunks)
    lens = [len(w) for w in want_chunks]
    flat = [e for w in want_chunks for e in w]
    assert rows.size == n + 1 and int(rows[0]) == 0 and int(rows[n]) == len(got), (where, rows[:8].tolist(), len(got))
    assert np.diff(rows.astype(np.int64)).tolist() == lens, (where, "row lengths")
    assert got == flat, (where, "the flat result")
    for c in (0, 2, 4, n // 2, n - 3, n - 2, n - 1):  # (spelled out for a few chunks: the cut at the rows)
        if 0 <= c < n:
            assert got[int(rows[c]):int(rows[c + 1])] == want_chunks[c], (where, "chunk", c)


def check_mode(s, mode, want, where):
    n = run_search(s, mode)
    if mode in U64_MODES:
        before = get_u64(s, n)
        rows = s.result_chunk_ptr()
        assert get_u64(s, n) == before, (where, "xsg_result_u64 after the call")
        assert s.result_chunk_ptr().tolist() == rows.tolist(), (where, "a second call")
        check_rows(rows, before, want[U64_MODES[mode]], where)
        with pytest.raises(xsg.XsgError) as e:
            s.result_chunk_ptr(with_bytes=True)
        assert e.value.code == xsg.EINVAL, where
        assert get_u64(s, n) == before, (where, "xsg_result_u64 after the refused call")
        return rows
    lens, before, nbytes = get_packed(s)
    assert len(before) == n
    rows, byte_ptr = s.result_chunk_ptr(with_bytes=True)
    lens2, after, _ = get_packed(s)
    assert (lens2, after) == (lens, before), (where, "xsg_result_lines after the call")
    assert s.result_chunk_ptr().tolist() == rows.tolist(), (where, "a second call, without byte_ptr")
    check_rows(rows, before, want["lines" if mode == xsg.LINES else "matches"], where)
    cum = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    assert byte_ptr.astype(np.int64).tolist() == cum[rows.astype(np.int64)].tolist(), (where, "byte_ptr")
    assert int(byte_ptr[-1]) == nbytes, (where, "byte_ptr[n]")
    # the view squeezes the dropped lines out of the pinned mirrors in place: the rows do not move
    vl, view = get_packed_view(s)
    assert (vl, view) == (lens, before), (where, "xsg_result_lines_view after the call")
    r3, b3 = s.result_chunk_ptr(with_bytes=True)
    assert (r3.tolist(), b3.tolist()) == (rows.tolist(), byte_ptr.tolist()), (where, "rows after the view")
    return rows


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


@pytest.fixture(scope="module")
def bindings():
    out = {}
    for name in BINDINGS:
        blocks = make_blocks(name)
        for b in blocks:
            b.setflags(write=False)
        out[name] = (blocks, *offsets_and_bases(len(blocks)))
    return out


def set_pattern(gs, kind, pat, pflags, flags):
    if kind == "anyof":
        gs.ctx.set_literals(b"\n".join(pat), flags)
    elif kind == "allof":
        gs.ctx.set_literals(b"\n".join(pat), flags, xsg.LIST_ALL_OF)
    else:
        gs.ctx.set_pattern(pat, pflags | flags)


@pytest.mark.parametrize("binding", BINDINGS)
@pytest.mark.parametrize("pid,kind,pat,pflags", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_rows(gs, oracle, bindings, monkeypatch, binding, pid, kind, pat, pflags):
    blocks, go, lb = bindings[binding]
    gs.bind(blocks, go, lb)
    s = gs.shard
    dropped = 0
    for flags, fname in FLAGS:
        if kind == "nl" and flags & (INV | CTX):
            # a pattern that can match '\n' has no complement and no context: refused where it is set
            with pytest.raises(xsg.XsgError) as e:
                set_pattern(gs, kind, pat, pflags, flags)
            assert e.value.code == xsg.ENOTSUP, (pid, fname)
            continue
        want = expected(oracle, kind, pat, pflags, flags, blocks, go, lb)
        modes = [xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES]
        if kind != "allof" and not flags & INV:
            modes = [xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES] + modes
        dropped += sum(len(a) - len(b) for a, b in zip(want["line_byte_offsets"], want["lines"]))
        for env, rname in ROUTES:
            monkeypatch.delenv("XSG_LIST_FAST", raising=False)
            monkeypatch.delenv("XSG_LIST_CAP", raising=False)
            if env:
                monkeypatch.setenv(*env)
            set_pattern(gs, kind, pat, pflags, flags)
            rows = {}
            for mode in modes:
                rows[mode] = check_mode(s, mode, want, (binding, pid, fname, rname, mode))
            if not flags & CTX and blocks:
                counts = {}
                if xsg.MATCH_BYTE_OFFSETS in modes:
                    counts[xsg.MATCH_BYTE_OFFSETS] = s.count_chunks(xsg.COUNT_MATCHES)[0]
                counts[xsg.LINE_BYTE_OFFSETS] = counts[xsg.LINE_INDICES] = s.count_chunks(xsg.COUNT_LINES)[0]
                for mode, cnt in counts.items():
                    assert np.diff(rows[mode].astype(np.int64)).tolist() == cnt.astype(np.int64).tolist(), (binding, pid, fname, rname, mode, "count_chunks")
    if binding not in ("0",) and kind != "nl":
        assert dropped > 0, "no case of this binding dropped an unterminated line: XSG_LINES rows were not exercised"


def test_matches_of_a_variable_length_expression(gs, oracle, bindings):
    """XSG_MATCHES of `colou?r` and `\\w+ing`: entries of different lengths, so byte_ptr is not a multiple of the rows"""
    blocks, go, lb = bindings["513"]
    gs.bind(blocks, go, lb)
    for pat in (b"colou?r", b"\\w+ing"):
        gs.ctx.set_pattern(pat, RX)
        want = expected(oracle, "rx", pat, RX, 0, blocks, go, lb)
        assert len({len(s) for w in want["matches"] for s, _ in w}) > 1
        rows = check_mode(gs.shard, xsg.MATCHES, want, ("513", pat))
        assert int(rows[-1]) > 0


def test_state_and_arguments(gs, oracle, bindings):
    blocks, go, lb = bindings["257"]
    n = len(blocks)
    lib = xsg.load()
    rows = np.zeros(n + 1, dtype=np.uint64)
    bytes_ = np.zeros(n + 1, dtype=np.uint64)
    call = lambda s, cap, bp=None: lib.xsg_result_chunk_ptr(s.h, C.c_void_p(rows.ctypes.data), cap, C.c_void_p(bp.ctypes.data) if bp is not None else None)
    fresh = GpuSearch()
    fresh.bind(blocks, go, lb)
    fresh.ctx.set_pattern(b"that", 0)
    assert call(fresh.shard, n + 1) == xsg.ESTATE, "before any search"
    fresh.shard.count(xsg.COUNT_LINES)
    assert call(fresh.shard, n + 1) == xsg.ESTATE, "a count is no list result"
    s = fresh.shard
    total = run_search(s, xsg.LINE_BYTE_OFFSETS)
    assert call(s, n + 1) == xsg.OK and int(rows[n]) == total
    assert call(s, n) == xsg.EINVAL, "cap_rows < n + 1"
    assert lib.xsg_result_chunk_ptr(s.h, None, n + 1, None) == xsg.EINVAL, "chunk_ptr is NULL"
    assert call(s, n + 1, bytes_) == xsg.EINVAL, "byte_ptr after a uint64 mode"
    assert call(s, n + 1) == xsg.OK, "the refusals left the result in place"
    assert get_u64(s, total) == s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    run_search(s, xsg.LINES)
    assert call(s, n + 1, bytes_) == xsg.OK
    fresh.bind(blocks, go, lb)
    assert call(s, n + 1) == xsg.ESTATE, "after a rebind"
    run_search(s, xsg.MATCHES)
    assert call(s, n + 1, bytes_) == xsg.OK
    s.invalidate()
    assert call(s, n + 1) == xsg.ESTATE, "after an invalidate"
    # a search that fails leaves nothing to ask for: refused before any launch ...
    run_search(s, xsg.LINE_INDICES)
    assert call(s, n + 1) == xsg.OK
    fresh.ctx.set_pattern(b"that", INV)
    with pytest.raises(xsg.XsgError) as e:
        run_search(s, xsg.MATCH_BYTE_OFFSETS)
    assert e.value.code == xsg.ENOTSUP
    assert call(s, n + 1) == xsg.ESTATE, "after a search that was refused"
    # ... or by the scan: non-ASCII data under an ASCII-only expression
    fresh.bind([_u8("grüße that\n".encode())])
    fresh.ctx.set_pattern(b"that", 0)
    assert run_search(s, xsg.LINES) == 1 and call(s, 2) == xsg.OK and rows[:2].tolist() == [0, 1]
    fresh.ctx.set_pattern(b"t.at", RX)
    with pytest.raises(xsg.XsgError) as e:
        run_search(s, xsg.LINES)
    assert e.value.code == xsg.ENOTSUP
    assert call(s, 2) == xsg.ESTATE, "after a search that failed"
    s.close()
