"""Every route on small chunks that lie at buffer offsets beyond 2^31 and 2^32 (tests/high_offsets.py: the layouts
"abutting" and "straddling", their decoys and guards; tests/test_high_offsets_layout.py shows on the CPU that a read
which loses the high bits of an address reports something else for every pattern and every chunk up there).

One buffer of about 6 GiB per layout is allocated, never filled: only the chunks (less than 1 MiB), their decoys and the
guards are written, and only the chunks are bound.  Work follows the bound bytes, so every case is as cheap as on a small
buffer.  Expected values come from the CPU models, chunk by chunk (high_offsets.chunk_plain / chunk_matches: tests/
per_chunk_model.py, and tests/words_model.py for the whole-word lists), never from a second binding; every comparison is
exact equality.  Per pattern, flag set and route: all seven tags, the counts with newlines and bytes, count_async into a
device buffer, count_chunks for both count tags with the newlines column, result_chunk_ptr with byte_ptr for the two
string tags.  What is refused is asserted by its code: the match tags under XSG_FLAG_INVERT and for an all-of list, a
pattern that holds '\\n' under invert or context, the stream-ordered counts of a literal list and of the line count of
a pattern that holds '\\n'."""
import numpy as np
import pytest

import context_model
import high_offsets as H
import literal_counts_model as LM
import literal_csr_model as CM
import literal_find_model as FM
import literal_matrix_model as MM
import words_model as WM
import xsg
from per_chunk_model import CTX, IC, INV, X
from test_gpu_chunk_rows import U64_MODES, check_mode
from test_gpu_literal_csr import Side as CsrSide
from test_gpu_literal_find import Side as FindSide

pytestmark = pytest.mark.gpu

FLAGS = [(0, "none"), (IC, "icase"), (X, "exact"), (INV, "invert"), (CTX, "context"), (INV | CTX, "invert+context")]
ROUTES = [(None, "default"), (("XSG_LIST_FAST", "0"), "exact route"), (("XSG_LIST_CAP", "3"), "capacity 3")]
LAYOUTS = ("abutting", "straddling")
NL = xsg.WITH_NEWLINES
_WANT = {}  # (pattern id, flags, chunk name) -> the oracle's dicts: the layouts share most chunks


class Bound:
    """a layout in device memory: the buffer, a context and the shard bound to the layout's chunks"""

    def __init__(self, lay):
        import torch
        self.torch = torch
        self.lay = lay
        self.buf = torch.empty(lay.capacity, dtype=torch.uint8, device="cuda:0")
        for addr, data in lay.writes:
            self.buf[addr:addr + data.size].copy_(torch.from_numpy(data.copy()))
        torch.cuda.synchronize()
        self.blocks, self.go, self.lb = lay.blocks(), lay.global_offsets(), lay.line_bases()
        self.chunks = xsg.make_chunks(np.array([c.offset for c in lay.chunks], dtype=np.uint64),
                                      np.array([b.size for b in self.blocks], dtype=np.uint64), self.go, self.lb)
        self.ctx = xsg.Context(0)
        self.shard = xsg.Shard(self.ctx, self.buf.data_ptr(), lay.capacity, self.chunks)
        self.counters = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")

    def close(self):
        self.shard.close()
        self.ctx.close()
        self.buf = None
        self.torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=LAYOUTS)
def bound(request):
    b = Bound(H.layouts()[request.param])
    yield b
    b.close()


def refused(fn, *args):
    with pytest.raises(xsg.XsgError) as e:
        fn(*args)
    return e.value.code


def set_pattern(ctx, kind, pat, pflags, flags):
    if kind.startswith("anyof") or kind.startswith("allof"):
        lf = (xsg.LIST_ALL_OF if kind.startswith("allof") else 0) | (xsg.LIST_WHOLE_WORDS if kind.endswith("_w") else 0)
        ctx.set_literals(b"\n".join(pat), flags, lf)
    else:
        ctx.set_pattern(pat, pflags | flags)


def expected(oracle, lay, pid, kind, pat, pflags, flags):
    """-> per-chunk lists by tag ("lines" / "matches" as (bytes, offset) pairs), and the per-chunk counts"""
    want = {k: [] for k in ("match_byte_offsets", "line_byte_offsets", "line_indices", "lines", "matches", "count_matches",
                            "count_lines", "newlines", "bytes")}
    with_matches = not kind.startswith("allof") and not flags & INV
    for c in lay.chunks:
        key = (pid, flags, c.name)
        if key not in _WANT:
            b = c.block
            w = H.chunk_plain(oracle, kind, pat, pflags, flags, b, c.global_offset, c.line_base)
            e = {"count_lines": int(w["count_lines"]), "newlines": int(w["newlines"]), "bytes": int(w["bytes"])}
            if flags & CTX:  # (the match tags and the counts ignore the bits)
                cw = context_model.context_all_modes(w, [b], 1, 2, [c.global_offset], [c.line_base])
                w = {**w, **{k: cw[k] for k in ("line_byte_offsets", "line_indices", "lines", "lines_offsets")}}
            for k in ("line_byte_offsets", "line_indices"):
                e[k] = [int(x) for x in w[k]]
            e["lines"] = list(zip(w["lines"], [int(x) for x in w["lines_offsets"]]))
            if with_matches:
                e["count_matches"] = int(w["count_matches"])
                e["match_byte_offsets"] = [int(x) for x in w["match_byte_offsets"]]
                s, o = H.chunk_matches(oracle, kind, pat, pflags, flags, b, c.global_offset)
                e["matches"] = list(zip(s, [int(x) for x in o]))
            _WANT[key] = e
        for k, v in _WANT[key].items():
            want[k].append(v)
    return want


def check_counts(bd, kind, flags, want, where):
    s, torch = bd.shard, bd.torch
    with_matches = not kind.startswith("allof") and not flags & INV
    is_list = kind.startswith("anyof") or kind.startswith("allof")
    nl, nbytes = sum(want["newlines"]), sum(want["bytes"])
    totals = {}
    for mode, ctr, key in ((xsg.COUNT_MATCHES, xsg.CTR_MATCHES, "count_matches"), (xsg.COUNT_LINES, xsg.CTR_LINES, "count_lines")):
        if mode == xsg.COUNT_MATCHES and not with_matches:
            assert refused(s.count, mode | NL) == xsg.ENOTSUP, where
            assert refused(s.count_chunks, mode | NL) == xsg.ENOTSUP, where
            assert refused(s.count_async, mode, 0, bd.counters.data_ptr()) == xsg.ENOTSUP, where
            continue
        c = s.count(mode | NL)
        assert (int(c[ctr]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])) == (sum(want[key]), nl, nbytes), (where, key, "count")
        counts, newlines, tot = s.count_chunks(mode | NL)
        assert counts.tolist() == want[key], (where, key, "count_chunks")
        assert newlines.tolist() == want["newlines"], (where, key, "count_chunks: newlines")
        assert tot.tolist() == c.tolist(), (where, key, "count_chunks: totals")
        totals[mode] = counts
        # the stream-ordered count into a device buffer
        amode = mode | (NL if mode == xsg.COUNT_LINES else 0)
        if is_list or (mode == xsg.COUNT_LINES and kind == "nl"):
            assert refused(s.count_async, amode, 0, bd.counters.data_ptr()) == xsg.ENOTSUP, (where, key, "count_async")
            continue
        bd.counters.fill_(77)
        torch.cuda.synchronize()
        s.count_async(amode, 0, bd.counters.data_ptr())
        torch.cuda.synchronize()
        got = bd.counters.cpu().tolist()
        assert got[ctr] == sum(want[key]), (where, key, "count_async")
        if amode & NL:
            assert got[xsg.CTR_NEWLINES] == nl, (where, key, "count_async: newlines")
    return totals


@pytest.mark.parametrize("pid,kind,pat,pflags", H.PATTERNS, ids=[p[0] for p in H.PATTERNS])
def test_every_tag(bound, oracle, monkeypatch, pid, kind, pat, pflags):
    lay, s = bound.lay, bound.shard
    dropped = 0
    for flags, fname in FLAGS:
        if kind == "nl" and flags & (INV | CTX):
            # a pattern that can match '\n' has no complement and no context: refused where it is set
            assert refused(set_pattern, bound.ctx, kind, pat, pflags, flags) == xsg.ENOTSUP, (pid, fname)
            continue
        want = expected(oracle, lay, pid, kind, pat, pflags, flags)
        with_matches = not kind.startswith("allof") and not flags & INV
        modes = [xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES]
        if with_matches:
            modes = [xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES] + modes
        above = [i for i, c in enumerate(lay.chunks) if c.offset >= H.B32]
        dropped += sum(len(want["line_byte_offsets"][i]) - len(want["lines"][i]) for i in above)
        for env, rname in ROUTES:
            monkeypatch.delenv("XSG_LIST_FAST", raising=False)
            monkeypatch.delenv("XSG_LIST_CAP", raising=False)
            if env:
                monkeypatch.setenv(*env)
            where = (lay.name, pid, fname, rname)
            set_pattern(bound.ctx, kind, pat, pflags, flags)
            rows = {}
            for mode in modes:
                rows[mode] = check_mode(s, mode, want, where + (mode,))
            if not with_matches:
                for mode in (xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES):
                    assert refused(s.search_u64, mode) == xsg.ENOTSUP, where + (mode,)
            counts = check_counts(bound, kind, flags, want, where)
            if not flags & CTX:  # the rows of the list tags are the counts per chunk
                for mode, cmode in ((xsg.MATCH_BYTE_OFFSETS, xsg.COUNT_MATCHES), (xsg.LINE_BYTE_OFFSETS, xsg.COUNT_LINES),
                                    (xsg.LINE_INDICES, xsg.COUNT_LINES)):
                    if mode in rows:
                        assert np.diff(rows[mode].astype(np.int64)).tolist() == counts[cmode].astype(np.int64).tolist(), where + (U64_MODES[mode], "rows")
    if kind != "nl":
        assert dropped > 0, "no unterminated last line above 2^32 was dropped: the rows of XSG_LINES were not exercised there"


# ---- the counters per literal ---------------------------------------------------------------------------------------------------
LIST_FORMS = [("plain", 0, 0), ("icase", IC, 0), ("whole_words", 0, xsg.LIST_WHOLE_WORDS)]


@pytest.mark.parametrize("form,flags,list_flags", LIST_FORMS, ids=[f[0] for f in LIST_FORMS])
def test_literal_counters(bound, form, flags, list_flags):
    lay, s = bound.lay, bound.shard
    lits, blocks, n, k = list(H.LITERALS), bound.blocks, len(bound.blocks), len(H.LITERALS)
    icase, words = bool(flags & IC), bool(list_flags)
    bound.ctx.set_literals(xsg.literal_list(lits), flags, list_flags)
    rows = WM.matrix(blocks, lits, icase) if words else MM.matrix(blocks, lits, icase)
    totals = WM.counts(blocks, lits, icase) if words else LM.counts(blocks, lits, icase)
    assert totals == [sum(r[j] for r in rows) for j in range(k)] and totals[9] == 0 and totals[0] == totals[5] > 0
    where = (lay.name, form)
    assert s.count_literals().tolist() == totals, (where, "count_literals")
    m, w = s.count_literals_chunks()
    assert m.tolist() == rows, (where, "count_literals_chunks")
    assert w.tolist() == MM.chunks_with(rows, k), (where, "chunks_with")
    # CSR: the kept result and the stream-ordered form
    want_csr = CM.from_rows(rows)
    assert tuple(x.tolist() for x in s.count_literals_csr()) == want_csr, (where, "count_literals_csr")
    rp, cols, vals, status = CsrSide().run(s, n, len(want_csr[1]))
    assert status == xsg.STATUS_OK and (rp, cols, vals) == want_csr, (where, "count_literals_csr_async")
    # the occurrences: kept, stream-ordered, and clipped at a capacity below the total
    want = FM.find(blocks, lits, icase, words, bound.go)
    total = len(want[1])
    assert total > 1000 and max(want[1]) < (1 << 40)
    assert tuple(x.tolist() for x in s.find_literals()) == want, (where, "find_literals")
    side = FindSide()
    cp, pos, lit, status = side.run(s, n, total)
    assert status == xsg.STATUS_OK and (cp, pos, lit) == want, (where, "find_literals_async")
    cap = want[0][-2]  # the entries of the last chunk do not fit
    assert 0 < cap < total
    cp, pos, lit, status = side.run(s, n, cap)  # (asserts that nothing at or behind cap was written)
    assert status == xsg.STATUS_OVERFLOW, (where, "clipped: status")
    assert cp == want[0], (where, "clipped: chunk_ptr is complete")
    assert pos == want[1][:cap] and lit == want[2][:cap], (where, "clipped: the entries below the capacity")
