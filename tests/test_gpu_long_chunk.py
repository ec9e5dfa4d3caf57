"""One chunk longer than 4 GiB: positions inside a chunk at and beyond 2^31 and 2^32 on every route.

The binding has two chunks: chunk 0 of 2^32 + 40 KiB + 5 bytes with an unterminated last line, and a 35 KiB word-salad
chunk behind it, so rows and per-chunk counts have a cut above 2^32.  Their global offsets and line bases are non-zero
and not in chunk order.  Chunk 0 is filled on the device with filler lines of 4095 '-' and a newline; four windows of
seeded word salad with short lines replace whole filler lines:
  [0, 16 KiB) | 16 KiB around 2^31 | 16 KiB around 2^32 | from 2^32 + 24 KiB to the chunk's end
The windows around 2^31 and 2^32 hold a match (`that`) and a line across the boundary.  The four hold different text: a
position cut to 32 (or 31) bits lands in the first window, in the half of another one, or in filler, and reports
something else (test_the_windows_on_the_cpu).

EXPECTED VALUES are the oracle's on the windows alone (tests/high_offsets.py: chunk_plain / chunk_matches), offsets
shifted by the window's start, line indices by arithmetic: filler lines in front plus the newlines of earlier windows.
That is the search of the whole chunk because the filler matches nothing (asserted on 1 MiB of it for every pattern),
lines are independent, and every window begins and ends with three short lines without a match, so context (1 before,
2 after) never reaches a filler line; the last window ends with the chunk, in a matching line without its newline.
Under XSG_FLAG_INVERT the expected lists are the windows' own complements plus, by arithmetic, every filler line
outside the windows: about a million entries, compared as arrays.

Checked per pattern and route: the counts with newlines and bytes, count_chunks, the three uint64 list tags, XSG_LINES,
XSG_MATCHES for the literals and the class sequence (an expression of variable length keeps its XSG_ENOTSUP on such a
chunk: asserted once for `colou?r`), result_chunk_ptr with byte_ptr, the line tags under context, and under invert
COUNT_LINES, count_chunks, LINE_INDICES and LINE_BYTE_OFFSETS.  XSG_LINES under invert is left out: it would gather the
4 GiB of filler.  The counters per literal (count_literals, the CSR matrix, find_literals with positions beyond 2^32
inside one chunk) run on the same binding."""
import numpy as np
import pytest

import context_model
import high_offsets as H
import literal_counts_model as LM
import literal_find_model as FM
import literal_matrix_model as MM
import literal_csr_model as CM
import xsg
from per_chunk_model import CTX, INV
from test_gpu_chunk_rows import check_mode

ROW = 4096
L0 = H.B32 + (40 << 10) + 5
OFF1 = (L0 + 15) // 16 * 16
L1 = 35 << 10
CAP = OFF1 + L1 + 4096
GO, LB = (7_000_000_000_013, 13), (5_000_007, 7)
WIN = 16 << 10
WINDOWS = [(0, WIN), (H.B31 - WIN // 2, WIN), (H.B32 - WIN // 2, WIN), (H.B32 + (24 << 10), L0 - H.B32 - (24 << 10))]
QUIET = b"plain words\nlamp\nthe bat\n"  # three short lines without a match of any pattern
PATTERNS = [p for p in H.PATTERNS if p[0] in ("literal", "aa_overlapping", "class_sequence", "prefilter", "line_walk",
                                              "anchored_begin", "any_of", "any_of_words", "all_of")]
FIXED_LENGTH = ("literal", "aa_overlapping", "class_sequence")
ROUTES = [(None, "default"), (("XSG_LIST_FAST", "0"), "exact route")]
NL = xsg.WITH_NEWLINES


def make_windows():
    out = []
    for k, (start, n) in enumerate(WINDOWS):
        rng = np.random.default_rng(7100 + k)
        last = k == len(WINDOWS) - 1
        b = H.big_block(rng, n, head=QUIET, tail=H.LAST_LINE if last else QUIET)
        for boundary in (H.B31, H.B32):
            at = boundary - start
            if 0 < at < n:  # `x colour going\nx aa th|at ing ab...`: a match and a line across the boundary
                b[at - 23] = 10
                b[at - 22:at + 39] = H.u8(H.RICH_B)
                b[at + 39] = 10
        assert start % ROW == 0 and (last or (n % ROW == 0 and b[-1] == 10))
        b.setflags(write=False)
        out.append(b)
    return out


_W = []


def windows():
    if not _W:
        _W.extend(make_windows())
    return _W


def chunk1():
    b = H.big_block(np.random.default_rng(7200), L1, terminated=False)
    b.setflags(write=False)
    return b


def newlines_before(k: int) -> int:
    """the newlines of chunk 0 in front of window k: the filler lines there plus the earlier windows' own"""
    ws = windows()
    replaced = sum(WINDOWS[j][1] for j in range(k))
    return (WINDOWS[k][0] - replaced) // ROW + sum(int((ws[j] == 10).sum()) for j in range(k))


def filler_segments():
    """[(first byte, number of filler lines, newlines in front)] of the filler between the windows"""
    out = []
    for k in range(len(WINDOWS) - 1):
        lo = WINDOWS[k][0] + WINDOWS[k][1]
        hi = WINDOWS[k + 1][0]
        assert lo % ROW == 0 and hi % ROW == 0 and hi > lo
        out.append((lo, (hi - lo) // ROW, newlines_before(k + 1) - (hi - lo) // ROW))
    return out


def test_the_windows_on_the_cpu(oracle):
    ws = windows()
    filler = np.full(1 << 20, ord("-"), dtype=np.uint8)
    filler[ROW - 1::ROW] = 10
    half = WIN // 2
    for p in PATTERNS:
        sig = lambda b: H.signature(oracle, p[1], p[2], p[3], np.ascontiguousarray(b))
        cnt, lines = sig(filler)
        assert not cnt and not lines, (p[0], "the filler matches")
        sigs = [sig(w) for w in ws]
        assert all(s[1] and s[0] != 0 for s in sigs), (p[0], "a window without a match")
        assert all(sigs[a] != sigs[b] for a in range(4) for b in range(a + 1, 4)), (p[0], "two windows report the same")
        # what a position cut to 31 or 32 bits reads instead: the first window's first half, the 2^31 window's first half
        assert sig(ws[1][half:]) != sig(ws[0][:half]) and sig(ws[2][half:]) != sig(ws[0][:half]), p[0]
        assert sig(ws[2][:half]) != sig(ws[1][:half]), p[0]
        for k, w in enumerate(ws):  # three lines without a match at both ends (the last window ends with the chunk)
            d = w.tobytes()
            assert d.startswith(QUIET) and (k == 3 or d.endswith(QUIET))
            assert not sig(H.u8(QUIET))[1]
    for k, boundary in ((1, H.B31), (2, H.B32)):
        at = boundary - WINDOWS[k][0]
        d = ws[k].tobytes()
        assert d[at - 2:at + 2] == b"that" and 10 not in d[at - 7:at + 39]
    assert ws[3][-1] != 10 and WINDOWS[3][0] + WINDOWS[3][1] == L0
    assert newlines_before(0) == 0 and filler_segments()[0][2] == int((ws[0] == 10).sum())


class Bound:
    def __init__(self):
        import torch
        self.torch = torch
        self.buf = torch.empty(CAP, dtype=torch.uint8, device="cuda:0")
        rows = (L0 + ROW - 1) // ROW  # (the last row runs past chunk 0 into the pad and chunk 1, written below)
        v = self.buf[:rows * ROW].view(-1, ROW)
        v.fill_(ord("-"))
        v[:, ROW - 1] = 10
        self.buf[rows * ROW:].fill_(H.GUARD_BYTE)
        for (start, n), w in zip(WINDOWS, windows()):
            self.buf[start:start + n].copy_(torch.from_numpy(w.copy()))
        self.buf[L0:OFF1].fill_(H.GUARD_BYTE)
        self.c1 = chunk1()
        self.buf[OFF1:OFF1 + L1].copy_(torch.from_numpy(self.c1.copy()))
        self.buf[OFF1 + L1:].fill_(H.GUARD_BYTE)
        torch.cuda.synchronize()
        self.ctx = xsg.Context(0)
        self.shard = xsg.Shard(self.ctx, self.buf.data_ptr(), CAP, xsg.make_chunks([0, OFF1], [L0, L1], list(GO), list(LB)))

    def close(self):
        self.shard.close()
        self.ctx.close()
        self.buf = None
        self.torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def bound():
    b = Bound()
    yield b
    b.close()


def refused(fn, *args):
    with pytest.raises(xsg.XsgError) as e:
        fn(*args)
    return e.value


def set_pattern(ctx, kind, pat, pflags, flags):
    if kind.startswith("anyof") or kind.startswith("allof"):
        lf = (xsg.LIST_ALL_OF if kind.startswith("allof") else 0) | (xsg.LIST_WHOLE_WORDS if kind.endswith("_w") else 0)
        ctx.set_literals(b"\n".join(pat), flags, lf)
    else:
        ctx.set_pattern(pat, pflags | flags)


def pieces(c1):
    """[(block, global offset, line base)] of chunk 0's windows, then chunk 1: what the oracle is run on"""
    return [(w, GO[0] + WINDOWS[k][0], LB[0] + newlines_before(k)) for k, w in enumerate(windows())] + [(c1, GO[1], LB[1])]


def expected(oracle, c1, kind, pat, pflags, flags, with_matches):
    """-> the per-chunk lists (two chunks) of the tags without invert, and the per-chunk counts"""
    want = {k: [[], []] for k in ("match_byte_offsets", "line_byte_offsets", "line_indices", "lines", "matches")}
    counts = {"count_matches": [0, 0], "count_lines": [0, 0], "newlines": [0, 0]}
    ps = pieces(c1)
    for i, (b, g, lb) in enumerate(ps):
        c = int(i == len(ps) - 1)
        w = H.chunk_plain(oracle, kind, pat, pflags, flags, b, g, lb)
        counts["count_lines"][c] += int(w["count_lines"])
        counts["newlines"][c] += int(w["newlines"])
        if flags & CTX:
            cw = context_model.context_all_modes(w, [b], 1, 2, [g], [lb])
            w = {**w, **{k: cw[k] for k in ("line_byte_offsets", "line_indices", "lines", "lines_offsets")}}
        for k in ("line_byte_offsets", "line_indices"):
            want[k][c] += [int(x) for x in w[k]]
        want["lines"][c] += list(zip(w["lines"], [int(x) for x in w["lines_offsets"]]))
        if with_matches:
            counts["count_matches"][c] += int(w["count_matches"])
            want["match_byte_offsets"][c] += [int(x) for x in w["match_byte_offsets"]]
            s, o = H.chunk_matches(oracle, kind, pat, pflags, flags, b, g)
            want["matches"][c] += list(zip(s, [int(x) for x in o]))
    segs = filler_segments()
    counts["newlines"][0] += sum(n for _, n, _ in segs)
    return want, counts


def expected_inverted(oracle, c1, kind, pat, pflags):
    """-> (line_byte_offsets, line_indices) as uint64 arrays over both chunks, and the per-chunk line counts"""
    offs, idx, counts = [], [], [0, 0]
    ps, segs = pieces(c1), filler_segments()
    for i, (b, g, lb) in enumerate(ps):
        c = int(i == len(ps) - 1)
        w = H.chunk_plain(oracle, kind, pat, pflags, INV, b, g, lb)
        offs.append(np.array(w["line_byte_offsets"], dtype=np.uint64))
        idx.append(np.array(w["line_indices"], dtype=np.uint64))
        counts[c] += int(w["count_lines"])
        if i < len(segs):  # the filler lines behind this window: none of them matches
            lo, n, nlb = segs[i]
            offs.append(np.uint64(GO[0] + lo) + np.arange(n, dtype=np.uint64) * np.uint64(ROW))
            idx.append(np.uint64(LB[0] + nlb) + np.arange(n, dtype=np.uint64))
            counts[0] += n
    return np.concatenate(offs), np.concatenate(idx), counts


def check_counts(s, want_matches, counts, where):
    nl = sum(counts["newlines"])
    for mode, ctr, key in ((xsg.COUNT_MATCHES, xsg.CTR_MATCHES, "count_matches"), (xsg.COUNT_LINES, xsg.CTR_LINES, "count_lines")):
        if mode == xsg.COUNT_MATCHES and not want_matches:
            assert refused(s.count, mode | NL).code == xsg.ENOTSUP, where
            continue
        c = s.count(mode | NL)
        assert (int(c[ctr]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])) == (sum(counts[key]), nl, L0 + L1), (where, key, "count")
        per, newlines, tot = s.count_chunks(mode | NL)
        assert per.tolist() == counts[key] and newlines.tolist() == counts["newlines"], (where, key, "count_chunks")
        assert tot.tolist() == c.tolist(), (where, key, "count_chunks: totals")


@pytest.mark.gpu
@pytest.mark.parametrize("pid,kind,pat,pflags", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_positions_beyond_2_32_inside_a_chunk(bound, oracle, monkeypatch, pid, kind, pat, pflags):
    s, c1 = bound.shard, bound.c1
    all_of = kind.startswith("allof")
    want, counts = expected(oracle, c1, kind, pat, pflags, 0, not all_of)
    want_ctx, _ = expected(oracle, c1, kind, pat, pflags, CTX, False)
    inv_offs, inv_idx, inv_counts = expected_inverted(oracle, c1, kind, pat, pflags)
    assert max(want["line_byte_offsets"][0]) - GO[0] > H.B32 and len(want["line_byte_offsets"][0]) > len(want["lines"][0])
    assert inv_counts[0] > (1 << 20) and inv_offs.size == sum(inv_counts)
    for env, rname in ROUTES:
        monkeypatch.delenv("XSG_LIST_FAST", raising=False)
        if env:
            monkeypatch.setenv(*env)
        where = (pid, rname)
        set_pattern(bound.ctx, kind, pat, pflags, 0)
        check_counts(s, not all_of, counts, where)
        modes = [xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES]
        if not all_of:
            modes.insert(0, xsg.MATCH_BYTE_OFFSETS)
        if pid in FIXED_LENGTH:
            modes.insert(1, xsg.MATCHES)
        for mode in modes:
            check_mode(s, mode, want, where + (mode,))
        if pid == "prefilter" and env is None:
            e = refused(s.search_matches)
            assert e.code == xsg.ENOTSUP and "4 GiB" in str(e)
        # context, without invert: the line tags
        set_pattern(bound.ctx, kind, pat, pflags, CTX)
        for mode in (xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES):
            check_mode(s, mode, want_ctx, where + ("context", mode))
        # invert: every filler line and the windows' complements
        set_pattern(bound.ctx, kind, pat, pflags, INV)
        check_counts(s, False, {"count_lines": inv_counts, "newlines": counts["newlines"]}, where + ("invert",))
        for mode, arr in ((xsg.LINE_BYTE_OFFSETS, inv_offs), (xsg.LINE_INDICES, inv_idx)):
            got = s.search_u64(mode)
            assert got.size == arr.size and np.array_equal(got, arr), (where, "invert", mode, np.flatnonzero(got[:arr.size] != arr[:got.size])[:4])
            assert s.result_chunk_ptr().tolist() == [0, inv_counts[0], sum(inv_counts)], (where, "invert", mode, "rows")


@pytest.mark.gpu
def test_literal_counters(bound):
    s, c1 = bound.shard, bound.c1
    lits, k = list(H.LITERALS), len(H.LITERALS)
    ws = windows()
    bound.ctx.set_literals(xsg.literal_list(lits), 0, 0)
    rows = MM.matrix(ws + [c1], lits)
    rows = [[sum(r[j] for r in rows[:-1]) for j in range(k)], rows[-1]]
    assert s.count_literals().tolist() == LM.counts(ws + [c1], lits)
    m, w = s.count_literals_chunks()
    assert m.tolist() == rows and w.tolist() == MM.chunks_with(rows, k)
    assert tuple(x.tolist() for x in s.count_literals_csr()) == CM.from_rows(rows)
    cp, pos, lit = FM.find(ws + [c1], lits, False, False, [g for _, g, _ in pieces(c1)])
    assert max(pos) - GO[0] > H.B32
    got = s.find_literals()
    assert got[0].tolist() == [0, cp[-2], cp[-1]] and got[1].tolist() == pos and got[2].tolist() == lit
