"""The inputs of test_gpu_chains.py reach every branch of the occurrence-chain walks -- a condition on the inputs, checked
without a GPU -- and the oracle they are compared with agrees with a second, ten-line reference on every one of them.

chain_cases.py labels each binding with the branches of k_greedy_keep, k_greedy_links, close_chains, k_nlpat_links,
k_rx_verify and the overlap probe that it takes; the labels a family must reach are listed HERE, by name, so that a case
which silently stops reaching its branch fails here.  Labels that depend on the whole occurrence list (where the list ends,
how many rounds the closure needs) are asked of the cases that test_gpu_chains.py binds alone.
"""
import bisect

import numpy as np
import pytest

import chain_cases as C
import xsg
from xs_oracle import compile_class_sequence

GREEDY = ("budget", "seams", "rounds", "links")
TAIL_MODES = (0, C.EXACT)


def modes_of(b):
    return (b.flags,) if b.flags & C.REGEX else tuple(b.flags | t for t in TAIL_MODES)


def raw_of(b, flags):
    return [C.raw_occurrences(c, b.pattern, flags) for _, c in b.chunks]


_labels = {}


def labels(family):
    """-> (labels of the bindings as they are bound together, labels of the cases bound alone, {binding, case: its labels})"""
    if family not in _labels:
        tog, solo, per = set(), set(), {}
        for b in C.bindings(family):
            plen = C.pattern_length(b.pattern, b.flags) if family != "verify" else 0
            for flags in modes_of(b):
                if family in GREEDY:
                    r = raw_of(b, flags)
                    tog |= C.greedy_labels(r, plen)
                    for i in b.solo:
                        per[b.name, b.chunks[i][0], flags] = C.greedy_labels([r[i]], plen)
                elif family == "newline":
                    r, ch = raw_of(b, flags), C.blocks_of(b)
                    tog |= C.nlpat_labels(ch, r, b.pattern)
                    for i in b.solo:
                        per[b.name, b.chunks[i][0], flags] = C.nlpat_labels([ch[i]], [r[i]], b.pattern)
                elif family == "verify":
                    per[b.name, "", flags] = C.verify_labels(C.blocks_of(b), b.pattern)
                    tog |= per[b.name, "", flags]
                else:
                    per[b.name, "", flags] = C.probe_labels(C.blocks_of(b), b.pattern)
                    tog |= per[b.name, "", flags]
        for v in per.values():
            solo |= v
        _labels[family] = (tog, solo, per)
    return _labels[family]


def test_the_constants_are_the_librarys():
    assert (C.EXACT, C.ICASE, C.REGEX) == (xsg.FLAG_EXACT_TAIL, xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX)
    assert C.MAX_PATTERN == xsg.MAX_PATTERN


def test_the_models_on_hand_made_lists():
    a = lambda n: np.arange(n, dtype=np.int64)
    # `aa` on runs: F followers, budget, flag
    for n, flag, left in ((4096, False, 0), (4097, False, 0), (4098, True, 1)):  # n entries: F = n - 1
        keep, f, unfinished = C.sequential_marks(a(n), np.zeros(n, dtype=np.int64), 2)
        assert (f, unfinished) == (flag, left), n
        assert keep[:4097:2].all() and not keep[1::2].any() and not keep[4097:].any()
    # F = 4096 with one more entry behind (a head of its own): the flag goes up, nothing is left to close
    pos = np.append(a(4097), 5000)
    keep, f, unfinished = C.sequential_marks(pos, np.zeros(4098, dtype=np.int64), 2)
    assert (f, unfinished) == (True, 0) and keep[4097]
    assert "F=4096 with entries behind: flag, nothing left to close" in C.greedy_labels([pos], 2)
    assert "F=4096 at the list's end: no flag" in C.greedy_labels([a(4097)], 2)
    # links: in the chunk, clamped, into the next chunk
    J, clamped = C.greedy_links(np.array([0, 1, 2, 3, 0, 1]), np.array([0, 0, 0, 0, 1, 1]), 2)
    assert J.tolist() == [2, 3, C.NOLINK, C.NOLINK, C.NOLINK, C.NOLINK] and clamped.tolist() == [False, False, False, False, True, True]
    # closure: n reported entries behind the walk need ceil(log2(n + 1)) marking rounds
    for n, rounds in ((1, 1), (2, 2), (3, 2), (4, 3), (7, 3), (8, 4)):
        assert C.greedy_rounds([a(C.BUDGET + 2 * n + 1)], 2) == rounds, n
    # heads: the chunk test alone
    assert "head by the chunk test alone" in C.greedy_labels([np.array([10]), np.array([11, 12])], 2)
    assert C.chain_heads(np.array([0, 3, 5, 8]), np.zeros(4, dtype=np.int64), 3)[1].tolist() == [0, 1, 0]
    # newline literals: `a\n` on three lines and a rest without a newline
    ch = [np.frombuffer(b"a\na\na\nxx", dtype=np.uint8)]
    heads, J, behind = C.nlpat_links(ch, [np.array([0, 2, 4])], 2)
    assert heads.tolist() == [True, False, False] and J.tolist() == [2, C.NOLINK, C.NOLINK] and behind.tolist() == [3, 5, -1]
    # the probe
    assert [C.borders(p) for p in (b"aXa", b"abaXaba", b"aaaa", b"aaaaa", b"abc")] == [[1], [3, 1], [3, 2, 1], [4, 3, 2, 1], []]
    assert C.overlap_words(b"abaXaba") == [b"abaXabaXaba", b"abaXababaXaba"] and C.overlap_words(b"aaaaa") == []
    assert C.overlap_words(C.long_literal()) == [] and C.borders(C.long_literal()) == [1] and len(C.long_literal()) == 20_000
    # the verify budget: x and 4095 / 4094 `a`, the chunk goes on
    f = lambda n, tail: C.verify_labels([np.frombuffer(b"." * 600_000 + b"x" + b"a" * n + tail, dtype=np.uint8)], b"xaa+")
    assert f(4095, b" ...") == {"alive at the budget: flag"} and f(4094, b" ...") == {"dies one byte short of the budget"}
    assert f(4095, b"") == {"alive at the chunk's end, exactly the budget: no flag"}
    assert f(4096, b"") == {"alive at the budget, the chunk one byte longer: flag"}
    assert f(40, b"") == {"alive at the chunk's end: no flag"}


def test_the_generator_is_fixed_and_small():
    for family in C.FAMILIES:
        names = set()
        for b in C.bindings(family):
            assert b.name not in names, b.name
            names.add(b.name)
            assert len({n for n, _ in b.chunks}) == len(b.chunks) or family in ("verify", "probe"), b.name
            assert all(c.size <= 200 * 1024 for _, c in b.chunks), b.name     # (`\nab\n` on 65 537 lines of three bytes: 192 KiB)
            assert sum(c.size for _, c in b.chunks) <= 2 << 20, b.name
            assert all(0 <= i < len(b.chunks) for i in b.solo)
    again = C._BUILD["budget"]()
    assert all((x[1] == y[1]).all() for a, b in zip(again, C.bindings("budget")) for x, y in zip(a.chunks, b.chunks))


BUDGET_TOGETHER = (
    ["F=0", "under budget", "F=4095: the last fetch within budget is full", "F=4096 with entries behind: flag, nothing left to close",
     "over budget: flag", "over budget with entries behind", "several chains over budget", "over budget by more than a fetch",
     "ends with its chunk", "next head exactly plen behind", "next head more than plen behind", "follower at plen - 1"] +
    [f"over budget by {k}" for k in (1, 2, 7, 8, 9)] + [f"chain ends in fetch slot {k}" for k in range(C.FETCH)])
BUDGET_ALONE = ["F=4096 at the list's end: no flag", "ends with the list, inside a fetch", "ends with the list, on a fetch border",
                "no flag: no closure", "link window clamped at M", "no link: the search ends at M", "over budget: flag"]
SEAMS = ["ends with its chunk", "ends with its chunk: only the chunk test says so", "head by the chunk test alone",
         "no link: the target lies in the next chunk", "over budget: flag", "several chains over budget", "F=0"]
LINKS_TOGETHER = ["link to i+1", "link to i+2", "link to i+3", "link to i+plen", "link inside the window",
                  "no link: the target lies in the next chunk", "no link: the search ends at M", "over budget with entries behind"]
LINKS_ALONE = ["link window clamped at M", "ends with the list, inside a fetch", "over budget: flag"]
NEWLINE = ["line start one byte behind the match start", "line start behind the last newline before the match", "link found",
           "no newline behind the match", "no occurrence left in the chunk, r1 < M", "no occurrence left in the chunk, r1 == M",
           "occurrence ends with the chunk", "the only newline behind the match is the chunk's last byte",
           "a chunk without any newline", "empty chunks between two chunks with occurrences"]
VERIFY = ["dies early", "dies one byte short of the budget", "alive at the chunk's end: no flag",
          "alive at the chunk's end, exactly the budget: no flag", "alive at the budget: flag",
          "alive at the budget, the chunk one byte longer: flag", "the first of hundreds of candidates outruns the budget",
          "the last of hundreds of candidates outruns the budget", "candidates too dense: none is verified"]
PROBE = ["1 border", "2 borders", "3 borders", "more than three borders: not probed",
         "a probe word longer than XSG_MAX_PATTERN: not probed", "word 1 finds a pair", "word 2 finds a pair", "word 3 finds a pair",
         "no word finds a pair: overlap-free"]


@pytest.mark.parametrize("family,together,alone", [
    ("budget", BUDGET_TOGETHER, BUDGET_ALONE), ("seams", SEAMS, []), ("links", LINKS_TOGETHER, LINKS_ALONE),
    ("newline", NEWLINE, []), ("verify", VERIFY, []), ("probe", PROBE, [])])
def test_every_branch_is_reached(family, together, alone):
    tog, solo, _ = labels(family)
    assert not [x for x in together if x not in tog], sorted(tog)
    assert not [x for x in alone if x not in solo], sorted(solo)


def test_every_budget_pattern_has_every_follower_count():
    """F_LIST for every pattern, in its three places, and the honest form of "over budget": F > 4096 with entries behind"""
    for b in C.bindings("budget"):
        plen = C.pattern_length(b.pattern, b.flags)
        for flags in modes_of(b):
            seen = {}
            for (name, c) in b.chunks:
                pos = C.raw_occurrences(c, b.pattern, flags)
                heads, F = C.chain_heads(pos, np.zeros(len(pos), dtype=np.int64), plen)
                if name.startswith("F="):
                    want = sum(int(x) for x in name.split()[0][2:].split("+"))
                    assert F[0] == want, (b.name, name, F[:3])
                    seen.setdefault(name.split()[1], []).append(want)
                    if want > C.BUDGET and "then-head" in name:  # (the others have entries behind them in the binding, not in their chunk)
                        assert heads[0] + F[0] + 1 < len(pos), (b.name, name)
                else:
                    assert sum(F > C.BUDGET) >= 3 and (F[1:] < 20).sum() >= 4, (b.name, name, F)
            assert seen["last"] == list(C.F_LIST) == seen["then-head"] and seen["same-chain"] == [f + 6 for f in C.F_LIST], b.name


def test_the_closure_needs_every_number_of_rounds():
    """family C: for every r in 1 .. 16 a case that needs r marking rounds and one that needs r + 1 -- bound alone"""
    (b,) = C.bindings("rounds")
    r = raw_of(b, 0)
    rounds = {name: C.greedy_rounds([r[i]], 2) for i, (name, _) in enumerate(b.chunks)}
    assert sorted(set(rounds.values())) == list(range(1, 18)), rounds
    for k in range(1, 17):
        assert rounds[f"{2 ** k - 1} reported entries behind the budget"] == k
        assert rounds[f"{2 ** k} reported entries behind the budget"] == k + 1 == rounds[f"{2 ** k + 1} reported entries behind the budget"]
    assert set(b.solo) == set(range(len(b.chunks)))
    # the newline chains, which have no budget: every number of rounds up to 16 as well
    _, _, per = labels("newline")
    got = {int(x.split()[1]) for v in per.values() for x in v if x.startswith("closure:")}
    assert got >= set(range(0, 17)), sorted(got)


# ---------------------------------------------------------------------------------------------------------------------
# two references: the oracle, and the walk in ten lines
# ---------------------------------------------------------------------------------------------------------------------
def walk(data: bytes, occ, plen, lines):
    """search_wrappers.h:29-50 on the list of ALL occurrences: report the leftmost one at or behind `shift`; then shift =
    match + plen and, in the line modes, the byte behind the first '\\n' at or behind that -> the reported match starts"""
    out, shift = [], 0
    while True:
        i = bisect.bisect_left(occ, shift)
        if i == len(occ):
            return out
        out.append(occ[i])
        shift = occ[i] + plen
        if lines:
            nl = data.find(b"\n", shift)
            if nl < 0:
                return out
            shift = nl + 1


def line_start(data: bytes, m):
    """search_wrappers.h:111-123: tests the match's first byte first"""
    return m + 1 if data[m] == 10 else data.rfind(b"\n", 0, m) + 1


# the cases that are there to hold nothing (a single line holds no pattern that begins or goes on behind its newline)
NOTHING_TO_REPORT = ("empty", "empty again", "shorter than the pattern", "no newline at all", "1 lines")


@pytest.mark.parametrize("family", GREEDY + ("newline",))
def test_the_oracle_agrees_with_the_ten_line_walk(oracle, family):
    for b in C.bindings(family):
        plen = C.pattern_length(b.pattern, b.flags)
        cs = compile_class_sequence(b.pattern, False) if b.flags & C.REGEX else None
        pat = b.pattern.lower() if b.flags & C.ICASE else b.pattern
        total = 0
        for name, c in b.chunks:
            if b.flags & C.ICASE:
                c = oracle.lower(c)
            d = c.tobytes()
            occ = C.all_occurrences(c, b.pattern, b.flags).tolist()
            m, ml = walk(d, occ, plen, False), walk(d, occ, plen, True)
            ls = [line_start(d, x) for x in ml]
            total += len(m)
            assert m or name in NOTHING_TO_REPORT, (b.name, name)
            if cs is not None:  # (a class sequence has no lossy tail)
                got = (oracle.regex_byte_offsets_match(c, cs, False).tolist(), oracle.regex_byte_offsets_match(c, cs, True).tolist(),
                       oracle.regex_byte_offsets_line(c, cs).tolist())
                assert got == (m, ml, ls), (b.name, name)
                continue
            oracle.set_exact(True)
            try:
                got = (oracle.byte_offsets_match(c, pat, False).tolist(), oracle.byte_offsets_match(c, pat, True).tolist(),
                       oracle.byte_offsets_line(c, pat).tolist())
            finally:
                oracle.set_exact(False)
            assert got == (m, ml, ls), (b.name, name, "exact")
            # the reference's own end of chunk is lossy in its last plen + 31 bytes: below that zone the same walk
            Z = C.tail_zone_begin(len(d), plen, 0)
            for lines, mine in ((False, m), (True, ml)):
                theirs = oracle.byte_offsets_match(c, pat, lines).tolist()
                assert [x for x in theirs if x < Z] == [x for x in mine if x < Z], (b.name, name, "lossy", lines)
        assert total >= 1, b.name  # every binding has something to report


def test_verify_cases_are_honest(oracle):
    from gpu_util import oracle_regex_all_modes
    for b in C.bindings("verify"):
        assert xsg.regex_prefix(b.pattern)[0] >= 3, b.pattern
        want, with_lines = oracle_regex_all_modes(oracle, C.blocks_of(b), b.pattern, False)
        assert with_lines and want["count_matches"] >= 1 and want["count_lines"] >= 1, b.name
    _, _, per = labels("verify")
    for expr in (b"xaa+", b"xaa+y", b"aaa+b?"):  # every expression on both sides of its budget, and with the chunk's end at and one behind it
        got = set().union(*(v for (name, _, _), v in per.items() if name.startswith(f"verify {expr.decode()}")))
        assert got >= set(VERIFY[:6]), (expr, sorted(got))


def test_probe_cases_are_honest(oracle):
    """an overlap-free binding: the oracle reports every occurrence; an overlapping one: strictly fewer.  Whether the
    library may KNOW a binding to be overlap-free is the documented rule (include/xsg.h) -- at most three borders, probe
    words within XSG_MAX_PATTERN, no overlapping pair in a chunk -- which is what test_gpu_chains.py expects."""
    seen = set()
    for b in C.bindings("probe"):
        blocks = C.blocks_of(b)
        occ = sum(len(C.all_occurrences(c, b.pattern, 0)) for c in blocks)
        oracle.set_exact(True)
        try:
            exact = sum(oracle.count(c, b.pattern, False) for c in blocks)
        finally:
            oracle.set_exact(False)
        lossy = sum(oracle.count(c, b.pattern, False) for c in blocks)
        assert lossy >= 1, b.name
        data = b.name.split(": ")[1]
        if data in ("no pair", "pair across a seam"):
            assert not C.overlaps_in_data(blocks, b.pattern, 0) and exact == occ, b.name
            assert C.known_overlap_free(blocks, b.pattern, 0) == (b.pattern in (b"aXa", b"abaXaba", b"aaaa", b"abacabadabacaba")), b.name
        else:
            assert C.overlaps_in_data(blocks, b.pattern, 0) and exact < occ and lossy < occ, b.name
            assert not C.known_overlap_free(blocks, b.pattern, 0)
        if data == "pair in the tail zone":  # the pair's second occurrence starts inside the last plen + 31 bytes
            c = blocks[1]
            assert C.all_occurrences(c, b.pattern, 0)[-1] >= C.tail_zone_begin(len(c), len(b.pattern), 0), b.name
        seen.add((b.pattern[:8], data))
    assert len(seen) == 6 * len(C.PROBE_DATA)
