"""Line anchors, (?m) [^] BODY [$], without a GPU: what XSG_FLAG_REGEX accepts and refuses (xsg_regex_check /
xsg_regex_info), and the restated walks of tests/anchor_oracle.py against known answers and a per-line brute force."""
import numpy as np
import pytest

import anchor_oracle
import corpus
import xsg

CLASS_ROUTE = [b"(?m)^Sherlock", b"(?m)^She[r ]lock", b"(?m)Holmes[.,]$", b"(?m)^[A-Z][a-z]{3}$", b"(?m)^(?:ab|cd)",
               b"(?m)abc", b"(?m)^ab", b"(?m)ab$", b"(?m)^aa", b"(?m)^a[ab]{12}", b"(?m)a[ab]{12}$",
               b"(?m)^a[ab]{12}$"]
AUTOMATON_ROUTE = [b"(?m)^Sher.*mes", b"(?m)^\\w+ing", b"(?m)colou?r$", b"(?m)\\w+ing$", b"(?m)^[A-Z][a-z]+ [A-Z][a-z]+$",
                   b"(?m)^a{40}", b"(?m)^a+?$", b"(?m)^a+", b"(?m)[a-z]+ing$", b"(?m)^[A-Z][a-z]+$"]
REFUSED = [b"^ab", b"ab$", b"\\bab", b"\\Bab", b"\\Aab", b"ab\\z", b"(?i)ab", b"(?m)a^b", b"(?m)a$b", b"(?m)(^a)",
           b"(?m)^a|b", b"(?m)^a|^b", b"a(?m)^b", b"(?m:^a)", b"(?mi)^a", b"(?s)a", b"(?m)^$", b"(?m)^a*$", b"(?m)^",
           b"(?m)$", b"(?m)^a\\s+b", b"(?m)^[^,]+$", b"(?m)^^a", b"(?m)^a$$"]


@pytest.mark.parametrize("icase", [False, True])
@pytest.mark.parametrize("expr", CLASS_ROUTE)
def test_served_fixed_length_forms_report_their_body(expr, icase):
    flags = xsg.FLAG_IGNORE_CASE if icase else 0
    body, _, _ = anchor_oracle.split(expr)
    n, sets = xsg.regex_check(expr, flags)
    nb, bsets = xsg.regex_check(body, flags)
    assert n == nb and n > 0 and np.array_equal(sets, bsets)
    info, binfo = xsg.regex_info(expr, flags), xsg.regex_info(body, flags)
    assert info[:3] == binfo[:3] and np.array_equal(info[3], binfo[3])


@pytest.mark.parametrize("icase", [False, True])
@pytest.mark.parametrize("expr", AUTOMATON_ROUTE)
def test_served_variable_length_forms_report_no_positions(expr, icase):
    flags = xsg.FLAG_IGNORE_CASE if icase else 0
    assert xsg.regex_check(expr, flags)[0] == 0
    assert xsg.regex_info(expr, flags)[:2] == (0, 0)


@pytest.mark.parametrize("expr", REFUSED)
def test_refused_forms(expr):
    for flags in (0, xsg.FLAG_IGNORE_CASE):
        with pytest.raises(xsg.XsgError, match="not supported"):
            xsg.regex_check(expr, flags)
        with pytest.raises(xsg.XsgError, match="not supported"):
            xsg.regex_info(expr, flags)


def test_escaped_dollar_is_a_literal():
    assert xsg.regex_check(b"(?m)^a\\$")[0] == 2
    assert anchor_oracle.split(b"(?m)^a\\$") == (b"a\\$", True, False)
    assert anchor_oracle.split(b"(?m)^a\\\\$") == (b"a\\\\", True, True)


KNOWN = [  # expression, chunk, match-tag offsets, line-walk match starts
    (b"(?m)^ab", b"abab\nxab\nab", [0, 2, 9], [0, 9]),
    (b"(?m)^ab", b"xxab", [], []),
    (b"(?m)ab$", b"abab\nab", [2, 5], [2, 5]),
    (b"(?m)ab$", b"abyy\n", [], []),
    (b"(?m)^aa", b"aaaaa\n", [0, 2], [0]),
    (b"(?m)^(?:ab|cd)", b"abcdab cd\ncd\n", [0, 2, 4, 10], [0, 10]),
    (b"(?m)^a+", b"aaab aa\n", [0], [0]),
    (b"(?m)^[A-Z][a-z]+$", b"Holmes\nHolmes.\nWatson", [0, 15], [0, 15]),
    (b"(?m)[a-z]+ing$", b"king sing\nringing\n", [5, 10], [5, 10]),
]


@pytest.mark.parametrize("expr,chunk,matches,walk", KNOWN)
def test_known_answers(expr, chunk, matches, walk):
    prog = anchor_oracle.AnchorProgram(expr)
    assert prog.match_starts(chunk) == matches
    assert prog.line_walk(chunk) == walk
    got = anchor_oracle.all_modes([np.frombuffer(chunk, dtype=np.uint8)], expr)
    assert got["match_byte_offsets"] == matches and got["count_matches"] == len(matches)
    assert got["count_lines"] == len(walk)


def test_lines_keeps_only_terminated_lines():
    got = anchor_oracle.all_modes([np.frombuffer(b"Holmes\nHolmes.\nWatson", dtype=np.uint8)], b"(?m)^[A-Z][a-z]+$")
    assert got["lines"] == [b"Holmes"] and got["lines_offsets"] == [0]
    assert got["line_byte_offsets"] == [0, 15] and got["line_indices"] == [0, 2]


def test_search_from_an_offset_is_not_the_reference_walk():
    """why the oracle slices: CPython does not treat the `pos` of search() as a line start"""
    import re
    assert re.compile(rb"^ab", re.M).search(b"xxab\nab", 2).start() == 5
    assert anchor_oracle.AnchorProgram(b"(?m)^ab").match_starts(b"xxab\nab"[2:]) == [0, 3]


# fixed-length BODYs over {a, b}: the sets per position, for the brute force
BODIES = {b"ab": [b"a", b"b"], b"a[ab]": [b"a", b"ab"], b"aa": [b"a", b"a"], b"[ab]b": [b"ab", b"b"],
          b"(?:ab|ba)": None, b"aba": [b"a", b"b", b"a"]}


def _matches_at(line: np.ndarray, body: bytes) -> np.ndarray:
    """positions p of `line` at which the fixed-length BODY matches line[p:p+L] (numpy, no regex)"""
    if body == b"(?:ab|ba)":
        if line.size < 2:
            return np.zeros(0, dtype=bool)
        a, b = line[:-1], line[1:]
        return ((a == 97) & (b == 98)) | ((a == 98) & (b == 97))
    sets = BODIES[body]
    L = len(sets)
    if line.size < L:
        return np.zeros(0, dtype=bool)
    ok = np.ones(line.size - L + 1, dtype=bool)
    for k, st in enumerate(sets):
        ok &= np.isin(line[k:line.size - L + 1 + k], np.frombuffer(st, dtype=np.uint8))
    return ok


def _brute(d: np.ndarray, body: bytes, bol: bool, eol: bool):
    """-> (match-tag starts, line-walk starts), line by line; the chunk's edges are line edges"""
    L = 3 if body == b"aba" else 2
    nl = np.flatnonzero(d == 10)
    starts = np.concatenate([[0], nl + 1])
    ends = np.concatenate([nl, [d.size]])
    m_out, l_out = [], []
    for s, e in zip(starts.tolist(), ends.tolist()):
        ok = _matches_at(d[s:e], body)
        if bol and eol:
            hits = [s] if e - s == L and ok.size and ok[0] else []
        elif bol:
            hits, p = [], s
            while p - s < ok.size and ok[p - s]:
                hits.append(p)
                p += L
        elif eol:
            hits = [e - L] if ok.size and ok[-1] else []
        else:
            raise AssertionError
        m_out += hits
        l_out += hits[:1]
    return m_out, l_out


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("anchors", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("body", list(BODIES))
def test_oracle_equals_a_per_line_brute_force(body, anchors, seed):
    bol, eol = anchors
    expr = b"(?m)" + (b"^" if bol else b"") + body + (b"$" if eol else b"")
    d = corpus.small_alphabet(seed * 31 + len(body), 3000)
    prog = anchor_oracle.AnchorProgram(expr)
    want_m, want_l = _brute(d, body, bol, eol)
    raw = d.tobytes()
    assert prog.match_starts(raw) == want_m
    assert prog.line_walk(raw) == want_l


def test_the_anchored_forms_are_new():
    """on the code before line anchors every (?m) form was refused"""
    for expr in CLASS_ROUTE + AUTOMATON_ROUTE:
        xsg.regex_check(expr)


def _dollar_walk(expr: bytes, d: bytes, flags: int = 0):
    """the line walk of a `$`-only form as k_rx_count / k_rx_scan run it (csrc/xsg_rx_kernels.hip: rx_walk_line), on
    the reverse automaton xsg_regex_dfa_info hands out: per line, back from its end to its start, the last accepting
    position is the match's start"""
    info, fwd, rev = xsg.regex_dfa(expr, flags)
    assert fwd.size == 0  # the unanchored automaton is not built for the line-anchor form
    ncls, cls = info.ncls, info.class_of
    flat = rev.reshape(-1)
    out, cur = [], 0
    while cur <= len(d):
        e = d.find(b"\n", cur)
        e = len(d) if e < 0 else e
        rs, start = info.rev_start * ncls, None
        for r in range(e, cur, -1):
            rs = int(flat[rs + cls[d[r - 1]]])
            if rs == 0:
                break
            if rs >= info.rev_first_acc * ncls:
                start = r - 1
        if start is not None:
            out.append(start)
        cur = e + 1
    return out


@pytest.mark.parametrize("expr", [b"(?m)ab$", b"(?m)a+?$", b"(?m)a[ab]{12}$", b"(?m)(?:ab|b)a$", b"(?m)[ab]b+$",
                                  b"(?m)(?:a|ab)b?b$"])
def test_dollar_walk_on_the_reverse_automaton_equals_the_oracle(expr):
    prog = anchor_oracle.AnchorProgram(expr)
    for seed in range(4):
        d = corpus.small_alphabet(seed + 100, 4000, alphabet=b"ab\n" + b"ab" * (2 + 2 * seed)).tobytes()
        want = prog.match_starts(d)
        assert _dollar_walk(expr, d) == want
        assert prog.line_walk(d) == want  # a line has one match at most
