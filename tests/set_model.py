"""A literal list (xsg_set_literals, include/xsg.h) restated without a GPU and without a regex engine.

The search is leftmost-first in listing order: at the leftmost position at or behind the resume point where any literal
occurs, the first-listed literal that occurs there is the match, and the walk resumes at its end.  The tags are derived
from that one `search` exactly as oracle/xs_oracle.py derives them from `prog.re.search` for a variable-length
expression (Oracle.rx_byte_offsets / rx_lines_spans / rx_line_indices, the reference's walks of search_wrappers.h), so
the dict of all_modes() has the layout of gpu_util.oracle_rx_all_modes.  Literals are bytes: values >= 0x80 that are no
UTF-8, which the oracle's reader refuses, are served here.  tests/test_set_host.py pins this model to the oracle on every
list the oracle reads."""
import bisect
import string

import numpy as np

_PUNCT = frozenset(string.punctuation.encode())


def esc(lit: bytes) -> bytes:
    """backslash-escape ASCII punctuation (tools/xsgrep.cpp: re2_literal)"""
    return b"".join(b"\\" + bytes([b]) if b in _PUNCT else bytes([b]) for b in lit)


def expression(literals) -> bytes:
    """E(S) = esc(l1)|esc(l2)|...|esc(lk): the expression whose XSG_FLAG_REGEX search defines the list's"""
    return b"|".join(esc(l) for l in literals)


def _bytes(block) -> bytes:
    return block if isinstance(block, bytes) else np.asarray(block, dtype=np.uint8).tobytes()


class Occurrences:
    """every position of one chunk where a literal occurs, with the first-listed literal that occurs there"""

    def __init__(self, data, literals, icase=False):
        self.d = _bytes(data)
        d = self.d.lower() if icase else self.d  # (bytes.lower folds ASCII letters only)
        best = {}
        for idx, lit in enumerate(literals):
            assert lit and b"\n" not in lit
            needle = lit.lower() if icase else lit
            at = d.find(needle)  # every occurrence, overlapping ones included
            while at >= 0:
                best.setdefault(at, len(lit))  # (an earlier literal at the position wins: idx ascends)
                at = d.find(needle, at + 1)
        self.pos = sorted(best)
        self.len = [best[p] for p in self.pos]

    def search(self, start: int):
        """-> (begin, end) of the leftmost-first match at or behind `start`, or None"""
        k = bisect.bisect_left(self.pos, start)
        if k == len(self.pos):
            return None
        return self.pos[k], self.pos[k] + self.len[k]

    def spans(self):
        """[(start, len)] of the match walk: what XSG_MATCH_BYTE_OFFSETS / XSG_MATCHES report"""
        out, pos = [], 0
        while True:
            m = self.search(pos)
            if m is None:
                return out
            out.append((m[0], m[1] - m[0]))
            pos = m[1]

    def line_walk(self):
        """the line walk (count_lines, line_byte_offsets): [(line start, match start, match end)], first match per line;
        after a match the walk skips to behind the next newline and ends if there is none"""
        d, out, pos = self.d, [], 0
        while True:
            m = self.search(pos)
            if m is None:
                return out
            out.append((d.rfind(b"\n", 0, m[0]) + 1, m[0], m[1]))
            nl = d.find(b"\n", m[1])
            if nl < 0:
                return out
            pos = nl + 1

    def lines_spans(self):
        """xs::lines: the lines of line_walk that are terminated, (start, length without the newline)"""
        d, out = self.d, []
        for b, _, e in self.line_walk():
            nl = d.find(b"\n", e)
            if nl < 0:
                break
            out.append((b, nl - b))
        return out


def all_modes(blocks, literals, icase=False, global_offsets=None, line_bases=None):
    """the dict of gpu_util.oracle_rx_all_modes for a literal list"""
    out = {"count_matches": 0, "newlines": 0, "bytes": 0, "match_byte_offsets": [], "count_lines": 0,
           "line_byte_offsets": [], "line_indices": [], "lines": [], "lines_offsets": []}
    goff, nl_before = 0, 0
    for i, blk in enumerate(blocks):
        occ = Occurrences(blk, literals, icase)
        d = occ.d
        g = goff if global_offsets is None else int(global_offsets[i])
        lb = nl_before if line_bases is None else int(line_bases[i])
        spans = occ.spans()
        out["count_matches"] += len(spans)
        out["match_byte_offsets"] += [g + s for s, _ in spans]
        walk = occ.line_walk()
        out["count_lines"] += len(walk)
        out["line_byte_offsets"] += [g + b for b, _, _ in walk]
        # (an entry for every line of the walk, terminated or not: Oracle.rx_line_indices)
        out["line_indices"] += [lb + d.count(b"\n", 0, b) for b, _, _ in walk]
        ls = occ.lines_spans()
        out["lines"] += [d[b:b + n] for b, n in ls]
        out["lines_offsets"] += [g + b for b, _ in ls]
        nl = d.count(b"\n")
        out["newlines"] += nl
        out["bytes"] += len(d)
        goff += len(d)
        nl_before += nl
    return out


def matches(blocks, literals, icase=False, global_offsets=None):
    """-> (strings, global offsets, lengths): what Shard.search_matches() must hand out"""
    strings, offsets, lengths = [], [], []
    goff = 0
    for i, blk in enumerate(blocks):
        occ = Occurrences(blk, literals, icase)
        g = goff if global_offsets is None else int(global_offsets[i])
        for s, n in occ.spans():
            strings.append(occ.d[s:s + n])
            offsets.append(g + s)
            lengths.append(n)
        goff += len(occ.d)
    return strings, offsets, lengths
