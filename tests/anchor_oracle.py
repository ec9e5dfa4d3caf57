"""The reference's walks restated for line-anchored expressions, (?m) [^] BODY [$] (include/xsg.h, XSG_FLAG_REGEX;
DESIGN.md 4a "Line anchors").

RE2's PartialMatch runs on the re-sliced input d[r:], so under (?m) `^` holds at the resume point r as well as after
every '\\n', and `$` before every '\\n' and at the chunk's end.  CPython's re.M on memoryview(d)[r:] computes the same;
pattern.search(d, r) does NOT (it does not treat r as a line start), so every walk here slices.

BODY's CPython source comes from the oracle's own reader (oracle/xs_oracle.py: RegexProgram), which emits explicit
byte classes (closed under case for ignore_case), so the wrapped pattern is compiled with re.M | re.S.
"""
import re

import numpy as np

from xs_oracle import RegexProgram, UnsupportedRegex


def split(expr: bytes):
    """-> (BODY, anchor_begin, anchor_end) of the served form; an expression without a leading (?m) is its own BODY"""
    if not expr.startswith(b"(?m)"):
        return expr, False, False
    body, bol, eol = expr[4:], False, False
    if body.startswith(b"^"):
        body, bol = body[1:], True
    if body.endswith(b"$"):
        k = len(body) - 1
        while k > 0 and body[k - 1:k] == b"\\":
            k -= 1
        if (len(body) - 1 - k) % 2 == 0:
            body, eol = body[:-1], True
    return body, bol, eol


class AnchorProgram:
    def __init__(self, expr: bytes, ignore_case: bool = False):
        body, self.bol, self.eol = split(bytes(expr))
        if not body:
            raise UnsupportedRegex("empty body")
        prog = RegexProgram(body, ignore_case)
        if prog.multiline:
            raise UnsupportedRegex("a body that spans lines")
        src = b"(?:" + prog.source + b")"
        if self.bol:
            src = b"^" + src
        if self.eol:
            src = src + b"$"
        self.re = re.compile(src, re.M | re.S)
        self.ascii_only = prog.ascii_only

    def _search(self, d: bytes, r: int):
        m = self.re.search(memoryview(d)[r:])
        return None if m is None else (r + m.start(), r + m.end())

    def match_starts(self, d: bytes):
        """the match tags' walk: resume at the end of each match"""
        out, r = [], 0
        while True:
            m = self._search(d, r)
            if m is None:
                return out
            out.append(m[0])
            r = m[1]

    def line_walk(self, d: bytes):
        """the line tags' walk (regex::count / byte_offsets_line): resume behind the next '\\n' at or after the end of
        each match, stop if there is none -> the match starts"""
        out, r = [], 0
        while True:
            m = self._search(d, r)
            if m is None:
                return out
            out.append(m[0])
            nl = d.find(b"\n", m[1])
            if nl < 0:
                return out
            r = nl + 1

    def lines_spans(self, d: bytes):
        """xs::lines: the `line` walk, which drops a final line without its '\\n'"""
        beg, ln, r = [], [], 0
        while r < len(d):
            m = self._search(d, r)
            if m is None:
                break
            b = d.rfind(b"\n", 0, m[0]) + 1
            e = d.find(b"\n", m[1])
            if e < 0:
                break
            r = e + 1
            beg.append(b)
            ln.append(e - b)
        return beg, ln


def all_modes(blocks, expr: bytes, ignore_case=False, global_offsets=None, line_bases=None):
    """the dict of tests/gpu_util.py: oracle_regex_all_modes (all six tags), chunk by chunk"""
    prog = AnchorProgram(expr, ignore_case)
    out = {"count_matches": 0, "newlines": 0, "bytes": 0, "match_byte_offsets": [], "count_lines": 0,
           "line_byte_offsets": [], "line_indices": [], "lines": [], "lines_offsets": []}
    goff, nl_before = 0, 0
    for i, blk in enumerate(blocks):
        d = bytes(np.asarray(blk, dtype=np.uint8).tobytes()) if not isinstance(blk, bytes) else blk
        if prog.ascii_only and any(b >= 0x80 for b in d):
            raise UnsupportedRegex("ascii-only expression on non-ASCII data")
        g = goff if global_offsets is None else int(global_offsets[i])
        lb = nl_before if line_bases is None else int(line_bases[i])
        ms = prog.match_starts(d)
        out["count_matches"] += len(ms)
        out["match_byte_offsets"] += [s + g for s in ms]
        ls = prog.line_walk(d)
        out["count_lines"] += len(ls)
        starts = [d.rfind(b"\n", 0, s) + 1 for s in ls]
        out["line_byte_offsets"] += [s + g for s in starts]
        out["line_indices"] += [lb + d.count(b"\n", 0, s) for s in starts]
        beg, ln = prog.lines_spans(d)
        out["lines"] += [d[b:b + n] for b, n in zip(beg, ln)]
        out["lines_offsets"] += [b + g for b in beg]
        nl = d.count(b"\n")
        out["newlines"] += nl
        out["bytes"] += len(d)
        goff += len(d)
        nl_before += nl
    return out
