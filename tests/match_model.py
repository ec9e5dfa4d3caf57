"""XSG_MATCHES restated without a GPU (include/xsg.h): the existing oracle's match list plus a length.

Nothing here searches on its own.  The starts are what the oracle reports for XSG_MATCH_BYTE_OFFSETS; the length is the
pattern's for a literal, the number of positions for a class sequence, and the end of the oracle's own regex match on the
automaton route and for the (?m) forms -- there the walk of oracle/xs_oracle.py: Oracle.rx_byte_offsets / of
anchor_oracle.AnchorProgram.match_starts is repeated recording the ends, and its starts are asserted equal to what
that function returns, so the model cannot drift from the oracle."""
import numpy as np

import anchor_oracle
import xsg
from gpu_util import oracle_all_modes, oracle_regex_all_modes
from xs_oracle import RegexProgram, UnsupportedRegex, compile_class_sequence


def _bytes(block) -> bytes:
    return block if isinstance(block, bytes) else np.asarray(block, dtype=np.uint8).tobytes()


def chunk_spans(oracle, block, pat: bytes, flags: int = 0):
    """-> [(start, len)] of one chunk, chunk-relative, in the order of XSG_MATCH_BYTE_OFFSETS"""
    icase = bool(flags & xsg.FLAG_IGNORE_CASE)
    b = np.frombuffer(_bytes(block), dtype=np.uint8)
    d = _bytes(block)
    if not flags & xsg.FLAG_REGEX:
        want = oracle_all_modes(oracle, [b], pat, exact=bool(flags & xsg.FLAG_EXACT_TAIL), ignore_case=icase)
        return [(int(s), len(pat)) for s in want["match_byte_offsets"]]
    if pat.startswith(b"(?m)"):
        prog = anchor_oracle.AnchorProgram(pat, icase)
        if prog.ascii_only and any(x >= 0x80 for x in d):
            raise UnsupportedRegex("ascii-only expression on non-ASCII data")
        out, r = [], 0
        while True:
            m = prog._search(d, r)
            if m is None:
                break
            out.append((m[0], m[1] - m[0]))
            r = m[1]
        assert [s for s, _ in out] == prog.match_starts(d), "the model's walk left the oracle's"
        return out
    try:
        compile_class_sequence(pat, icase)
        fixed = True
    except UnsupportedRegex:
        fixed = False
    if fixed:
        positions, _ = xsg.regex_check(pat, xsg.FLAG_IGNORE_CASE if icase else 0)
        assert positions > 0
        want, _ = oracle_regex_all_modes(oracle, [b], pat, icase)
        return [(int(s), positions) for s in want["match_byte_offsets"]]
    prog = RegexProgram(pat, icase)
    starts = [int(x) for x in oracle.rx_byte_offsets(b, prog, False)]  # (raises for an ascii-only expression on other data)
    out, pos = [], 0
    while True:
        m = prog.re.search(d, pos)
        if m is None:
            break
        out.append((m.start(), m.end() - m.start()))
        pos = m.end()
    assert [s for s, _ in out] == starts, "the model's walk left the oracle's"
    return out


def matches(oracle, blocks, pat: bytes, flags: int = 0, global_offsets=None):
    """-> (strings, global offsets, lengths) over the chunks in order: what Shard.search_matches() must hand out"""
    strings, offsets, lengths = [], [], []
    goff = 0
    for i, blk in enumerate(blocks):
        d = _bytes(blk)
        g = goff if global_offsets is None else int(global_offsets[i])
        for s, n in chunk_spans(oracle, blk, pat, flags):
            assert n > 0 and s + n <= len(d)
            strings.append(d[s:s + n])
            offsets.append(g + s)
            lengths.append(n)
        goff += len(d)
    return strings, offsets, lengths
