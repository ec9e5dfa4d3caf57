"""The CPU oracle for ONE pattern of any kind on a list of blocks: the dispatch the per-chunk and per-file tests share
(tests/test_gpu_chunk_rows.py, tests/test_gpu_fileset*.py).  Nothing here searches on its own: gpu_util.oracle_*_all_modes,
anchor_oracle, set_model, all_of_model and match_model do, invert_model and context_model build on their results.

kind: "lit" / "nl" (a literal; one that holds a newline), "rx" (XSG_FLAG_REGEX), "anchor" ((?m) forms), "anyof" / "allof"
(a tuple of literals)."""
import all_of_model
import anchor_oracle
import context_model
import invert_model
import match_model
import set_model
import xsg
from gpu_util import oracle_all_modes, oracle_regex_all_modes

X, IC, RX, INV = xsg.FLAG_EXACT_TAIL, xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX, xsg.FLAG_INVERT
CTX = xsg.flag_context(1, 2)


def chunk_plain(oracle, kind, pat, pflags, flags, b, g, lb):
    """the oracle's dict for a binding of this chunk alone, context bits aside (under INVERT: the complement)"""
    icase = bool(flags & IC)
    if kind in ("lit", "nl"):
        want = oracle_all_modes(oracle, [b], pat, exact=bool(flags & X), global_offsets=[g], line_bases=[lb], ignore_case=icase)
    elif kind == "anchor":
        want = anchor_oracle.all_modes([b], pat, icase, global_offsets=[g], line_bases=[lb])
    elif kind == "rx":
        want, with_lines = oracle_regex_all_modes(oracle, [b], pat, icase, global_offsets=[g], line_bases=[lb])
        assert with_lines
    elif kind == "anyof":
        want = set_model.all_modes([b], list(pat), icase, global_offsets=[g], line_bases=[lb])
    else:
        return all_of_model.all_modes([b], list(pat), icase, False, bool(flags & INV), global_offsets=[g], line_bases=[lb])
    if flags & INV:
        want = invert_model.invert_all_modes(want, [b], [g], [lb])
    return want


def chunk_matches(oracle, kind, pat, pflags, flags, b, g):
    """-> (strings, offsets) of XSG_MATCHES for this chunk alone"""
    if kind == "anyof":
        s, o, _ = set_model.matches([b], list(pat), bool(flags & IC), [g])
        return s, o
    s, o, _ = match_model.matches(oracle, [b], pat, pflags | (flags & (X | IC)), [g])
    return s, o


def file_results(oracle, kind, pat, pflags, flags, blocks):
    """What a search of ONE file reports whose chunks are `blocks` (consecutive pieces, all but the last ending in a
    newline; a file searched as one chunk is a list of one): offsets relative to the file, line indices from 0, context
    (CTX: one line before, two after) over the whole file.  -> dict of the seven tags; "lines" / "matches" hold bytes."""
    icase = bool(flags & IC)
    if kind in ("lit", "nl"):
        want = oracle_all_modes(oracle, blocks, pat, exact=bool(flags & X), ignore_case=icase)
    elif kind == "anchor":
        want = anchor_oracle.all_modes(blocks, pat, icase)
    elif kind == "rx":
        want, with_lines = oracle_regex_all_modes(oracle, blocks, pat, icase)
        assert with_lines
    elif kind == "anyof":
        want = set_model.all_modes(blocks, list(pat), icase)
    else:
        want = all_of_model.all_modes(blocks, list(pat), icase, False, bool(flags & INV))
    if flags & INV and kind != "allof":
        want = invert_model.invert_all_modes(want, blocks)
    if flags & CTX:
        want = {**want, **context_model.whole_file(want, blocks, 1, 2)}
    out = {"count_lines": want["count_lines"], "line_byte_offsets": [int(x) for x in want["line_byte_offsets"]],
           "line_indices": [int(x) for x in want["line_indices"]], "lines": list(want["lines"])}
    if kind != "allof" and not flags & INV:
        out["count_matches"] = want["count_matches"]
        out["match_byte_offsets"] = [int(x) for x in want["match_byte_offsets"]]
        if kind == "anyof":
            out["matches"] = set_model.matches(blocks, list(pat), icase)[0]
        else:
            out["matches"] = match_model.matches(oracle, blocks, pat, pflags | (flags & (X | IC)))[0]
    return out
