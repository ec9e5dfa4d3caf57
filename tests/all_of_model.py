"""A literal list under XSG_LIST_ALL_OF (include/xsg.h) restated without a GPU: the definition in a few lines.

The lines of a chunk are those defined under XSG_FLAG_INVERT: the chunk split at its newlines, a last line without a
newline included, nothing behind a final newline.  A line is SELECTED iff for every literal of the list at least one
occurrence of it starts in the line -- both sides ASCII-lowered under ignore-case, and under XSG_LIST_WHOLE_WORDS only
occurrences that are admissible IN THE CHUNK (words_model.admissible: the chunk's edges are word boundaries, a line's edge
is a newline, which is no word byte).  all_modes builds from the selected lines what set_model.all_modes builds from its
line walk for the line tags; the match tags are refused for such a list and have no entry here.  Context lines are
context_model's interval arithmetic over this dict, as for every other search."""
import set_model
import words_model


def chunk_lines(d: bytes):
    """[(start, end, terminated)] of the chunk's lines; end excludes the newline"""
    out, at = [], 0
    while at < len(d):
        nl = d.find(b"\n", at)
        if nl < 0:
            out.append((at, len(d), False))
            break
        out.append((at, nl, True))
        at = nl + 1
    return out


def occurs(d: bytes, folded: bytes, needle: bytes, lo: int, hi: int, words: bool) -> bool:
    """an occurrence of needle starts in [lo, hi) of the chunk and ends there (a literal holds no newline)"""
    at = folded.find(needle, lo, hi)
    while at >= 0:
        if not words or words_model.admissible(d, at, len(needle)):
            return True
        at = folded.find(needle, at + 1, hi)
    return False


def selected(block, literals, icase=False, words=False, invert=False):
    """[(start, end, terminated)] of the selected lines of one chunk (invert: of the others)"""
    d = set_model._bytes(block)
    folded = d.lower() if icase else d
    needles = [(l.lower() if icase else l) for l in literals]
    for n in needles:
        assert n and b"\n" not in n
    return [ln for ln in chunk_lines(d)
            if all(occurs(d, folded, n, ln[0], ln[1], words) for n in needles) != invert]


def all_modes(blocks, literals, icase=False, words=False, invert=False, global_offsets=None, line_bases=None):
    """the line tags of set_model.all_modes's dict, plus the count per chunk (xsg_count_chunks)"""
    out = {"count_lines": 0, "line_byte_offsets": [], "line_indices": [], "lines": [], "lines_offsets": [],
           "chunk_counts": [], "newlines": 0, "bytes": 0}
    goff, nl_before = 0, 0
    for i, blk in enumerate(blocks):
        d = set_model._bytes(blk)
        g = goff if global_offsets is None else int(global_offsets[i])
        lb = nl_before if line_bases is None else int(line_bases[i])
        sel = selected(d, literals, icase, words, invert)
        out["count_lines"] += len(sel)
        out["chunk_counts"].append(len(sel))
        out["line_byte_offsets"] += [g + b for b, _, _ in sel]
        out["line_indices"] += [lb + d.count(b"\n", 0, b) for b, _, _ in sel]
        out["lines"] += [d[b:e] for b, e, t in sel if t]  # (xs::lines: a line without its newline is not reported)
        out["lines_offsets"] += [g + b for b, _, t in sel if t]
        nl = d.count(b"\n")
        out["newlines"] += nl
        out["bytes"] += len(d)
        goff += len(d)
        nl_before += nl
    return out

