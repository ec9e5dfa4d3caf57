"""XSG_FLAG_CONTEXT restated without a GPU (include/xsg.h): the results with context lines as the plain oracle results
plus interval arithmetic over the line starts of every chunk.  The plain results come from the existing oracle calls
(gpu_util.oracle_*_all_modes, anchor_oracle.all_modes) or, under XSG_FLAG_INVERT, from invert_model; nothing here
searches."""
import numpy as np

import invert_model

NONE = (1 << 64) - 1  # xsg_context_edge.first / .last of a chunk that reports nothing
PASS_THROUGH = ("count_matches", "count_lines", "match_byte_offsets", "newlines", "bytes")  # tags that ignore the bits


def chunk_context(n: int, reported: list[int], before: int, after: int) -> list[int]:
    """C = { q : 0 <= q < n and some r in R has r - before <= q <= r + after }, ascending, by merging intervals"""
    out, nxt = [], 0
    for r in sorted(reported):
        lo, hi = max(r - before, nxt), min(r + after, n - 1)
        out.extend(range(lo, hi + 1))
        nxt = max(nxt, hi + 1)
    return out


def _per_chunk(plain: dict, blocks, global_offsets=None):
    """-> per chunk (uint8 array, global offset, line starts, indices of the reported lines among them)"""
    reported = [int(x) for x in plain["line_byte_offsets"]]
    assert len(set(reported)) == len(reported), "a line start is reported twice"
    left, goff, out = set(reported), 0, []
    for i, b in enumerate(blocks):
        b = np.asarray(b, dtype=np.uint8)
        g = goff if global_offsets is None else int(global_offsets[i])
        starts = invert_model.lines(b)
        idx = [k for k, s in enumerate(starts) if g + s in left]
        left.difference_update(g + starts[k] for k in idx)
        out.append((b, g, starts, idx))
        goff += int(b.size)
    assert not left, "the oracle reports a start that is not a line start of its chunk (or global ranges overlap)"
    return out


def context_all_modes(plain: dict, blocks, before: int, after: int, global_offsets=None, line_bases=None) -> dict:
    """plain: a dict of `blocks` with the same global offsets and line bases and the same flags but the context bits.
    -> the dict XSG_FLAG_CONTEXT(before, after) must produce: line_byte_offsets, line_indices, lines, lines_offsets, and
    everything that ignores the bits as it was.  The chunks' global ranges must not overlap."""
    out = {"line_byte_offsets": [], "line_indices": [], "lines": [], "lines_offsets": []}
    for k in PASS_THROUGH:
        if k in plain:
            out[k] = plain[k]
    nl_before = 0
    for i, (b, g, starts, idx) in enumerate(_per_chunk(plain, blocks, global_offsets)):
        lb = nl_before if line_bases is None else int(line_bases[i])
        nl_pos = np.flatnonzero(b == 10)
        for q in chunk_context(len(starts), idx, before, after):
            s = starts[q]
            out["line_byte_offsets"].append(g + s)
            out["line_indices"].append(lb + q)  # (q newlines lie before line q)
            if q < nl_pos.size:  # terminated: a last line without its newline is never handed out
                out["lines"].append(b[s:int(nl_pos[q])].tobytes())
                out["lines_offsets"].append(g + s)
        nl_before += int(nl_pos.size)
    return out


def edges(plain: dict, blocks, before: int, after: int, global_offsets=None) -> list[tuple]:
    """-> per chunk (lines, first, last, open_before, open_after): what xsg_result_context_edges must hand out"""
    out = []
    for b, g, starts, idx in _per_chunk(plain, blocks, global_offsets):
        n = len(starts)
        c = chunk_context(n, idx, before, after)
        if not idx:
            out.append((n, NONE, NONE, 0, 0))
        else:
            out.append((n, c[0], c[-1], max(0, before - idx[0]), max(0, after - (n - 1 - idx[-1]))))
    return out


def whole_file(plain: dict, chunks, before: int, after: int) -> dict:
    """A job's result: the context of the whole searched range, whatever the chunks (consecutive pieces of one file, each
    searched on its own: `plain` is their chunk-wise oracle dict with running offsets and line bases).  Lines are cut at
    '\\n' only, so the pieces must end in one (the file's last may not)."""
    assert all(np.asarray(c).size and np.asarray(c)[-1] == 10 for c in chunks[:-1]), "a chunk does not end in a newline"
    return context_all_modes(plain, [np.concatenate([np.asarray(c, dtype=np.uint8) for c in chunks])], before, after)


def job_refuses(plain: dict, chunks, before: int, after: int) -> bool:
    """the one-neighbour rule of the file pipeline (x-search_amd/csrc/xsg_context.h), from the edges"""
    e = edges(plain, chunks, before, after)
    for k in range(1, len(e)):
        if e[k][3] > e[k - 1][0] and k - 1 != 0:
            return True
        if e[k - 1][4] > e[k][0] and k + 1 != len(e):
            return True
    return False
