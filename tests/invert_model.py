"""XSG_FLAG_INVERT restated without a GPU (include/xsg.h): the lines of a chunk, and the inverted results as the plain
oracle results plus one set difference.  The plain results come from the existing oracle calls (gpu_util.oracle_*_all_modes
or anchor_oracle.all_modes); nothing here searches."""
import numpy as np


def lines(chunk) -> list[int]:
    """Line starts of a chunk of `len` bytes: 0 if len > 0, and p + 1 for every '\\n' at p with p + 1 < len."""
    b = np.frombuffer(bytes(chunk), dtype=np.uint8) if isinstance(chunk, (bytes, bytearray)) else np.asarray(chunk, dtype=np.uint8)
    if b.size == 0:
        return []
    s = np.flatnonzero(b == 10) + 1
    return [0] + [int(x) for x in s[s < b.size]]


def line_end(b: np.ndarray, start: int):
    """offset of the '\\n' that terminates the line starting at `start`, or None (the chunk's last line lacks it)"""
    nl = np.flatnonzero(b[start:] == 10)
    return start + int(nl[0]) if nl.size else None


def invert_all_modes(plain: dict, blocks, global_offsets=None, line_bases=None) -> dict:
    """plain: an oracle_*_all_modes dict of `blocks` (same global offsets and line bases, no XSG_FLAG_INVERT).
    -> the dict XSG_FLAG_INVERT must produce: count_lines, line_byte_offsets, line_indices, lines, lines_offsets
    (and newlines / bytes as they were).  The chunks' global ranges must not overlap (R is told apart by offset)."""
    reported = set(int(x) for x in plain["line_byte_offsets"])
    assert len(reported) == len(plain["line_byte_offsets"]), "a line start is reported twice"
    out = {"count_lines": 0, "line_byte_offsets": [], "line_indices": [], "lines": [], "lines_offsets": []}
    for k in ("newlines", "bytes"):
        if k in plain:
            out[k] = plain[k]
    goff, nl_before, seen, covered = 0, 0, 0, []
    for i, b in enumerate(blocks):
        b = np.asarray(b, dtype=np.uint8)
        g = goff if global_offsets is None else int(global_offsets[i])
        lb = nl_before if line_bases is None else int(line_bases[i])
        assert all(g + b.size <= lo or hi <= g for lo, hi in covered if b.size and hi > lo), "global ranges overlap"
        covered.append((g, g + int(b.size)))
        nl_pos = np.flatnonzero(b == 10)
        for s in lines(b):
            if g + s in reported:
                seen += 1
                continue
            out["count_lines"] += 1
            out["line_byte_offsets"].append(g + s)
            k = int(np.searchsorted(nl_pos, s, side="left"))  # newlines before the line = index of the one that ends it
            out["line_indices"].append(lb + k)
            if k < nl_pos.size:  # terminated: the reference never hands out a last line without its newline
                out["lines"].append(b[s:int(nl_pos[k])].tobytes())
                out["lines_offsets"].append(g + s)
        goff += int(b.size)
        nl_before += int(nl_pos.size)
    assert seen == len(reported), "the oracle reports a start that is not a line start of its chunk"
    return out


def properties(plain: dict, blocks, global_offsets=None) -> None:
    """The three facts the complement rests on: every reported start is a line start, none is reported twice, and the
    line count is the length of the line list."""
    r = [int(x) for x in plain["line_byte_offsets"]]
    assert len(set(r)) == len(r), "a line start is reported twice"
    all_starts, goff = set(), 0
    for i, b in enumerate(blocks):
        g = goff if global_offsets is None else int(global_offsets[i])
        all_starts.update(g + s for s in lines(b))
        goff += int(np.asarray(b).size)
    assert set(r) <= all_starts, "a reported start is not a line start"
    assert plain["count_lines"] == len(r), "count(skip_to_nl) != len(byte_offsets_line)"
