"""xsg_set_max_count restated without a GPU (include/xsg.h): the limited results as the plain oracle results cut per chunk.
The plain results come from the existing oracle calls (gpu_util.oracle_*_all_modes, anchor_oracle, set_model, all_of_model,
match_model) or, under XSG_FLAG_INVERT, from invert_model; context_model widens what comes out of here.  The order is
oracle -> invert_model -> limit -> context_model; nothing here searches.

A dict's lists are in chunk order and a chunk's values lie in its global range, so a chunk's entries are the run at the
front of what is left that lies in [global_offset, global_offset + len): the ranges must not overlap."""
import numpy as np

LINE_KEYS = ("line_byte_offsets", "line_indices", "lines", "lines_offsets")


def _ranges(blocks, global_offsets=None):
    out, goff = [], 0
    for i, b in enumerate(blocks):
        size = int(np.asarray(b).size)
        g = goff if global_offsets is None else int(global_offsets[i])
        assert all(g + size <= lo or hi <= g for lo, hi in out if size and hi > lo), "global ranges overlap"
        out.append((g, g + size))
        goff += size
    return out


def split(values, ranges) -> list[list[int]]:
    """the indices of `values` (global offsets in chunk order) chunk by chunk"""
    out, i = [], 0
    for lo, hi in ranges:
        j = i
        while j < len(values) and lo <= int(values[j]) < hi:
            j += 1
        out.append(list(range(i, j)))
        i = j
    assert i == len(values), "a reported offset lies in no chunk, or the lists are not in chunk order"
    return out


def _terminated(plain, keep_lines) -> list[int]:
    """indices into plain["lines"] of the kept lines: lines_offsets is the subsequence of line_byte_offsets whose lines end
    in a newline, so the two are walked side by side"""
    lbo, lo = plain["line_byte_offsets"], plain["lines_offsets"]
    kept, out, k = set(keep_lines), [], 0
    for i, x in enumerate(lbo):
        if k < len(lo) and int(lo[k]) == int(x):
            if i in kept:
                out.append(k)
            k += 1
    assert k == len(lo), "lines_offsets is not a subsequence of line_byte_offsets"
    return out


def _cut(plain: dict, keep_lines, keep_matches, matches=None):
    out = {k: plain[k] for k in ("newlines", "bytes") if k in plain}
    if "line_byte_offsets" in plain:
        assert plain["count_lines"] == len(plain["line_byte_offsets"]) == len(plain["line_indices"])
        out["count_lines"] = len(keep_lines)
        out["line_byte_offsets"] = [int(plain["line_byte_offsets"][i]) for i in keep_lines]
        out["line_indices"] = [int(plain["line_indices"][i]) for i in keep_lines]
        t = _terminated(plain, keep_lines)
        out["lines"] = [plain["lines"][k] for k in t]
        out["lines_offsets"] = [int(plain["lines_offsets"][k]) for k in t]
    if keep_matches is not None:
        assert plain["count_matches"] == len(plain["match_byte_offsets"])
        out["count_matches"] = len(keep_matches)
        out["match_byte_offsets"] = [int(plain["match_byte_offsets"][i]) for i in keep_matches]
        if matches is not None:
            strings, offsets = matches[0], matches[1]
            assert [int(x) for x in offsets] == [int(x) for x in plain["match_byte_offsets"]]
            out["matches"] = [strings[i] for i in keep_matches]
            out["matches_offsets"] = [int(offsets[i]) for i in keep_matches]
    return out


def limit_all_modes(plain: dict, blocks, n: int, global_offsets=None, line_bases=None, matches=None) -> dict:
    """plain: a dict of `blocks` with the same global offsets, line bases and flags but the context bits (under
    XSG_FLAG_INVERT: invert_model's).  n: the limit, 0 = none.  matches: (strings, offsets) of XSG_MATCHES, optional.
    -> the dict xsg_set_max_count(n) must produce: every list cut to each chunk's first n entries, lines, indices and counts
    recomputed from the cut lists (an unterminated Nth line is cut in, then not handed out: n - 1 lines), and
    count_lines_chunks / count_matches_chunks = min(chunk's count, n).  line_bases is taken for the signature's symmetry
    with invert_model and context_model: the indices are selected, not recomputed."""
    r = _ranges(blocks, global_offsets)
    cap = (lambda idx: idx) if n == 0 else (lambda idx: idx[:n])
    keep_lines = keep_matches = None
    out_chunks = {}
    if "line_byte_offsets" in plain:
        per = [cap(idx) for idx in split(plain["line_byte_offsets"], r)]
        keep_lines = [i for idx in per for i in idx]
        out_chunks["count_lines_chunks"] = [len(idx) for idx in per]
    if "match_byte_offsets" in plain:
        per = [cap(idx) for idx in split(plain["match_byte_offsets"], r)]
        keep_matches = [i for idx in per for i in idx]
        out_chunks["count_matches_chunks"] = [len(idx) for idx in per]
    out = _cut(plain, keep_lines or [], keep_matches, matches)
    if keep_lines is None:
        for k in ("count_lines",) + LINE_KEYS:
            out.pop(k, None)
    out.update(out_chunks)
    return out


def limit_whole_file(plain: dict, n: int, matches=None) -> dict:
    """A job's or a file set's result for ONE file: the first n of the concatenated per-chunk results (`plain`: the file's
    chunk-wise dict with running offsets and line bases); the counts are min(total, n)."""
    cap = (lambda k: k) if n == 0 else (lambda k: min(k, n))
    keep_lines = list(range(cap(len(plain["line_byte_offsets"])))) if "line_byte_offsets" in plain else None
    keep_matches = list(range(cap(len(plain["match_byte_offsets"])))) if "match_byte_offsets" in plain else None
    out = _cut(plain, keep_lines or [], keep_matches, matches)
    if keep_lines is None:
        for k in ("count_lines",) + LINE_KEYS:
            out.pop(k, None)
    return out


def properties(plain: dict, blocks, n: int, global_offsets=None) -> None:
    """what the cut rests on and what it must keep: the count identities, and every chunk's row being a prefix of its
    unlimited row"""
    lim = limit_all_modes(plain, blocks, n, global_offsets)
    full = limit_all_modes(plain, blocks, 0, global_offsets)
    for tag in ("lines", "matches"):
        key = f"count_{tag}_chunks"
        if key not in lim:
            continue
        assert sum(lim[key]) == lim[f"count_{tag}"], "sum(counts) != total"
        assert lim[key] == [c if n == 0 else min(c, n) for c in full[key]], "counts[c] != min(count of chunk c, n)"
    assert len(lim.get("lines", [])) <= lim.get("count_lines", 0)
