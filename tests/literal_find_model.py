"""The model of xsg_find_literals (include/xsg.h, "occurrences per literal"): pure Python, no GPU.

Every occurrence (c, p, j) -- literal j's bytes at position p of chunk c, whole inside the chunk; folded on both sides
under ignore-case (bytes.lower folds A-Z and nothing else, the product's set_fold); under whole words only the
admissible ones of tests/words_model.py -- sorted by (c, p, j), as chunk_ptr / pos / lit.  pos = global offset + p; the
global offsets default to the running sum of the lengths, as xsg.make_chunks sets them."""
import numpy as np

import words_model as WM


def as_bytes(block) -> bytes:
    return block.tobytes() if isinstance(block, np.ndarray) else bytes(block)


def positions(text: bytes, lit: bytes):
    """every position where lit occurs in text, overlapping ones included, ascending"""
    at = text.find(lit)
    while at >= 0:
        yield at
        at = text.find(lit, at + 1)


def find(blocks, literals, icase=False, words=False, global_offsets=None):
    """-> (chunk_ptr [n + 1], pos [total], lit [total])"""
    chunk_ptr, pos, lit = [0], [], []
    goff = 0
    for c, b in enumerate(blocks):
        raw = as_bytes(b)
        d = raw.lower() if icase else raw
        g = goff if global_offsets is None else int(global_offsets[c])
        memo, hits = {}, []
        for j, l in enumerate(literals):
            key = l.lower() if icase else l
            if key not in memo:
                memo[key] = [p for p in positions(d, key) if not words or WM.admissible(raw, p, len(key))]
            hits += [(p, j) for p in memo[key]]
        hits.sort()
        pos += [g + p for p, _ in hits]
        lit += [j for _, j in hits]
        chunk_ptr.append(len(pos))
        goff += len(raw)
    return chunk_ptr, pos, lit


def bincount(lit, k):
    out = [0] * k
    for j in lit:
        out[j] += 1
    return out


def rows(chunk_ptr, lit, k):
    """the per-chunk bincount: what xsg_count_literals_chunks' matrix holds"""
    return [bincount(lit[chunk_ptr[c]:chunk_ptr[c + 1]], k) for c in range(len(chunk_ptr) - 1)]


def well_formed(chunk_ptr, pos, lit, k, starts=None, lengths=None):
    """chunk_ptr starts at 0, ascends and ends at the total; inside a chunk pos ascends and lit ascends strictly at equal
    pos; every lit is a listing index; with starts / lengths (the chunks' global offsets and lengths) every pos lies in
    its chunk"""
    if not chunk_ptr or chunk_ptr[0] != 0 or chunk_ptr[-1] != len(pos) or len(pos) != len(lit):
        return False
    if any(a > b for a, b in zip(chunk_ptr, chunk_ptr[1:])) or any(not 0 <= j < k for j in lit):
        return False
    for c in range(len(chunk_ptr) - 1):
        lo, hi = chunk_ptr[c], chunk_ptr[c + 1]
        for e in range(lo + 1, hi):
            if (pos[e - 1], lit[e - 1]) >= (pos[e], lit[e]):
                return False
        if starts is not None and any(not starts[c] <= p < starts[c] + lengths[c] for p in pos[lo:hi]):
            return False
    return True
