"""The model of xsg_count_literals (include/xsg.h, "counts per literal"): pure Python, no GPU.

counts[j] = the number of (chunk, position) pairs at which literal j occurs with its whole length inside the chunk --
bytes.find from `at + 1`, so overlapping occurrences all count; under ignore-case both sides go through bytes.lower(),
which folds A-Z and nothing else (the product's set_fold)."""
import numpy as np


def as_bytes(block) -> bytes:
    return block.tobytes() if isinstance(block, np.ndarray) else bytes(block)


def occurrences(text: bytes, lit: bytes) -> int:
    n, at = 0, text.find(lit)
    while at >= 0:
        n += 1
        at = text.find(lit, at + 1)
    return n


def counts(blocks, literals, icase=False):
    """-> [counts[j] for j in listing order]"""
    texts = [as_bytes(b) for b in blocks]
    if icase:
        texts = [t.lower() for t in texts]
    memo = {}
    out = []
    for lit in literals:
        key = lit.lower() if icase else lit
        if key not in memo:
            memo[key] = sum(occurrences(t, key) for t in texts)
        out.append(memo[key])
    return out


def borderless(lit: bytes) -> bool:
    """no proper prefix of the literal is also its suffix: two of its occurrences never overlap"""
    return not any(lit[:k] == lit[-k:] for k in range(1, len(lit)))
