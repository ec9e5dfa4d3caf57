"""A literal list under XSG_LIST_WHOLE_WORDS (include/xsg.h: xsg_set_literals_opts) restated without a GPU.

A word byte is one of 0-9 A-Z a-z _.  An occurrence of a literal at position p of a chunk of L bytes is ADMISSIBLE iff
p == 0 or chunk[p - 1] is no word byte, and p + len == L or chunk[p + len] is no word byte: the chunk's edges are word
boundaries.  The search is tests/set_model.py's restricted to admissible occurrences -- at the leftmost position where any
literal occurs admissibly, the first-listed literal that does so is the match -- and the counts are
tests/literal_counts_model.py's over admissible occurrences.  all_modes and matches ARE set_model's functions, run over
the Occurrences of this file; matrix, chunks_with and csr are built on the literal_*_model files the same way.
tests/test_words_host.py pins the walk to Python's re on (?<![0-9A-Za-z_])(?:l1|l2|...)(?![0-9A-Za-z_])."""
import types

import literal_csr_model as CM
import literal_matrix_model as MM
import set_model

WORD = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")
assert len(WORD) == 63


def admissible(d: bytes, p: int, n: int) -> bool:
    """the n bytes at d[p] stand between two bytes that are no word bytes (or the chunk's edges)"""
    return (p == 0 or d[p - 1] not in WORD) and (p + n == len(d) or d[p + n] not in WORD)


def _occurrences(d: bytes, needle: bytes):
    """every position where needle occurs in d, overlapping ones included"""
    at = d.find(needle)
    while at >= 0:
        yield at
        at = d.find(needle, at + 1)


class Occurrences(set_model.Occurrences):
    """every position of one chunk where a literal occurs ADMISSIBLY, with the first-listed literal that does so there;
    search, spans, line_walk and lines_spans are set_model's"""

    def __init__(self, data, literals, icase=False):
        self.d = set_model._bytes(data)
        d = self.d.lower() if icase else self.d  # (folding maps letters to letters: the word test is the same on either)
        best = {}
        for lit in literals:
            assert lit and b"\n" not in lit
            for at in _occurrences(d, lit.lower() if icase else lit):
                if admissible(self.d, at, len(lit)):
                    best.setdefault(at, len(lit))  # (an earlier literal at the position wins)
        self.pos = sorted(best)
        self.len = [best[p] for p in self.pos]


def _over_words(fn):
    """set_model's function, code and defaults, with this file's Occurrences where it names Occurrences"""
    return types.FunctionType(fn.__code__, {**vars(set_model), "Occurrences": Occurrences}, fn.__name__, fn.__defaults__)


all_modes = _over_words(set_model.all_modes)  # (blocks, literals, icase=False, global_offsets=None, line_bases=None)
matches = _over_words(set_model.matches)      # (blocks, literals, icase=False, global_offsets=None)


def regex(literals) -> bytes:
    """the expression whose backtracking leftmost-first search defines the walk (Python re, bytes)"""
    return b"(?<![0-9A-Za-z_])(?:" + set_model.expression(literals) + b")(?![0-9A-Za-z_])"


def counts(blocks, literals, icase=False):
    """-> [admissible occurrences of literal j over all chunks, for j in listing order]"""
    out = [0] * len(literals)
    for b in blocks:
        raw = set_model._bytes(b)
        d = raw.lower() if icase else raw
        memo = {}
        for j, lit in enumerate(literals):
            key = lit.lower() if icase else lit
            if key not in memo:
                memo[key] = sum(1 for at in _occurrences(d, key) if admissible(raw, at, len(key)))
            out[j] += memo[key]
    return out


def matrix(blocks, literals, icase=False):
    """-> [[counts of chunk c in listing order] for c in binding order]"""
    return [counts([b], literals, icase) for b in blocks]


chunks_with = MM.chunks_with


def csr(blocks, literals, icase=False):
    return CM.from_rows(matrix(blocks, literals, icase))
