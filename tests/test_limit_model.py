"""tests/limit_model.py checks itself against the oracle run chunk by chunk: no GPU, no library call.

  * a limit of at least the fullest chunk's count is the identity, and so is 0;
  * a limit of 1 is every chunk's first entry, taken from the oracle on that chunk alone;
  * counts[c] == min(count of chunk c, n), sum(counts) == total, and XSG_LINES hands out at most the cut lines;
  * the order oracle -> invert_model -> limit -> context_model: the context of the cut list, chunk by chunk, by
    context_model.chunk_context on the cut indices;
  * the whole-file form is the first n of the concatenation."""
import numpy as np
import pytest

import context_model
import invert_model
import limit_model
import match_model
from gpu_util import oracle_all_modes
from per_chunk_model import INV, chunk_plain


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


BLOCKS = [
    _u8(b""),
    _u8(b"plain words\nnothing here\n"),
    _u8(b"that one\nplain\nthat two that\nthat three\nplain\nthat four"),   # the fourth selected line lacks its newline
    _u8(b"that\n" * 5),
    _u8(b"x\nthat last"),                                                    # the FIRST selected line lacks it
    _u8(b"that a\nthat b\n"),
]
GO = [((i * 5) % 6) * 1000 + 3 for i in range(6)]  # disjoint, not in the chunks' order
LB = [((i * 7) % 6) * 100 + 1 for i in range(6)]
PAT = b"that"


@pytest.fixture(scope="module")
def plain(oracle):
    return oracle_all_modes(oracle, BLOCKS, PAT, global_offsets=GO, line_bases=LB)


@pytest.fixture(scope="module")
def inverted(plain):
    return invert_model.invert_all_modes(plain, BLOCKS, GO, LB)


def test_no_cut_is_the_identity(plain, inverted, oracle):
    m = match_model.matches(oracle, BLOCKS, PAT, 0, GO)
    for src in (plain, inverted):
        for n in (0, 5, (1 << 32) + 1, (1 << 64) - 1):
            lim = limit_model.limit_all_modes(src, BLOCKS, n, GO, LB, matches=m if src is plain else None)
            for k, v in src.items():
                assert lim[k] == (v if not isinstance(v, list) else [x if isinstance(x, bytes) else int(x) for x in v]), (n, k)
    lim = limit_model.limit_all_modes(plain, BLOCKS, 0, GO, LB, matches=m)
    assert (lim["matches"], lim["matches_offsets"]) == (m[0], [int(x) for x in m[1]])


@pytest.mark.parametrize("flags", [0, INV], ids=["plain", "inverted"])
def test_a_limit_of_one_is_every_chunks_first_entry(plain, inverted, oracle, flags):
    lim = limit_model.limit_all_modes(inverted if flags else plain, BLOCKS, 1, GO, LB)
    want = {k: [] for k in ("line_byte_offsets", "line_indices", "lines", "match_byte_offsets")}
    for i, b in enumerate(BLOCKS):
        w = chunk_plain(oracle, "lit", PAT, 0, flags, b, GO[i], LB[i])
        for k in ("line_byte_offsets", "line_indices") + (() if flags else ("match_byte_offsets",)):
            want[k] += [int(x) for x in w[k][:1]]
        if w["lines_offsets"] and int(w["lines_offsets"][0]) == int(w["line_byte_offsets"][0]):
            want["lines"].append(w["lines"][0])  # (else the first selected line is the unterminated one: cut in, not handed out)
    for k, v in want.items():
        if k in lim:
            assert lim[k] == v, k
    if not flags:
        assert lim["lines"] == [b"that one", b"that", b"that a"] and lim["count_lines"] == 4


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_count_identities(plain, inverted, n):
    limit_model.properties(plain, BLOCKS, n, GO)
    limit_model.properties(inverted, BLOCKS, n, GO)
    lim = limit_model.limit_all_modes(plain, BLOCKS, n, GO, LB)
    assert lim["count_lines_chunks"] == [min(c, n) for c in (0, 0, 4, 5, 1, 2)]
    assert lim["count_matches_chunks"] == [min(c, n) for c in (0, 0, 5, 5, 1, 2)]
    # the chunk whose fourth selected line is unterminated hands out n - 1 lines at n == 4, the one whose first is: none
    assert len(lim["lines"]) == sum(min(c, n) for c in (0, 0, 3, 5, 0, 2))


@pytest.mark.parametrize("before,after", [(1, 2), (2, 0)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_context_is_taken_around_the_cut_list(plain, inverted, before, after, n):
    for src in (plain, inverted):
        lim = limit_model.limit_all_modes(src, BLOCKS, n, GO, LB)
        got = context_model.context_all_modes(lim, BLOCKS, before, after, GO, LB)
        want = []
        for i, b in enumerate(BLOCKS):
            starts = invert_model.lines(b)
            sel = [k for k, s in enumerate(starts) if GO[i] + s in set(src["line_byte_offsets"])][:n]
            want += [GO[i] + starts[q] for q in context_model.chunk_context(len(starts), sel, before, after)]
        assert got["line_byte_offsets"] == want
        e = context_model.edges(lim, BLOCKS, before, after, GO)
        assert [x[0] for x in e] == [len(invert_model.lines(b)) for b in BLOCKS]


def test_whole_file_form(oracle):
    chunks = [_u8(b"that 1\nplain\n"), _u8(b"plain\n"), _u8(b"that 2 that\nthat 3\n"), _u8(b"that 4")]
    plain = oracle_all_modes(oracle, chunks, PAT)
    m = match_model.matches(oracle, chunks, PAT, 0)
    for n, lines, nm in ((1, [b"that 1"], 1), (2, [b"that 1", b"that 2 that"], 2), (4, [b"that 1", b"that 2 that", b"that 3"], 4),
                         (9, [b"that 1", b"that 2 that", b"that 3"], 5), (0, [b"that 1", b"that 2 that", b"that 3"], 5)):
        w = limit_model.limit_whole_file(plain, n, matches=m)
        assert w["lines"] == lines and w["count_lines"] == (min(4, n) if n else 4), n
        assert w["count_matches"] == nm == len(w["matches"]) and w["match_byte_offsets"] == [int(x) for x in m[1][:nm]], n
        assert w["line_byte_offsets"] == [int(x) for x in plain["line_byte_offsets"]][:w["count_lines"]]
