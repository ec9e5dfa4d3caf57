"""The layouts of tests/high_offsets.py, checked without a GPU: their geometry is what xsg_shard_create accepts, and they
make tests/test_gpu_high_offsets.py sensitive -- a search that read any chunk above 2^31 at its address mod 2^31 or
mod 2^32 would report something else than the oracle does, for every pattern and every such chunk."""
import numpy as np
import pytest

import high_offsets as H
import xsg

LAYOUTS = ("abutting", "straddling")


def test_the_constants_are_the_library_s():
    assert (H.X, H.IC, H.RX, H.INV) == (xsg.FLAG_EXACT_TAIL, xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX, xsg.FLAG_INVERT)
    assert H.TILE == xsg.TILE


@pytest.mark.parametrize("name", LAYOUTS)
def test_geometry(name):
    lay = H.layouts()[name]
    end = 0
    for c in lay.chunks:
        assert c.offset % 16 == 0 and c.offset >= end, c.name  # sorted, aligned, no overlap
        end = c.offset + int(c.block.size)
        assert c.offset + (int(c.block.size) + 15) // 16 * 16 <= lay.capacity, c.name
    by = {c.name: c for c in lay.chunks}
    assert by["control"].offset == 4096
    a = by["across_2_31"]
    assert a.offset == H.B31 - 5 * H.TILE - 16 and a.offset < H.B31 < a.offset + a.block.size
    if name == "abutting":
        assert by["ends_at_2_32"].offset + by["ends_at_2_32"].block.size == H.B32 and by["ends_at_2_32"].block.size % 16 == 0
        assert by["ends_at_2_32"].block.tobytes().endswith(b"that")
        assert by["begins_at_2_32"].offset == H.B32 and by["begins_at_2_32"].block.tobytes().startswith(b"x that")
    else:
        s = by["across_2_32"]
        assert s.offset == H.B32 - 3 * H.TILE - 16 and s.offset + s.block.size > H.B32
        k = H.B32 - s.offset
        d = s.block.tobytes()
        assert d[k - 2:k + 2] == b"that" and 10 not in d[k - 7:k + 39], "a match and a line across 2^32"
    assert by["empty"].offset == H.B32 + (1 << 20) and by["empty"].block.size == 0
    small = [c for c in lay.chunks if c.name.startswith("small")]
    assert len(small) == H.N_SMALL and small[0].offset == H.B32 + (1 << 21)
    for p, q in zip(small, small[1:]):
        assert q.offset == p.offset + (int(p.block.size) + 15) // 16 * 16, "packed at 16-byte steps"
    assert [i for i, c in enumerate(small) if c.block.size == 0] == [0, 1, 100, 101, 102, 103, 104, H.N_SMALL - 1]
    assert by["top_bit_of_low_word"].offset == H.B32 + H.B31 + 4096
    assert sum(int(c.block.size) for c in lay.chunks) < (1 << 20)
    go = sorted((c.global_offset, c.global_offset + int(c.block.size)) for c in lay.chunks)
    assert all(a[1] <= b[0] for a, b in zip(go, go[1:])), "global ranges overlap"
    assert [c.global_offset for c in lay.chunks] != sorted(c.global_offset for c in lay.chunks)
    # every bound chunk holds its own bytes in the filled buffer, and what lies around it is defined
    for c in lay.chunks:
        n = int(c.block.size)
        got = lay.read(max(c.offset - H.GUARD_BEFORE, 0), min(c.offset, H.GUARD_BEFORE) + n + 64)
        assert got[min(c.offset, H.GUARD_BEFORE):min(c.offset, H.GUARD_BEFORE) + n].tolist() == c.block.tolist(), c.name


@pytest.mark.parametrize("name", LAYOUTS)
def test_a_read_that_loses_the_high_bits_is_told_from_the_chunk(oracle, name):
    """(pattern, chunk, image) triples: the count printed is the one the pull request's summary quotes"""
    lay = H.layouts()[name]
    triples, memo = 0, {}
    sig = lambda p, b: memo.setdefault((p[0], b.tobytes()), H.signature(oracle, p[1], p[2], p[3], b))
    for i, c in enumerate(lay.chunks):
        if c.block.size == 0 or c.offset + c.block.size <= H.B31:
            continue
        images = [lay.image(i, m) for m in (H.B31, H.B32)]
        images = [im for im in images if im is not None]
        assert images, c.name
        for im in images:
            assert im.size == c.block.size
            for p in H.PATTERNS:
                assert sig(p, c.block) != sig(p, im), (name, c.name, p[0], "the image reports what the chunk reports")
                triples += 1
    print(f"{name}: {triples} (pattern, chunk, image) triples, 0 without a difference")
    assert triples >= len(H.PATTERNS) * 250


@pytest.mark.parametrize("name", LAYOUTS)
def test_every_pattern_matches_in_every_large_chunk(oracle, name):
    for c in H.layouts()[name].chunks:
        if c.block.size >= 33 << 10:
            for p in H.PATTERNS:
                cnt, lines = H.signature(oracle, p[1], p[2], p[3], c.block)
                assert lines and cnt != 0, (name, c.name, p[0])


@pytest.mark.parametrize("name", LAYOUTS)
def test_an_unterminated_last_line_above_2_32_is_dropped(oracle, name):
    dropped = 0
    for c in H.layouts()[name].chunks:
        if c.offset >= H.B32 and c.block.size:
            w = H.chunk_plain(oracle, "lit", b"colour", 0, 0, c.block, c.global_offset, c.line_base)
            dropped += len(w["line_byte_offsets"]) - len(w["lines"])
    assert dropped >= 2
