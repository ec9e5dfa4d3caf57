"""The span locator (x-search_amd/csrc/xsg_sketch.h: span_hash, span_index, span_entries, span_mask) on the CPU, through
tests/span_sketch_model.py: where its words live, that the span of an occurrence's window start always passes, and that on
the bench corpus it locates -- few of a tile's four spans pass."""
import numpy as np
import pytest

import corpus
import span_sketch_model as spm
from span_sketch_model import REACH, SPAN, SPANS, TILE

LENGTHS = (4, 5, 8, 16, 31, 32, 33, 40)
BENCH_BLOCK = 16 * 1024 * 1024 + 7  # bench.py's template size


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return spm.load(tmp_path_factory.mktemp("span_sketch_model"))


@pytest.fixture(scope="module")
def templates():
    """bench templates 0 and 1, full size"""
    out = [corpus.text_block(0x5EED, t, BENCH_BLOCK, needle=b"Sherlock") for t in (0, 1)]
    for b in out:
        b.setflags(write=False)
    return out


def windows(plen):
    """filter window offsets a needle of this length can be counted at: 0, and for kLong (plen > 8) koff > 0 as well"""
    return (0,) if plen <= 8 else (0, 1, (plen - 8) // 2, plen - 8)


# ---- 1. layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles", (1, 2, 63, 64, 65, 1000))
def test_index_is_a_bijection_onto_the_allocation(lib, ntiles):
    words = lib.spm_words()
    assert words * 32 == lib.spm_bits()
    alloc = lib.spm_alloc(ntiles)
    assert alloc == ntiles * words * SPANS  # 1 KiB per tile at 2048 bits per span, nothing more
    s = np.zeros((ntiles, words, SPANS), dtype=np.uint64)
    lib.spm_all(ntiles, s.ctypes.data)
    assert np.array_equal(np.sort(s.ravel()), np.arange(alloc, dtype=np.uint64))
    # word k of a tile's four spans: one aligned 16-byte group, span 0 first; a tile's words: one contiguous block
    assert np.array_equal(s[:, :, 0] % SPANS, np.zeros((ntiles, words), dtype=np.uint64))
    for k in range(1, SPANS):
        assert np.array_equal(s[:, :, k], s[:, :, 0] + np.uint64(k))
    assert np.array_equal(s[:, 0, 0], np.arange(ntiles, dtype=np.uint64) * np.uint64(words * SPANS))
    assert np.array_equal(s.ravel(), np.arange(alloc, dtype=np.uint64))  # tile-major, [tile][word][span]


def test_single_calls_agree_with_the_formula(lib):
    words = lib.spm_words()
    for t, w, s in ((0, 0, 0), (0, words - 1, 3), (63, 5, 2), ((1 << 32) - 2, words - 1, 3), (1 << 32, 3, 1)):
        assert lib.spm_index(t, w, s) == (t * words + w) * SPANS + s


def test_the_span_bit_uses_bits_the_tile_sketch_does_not(lib):
    rng = np.random.Generator(np.random.PCG64(7))
    bits = lib.spm_bits()
    shift = 20 - (bits.bit_length() - 1)
    for g in [int(x) for x in rng.integers(0, 1 << 32, size=2000)] + [0, 1, 0xffffffff]:
        m = lib.spm_mix(g)
        assert lib.spm_tile_hash(g) == m >> 20
        assert lib.spm_hash(g) == (m >> shift) & (bits - 1) < bits


# ---- 2. no false negative -----------------------------------------------------------------------------------------------
def check_every_occurrence(lib, data, pat, where):
    sp = spm.build(lib, data)
    occ = spm.occurrences(data, pat)
    for first in windows(len(pat)):
        masks = {}
        for o in occ:
            t, s = (o + first) // TILE, (o + first) % TILE // SPAN
            if t not in masks:
                masks[t] = spm.mask(lib, sp, t, pat, first)
            assert (masks[t] >> s) & 1, (where, pat, first, o, t, s, masks[t])
    return len(occ)


def needles_from(data, rng):
    """needles of every length that occur in `data`: cut from it at random places and across span and tile borders"""
    out = []
    for plen in LENGTHS:
        spots = [int(x) for x in rng.integers(0, data.size - plen, size=3)]
        spots += [SPAN - plen // 2, 3 * SPAN - 1, TILE - 3, TILE, 5 * TILE + 2 * SPAN - plen + 1]
        out += [data[o:o + plen].tobytes() for o in spots]
    return out


@pytest.mark.parametrize("t", (0, 1))
def test_no_false_negative_on_the_bench_templates(lib, templates, t):
    data = templates[t][:2 * 1024 * 1024]
    rng = np.random.Generator(np.random.PCG64(100 + t))
    total = check_every_occurrence(lib, data, b"Sherlock", t)
    for pat in needles_from(data, rng):
        n = check_every_occurrence(lib, data, pat, t)
        assert n >= 1
        total += n
    assert total >= len(LENGTHS) * 8


def test_no_false_negative_on_random_text_at_every_border(lib):
    rng = np.random.Generator(np.random.PCG64(11))
    for plen in LENGTHS:
        pat = bytes(rng.integers(1, 256, size=plen, dtype=np.uint8))
        # window starts right before and at the border for every window offset, and needles straddling it
        rel = {-plen // 2, -plen + 1, -REACH - 4}
        for first in windows(plen):
            rel |= {-1 - first, -first}
        # every (border, distance) in a pair of tiles of its own: no planted needle overwrites another
        spots = [(2 * k + 1) * TILE + border + r
                 for k, (border, r) in enumerate((b, r) for b in (SPAN, 2 * SPAN, 3 * SPAN, TILE) for r in sorted(rel))]
        data = rng.integers(0, 256, size=spots[-1] + 2 * TILE + 1234, dtype=np.uint8)
        spots += [0, data.size - plen]
        for o in spots:
            data[o:o + plen] = np.frombuffer(pat, dtype=np.uint8)
        assert check_every_occurrence(lib, data, pat, "random") >= len(spots) >= 4 * 5 + 2


def test_a_chunk_that_ends_inside_a_span_keeps_its_last_grams(lib):
    for L in (5, SPAN - 1, SPAN + 3, 2 * SPAN + REACH, TILE - 1, TILE + 4, TILE + SPAN + 9):
        data = np.full(L, ord("x"), dtype=np.uint8)
        pat = b"QRST"
        data[L - 4:] = np.frombuffer(pat, dtype=np.uint8)
        assert check_every_occurrence(lib, data, pat, L) == 1


# ---- 3. locating power: a condition, not a measurement --------------------------------------------------------------------
@pytest.mark.parametrize("t", (0, 1))
def test_sherlock_passes_at_most_two_spans_per_holding_tile(lib, templates, t):
    """this model gives 1.00 and 1.00 spans per tile that holds an occurrence at 2048 bits per span (1.29 and 1.53 at 1024);
    "every span" would be 4.0"""
    passed, tiles = spm.spans_per_holding_tile(lib, templates[t], b"Sherlock")
    assert tiles >= 5
    print(f"template {t}: {passed} spans pass in {tiles} tiles that hold an occurrence: {passed / tiles:.2f}")
    assert passed >= tiles            # the span of every occurrence passes
    assert passed <= 2.0 * tiles
