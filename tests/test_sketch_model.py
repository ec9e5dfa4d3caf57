"""The per-tile 4-gram sketch (x-search_amd/csrc/xsg_sketch.h) on the CPU: the header is compiled into a small host
helper here, the sketches of random and corpus text are built by its definition, and the three properties the gate of
k_scan rests on are checked against the oracle:

  superset     every tile in which the oracle reports a match start passes the pattern's test -- for needles that start
               in the last bytes of a tile, in a chunk's last tile, in chunks around the tile size;
  selectivity  on the bench corpus `Sherlock` passes in hardly any tile that does not hold it, at a fill <= 0.5;
  switch-off   `Holmes`, a word of the corpus' lexicon, passes in more than a quarter of the tiles: the verdict rule
               (fewer than a quarter of the sampled tiles pass) keeps the gate off for it.
"""
import numpy as np
import pytest

import corpus
from sketch_model import TILE, build, load, passes


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return load(tmp_path_factory.mktemp("sketch_model"))


def windows_of(plen):
    """filter-window offsets a pattern of this length can be counted at (PatternDev::koff): 0, and for the long kind
    a few of 0 .. plen - 8"""
    return [0] if plen <= 8 else sorted({0, 1, (plen - 8) // 2, plen - 8})


def check_superset(lib, oracle, data: np.ndarray, pat: bytes, must_hold=None):
    sk = build(lib, data)
    starts = [int(x) for x in oracle.byte_offsets_match(data, pat)]
    if must_hold is not None:
        assert must_hold in starts
    for o in starts:
        for f in windows_of(len(pat)):
            assert passes(lib, sk, (o + f) // TILE, pat, f), (len(pat), o, f, data.size)
    return len(starts)


NEEDLE_LENGTHS = (4, 5, 8, 9, 31, 32, 33, 40, 300)


def _text(rng, n):
    return rng.integers(ord("a"), ord("z") + 1, size=n).astype(np.uint8)


def test_gram_rule(model):
    assert model.skm_grams(3, 0) == 0
    assert model.skm_grams(4, 0) == 1
    assert model.skm_grams(8, 0) == 5
    assert model.skm_grams(31, 0) == 28
    assert model.skm_grams(32, 0) == 29
    assert model.skm_grams(300, 0) == 29
    assert model.skm_grams(300, 292) == 5
    assert all(model.skm_hash(g) < 4096 for g in (0, 1, 0xffffffff, 0x6c726568))


@pytest.mark.parametrize("plen", NEEDLE_LENGTHS)
def test_superset_at_tile_ends(model, oracle, plen):
    """the needle starts in the last 1 .. plen bytes of a tile, and of the chunk's last tile"""
    rng = np.random.Generator(np.random.PCG64(1000 + plen))
    pat = bytes(rng.integers(ord("A"), ord("Z") + 1, size=plen).astype(np.uint8))
    base = _text(rng, 2 * TILE + 5000)
    found = 0
    for j in range(1, plen + 1):
        d = base.copy()
        o = 2 * TILE - j  # starts j bytes before the end of the second tile, continues in the third
        d[o:o + plen] = np.frombuffer(pat, dtype=np.uint8)
        found += check_superset(model, oracle, d, pat, must_hold=o)
        # ... and in the chunk's last tile: the chunk ends with the needle's last byte, or a little behind it
        for tail in (0, 1, 17):
            e = np.concatenate([base[:2 * TILE + j + 3], np.frombuffer(pat, dtype=np.uint8), base[:tail]])
            found += check_superset(model, oracle, e, pat, must_hold=2 * TILE + j + 3)
    assert found >= 4 * plen


@pytest.mark.parametrize("length", (3, 4, TILE - 1, TILE, TILE + 1, TILE + 29))
def test_superset_in_chunks_around_the_tile_size(model, oracle, length):
    rng = np.random.Generator(np.random.PCG64(2000 + length))
    for plen in NEEDLE_LENGTHS:
        if plen > length:
            continue
        pat = bytes(rng.integers(ord("A"), ord("Z") + 1, size=plen).astype(np.uint8))
        for o in sorted({0, length - plen, max(0, min(length - plen, TILE - 2)), max(0, min(length - plen, TILE - plen))}):
            d = _text(rng, length)
            d[o:o + plen] = np.frombuffer(pat, dtype=np.uint8)
            check_superset(model, oracle, d, pat, must_hold=o)


@pytest.fixture(scope="module")
def bench_templates():
    """templates 0-3 of the benchmark corpus (bench.py: template_blocks, seed 0x5EED, 16 MiB chunks)"""
    seed = 0x5EED
    return [corpus.text_block(seed, i, (16 << 20) + 1 + (corpus._mix(seed, 1000 + i) % 61), needle=b"Sherlock") for i in range(4)]


def test_selectivity_on_the_bench_corpus(model, oracle, bench_templates):
    tiles = cand = hold = bits = 0
    holmes = 0
    for b in bench_templates:
        sk = build(model, b)
        n = sk.shape[0]
        holds = set(int(x) // TILE for x in oracle.byte_offsets_match(b, b"Sherlock"))
        c = [t for t in range(n) if passes(model, sk, t, b"Sherlock")]
        assert holds <= set(c)  # superset on the corpus itself
        tiles += n
        cand += len(c)
        hold += len(holds)
        bits += int(np.unpackbits(sk.view(np.uint8)).sum())
        holmes += sum(1 for t in range(n) if passes(model, sk, t, b"Holmes"))
    fill = bits / (tiles * 4096)
    print(f"tiles {tiles}: Sherlock held by {hold}, candidates {cand}; fill {fill:.3f}; Holmes passes in {holmes}")
    assert fill <= 0.5
    assert cand / tiles <= hold / tiles + 0.01
    # a word of the lexicon is everywhere: the verdict rule (fewer than a quarter of the tiles pass) switches the gate off
    assert holmes / tiles > 0.25
