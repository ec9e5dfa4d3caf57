"""The gated count pass as one persistent kernel: k_scan<..., GATED> (x-search_amd/csrc/xsg_kernels.hip: gated_pass): workgroup
b of G takes the units b, b + G, ... of 256 consecutive tiles, tests one tile per lane against the needle's sketch entries and
scans the tiles that pass, their chunk geometry handed from the passing lanes to all four waves through LDS.  Shards are sized around the edges of that code: the 256 tiles of a unit, grids of fewer and of more
workgroups than units (XSG_GATE_GRID), units without a candidate next to units full of them, chunk borders inside a unit,
the first and last lane of every wave, and bindings of another unit count behind one another on one Shard.

XSG_SKETCH=1 and XSG_SKETCH_MIN_BYTES=0; text, model and helpers of tests/test_gpu_sketch.py and
tests/test_gpu_sketch_select.py are reused.  Every case compares count, three back-to-back count_async calls without a host
sync between them, count_begin/count_end and match_byte_offsets with the oracle.
"""
import os

import numpy as np
import pytest

import sketch_model
import test_gpu_sketch as base
from gpu_util import oracle_all_modes
from test_gpu_sketch import GATED, TILE, Sketched
from test_gpu_sketch_select import ABSENT, async_many, build_with_absent_needle, needle, passing_tiles, plant

pytestmark = pytest.mark.gpu
UNIT = 256  # tiles a workgroup tests at a time


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return sketch_model.load(tmp_path_factory.mktemp("gated_fused_model"))


@pytest.fixture(scope="module")
def text():
    """1100 tiles of the lexicon's text, generated once; the tests take copies of slices of it"""
    rng = np.random.Generator(np.random.PCG64(9000))
    t = base._text(rng, 1100 * TILE)
    t.setflags(write=False)
    return t


@pytest.fixture
def sk():
    saved = {k: os.environ.pop(k, None) for k in ("XSG_SKETCH", "XSG_GATE_GRID")}
    os.environ["XSG_SKETCH"] = "1"  # a synchronous call builds the sketch before its first eligible pass
    s = Sketched()
    yield s
    s.close()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def gated_then_every_route(sk, oracle, blocks, pat, want, where):
    """a new pattern has no verdict: the stream-ordered calls gate on the sketch as it is; then every route"""
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(GATED), where
    assert async_many(sk) == [want["count_matches"]] * 3, where
    sk.check_routes(want, where)
    assert async_many(sk) == [want["count_matches"]] * 3, (where, "again")


# ---- one workgroup takes several units and looks past the last one; a grid asked for beyond the number of units ----------
@pytest.mark.parametrize("grid", (1, 2, 3, None), ids=("grid1", "grid2", "grid3", "default_grid"))
@pytest.mark.parametrize("ntiles", (255, 256, 257, 511, 512, 513))
def test_units_at_the_edges_under_small_grids(sk, oracle, text, ntiles, grid):
    rng = np.random.Generator(np.random.PCG64(9100 + ntiles))
    pat = needle(rng, 8)
    size = ntiles * TILE - 3
    b = text[:size].copy()
    tiles = sorted({0, 63, 64, 254, ntiles - 2, ntiles - 1} | {t for t in (255, 256, 257, 510, 511, 512) if t < ntiles})
    plant(b, pat, [t * TILE + 900 + t for t in tiles[:-1]] + [size - 8])
    blocks = [b]
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == len(tiles)
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    if grid is not None:
        os.environ["XSG_GATE_GRID"] = str(grid)
    gated_then_every_route(sk, oracle, blocks, pat, want, (ntiles, grid))
    assert sk.name().endswith(GATED)  # a handful of tiles pass: the verdict keeps the gate
    sk.ctx.set_pattern(ABSENT)
    assert async_many(sk) == [0] * 3
    os.environ.pop("XSG_GATE_GRID", None)  # and the default grid behind it, on the same words
    sk.ctx.set_pattern(pat)
    sk.check_routes(want, (ntiles, grid, "default grid"))


# ---- extreme candidate densities in neighbouring units ------------------------------------------------------------------
def test_empty_unit_full_unit_and_a_single_candidate_in_a_units_last_tile(sk, oracle, model, text):
    rng = np.random.Generator(np.random.PCG64(9200))
    pat = needle(rng, 8)
    n = 3 * UNIT
    b = text[:n * TILE - 11].copy()
    tiles = list(range(UNIT, 2 * UNIT)) + [3 * UNIT - 1]
    plant(b, pat, [t * TILE + 1500 + 5 * (t % 97) for t in tiles[:-1]] + [n * TILE - 11 - 8])
    blocks = [b]
    assert passing_tiles(model, blocks, pat) == len(tiles)
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == len(tiles)
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    # through the stream-ordered call ahead of any verdict: unit 0 has no candidate, unit 1 has 256, unit 2 one
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(GATED)
    assert async_many(sk) == [len(tiles)] * 3
    sk.check_routes(want, "densities")  # (a third of the tiles pass: the synchronous call's verdict switches the gate off)
    for grid in ("1", "2"):
        os.environ["XSG_GATE_GRID"] = grid
        sk.ctx.set_pattern(ABSENT)
        assert async_many(sk) == [0] * 3
        sk.ctx.set_pattern(pat)  # a new serial: no verdict again
        assert sk.name().endswith(GATED)
        assert async_many(sk) == [len(tiles)] * 3
    del os.environ["XSG_GATE_GRID"]
    assert async_many(sk) == [len(tiles)] * 3


# ---- chunk borders inside a unit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", (False, True), ids=("spaced", "packed"))
@pytest.mark.parametrize("plen", (4, 8, 9, 40))
def test_chunk_borders_inside_a_unit(sk, oracle, model, text, plen, packed):
    """unit 0 holds the tiles of eight chunks: 100 tiles + 5 B, 1 B, 3 B, TILE - 1, TILE, TILE + 1, 3 tiles + 1 B and the
    head of a large one; candidates in the last tile of a chunk and the first of the next, and in the tail zones"""
    rng = np.random.Generator(np.random.PCG64(9300 + plen))
    pat = needle(rng, plen)
    lead = text[:100 * TILE + 5].copy()
    plant(lead, pat, (0, 99 * TILE + 77, 100 * TILE + 5 - plen))  # ... ending with the chunk, in its last tile of 5 bytes
    small = []
    for length in (1, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        c = text[200 * TILE:200 * TILE + length].copy()
        if length >= 2 * plen:
            plant(c, pat, (0, length - plen))  # first tile of the chunk, and its tail zone
        if length > 3 * TILE:
            plant(c, pat, (TILE - 2, 2 * TILE + 100))  # its window starts in one tile, its end lies in the next
        small.append(c)
    big = text[300 * TILE:300 * TILE + 200 * TILE + 29].copy()
    plant(big, pat, (0, 144 * TILE - 1, 145 * TILE, 200 * TILE + 29 - plen))  # tiles 255 / 256 of the binding among them
    blocks = [lead] + small + [big]
    assert sum((b.size + TILE - 1) // TILE for b in blocks) == 101 + 1 + 1 + 1 + 1 + 2 + 4 + 201
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] >= 15
    gate = base.gate_expected(model, blocks, pat)
    sk.bind(blocks, packed_fill=(pat + b"\n" + pat[1:] + b" ") if packed else None)
    build_with_absent_needle(sk, oracle, blocks)
    gated_then_every_route(sk, oracle, blocks, pat, want, (plen, packed))
    base.check_name(sk, gate, "after every route")
    os.environ["XSG_GATE_GRID"] = "1"  # one workgroup takes both units, one after the other
    sk.ctx.set_pattern(ABSENT)
    assert async_many(sk) == [0] * 3
    gated_then_every_route(sk, oracle, blocks, pat, want, (plen, packed, "grid 1"))


# ---- the edges of a wave and of a unit ----------------------------------------------------------------------------------
def test_first_and_last_lane_of_every_wave_and_unit_borders(sk, oracle, model, text):
    rng = np.random.Generator(np.random.PCG64(9400))
    pat = needle(rng, 9)
    n = 3 * UNIT + 10
    b = text[:n * TILE - 1].copy()
    tiles = sorted({u * UNIT + w * 64 + l for u in range(3) for w in range(4) for l in (0, 63)} | {3 * UNIT, n - 1})
    plant(b, pat, [t * TILE + 40 + 3 * t for t in tiles])
    blocks = [b]
    assert passing_tiles(model, blocks, pat) == len(tiles)
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == len(tiles)
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    for grid in (None, "2"):
        if grid:
            os.environ["XSG_GATE_GRID"] = grid
        gated_then_every_route(sk, oracle, blocks, pat, want, grid)
        assert sk.name().endswith(GATED)
        sk.ctx.set_pattern(ABSENT)
        assert async_many(sk) == [0] * 3


# ---- another unit count on the same Shard: nothing of an earlier pass is left behind -----------------------------------
def test_rebinding_to_a_smaller_and_a_larger_text(sk, oracle, model, text):
    rng = np.random.Generator(np.random.PCG64(9500))
    some, one = needle(rng, 8), needle(rng, 9)

    def shard_of(n, salt):
        b = text[salt * TILE:(salt + n) * TILE - 5].copy()
        hits = [t for t in range(n) if t % 7 == 3]
        plant(b, some, [t * TILE + 1000 + t for t in hits])
        plant(b, one, ((n - 1) * TILE + 700,))
        return [b], len(hits)

    for n, salt in ((600, 0), (100, 40), (1090, 3)):  # 3 units, then 1, then 5, on one Shard
        blocks, n_some = shard_of(n, salt)
        sk.bind(blocks)
        if n != 600:
            assert GATED not in sk.name()  # no sketch of these bytes yet
        build_with_absent_needle(sk, oracle, blocks)
        for pat, count in ((some, n_some), (one, 1), (ABSENT, 0), (some, n_some)):
            want = oracle_all_modes(oracle, blocks, pat)
            assert want["count_matches"] == count
            gated_then_every_route(sk, oracle, blocks, pat, want, (n, pat))


# ---- chunk offsets beyond 2^31 and 2^32 ---------------------------------------------------------------------------------
def test_chunks_at_offsets_whose_low_word_has_its_top_bit_set(sk, oracle, model, text):
    """The candidates' chunk geometry travels through LDS and back into scalar registers as 32-bit halves.  The buffer is
    allocated, not filled: only the three small chunks are written and bound."""
    import xsg
    rng = np.random.Generator(np.random.PCG64(9600))
    pat = needle(rng, 8)
    torch = sk.torch
    blocks, offsets = [], []
    for k, o in enumerate(((1 << 31) - 5 * TILE - 16, (1 << 31) + (1 << 30) + 48, (1 << 32) + (1 << 31) + 4096)):
        b = text[k * 50 * TILE:(k * 50 + 40) * TILE + 7 + k].copy()  # the first one straddles 2^31
        plant(b, pat, (3, 5 * TILE - 4, 20 * TILE + 100, b.size - 8))
        blocks.append(b)
        offsets.append(o)
    cap = offsets[-1] + 41 * TILE
    t = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    for o, b in zip(offsets, blocks):
        t[o:o + b.size].copy_(torch.from_numpy(b))
    torch.cuda.synchronize()
    chunks = xsg.make_chunks(np.array(offsets, dtype=np.uint64), np.array([b.size for b in blocks], dtype=np.uint64))
    sk.shard = xsg.Shard(sk.ctx, t.data_ptr(), cap, chunks)
    sk.keep = t
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == 12
    build_with_absent_needle(sk, oracle, blocks)
    gated_then_every_route(sk, oracle, blocks, pat, want, "high offsets")
    assert sk.name().endswith(GATED)
