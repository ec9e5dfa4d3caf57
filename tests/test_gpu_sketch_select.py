"""The gated count pass as a candidate list: k_sketch_select (one lane per tile over the word-major sketch, xsg_sketch.h:
sketch_index) lists the tiles whose sketch holds the needle's grams, and k_scan<..., GATED> is a bounded grid that strides
over that list (x-search_amd/csrc/xsg_kernels.hip).  Shards are sized around the edges of that code: the 64 tiles of a
sketch group, the 256 tiles of a select round, the 1024 tiles of a select workgroup, the grid of the strided pass
(XSG_GATE_GRID), the count and ticket words that every pass must leave at zero.

XSG_SKETCH_MIN_BYTES=0 and XSG_TEST_HOOKS=1 as in tests/test_gpu_sketch.py, whose low-entropy text (few tiles pass), model
and helpers are reused.  Every result is compared with the oracle on count, count_async on its own stream,
count_begin/count_end and match_byte_offsets; xsg_scan_kernel_name says whether the next plain count pass is a gated one.
"""
import os

import numpy as np
import pytest

import sketch_model
import test_gpu_sketch as base
import xsg
from gpu_util import oracle_all_modes
from test_gpu_sketch import GATED, TILE, Sketched, _u8

pytestmark = pytest.mark.gpu
ABSENT = b"QZXJKVWQ"  # no gram of it is in the lexicon's text or in a needle of this file (those are drawn from A..P)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return sketch_model.load(tmp_path_factory.mktemp("sketch_select_model"))


@pytest.fixture(scope="module")
def text():
    """1100 tiles of the lexicon's text, generated once; the tests take copies of slices of it"""
    rng = np.random.Generator(np.random.PCG64(8000))
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


def needle(rng, plen):
    return bytes(rng.integers(ord("A"), ord("P") + 1, size=plen).astype(np.uint8))


def plant(block, pat, offsets):
    for o in offsets:
        block[o:o + len(pat)] = _u8(pat)


def passing_tiles(model, blocks, pat, first=0):
    n = 0
    for b in blocks:
        s = sketch_model.build(model, b)
        n += sum(1 for t in range(s.shape[0]) if sketch_model.passes(model, s, t, pat, first))
    return n


def build_with_absent_needle(sk, oracle, blocks):
    """the binding gets its sketch from a synchronous count of a needle that no tile can hold: no candidate, count 0, gated"""
    sk.ctx.set_pattern(ABSENT)
    assert oracle_all_modes(oracle, blocks, ABSENT)["count_matches"] == 0
    assert sk.count() == 0
    assert sk.name().endswith(GATED)
    assert sk.count_async() == 0
    assert sk.count() == 0


def async_many(sk, times=3):
    """`times` stream-ordered counts back to back, no host sync in between; -> their match counts"""
    torch = sk.torch
    bufs = torch.full((times, xsg.NUM_COUNTERS), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for k in range(times):
        sk.shard.count_async(xsg.COUNT_MATCHES, sk.stream.cuda_stream, bufs[k].data_ptr())
    sk.stream.synchronize()
    return [int(x) for x in bufs[:, xsg.CTR_MATCHES].tolist()]


# ---- tile counts at every edge: sketch group (64), select round (256), select workgroup (1024) -------------------------
@pytest.mark.parametrize("last_len", (1, TILE - 1), ids=("last_tile_1B", "last_tile_short_by_1B"))
@pytest.mark.parametrize("ntiles", (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1024 + 65))
def test_tile_counts_at_the_edges(sk, oracle, model, text, ntiles, last_len):
    rng = np.random.Generator(np.random.PCG64(8100 + ntiles))
    pat = needle(rng, 8)
    size = (ntiles - 1) * TILE + last_len
    b = text[:size].copy()
    last0 = (ntiles - 1) * TILE
    spots = [min(5, max(size - 8, 0))]                              # the first tile
    spots.append(max(size - 8, 0))                                  # the last tile (where it has 1 byte: ending in it)
    spots += [t * TILE + 100 + t for t in (63, 64, 65) if (t + 1) * TILE <= last0]
    if size >= 8:
        plant(b, pat, spots)
    blocks = [b]
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == (len(set(spots)) if size >= 8 else 0)
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    sk.ctx.set_pattern(pat)  # a new pattern: no verdict, the stream-ordered call gates on the sketch as it is
    assert sk.name().endswith(GATED)
    assert async_many(sk) == [want["count_matches"]] * 3
    sk.check_routes(want, (ntiles, last_len))
    if ntiles >= 63:  # at most 6 of them pass: the verdict keeps the gate
        assert sk.name().endswith(GATED)
    sk.check_routes(want, (ntiles, last_len, "again"))
    sk.ctx.set_pattern(ABSENT)
    assert async_many(sk) == [0] * 3
    assert sk.count() == 0


# ---- several chunks: 64-tile groups straddle chunk borders; needle lengths with every filter kind the gate serves -------
@pytest.mark.parametrize("packed", (False, True), ids=("spaced", "packed"))
@pytest.mark.parametrize("plen", (4, 8, 9, 40))
def test_chunks_of_every_small_size_between_large_ones(sk, oracle, model, text, plen, packed):
    rng = np.random.Generator(np.random.PCG64(8200 + plen))
    pat = needle(rng, plen)
    small = base.placed_blocks(rng, pat)  # 5 tiles + 777, 3, 4, TILE - 1, TILE, TILE + 1, TILE + 29 bytes, then 64 tiles
    lead = text[:61 * TILE + 5].copy()    # 62 tiles in front: the first group ends inside the 5-tile chunk
    plant(lead, pat, (0, 61 * TILE + 5 - plen))
    tail = text[70 * TILE:70 * TILE + 130 * TILE + 29].copy()
    plant(tail, pat, (63 * TILE - 2, 64 * TILE, 129 * TILE + 29 - plen))
    blocks = [lead] + small + [tail]
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] >= 12
    gate = base.gate_expected(model, blocks, pat)
    sk.bind(blocks, packed_fill=(pat + b"\n" + pat[1:] + b" ") if packed else None)
    build_with_absent_needle(sk, oracle, blocks)
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(GATED)
    assert async_many(sk) == [want["count_matches"]] * 3
    sk.check_routes(want, (plen, packed))
    base.check_name(sk, gate, "after every route")
    sk.check_routes(want, (plen, packed, "again"))
    assert async_many(sk) == [want["count_matches"]] * 3


# ---- candidate counts: none, exactly one, every tile --------------------------------------------------------------------
def test_no_candidate_one_candidate_every_tile_a_candidate(sk, oracle, model, text):
    rng = np.random.Generator(np.random.PCG64(8300))
    one, every = needle(rng, 8), needle(rng, 8)
    n = 300
    b = text[:n * TILE - 77].copy()
    plant(b, one, (171 * TILE + 5000,))
    plant(b, every, [t * TILE + 2000 + 3 * t for t in range(n)])
    blocks = [b]
    assert passing_tiles(model, blocks, ABSENT) == 0
    assert passing_tiles(model, blocks, one) == 1
    assert passing_tiles(model, blocks, every) == n
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)  # no candidate, and the calls behind it are right
    sk.ctx.set_pattern(one)
    assert sk.name().endswith(GATED)
    assert async_many(sk) == [1] * 3
    sk.check_routes(oracle_all_modes(oracle, blocks, one), "one candidate")
    assert sk.name().endswith(GATED)
    # every tile: through the stream-ordered call ahead of any verdict the list holds all 300 tiles ...
    sk.ctx.set_pattern(every)
    assert sk.name().endswith(GATED)
    assert async_many(sk) == [n] * 3
    # ... and the synchronous call takes the verdict, which switches the gate off
    want = oracle_all_modes(oracle, blocks, every)
    assert want["count_matches"] == n
    sk.check_routes(want, "every tile")
    assert GATED not in sk.name()
    sk.ctx.set_pattern(ABSENT)
    assert async_many(sk) == [0] * 3
    sk.ctx.set_pattern(one)
    assert async_many(sk) == [1] * 3


# ---- the stride loop: a grid much smaller than the list -----------------------------------------------------------------
@pytest.mark.parametrize("grid", (1, 3, 7))
def test_a_small_grid_strides_over_the_list(sk, oracle, model, text, grid):
    rng = np.random.Generator(np.random.PCG64(8400))
    pat = needle(rng, 8)
    b = text[:1100 * TILE - 9].copy()
    tiles = sorted(int(t) for t in rng.choice(1100, size=40, replace=False))
    plant(b, pat, [t * TILE + 3000 + t for t in tiles[:-1]] + [tiles[-1] * TILE + 40])
    blocks = [b]
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == 40 and passing_tiles(model, blocks, pat) == 40
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    sk.ctx.set_pattern(pat)
    os.environ["XSG_GATE_GRID"] = str(grid)
    assert sk.name().endswith(GATED)
    assert async_many(sk) == [40] * 3
    sk.check_routes(want, grid)
    assert sk.name().endswith(GATED)
    del os.environ["XSG_GATE_GRID"]  # and the default grid behind it, on the same words
    sk.check_routes(want, (grid, "default grid"))


# ---- the count word at rest ---------------------------------------------------------------------------------------------
def test_count_and_ticket_are_at_rest_behind_every_pass(sk, oracle, model, text):
    rng = np.random.Generator(np.random.PCG64(8500))
    many, one = needle(rng, 8), needle(rng, 9)

    def shard_of(n, salt):
        b = text[salt * TILE:(salt + n) * TILE - 5].copy()
        hits = [t for t in range(n) if t % 3 != 1]
        plant(b, many, [t * TILE + 1000 + t for t in hits])
        plant(b, one, ((n // 2) * TILE + 7000,))
        return [b], len(hits)

    def round_of(blocks, which):
        for pat, want in which:
            assert oracle_all_modes(oracle, blocks, pat)["count_matches"] == want
            sk.ctx.set_pattern(pat)  # never a synchronous call with it: no verdict, every pass selects
            assert sk.name().endswith(GATED)
            assert async_many(sk) == [want] * 3, pat

    blocks, n_many = shard_of(500, 0)
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    round_of(blocks, ((many, n_many), (one, 1), (ABSENT, 0), (many, n_many)))
    for n, salt in ((90, 40), (1090, 3)):  # a smaller binding, then a larger one
        blocks, n_many = shard_of(n, salt)
        sk.bind(blocks)
        assert GATED not in sk.name()
        build_with_absent_needle(sk, oracle, blocks)
        round_of(blocks, ((many, n_many), (one, 1), (ABSENT, 0)))
    sk.ctx.set_pattern(one)
    sk.check_routes(oracle_all_modes(oracle, blocks, one), "synchronous, at the end")


# ---- gated launches back to back without a finish between them ----------------------------------------------------------
def test_count_after_a_gated_timing_loop(sk, oracle, model, text):
    rng = np.random.Generator(np.random.PCG64(8600))
    pat = needle(rng, 9)
    b = text[:400 * TILE + 31].copy()
    plant(b, pat, [t * TILE + 11 * t for t in (0, 63, 64, 200, 255, 256, 399)] + [400 * TILE + 31 - 9])
    blocks = [b]
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] == 8
    sk.bind(blocks)
    sk.ctx.set_pattern(pat)
    assert sk.count() == 8
    assert sk.name().endswith(GATED)
    for _ in range(2):
        sk.shard.time_scan_kernel(xsg.COUNT_MATCHES, 5)
        assert sk.name().endswith(GATED)
        assert sk.count() == 8
        assert async_many(sk) == [8] * 3
        assert sk.offsets() == want["match_byte_offsets"]
        sk.shard.time_scan_kernel(xsg.COUNT_MATCHES, 2)
        assert async_many(sk) == [8] * 3
        assert sk.count_begin_end() == 8
    sk.shard.tune(xsg.COUNT_MATCHES)  # the tuner sweeps the stagger on the strided kernel
    assert sk.name().endswith(GATED)
    sk.check_routes(want, "after tune")
