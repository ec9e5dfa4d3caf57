"""The finishing form of the gated count pass: k_scan_fin (x-search_amd/csrc/xsg_kernels.hip: gated_pass<..., FIN>).  A plain
match count behind the gate sums in registers, walks the end-of-chunk zones that hold an occurrence itself -- from an entry
it finds by walking the chunk's tiles backwards -- and writes the counters: one launch, no k_count_finish, no word of the
per-tile arrays written.

XSG_SKETCH=1 and XSG_SKETCH_MIN_BYTES=0; text and helpers of tests/test_gpu_sketch.py, test_gpu_sketch_select.py and
test_gpu_gated_fused.py are reused.  Every case asserts the name of the form it runs on and compares count, three
back-to-back count_async calls without a host sync, count_async_status and count_begin / count_end with the oracle, before
and after a list call (match_byte_offsets) on the same binding.  Needles are made of distinct bytes (no border: their
count never goes through a list) and every binding keeps the share of tiles that hold one under the verdict's quarter.
"""
import os

import numpy as np
import pytest

import test_gpu_sketch as base
import xsg
from test_gpu_call_sequences import shard_state
from test_gpu_gated_fused import UNIT
from test_gpu_sketch import GATED, TILE, Sketched
from test_gpu_sketch_select import async_many, build_with_absent_needle, plant

pytestmark = pytest.mark.gpu
FIN = " finishing (xsg::k_scan_fin)" + GATED
LETTERS = b"SHERLOCKXYZABDFGIJMNPQTUVW0123456789#$%&"  # distinct bytes, none of them in the lexicon's lower-case text


def needle(plen):
    assert plen <= len(LETTERS)
    return LETTERS[:plen]


@pytest.fixture(scope="module")
def text():
    rng = np.random.Generator(np.random.PCG64(9900))
    t = base._text(rng, 700 * TILE)
    t.setflags(write=False)
    return t


@pytest.fixture
def sk():
    saved = {k: os.environ.pop(k, None) for k in ("XSG_SKETCH", "XSG_GATE_GRID")}
    os.environ["XSG_SKETCH"] = "1"  # a synchronous call builds the sketch before its first eligible pass
    s = Sketched()
    s.status = s.torch.zeros(1, dtype=s.torch.int64, device="cuda:0")
    yield s
    s.close()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def wanted(oracle, blocks, pat):
    """-> (count, global match offsets) by the oracle, chunk by chunk"""
    n, offs, g = 0, [], 0
    for b in blocks:
        n += oracle.count(b, pat, False)
        offs += [int(x) + g for x in oracle.byte_offsets_match(b, pat)]
        g += int(b.size)
    assert n == len(offs)
    return n, offs


def count_with_status(sk):
    sk.buf.fill_(-1)
    sk.status.fill_(-1)
    sk.torch.cuda.synchronize()
    sk.shard.count_async_status(xsg.COUNT_MATCHES, sk.stream.cuda_stream, sk.buf.data_ptr(), sk.status.data_ptr())
    sk.stream.synchronize()
    return [int(x) for x in sk.buf.tolist()], int(sk.status.item())


def every_count_call(sk, n, nbytes, where, name=FIN):
    assert sk.name().endswith(name), (where, sk.name())
    assert sk.count() == n, (where, "count")
    assert sk.name().endswith(name), (where, "the verdict switched the gate off", sk.name())
    assert async_many(sk) == [n] * 3, (where, "count_async x 3")
    assert count_with_status(sk) == ([n, 0, 0, nbytes], 0), (where, "count_async_status")
    assert sk.count_begin_end() == n, (where, "count_begin / count_end")


def check(sk, oracle, blocks, pat, where, name=FIN):
    """a new pattern (no verdict: the stream-ordered call gates on the sketch as it is), every count call, a list call,
    every count call again"""
    n, offs = wanted(oracle, blocks, pat)
    nbytes = sum(int(b.size) for b in blocks)
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(name), (where, sk.name())
    assert async_many(sk) == [n] * 3, (where, "ahead of any verdict")
    every_count_call(sk, n, nbytes, where, name)
    assert sk.offsets() == offs, (where, "match_byte_offsets")
    every_count_call(sk, n, nbytes, (where, "after the list call"), name)
    return n


# ---- chunk lengths around the zone and the tile border ------------------------------------------------------------------
def edge_lengths(plen, k=2):
    short = (1, plen - 1, plen, plen + 30, plen + 31, plen + 32, TILE - 1, TILE, TILE + 1)
    return short + tuple(k * TILE + r for r in (1, plen - 1, plen, plen + 15, plen + 31))


def zone_variants(text, salt, L, pat, border):
    """chunks of L bytes: no needle; needles in the zone before the tile border, behind it, on both sides, across it; and a
    needle behind a partial prefix (the lossy scalar part skips it for some entries) with another one ahead of the zone"""
    plen = len(pat)
    Z = max(L - plen - 31, 0)
    out = []

    def chunk(spots, prefix_at=None):
        b = text[salt * 977 % (600 * TILE):][:L].copy()
        ok = [o for o in spots if 0 <= o <= L - plen]
        plant(b, pat, ok)
        if prefix_at is not None and prefix_at >= 1:
            b[prefix_at - 1] = pat[0]
        out.append(b)

    chunk([])
    if L < plen:
        return out
    chunk([L - plen])
    chunk([Z], prefix_at=Z)
    if border is not None and Z < border < L:
        before = border - plen if border - plen >= Z else None
        after = border if border + plen <= L else None
        across = border - plen // 2 if border - plen // 2 >= Z and border - plen // 2 + plen <= L else None
        for spots in ([before], [after], [before, after], [across]):
            if None not in spots:
                chunk(spots)
                chunk(spots + [max(Z - 2 * plen - 3, 0)], prefix_at=spots[0])  # an occurrence ahead of the zone: the entry
    return out


@pytest.mark.parametrize("grid", (1, 2, None), ids=("grid1", "grid2", "default_grid"))
@pytest.mark.parametrize("packed", (False, True), ids=("spaced", "packed"))
@pytest.mark.parametrize("plen", (4, 5, 8, 9, 33))
def test_chunk_lengths_many_chunks_in_a_unit(sk, oracle, text, plen, packed, grid):
    pat = needle(plen)
    blocks = []
    for i, L in enumerate(edge_lengths(plen)):
        blocks += zone_variants(text, 31 * i + plen, L, pat, 2 * TILE if L > 2 * TILE else None)
    tiles = sum((b.size + TILE - 1) // TILE for b in blocks)
    assert len(blocks) >= 40 and tiles < UNIT  # the chunks share the first unit ...
    blocks.append(text[:3 * tiles * TILE + 3].copy())  # ... and a chunk without a needle keeps the passing share low
    sk.bind(blocks, packed_fill=(pat + b"\n" + pat[1:] + b" " + pat[:1]) if packed else None)
    build_with_absent_needle(sk, oracle, blocks)
    if grid is not None:
        os.environ["XSG_GATE_GRID"] = str(grid)
    n = check(sk, oracle, blocks, pat, (plen, packed, grid))
    assert n >= 20


@pytest.mark.parametrize("plen", (4, 8, 33))
def test_chunk_lengths_one_chunk_per_binding(sk, oracle, text, plen):
    pat = needle(plen)
    k = 12  # tiles ahead of the border: at most two of the chunk's tiles hold a needle
    total = 0
    for i, r in enumerate((1, plen - 1, plen, plen + 15, plen + 31)):
        for j, b in enumerate(zone_variants(text, 7 * i + plen, k * TILE + r, pat, k * TILE)[3:]):
            sk.bind([b])
            build_with_absent_needle(sk, oracle, [b])
            total += check(sk, oracle, [b], pat, (plen, r, j))
    assert total >= 10


# ---- the walk's entry ---------------------------------------------------------------------------------------------------
def entry_chunk(text, salt, ntiles, pat, place, shift):
    """The zone (in the chunk's last tile) holds the needle behind a partial prefix.  The last occurrence ahead of the zone
    sits `shift` bytes before a fixed spot of: the zone's tile, the tile before it, tile 1 of the chunk; or nowhere.  A tile
    in between holds the needle's grams apart: it passes the sketch and holds no occurrence."""
    plen = len(pat)
    L = (ntiles - 1) * TILE + 3000
    Z = L - plen - 31
    b = text[salt * 1013 % (300 * TILE):][:L].copy()
    b[L - plen - 6] = pat[0]
    plant(b, pat, (L - plen - 5,))
    mid = (ntiles - 3) * TILE + 500
    plant(b, pat[:5], (mid,))
    plant(b, pat[2:], (mid + 200,))
    spot = {"zone_tile": Z - plen, "previous_tile": (ntiles - 1) * TILE - 2 * plen, "far": TILE + 100, "nowhere": None}[place]
    if spot is not None:
        plant(b, pat, (spot - shift,))
    return b, Z


def tail_counts(oracle, chunks, pat):
    """what the zone contributes per chunk: the oracle's count minus the occurrences that start ahead of the zone"""
    out = []
    for b, Z in chunks:
        ahead = sum(1 for o in oracle.byte_offsets_match(b[:Z + len(pat) - 1], pat) if int(o) < Z)
        out.append(oracle.count(b, pat, False) - ahead)
    return out


@pytest.mark.parametrize("place", ("zone_tile", "previous_tile", "nowhere"))
def test_entry_at_32_consecutive_positions(sk, oracle, text, place):
    pat = needle(8)
    chunks = [entry_chunk(text, s, 15, pat, place, s) for s in range(32)]
    blocks = [b for b, _ in chunks]
    if place != "nowhere":  # the cases depend on the entry: a pass that ignored it could not count them all
        assert len(set(tail_counts(oracle, chunks, pat))) == 2
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    check(sk, oracle, blocks, pat, place)
    os.environ["XSG_GATE_GRID"] = "1"
    check(sk, oracle, blocks, pat, (place, "grid 1"))


def test_entry_300_tiles_back_in_another_unit(sk, oracle, text):
    pat = needle(8)
    chunks = [entry_chunk(text, s, 303, pat, "far", s) for s in range(32)]  # the oracle on all of them, the GPU on two
    assert len(set(tail_counts(oracle, chunks, pat))) == 2
    by_tail = {}
    for (b, _), t in zip(chunks, tail_counts(oracle, chunks, pat)):
        by_tail.setdefault(t, b)
    blocks = list(by_tail.values())  # one chunk per tail count
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    check(sk, oracle, blocks, pat, "far")


# ---- what keeps the two launches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("plen", (34, 40))
def test_long_needles_with_the_lossy_tail_keep_the_finish_kernel(sk, oracle, text, plen):
    pat = needle(plen)
    blocks = []
    for i, L in enumerate(edge_lengths(plen)):
        blocks += zone_variants(text, 17 * i + plen, L, pat, 2 * TILE if L > 2 * TILE else None)
    tiles = sum((b.size + TILE - 1) // TILE for b in blocks)
    blocks.append(text[:3 * tiles * TILE + 3].copy())
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(GATED) and "finishing" not in sk.name()
    check(sk, oracle, blocks, pat, plen, name=GATED)
    assert "finishing" not in sk.name()
    sk.ctx.set_pattern(pat, xsg.FLAG_EXACT_TAIL)  # no zone to walk: any length finishes in its pass
    assert sk.name().endswith(FIN)
    oracle.set_exact(True)
    try:
        n = sum(oracle.count(b, pat, False) for b in blocks)
    finally:
        oracle.set_exact(False)
    assert async_many(sk) == [n] * 3
    assert sk.count() == n


def test_state_next_to_the_storing_form(sk, oracle, text):
    """a count with newline totals keeps the two launches; a list route and such a count behind a finishing pass are right;
    the binding's bookkeeping says what happened to tile_cnt: the finishing form neither writes nor reads it"""
    pat = needle(8)
    blocks = []
    for i, L in enumerate(edge_lengths(8)):
        blocks += zone_variants(text, 13 * i, L, pat, 2 * TILE if L > 2 * TILE else None)
    tiles = sum((b.size + TILE - 1) // TILE for b in blocks)
    blocks.append(text[:3 * tiles * TILE + 3].copy())
    n, offs = wanted(oracle, blocks, pat)
    newlines = sum(oracle.count_newlines(b) for b in blocks)
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(FIN)
    assert "finishing" not in sk.name(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)
    assert "finishing" not in sk.name(xsg.MATCH_BYTE_OFFSETS) and "finishing" not in sk.name(xsg.COUNT_LINES)

    def with_newlines():
        c = sk.shard.count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)
        return int(c[xsg.CTR_MATCHES]), int(c[xsg.CTR_NEWLINES])

    assert sk.count() == n
    assert shard_state(sk.shard)["cnt_clean"] == 1
    assert sk.offsets() == offs
    assert shard_state(sk.shard)["cnt_clean"] == 0  # the list route left its tile counts in place
    assert async_many(sk) == [n] * 3               # (the pass cleans them for whoever stores next; it does not read them)
    assert shard_state(sk.shard)["cnt_clean"] == 1
    assert with_newlines() == (n, newlines)        # the two launches, on per-tile arrays the finishing passes left at rest
    assert shard_state(sk.shard)["cnt_clean"] == 1
    assert sk.count() == n
    assert with_newlines() == (n, newlines)
    assert sk.offsets() == offs
    assert async_many(sk) == [n] * 3
    assert sk.shard.time_scan_kernel(xsg.COUNT_MATCHES, 3) > 0  # times the finishing form, into scratch counters
    assert shard_state(sk.shard)["cnt_clean"] == 1             # ... so a timing loop leaves the tile counts at rest too
    assert sk.count() == n
    assert async_many(sk) == [n] * 3
    assert sk.offsets() == offs
