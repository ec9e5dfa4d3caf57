"""The per-tile 4-gram sketch of a binding and the gate it puts in front of the plain count pass (k_scan<..., GATED>;
x-search_amd/csrc/xsg_sketch.h, xsg_count.cpp: sketch_before_pass), on shards of a few tiles to a few MiB.

XSG_SKETCH_MIN_BYTES=0 (read when the context is created) lets bindings of any size build one.  Every result is compared
with the oracle; which kernel ran is read from xsg_scan_kernel_name, which ends in GATED when the next plain count pass
of the binding would run behind the gate.
"""
import os

import numpy as np
import pytest

import corpus
import sketch_model
import xsg
from gpu_util import oracle_all_modes, oracle_regex_all_modes, upload

pytestmark = pytest.mark.gpu
TILE = 16384
GATED = " gated by xsg::k_sketch (512 B/tile)"
NEEDLE_LENGTHS = (4, 5, 8, 9, 31, 32, 33, 40, 300)


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


# Text of few distinct 4-grams (a tile's sketch fills to a few per cent), so that the gate of a planted needle -- even of
# a single gram -- lets few tiles through.  Random bytes would do the opposite: 16 K distinct grams fill a tile's 4096 bits.
WORDS = [b"that", b"with", b"have", b"this", b"from", b"they", b"which", b"would"]


def _text(rng, n):
    return corpus.text_block(int(rng.integers(1, 1 << 30)), 0, max(int(n), 2), needle_rate=0.0, lexicon=WORDS)[:n].copy()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return sketch_model.load(tmp_path_factory.mktemp("sketch_model"))


def gate_expected(model, blocks, pat: bytes):
    """What the verdict (fewer than a quarter of the tiles pass) should be by the CPU model: True / False, or None where the
    share is too close to the rule's quarter to call (the device sketch is a superset of the model's by the bytes that
    follow a chunk's end).  A long needle is judged at every filter window it may be counted at."""
    firsts = [0] if len(pat) <= 8 else range(0, len(pat) - 7)
    shares = [sketch_model.pass_share(model, blocks, pat, f) for f in firsts]
    if max(shares) < 0.20:
        return True
    if min(shares) > 0.30:
        return False
    return None


def check_name(sk, expected, where=""):
    if expected is not None:
        assert sk.name().endswith(GATED) == expected, (where, sk.name())


def _needle(rng, plen):
    return bytes(rng.integers(ord("A"), ord("Z") + 1, size=plen).astype(np.uint8))


def placed_blocks(rng, pat: bytes):
    """chunks with the needle at the places where a gate could lose it: starting in the last 1 .. plen bytes of a tile,
    in a chunk's last tile up to its last byte, in chunks of 3, 4, tile - 1, tile, tile + 1 and tile + 29 bytes -- and a
    chunk of 64 tiles without it, so that the tiles that hold it stay a small share (the verdict wants < 1/4)"""
    plen = len(pat)
    p = _u8(pat)
    blocks = []
    a = _text(rng, 5 * TILE + 777)
    for k, j in zip((1, 2, 3, 4), (1, plen, plen // 2 + 1, min(plen, 3))):
        o = k * TILE - j
        a[o:o + plen] = p
    a[a.size - plen:] = p  # the chunk's last bytes, in its last tile
    blocks.append(a)
    for length in (3, 4, TILE - 1, TILE, TILE + 1, TILE + 29):
        b = _text(rng, length)
        if plen <= length:
            b[length - plen:] = p
            if 2 * plen <= length:
                b[:plen] = p
        blocks.append(b)
    blocks.append(_text(rng, 64 * TILE))
    return blocks


def upload_packed(blocks, fill: bytes):
    """tightly packed: capacity = sum(round_up16(length)), the pad bytes behind every chunk end and a guard on either side
    hold `fill` repeated -- bytes of another text, needles included, that belong to no chunk"""
    import torch
    guard = 4096
    lengths = np.array([int(b.size) for b in blocks], dtype=np.uint64)
    padded = (lengths + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    offsets = np.concatenate([[np.uint64(0)], np.cumsum(padded)[:-1]]).astype(np.uint64)
    cap = int(padded.sum())
    host = np.resize(_u8(fill), guard + cap + guard)
    for o, b in zip(offsets, blocks):
        host[guard + int(o):guard + int(o) + b.size] = b
    t = torch.from_numpy(host).to("cuda:0")
    return t, t.data_ptr() + guard, cap, xsg.make_chunks(offsets, lengths)


class Sketched:
    """one context (XSG_SKETCH_MIN_BYTES=0 unless min_bytes says otherwise) and one shard"""

    def __init__(self, min_bytes="0"):
        import torch
        self.torch = torch
        old = os.environ.get("XSG_SKETCH_MIN_BYTES")
        if min_bytes is None:
            os.environ.pop("XSG_SKETCH_MIN_BYTES", None)
        else:
            os.environ["XSG_SKETCH_MIN_BYTES"] = min_bytes
        try:
            self.ctx = xsg.Context(0)
        finally:
            os.environ.pop("XSG_SKETCH_MIN_BYTES", None) if old is None else os.environ.__setitem__("XSG_SKETCH_MIN_BYTES", old)
        self.shard = None
        self.keep = None
        self.stream = torch.cuda.Stream()
        self.buf = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")

    def bind(self, blocks, packed_fill=None):
        if packed_fill is None:
            t, chunks = upload(blocks)
            base, cap = t.data_ptr(), t.numel()
        else:
            t, base, cap, chunks = upload_packed(blocks, packed_fill)
        self.torch.cuda.synchronize()
        if self.shard is None:
            self.shard = xsg.Shard(self.ctx, base, cap, chunks)
        else:
            self.shard.rebind(base, cap, chunks)
        self.keep = t

    def name(self, mode=xsg.COUNT_MATCHES):
        return self.shard.scan_kernel_name(mode)

    def count(self):
        return int(self.shard.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES])

    def count_async(self):
        self.buf.fill_(-1)
        self.torch.cuda.synchronize()
        self.shard.count_async(xsg.COUNT_MATCHES, self.stream.cuda_stream, self.buf.data_ptr())
        self.stream.synchronize()
        return int(self.buf[xsg.CTR_MATCHES].item())

    def count_begin_end(self):
        self.shard.count_begin(xsg.COUNT_MATCHES)
        return int(self.shard.count_end()[xsg.CTR_MATCHES])

    def offsets(self):
        return self.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist()

    def check_routes(self, want, where):
        assert self.count() == want["count_matches"], (where, "count")
        assert self.count_async() == want["count_matches"], (where, "count_async")
        assert self.count_begin_end() == want["count_matches"], (where, "count_begin/count_end")
        assert self.offsets() == want["match_byte_offsets"], (where, "match_byte_offsets")

    def close(self):
        self.torch.cuda.synchronize()
        self.ctx.close()


@pytest.fixture
def sk():
    saved = os.environ.pop("XSG_SKETCH", None)
    s = Sketched()
    yield s
    s.close()
    os.environ.pop("XSG_SKETCH", None)
    if saved is not None:
        os.environ["XSG_SKETCH"] = saved


@pytest.mark.parametrize("packed", (False, True), ids=("spaced", "packed"))
@pytest.mark.parametrize("plen", NEEDLE_LENGTHS)
def test_every_count_route_ungated_then_gated(sk, oracle, model, plen, packed):
    rng = np.random.Generator(np.random.PCG64(7000 + plen))
    pat = _needle(rng, plen)
    blocks = placed_blocks(rng, pat)
    want = oracle_all_modes(oracle, blocks, pat)
    assert want["count_matches"] >= 8
    gate = gate_expected(model, blocks, pat)
    assert gate or plen < 8  # from 8 bytes on the gate must be what this test runs behind
    # packed: behind every chunk end, in its pad bytes, lies the needle again (and around the whole buffer)
    sk.bind(blocks, packed_fill=(pat + b"\n" + pat[1:] + b" ") if packed else None)
    sk.ctx.set_pattern(pat)
    os.environ["XSG_SKETCH"] = "0"  # the feature off: the full scan
    assert GATED not in sk.name()
    sk.check_routes(want, "ungated")
    assert GATED not in sk.name()
    del os.environ["XSG_SKETCH"]
    # a synchronous entry point builds the sketch before its second eligible pass over the binding
    assert sk.count() == want["count_matches"]
    assert GATED not in sk.name()
    assert sk.count() == want["count_matches"]
    check_name(sk, gate, "second pass")
    sk.check_routes(want, "gated")
    check_name(sk, gate, "after every route")
    assert GATED not in sk.name(xsg.COUNT_LINES)  # count_lines stays on the full scan
    assert int(sk.shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == want["count_lines"]
    assert sk.count() == want["count_matches"]


def test_async_before_any_verdict_gates_on_an_existing_sketch(sk, oracle, model):
    """xsg_count_async never builds and never measures: with a sketch in place and no verdict for the pattern it gates"""
    rng = np.random.Generator(np.random.PCG64(7100))
    pat, other = _needle(rng, 8), _needle(rng, 12)
    blocks = placed_blocks(rng, pat)
    for k, b in enumerate(blocks[:3]):
        if b.size > 2 * len(other):
            b[1:1 + len(other)] = _u8(other)
    os.environ["XSG_SKETCH"] = "1"  # build before the first pass
    assert gate_expected(model, blocks, pat) and gate_expected(model, blocks, other)
    sk.bind(blocks)
    sk.ctx.set_pattern(pat)
    assert sk.count_async() == oracle_all_modes(oracle, blocks, pat)["count_matches"]  # no sketch yet: the full scan
    assert GATED not in sk.name()
    assert sk.count() == oracle_all_modes(oracle, blocks, pat)["count_matches"]
    assert sk.name().endswith(GATED)
    sk.ctx.set_pattern(other)  # a new pattern serial: no verdict
    assert sk.name().endswith(GATED)
    want = oracle_all_modes(oracle, blocks, other)
    assert want["count_matches"] >= 1
    assert sk.count_async() == want["count_matches"]
    sk.check_routes(want, "second pattern")


def test_a_needle_whose_grams_are_everywhere_switches_the_gate_off(sk, oracle):
    blocks = [corpus.text_block(77, i, 300_000 + 1111 * i, needle_rate=5e-4) for i in range(3)]
    os.environ["XSG_SKETCH"] = "1"
    sk.bind(blocks)
    for pat in (b"Holmes", b"that", b"detective street"):
        sk.ctx.set_pattern(pat)
        want = oracle_all_modes(oracle, blocks, pat)
        assert sk.count() == want["count_matches"]
        assert GATED not in sk.name(), pat  # the verdict: most tiles pass
        sk.check_routes(want, pat)
    sk.ctx.set_pattern(b"Sherlock")  # planted every ~10 KiB here: it is in most tiles too
    want = oracle_all_modes(oracle, blocks, b"Sherlock")
    sk.check_routes(want, "Sherlock, dense")


def test_ineligible_patterns_are_never_gated(sk, oracle, model):
    blocks = [corpus.text_block(78, i, 400_000 + 999 * i) for i in range(2)] + [corpus.text_block(79, 0, 40 * TILE)]
    blocks[0][5 * TILE - 3:5 * TILE + 5] = _u8(b"Sherlock")
    os.environ["XSG_SKETCH"] = "1"
    sk.bind(blocks)
    assert gate_expected(model, blocks, b"Sherlock")
    sk.ctx.set_pattern(b"Sherlock")
    want = oracle_all_modes(oracle, blocks, b"Sherlock")
    sk.check_routes(want, "Sherlock")
    assert sk.name().endswith(GATED)  # the binding has a sketch and it pays for this needle
    for pat, flags in ((b"She", 0), (b"sherlock", xsg.FLAG_IGNORE_CASE), (b"She[r ]lock", xsg.FLAG_REGEX),
                       (b"colou?r|lock(ed|s)?", xsg.FLAG_REGEX)):
        sk.ctx.set_pattern(pat, flags)
        if flags & xsg.FLAG_REGEX:
            want, _ = oracle_regex_all_modes(oracle, blocks, pat, False)
        else:
            want = oracle_all_modes(oracle, blocks, pat, ignore_case=bool(flags & xsg.FLAG_IGNORE_CASE))
        for _ in range(2):
            assert GATED not in sk.name(), pat
            assert sk.count() == want["count_matches"], pat
        assert sk.offsets() == want["match_byte_offsets"], pat
        assert GATED not in sk.name(xsg.COUNT_LINES), pat
    sk.ctx.set_pattern(b"Sherlock")
    want = oracle_all_modes(oracle, blocks, b"Sherlock")
    assert GATED not in sk.name(xsg.COUNT_LINES)
    assert int(sk.shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == want["count_lines"]
    c = sk.shard.count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)
    assert (int(c[xsg.CTR_MATCHES]), int(c[xsg.CTR_NEWLINES])) == (want["count_matches"], want["newlines"])


@pytest.mark.parametrize("overlapping", (False, True))
def test_a_bordered_needle_through_the_overlap_check(sk, oracle, model, overlapping):
    rng = np.random.Generator(np.random.PCG64(7300 + overlapping))
    blocks = [_text(rng, 3 * TILE + 100), _text(rng, 40 * TILE)]
    for o in (5, TILE - 2, 2 * TILE - 4, 3 * TILE + 96):
        blocks[0][o:o + 4] = _u8(b"abab")
    if overlapping:
        blocks[0][2 * TILE + 50:2 * TILE + 58] = _u8(b"abababab")
        blocks[0][TILE - 4:TILE + 2] = _u8(b"ababab")
    os.environ["XSG_SKETCH"] = "1"
    sk.bind(blocks)
    sk.ctx.set_pattern(b"abab")
    want = oracle_all_modes(oracle, blocks, b"abab")
    sk.check_routes(want, "abab")
    sk.check_routes(want, "abab again")
    check_name(sk, gate_expected(model, blocks, b"abab"))


def test_rewritten_bytes_invalidate_and_a_larger_rebind(sk, oracle, model):
    rng = np.random.Generator(np.random.PCG64(7400))
    pat = _needle(rng, 8)
    blocks = placed_blocks(rng, pat)
    os.environ["XSG_SKETCH"] = "1"
    sk.bind(blocks)
    sk.ctx.set_pattern(pat)
    want = oracle_all_modes(oracle, blocks, pat)
    assert gate_expected(model, blocks, pat)
    sk.check_routes(want, "before")
    assert sk.name().endswith(GATED)
    # other bytes of the same lengths, in place: the needle moves into tiles whose old sketch does not hold it
    fresh = [_text(rng, b.size) for b in blocks]
    for b in fresh:
        if b.size >= 3 * TILE:
            for o in (TILE + 100, 2 * TILE - 5, b.size - len(pat)):
                b[o:o + len(pat)] = _u8(pat)
    off, _, cap = corpus.chunk_table([b.size for b in fresh])
    host = np.zeros(max(cap, 256), dtype=np.uint8)
    for o, b in zip(off, fresh):
        host[int(o):int(o) + b.size] = b
    sk.keep.copy_(sk.torch.from_numpy(host))
    sk.torch.cuda.synchronize()
    sk.shard.invalidate()
    assert GATED not in sk.name()  # no sketch until it is rebuilt
    want = oracle_all_modes(oracle, fresh, pat)
    assert gate_expected(model, fresh, pat)
    assert want["count_matches"] != oracle_all_modes(oracle, blocks, pat)["count_matches"]
    assert sk.count_async() == want["count_matches"]  # the stream-ordered entry point builds none
    assert GATED not in sk.name()
    sk.check_routes(want, "after invalidate")
    assert sk.name().endswith(GATED)
    # a re-bind to a larger table: more chunks, more tiles
    more = fresh + placed_blocks(rng, pat)
    assert gate_expected(model, more, pat)
    sk.bind(more)
    assert GATED not in sk.name()
    want = oracle_all_modes(oracle, more, pat)
    sk.check_routes(want, "after the re-bind")
    assert sk.name().endswith(GATED)
    sk.check_routes(want, "after the re-bind, gated")


def test_tune_builds_the_sketch_only_above_the_size_limit(oracle, model):
    rng = np.random.Generator(np.random.PCG64(7500))
    pat = _needle(rng, 8)
    blocks = placed_blocks(rng, pat)
    want = oracle_all_modes(oracle, blocks, pat)
    assert gate_expected(model, blocks, pat)
    saved = os.environ.pop("XSG_SKETCH", None)
    try:
        for min_bytes, gated in (("0", True), (None, False)):  # None: the default limit, 64 MiB
            s = Sketched(min_bytes)
            try:
                s.bind(blocks)
                s.ctx.set_pattern(pat)
                s.shard.tune(xsg.COUNT_MATCHES)
                assert s.name().endswith(GATED) == gated, (min_bytes, s.name())
                s.check_routes(want, f"after tune, limit {min_bytes}")
                s.check_routes(want, f"after tune, limit {min_bytes}, again")
                assert s.name().endswith(GATED) == gated
            finally:
                s.close()
    finally:
        if saved is not None:
            os.environ["XSG_SKETCH"] = saved


def test_count_after_a_timing_loop_and_after_a_list_pass(sk, oracle, model):
    """both leave the per-tile arrays dirty: the gated pass that follows must find them cleaned"""
    rng = np.random.Generator(np.random.PCG64(7600))
    pat = _needle(rng, 9)
    blocks = placed_blocks(rng, pat)
    want = oracle_all_modes(oracle, blocks, pat)
    assert gate_expected(model, blocks, pat)
    os.environ["XSG_SKETCH"] = "1"
    sk.bind(blocks)
    sk.ctx.set_pattern(pat)
    assert sk.count() == want["count_matches"]
    assert sk.name().endswith(GATED)
    for _ in range(2):
        sk.shard.time_scan_kernel(xsg.COUNT_MATCHES, 3)
        assert sk.count() == want["count_matches"]
        assert sk.count_async() == want["count_matches"]
        assert sk.offsets() == want["match_byte_offsets"]
        assert sk.count_async() == want["count_matches"]
        assert sk.shard.search_u64(xsg.LINE_BYTE_OFFSETS).tolist() == want["line_byte_offsets"]
        assert sk.count() == want["count_matches"]
        assert int(sk.shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == want["count_lines"]
        assert sk.count_begin_end() == want["count_matches"]
