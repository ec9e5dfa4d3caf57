"""xsg_count_literals_chunks / xsg_count_literals_chunks_async: a count per bound chunk and literal of a list, and the number
of chunks that hold each literal, in one pass.

Expected values are tests/literal_matrix_model.py's (tests/literal_counts_model.py per chunk): exact equality everywhere.
Every case runs the synchronous form, the same with every flush a sweep (XSG_LITMATRIX_TOUCHED=0), once more without
chunks_with, and the stream-ordered form on a side stream into buffers pre-filled with 0xFF that are 8 words longer than
needed; the column sums are compared with xsg_count_literals on the same binding."""
import ctypes as C
import os

import numpy as np
import pytest

import corpus
import literal_counts_model as LM
import literal_matrix_model as MM
import set_cases as SC
import xsg
from gpu_util import GpuSearch
from set_gpu_util import IC, bind_tight, list_all_modes

pytestmark = pytest.mark.gpu
TILE = SC.TILE
SPARE = 8


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


class Side:
    """a side stream for the stream-ordered form; the buffers are made per call, SPARE words longer than needed"""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()

    def run(self, shard, n, k, with_chunks=True):
        """-> (matrix rows, chunks_with or None)"""
        torch = self.torch
        m = torch.full((n * k + SPARE,), -1, dtype=torch.int64, device="cuda:0")  # every byte 0xFF
        w = torch.full((k + SPARE,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        shard.count_literals_chunks_async(self.stream.cuda_stream, m.data_ptr(), n * k, w.data_ptr() if with_chunks else 0,
                                          k if with_chunks else 0)
        self.stream.synchronize()
        gm, gw = m.cpu().numpy(), w.cpu().numpy()
        assert (gm[n * k:] == -1).all(), "words behind the matrix were written"
        assert (gw[k if with_chunks else 0:] == -1).all(), "words behind chunks_with were written"
        return gm[:n * k].reshape(n, k).tolist(), gw[:k].tolist() if with_chunks else None


@pytest.fixture(scope="module")
def side():
    return Side()


def with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sync(gs, with_chunks=True):
    m, w = gs.shard.count_literals_chunks(with_chunks)
    assert m.dtype == np.uint64 and (w is None) == (not with_chunks)
    return m.tolist(), None if w is None else w.tolist()


def check(gs, side, blocks, lits, flags, what, want=None):
    """every form against the model -> (the expected rows, the expected chunks_with)"""
    blocks = list(blocks)
    n, k = len(blocks), len(lits)
    rows = MM.matrix(blocks, lits, bool(flags & IC)) if want is None else want
    freq = MM.chunks_with(rows, k)
    gs.ctx.set_literals(xsg.literal_list(lits), flags)
    got = sync(gs)
    print(what, "n", n, "k", k, "sum", sum(map(sum, rows)), "chunks_with", freq[:12], "got", got[1][:12])
    assert got[0] == rows, (what, "synchronous, matrix")
    assert got[1] == freq, (what, "synchronous, chunks_with")
    assert with_env({"XSG_LITMATRIX_TOUCHED": "0"}, lambda: sync(gs)) == (rows, freq), (what, "every flush a sweep")
    assert sync(gs, False) == (rows, None), (what, "synchronous, no chunks_with")
    assert side.run(gs.shard, n, k) == (rows, freq), (what, "stream-ordered")
    assert side.run(gs.shard, n, k, False) == (rows, None), (what, "stream-ordered, no chunks_with")
    sums = [sum(r[j] for r in rows) for j in range(k)]
    assert gs.shard.count_literals().tolist() == sums, (what, "column sums against xsg_count_literals")
    return rows, freq


# ---- 1. text: about 1 MiB in 5 chunks, lists of 1, 2, 9 and 300 literals ---------------------------------------------------------
@pytest.mark.parametrize("flags", [0, IC], ids=["plain", "icase"])
@pytest.mark.parametrize("k", SC.LIST_SIZES)
def test_text(gs, side, k, flags):
    blocks = SC.text_blocks()
    lits = SC.word_list(k)
    gs.bind(list(blocks))
    rows, freq = check(gs, side, blocks, lits, flags, ("text", k, flags))
    assert sum(map(sum, rows)) > 0 and max(freq) == len(blocks)
    if k == 9:  # row c is count_literals() of a binding that holds block c alone
        for c, b in enumerate(blocks):
            gs.bind([b])
            gs.ctx.set_literals(xsg.literal_list(lits), flags)
            assert gs.shard.count_literals().tolist() == rows[c], ("text, chunk alone", c, flags)


# ---- 2. a boundary at every tile: hundreds of small chunks packed tightly, stale bytes behind every end -------------------------
def boundary_plan(g):
    """-> ((chunk, lack), ...): SC.end_plan(g), then chunks of 0..3000 bytes whose ends are whole occurrences, occurrences
    cut short by one byte (the bytes behind the end complete them: `lack`), or plain text; every 23rd is empty"""
    short, long_ = SC.END_LITS[g]
    plan = list(SC.end_plan(g))
    rng = np.random.Generator(np.random.PCG64(4200 + g))
    tails = [(long_, b""), (short, b""), (long_[:-1], long_[-1:]), (b"", b"")] + ([(short[:-1], short[-1:])] if g > 1 else [])
    for i in range(640):
        n = 0 if i % 23 == 5 else int(rng.integers(0, 3001))
        tail, lack = tails[i % len(tails)]
        if n < len(tail) + 8:
            plan.append((SC.u8(short * 17)[:n], b""))
            continue
        body = bytearray(SC._ending_in(tail, n).tobytes())
        for _ in range(int(rng.integers(0, 4))):  # occurrences inside the chunk as well
            lit = (short, long_)[int(rng.integers(0, 2))]
            at = int(rng.integers(0, n - len(tail) - len(lit)))
            body[at:at + len(lit)] = lit
        # (a lack that the chunk's own pad cannot hold would land in the next chunk: leave such an end alone)
        plan.append((SC.u8(body), lack if len(lack) <= -n % 16 else b""))
    return plan


def boundary_fill(g, plan):
    short, long_ = SC.END_LITS[g]

    def fill(i, n):  # the gap in FRONT of chunk i: it begins with what chunk i - 1 lacks; stale occurrences follow
        head = plan[i - 1][1] if i > 0 else b""
        return SC.u8((head + (b" " + long_ + b"\n" + short) * (n // 4 + 2))[:n])
    return fill


@pytest.mark.parametrize("flags", [0, IC], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_a_boundary_at_every_tile(gs, side, g, flags):
    plan = boundary_plan(g)
    blocks = [b for b, _ in plan]
    assert len(blocks) >= 600 and sum(1 for b in blocks if b.size == 0) >= 10
    assert sum(1 for _, lack in plan if lack) >= 100  # ends that only the stale bytes behind them complete
    bind_tight(gs, blocks, boundary_fill(g, plan))
    rows, freq = check(gs, side, blocks, SC.END_LITS[g], flags, ("boundaries", g, flags))
    # (by default every workgroup has one tile here) one workgroup and seven flush hundreds of times each
    for grid in ("1", "7"):
        assert with_env({"XSG_LITMATRIX_GRID": grid}, lambda: sync(gs)) == (rows, freq), ("boundaries", g, flags, "grid", grid)
    assert all(r == [0, 0] for r, b in zip(rows, blocks) if b.size == 0)
    assert min(freq) > 100 and max(freq) < len(blocks)


# ---- 3. a chunk shared by workgroups -----------------------------------------------------------------------------------------------
def shared_blocks():
    """about 12 tiles: chunks of 1, 2, 5, 1, 2, 1 tiles (none a whole number of tiles long), an empty one among them"""
    sizes = (TILE - 100, TILE + 77, 4 * TILE + 4097, 0, 333, 2 * TILE - 1, TILE - 15)
    return [corpus.text_block(17, i, n, needle_rate=2e-3) if n else np.zeros(0, dtype=np.uint8) for i, n in enumerate(sizes)]


def shared_literals(blocks):
    """seven bytes across each of the big chunk's four tile edges -- where one workgroup's range ends and the next one's
    begins -- then a dense letter, a bigram and a piece of another chunk"""
    big = blocks[2].tobytes()
    lits = []
    for t in range(1, 5):
        at = next(a for a in range(t * TILE - 6, t * TILE) if b"\n" not in big[a:a + 7])
        lits.append(big[at:at + 7])
    return tuple(lits) + (b"e", b"th", blocks[0].tobytes()[100:109].replace(b"\n", b" "))


def test_a_chunk_shared_by_workgroups(gs, side):
    blocks = shared_blocks()
    ntiles = sum((b.size + TILE - 1) // TILE for b in blocks)
    assert ntiles == 12 and (blocks[2].size + TILE - 1) // TILE == 5
    lits = shared_literals(blocks)
    rows = MM.matrix(blocks, lits)
    assert min(rows[2][:6]) > 0  # these occur in the big chunk: its row is written by several workgroups
    gs.bind(blocks)
    for grid in ("1", "2", "3", "5", "7", str(ntiles), str(ntiles + 5), None):
        got = with_env({"XSG_LITMATRIX_GRID": grid}, lambda: check(gs, side, blocks, lits, 0, ("shared", grid), want=rows))
        assert got[1] == MM.chunks_with(rows, len(lits)) and max(got[1]) <= len(blocks) - 1


# ---- 4. the touched list's edge ----------------------------------------------------------------------------------------------------
def distinct_literals(k):
    """k distinct literals of two and three bytes over an alphabet that holds no blank: none occurs across a blank"""
    alphabet = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789#%"
    two = [bytes((a, b)) for a in alphabet for b in alphabet]
    three = [bytes((a, b, c)) for a in alphabet[:16] for b in alphabet[:16] for c in alphabet[:16]]
    lits = two[:k - k // 4] + three[:k // 4]
    assert len(lits) == k == len(set(lits))
    return lits


def touched_sizes():
    t = xsg.literals_chunks_touched_capacity()  # read from the library: the kernel's kLitTouched
    return [t - 1, t, t + 1, xsg.MAX_LITERALS]


@pytest.mark.parametrize("which", range(4))
def test_the_touched_lists_edge(gs, side, which):
    k = touched_sizes()[which]
    assert 3 < k <= xsg.MAX_LITERALS
    lits = distinct_literals(k)
    spelled = SC.u8(b" ".join(lits))  # ONE chunk, below a tile, in which every literal occurs
    assert spelled.size < TILE
    few = SC.u8(b" ".join((lits[0], lits[k // 2], lits[-1])))  # beside it a chunk that holds three of them
    blocks = [few, spelled, few]
    gs.bind(blocks)
    rows, freq = check(gs, side, blocks, lits, 0, ("touched", k))
    assert min(rows[1]) >= 1 and min(freq) >= 1 and freq[0] == freq[-1] == 3
    assert sum(1 for v in rows[0] if v) < 40  # (a three-byte literal holds two-byte ones)
    # one workgroup walks all three chunks, and one per chunk
    for grid in ("1", "3"):
        assert with_env({"XSG_LITMATRIX_GRID": grid}, lambda: sync(gs)) == (rows, freq), ("touched", k, "grid", grid)


# ---- 5. dense and overlapping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lits,blocks", SC.ORDER_CASES, ids=[c[0] for c in SC.ORDER_CASES])
def test_prefix_infix_and_duplicate_literals_all_count(gs, side, name, lits, blocks):
    gs.bind(list(blocks))
    rows, freq = check(gs, side, blocks, lits, 0, name)
    dup = tuple(lits) + (lits[0], lits[-1])  # duplicates get the same number each
    drows, dfreq = check(gs, side, blocks, dup, 0, (name, "dup"))
    assert drows == [r + [r[0], r[-1]] for r in rows] and dfreq == freq + [freq[0], freq[-1]]
    if name == "aa-a-run":
        assert rows == [[65535, 65536]]


def test_dense_list_on_text(gs, side):
    blocks = SC.dense_blocks()
    gs.bind(list(blocks))
    rows, freq = check(gs, side, blocks, SC.DENSE_LIST, 0, "dense")
    assert max(rows[0]) > 20_000 and freq == [2, 2]


# ---- 6. refusals and edges ---------------------------------------------------------------------------------------------------------
def test_refusals(gs, side):
    import torch
    blocks = SC.raw_blocks()
    lits = SC.RAW_LIST
    n, k = len(blocks), len(lits)
    want = (MM.matrix(blocks, lits), MM.chunks_with(MM.matrix(blocks, lits), k))

    def good():
        gs.ctx.set_literals(xsg.literal_list(lits), 0)
        assert sync(gs) == want and side.run(gs.shard, n, k) == want

    fresh = GpuSearch()
    fresh.bind(blocks)
    with pytest.raises(xsg.XsgError) as e:  # the context holds no pattern
        fresh.shard.count_literals_chunks()
    assert e.value.code == xsg.ESTATE
    fresh.ctx.close()
    gs.bind(blocks)
    good()
    gs.ctx.set_pattern(b"caf", 0)
    for call in (lambda: gs.shard.count_literals_chunks(), lambda: side.run(gs.shard, n, k)):
        with pytest.raises(xsg.XsgError) as e:  # the pattern is no list
            call()
        assert e.value.code == xsg.ENOTSUP and "xsg_set_literals" in str(e.value)
    good()
    gs.ctx.set_literals(xsg.literal_list(lits), xsg.FLAG_INVERT)
    for call in (lambda: gs.shard.count_literals_chunks(), lambda: side.run(gs.shard, n, k)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "XSG_FLAG_INVERT" in str(e.value)
    good()
    lib, h = gs.shard._lib, gs.shard.h
    out = np.zeros(n * k + 2, dtype=np.uint64)
    freq = np.zeros(k + 2, dtype=np.uint64)
    dev = torch.zeros(n * k + 2, dtype=torch.int64, device="cuda:0")
    dfreq = torch.zeros(k + 2, dtype=torch.int64, device="cuda:0")
    po, pf, pd, pdf = (C.c_void_p(x) for x in (out.ctypes.data, freq.ctypes.data, dev.data_ptr(), dfreq.data_ptr()))
    for rc in (lib.xsg_count_literals_chunks(h, po, n * k - 1, pf, k),  # one word short
               lib.xsg_count_literals_chunks(h, None, n * k, pf, k),  # counts is null
               lib.xsg_count_literals_chunks(h, po, n * k, pf, k - 1),  # chunks_with given, one literal short
               lib.xsg_count_literals_chunks_async(h, None, pd, n * k - 1, pdf, k),
               lib.xsg_count_literals_chunks_async(h, None, None, n * k, pdf, k),
               lib.xsg_count_literals_chunks_async(h, None, pd, n * k, pdf, k - 1)):
        assert rc == xsg.EINVAL
        good()
    assert not out.any() and not freq.any() and not dev.any().item() and not dfreq.any().item()  # a refusal writes nothing
    assert lib.xsg_count_literals_chunks(h, po, n * k + 2, pf, k + 2) == xsg.OK  # room to spare
    assert out.tolist() == sum(want[0], []) + [0, 0] and freq.tolist() == want[1] + [0, 0]
    assert lib.xsg_count_literals_chunks(h, po, n * k, None, 0) == xsg.OK  # chunks_with absent: cap_literals is not looked at
    # the CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and change nothing
    for flags in (xsg.FLAG_EXACT_TAIL, xsg.flag_context(2, 3), xsg.FLAG_EXACT_TAIL | xsg.flag_context(4095, 1)):
        gs.ctx.set_literals(xsg.literal_list(lits), flags)
        assert sync(gs) == want
    # a binding of no chunks: XSG_OK, nothing in the matrix, zeros in chunks_with
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    gs.shard.rebind(t.data_ptr(), 256, xsg.make_chunks([], []))
    gs.keep = t
    assert check(gs, side, [], lits, 0, "no chunks") == ([], [0] * k)
    freq[:] = 7
    assert lib.xsg_count_literals_chunks(h, po, 0, pf, k) == xsg.OK and freq.tolist() == [0] * k + [7, 7]
    gs.bind(blocks)
    good()


def test_chunks_of_length_0_and_a_one_chunk_binding(gs, side):
    empty = np.zeros(0, dtype=np.uint8)
    one = [corpus.text_block(7, 0, 3 * TILE + 77, needle_rate=1e-3)]
    gs.bind(one)  # (tile_chunk == nullptr: the only flush is the one behind the workgroup's last tile)
    rows, freq = check(gs, side, one, SC.word_list(9), IC, "one chunk")
    assert sum(rows[0]) > 0 and set(freq) <= {0, 1}
    blocks = [empty, one[0][:TILE + 1].copy(), empty, empty, one[0][:50].copy(), empty]
    gs.bind(blocks)
    rows, _ = check(gs, side, blocks, SC.word_list(9), 0, "empty chunks")
    assert all(rows[c] == [0] * 9 for c in (0, 2, 3, 5)) and sum(rows[1]) > 0
    gs.bind([empty, empty])  # chunks, but no tile
    assert check(gs, side, [empty, empty], SC.word_list(2), 0, "no tiles") == ([[0, 0], [0, 0]], [0, 0])


# ---- 7. neighbours untouched -------------------------------------------------------------------------------------------------------
def test_neighbours_are_untouched(gs, side):
    """count, search (all seven tags), count_chunks and count_literals give the same before and after a matrix call, in
    both orders, and the matrix the same before and after them"""
    blocks = list(SC.text_blocks())
    lits = SC.word_list(9)
    n, k = len(blocks), len(lits)
    rows = MM.matrix(blocks, lits)
    want = (rows, MM.chunks_with(rows, k))

    def neighbours():
        out = list_all_modes(gs, lits, 0)
        out["count_chunks"] = [x.tolist() if hasattr(x, "tolist") else x for x in gs.shard.count_chunks(xsg.COUNT_MATCHES)]
        out["count_literals"] = gs.shard.count_literals().tolist()
        return out

    gs.bind(blocks)
    before = neighbours()
    assert before["count_literals"] == LM.counts(blocks, lits)
    assert sync(gs) == want and side.run(gs.shard, n, k) == want
    assert neighbours() == before
    assert sync(gs) == want
    gs.bind(blocks)  # the other order: the matrix first on a fresh binding
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    assert sync(gs) == want
    assert neighbours() == before
    assert side.run(gs.shard, n, k) == want
