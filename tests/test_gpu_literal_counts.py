"""xsg_count_literals / xsg_count_literals_async / xsg_literal_counter_*: one count per literal of a list in one pass.

Expected values are tests/literal_counts_model.py's (bytes.find per literal and chunk; tests/test_literal_counts_host.py
pins it to the oracle): exact equality everywhere.  Every case runs the synchronous form, the stream-ordered form on a
side stream into a buffer pre-filled with 0xFF, and a LiteralCounter fed the same blocks.  The cases are those of the
literal-list tests, which sit at the edges of k_set_scan's tile loop."""
import ctypes as C

import numpy as np
import pytest

import corpus
import literal_counts_model as LM
import set_cases as SC
import set_edge_cases as E
import xsg
from gpu_util import GpuSearch
from set_gpu_util import IC, bind_tight, list_all_modes

pytestmark = pytest.mark.gpu
TILE, WAVE_LOAD = SC.TILE, SC.WAVE_LOAD


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


class Side:
    """a side stream and a device buffer of MAX_LITERALS + 8 words for the stream-ordered form"""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()
        self.buf = torch.empty(xsg.MAX_LITERALS + 8, dtype=torch.int64, device="cuda:0")

    def run(self, shard, k):
        self.buf.fill_(-1)  # every byte 0xFF
        self.torch.cuda.synchronize()
        shard.count_literals_async(self.stream.cuda_stream, self.buf.data_ptr(), k)
        self.stream.synchronize()
        got = self.buf.cpu().numpy()
        assert (got[k:] == -1).all(), "words behind the list's were written"
        return got[:k].tolist()


@pytest.fixture(scope="module")
def side():
    return Side()


def check(gs, side, blocks, lits, flags, what, counter=True):
    """all three forms against the model -> the expected counts"""
    blocks = list(blocks)
    lst = xsg.literal_list(lits)
    want = LM.counts(blocks, lits, bool(flags & IC))
    gs.ctx.set_literals(lst, flags)
    got = gs.shard.count_literals()
    print(what, "k", len(lits), "sum", int(got.sum()), "first", got.tolist()[:12], "want", want[:12])
    assert got.dtype == np.uint64 and got.tolist() == want, (what, "synchronous")
    assert side.run(gs.shard, len(lits)) == want, (what, "stream-ordered")
    if counter:
        lc = xsg.LiteralCounter(0, lst, flags)
        try:
            for i, b in enumerate(blocks):
                lc.add(b)
                if i == 0:  # a get between adds: the first chunk's table
                    first, nbytes = lc.get()
                    assert first.tolist() == LM.counts(blocks[:1], lits, bool(flags & IC)) and nbytes == blocks[0].size, (what, "first chunk")
            got, nbytes = lc.get()
        finally:
            lc.close()
        assert got.tolist() == want and nbytes == sum(int(b.size) for b in blocks), (what, "LiteralCounter")
    return want


# ---- text: about 1 MiB in 5 chunks, lists of 1, 2, 9 and 300 literals ------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, IC], ids=["plain", "icase"])
@pytest.mark.parametrize("k", SC.LIST_SIZES)
def test_text(gs, side, k, flags):
    blocks = SC.text_blocks()
    gs.bind(list(blocks))
    want = check(gs, side, blocks, SC.word_list(k), flags, ("text", k, flags))
    assert sum(want) > 0


@pytest.mark.parametrize("name,lits,blocks", SC.ORDER_CASES, ids=[c[0] for c in SC.ORDER_CASES])
def test_prefix_infix_and_duplicate_literals_all_count(gs, side, name, lits, blocks):
    gs.bind(list(blocks))
    want = check(gs, side, blocks, lits, 0, name)
    assert all(w > 0 for w in want)
    dup = tuple(lits) + (lits[0], lits[-1])  # duplicates get the same number each
    assert check(gs, side, blocks, dup, 0, (name, "dup"), counter=False) == want + [want[0], want[-1]]
    if name == "aa-a-run":
        assert want == [65535, 65536]


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_every_alignment_round_the_tile_and_the_wave_load_edge(gs, side, g):
    blocks = SC.align_blocks()
    gs.bind(list(blocks))
    want = check(gs, side, blocks, SC.align_list(g), 0, ("align", g), counter=g == 4)
    assert want[:2] == [len(blocks), len(blocks)]


@pytest.mark.parametrize("flags", [0, IC], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_chunk_ends_with_stale_bytes_behind_them(gs, side, g, flags):
    """literals end exactly at a chunk's end, one byte short of it, and are completed only by the bytes behind it"""
    blocks = SC.end_blocks(g)
    bind_tight(gs, blocks, SC.end_fill(g))
    want = check(gs, side, blocks, SC.END_LITS[g], flags, ("ends", g, flags), counter=False)
    assert sum(want) > 0 and len(SC.end_cut_chunks(g)) > 0


@pytest.fixture(scope="module")
def grid():
    import torch
    return E.GRID_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("layout", ["upload", "tight"])
def test_grid_stride(gs, side, grid, layout):
    """more than 2 * grid tiles: every workgroup flushes a histogram built over several tiles and chunks"""
    case = E.grid_case(grid)
    assert len(E.tiles_of(case.blocks)) > 2 * grid
    if layout == "tight":
        bind_tight(gs, case.blocks, E.grid_fill(case))
    else:
        gs.bind(list(case.blocks))
    for flags in (0, IC):
        want = check(gs, side, case.blocks, E.GRID_LITS, flags, ("grid", layout, flags), counter=False)
        assert sum(want) > grid


@pytest.mark.parametrize("g,gi", E.FOLD_CASES, ids=["g%d-%s" % (g, E.FOLD_GROUPS[gi].name) for g, gi in E.FOLD_CASES])
def test_fold(gs, side, g, gi):
    case = E.fold_case(g, gi)
    gs.bind(list(case.blocks))
    want = check(gs, side, case.blocks, case.lits, IC, case.name, counter=False)
    assert sum(want) >= 16 * len(case.lits) - 2
    if (g, gi) in E.FOLD_PLAIN:
        check(gs, side, case.blocks, case.lits, 0, (case.name, "plain"), counter=False)


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [3, 4])
def test_candidates_that_no_literal_owns(gs, side, g, icase):
    lits, blocks, fakes = E.collision_case(g)
    gs.bind(list(blocks))
    want = check(gs, side, blocks, lits, IC if icase else 0, ("collisions", g, icase), counter=False)
    assert sum(want) >= 4 * len(lits) + 4


@pytest.mark.parametrize("name", [n for n, _ in E.LIMIT_LISTS])
def test_list_limits(gs, side, name):
    """4096 literals under one gram, 4096 distinct grams, the 255-byte literal; in `distinct` every literal occurs at
    least once, so the largest possible flush -- 4096 non-zero words -- is compared word for word"""
    lits = dict(E.LIMIT_LISTS)[name]()
    case = E.limit_blocks()
    blocks = list(case.blocks)
    if name == "distinct":
        blocks.append(SC.u8(b"".join(lits)))
        gs.bind(blocks)
    else:
        bind_tight(gs, blocks, E.limit_fill(case))
    want = check(gs, side, blocks, lits, 0, ("limits", name))
    assert sum(want) > 0
    if name == "distinct":
        assert min(want) >= 1 and len(want) == xsg.MAX_LITERALS
    if name == "shared":
        assert want[lits.index(E.ROOM_SHORT)] >= 2  # (the chunk that ends in it gives it the room no 7-byte literal has)


@pytest.mark.parametrize("layout", ["upload", "tight"])
@pytest.mark.parametrize("k", range(len(E.NUL_LISTS)))
def test_nul_bytes(gs, side, k, layout):
    blocks = E.nul_blocks()
    if layout == "tight":
        bind_tight(gs, blocks, lambda i, n: np.zeros(n, dtype=np.uint8))
    else:
        gs.bind(blocks)
    assert len(E.nul_cut_chunks()) > 0
    for flags in (0, IC):
        want = check(gs, side, blocks, E.NUL_LISTS[k], flags, ("nul", k, layout, flags), counter=layout == "upload" and flags == 0)
        assert sum(want) > 0


def test_bytes_that_are_no_utf8(gs, side):
    blocks = SC.raw_blocks()
    gs.bind(blocks)
    plain = check(gs, side, blocks, SC.RAW_LIST, 0, "raw")
    folded = check(gs, side, blocks, SC.RAW_LIST, IC, "raw icase")
    assert folded[1] == plain[1] + 1  # `CAF\xe9`: the letters fold, the byte >= 0x80 does not


def test_dense_list_six_figure_counts_in_one_word(gs, side):
    blocks = SC.dense_blocks()
    gs.bind(list(blocks))
    want = check(gs, side, blocks, SC.DENSE_LIST, 0, "dense")
    assert max(want) > 20_000


# ---- new cases ---------------------------------------------------------------------------------------------------------------------
def test_overlapping_occurrences_across_lane_wave_load_and_tile_edges(gs, side):
    blocks = [np.full(TILE + 1, ord("a"), dtype=np.uint8)]
    gs.bind(blocks)  # (a one-chunk binding: tile_chunk == nullptr)
    assert check(gs, side, blocks, (b"aa",), 0, "aa run") == [TILE]
    assert check(gs, side, blocks, (b"aa", b"aaa", b"a", b"aa"), IC, "aa aaa a aa") == [TILE, TILE - 1, TILE + 1, TILE]


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_chunks_shorter_than_the_gram(gs, side, g):
    short, long_ = SC.END_LITS[g]
    rep = short * 3
    blocks = [SC.u8(rep[:n]) for n in (0, 1, g - 1, g, 0, g + 1)] + [SC.u8(long_), np.zeros(0, dtype=np.uint8)]
    gs.bind(blocks)
    want = check(gs, side, blocks, (short, long_), 0, ("short chunks", g))
    assert want == [4 if g == 1 else 2, 1]


def test_one_chunk_binding_and_a_binding_of_no_chunks(gs, side):
    import torch
    one = [corpus.text_block(7, 0, 3 * TILE + 77, needle_rate=1e-3)]
    gs.bind(one)
    want = check(gs, side, one, SC.word_list(9), IC, "one chunk")
    assert sum(want) > 0
    t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    gs.shard.rebind(t.data_ptr(), 256, xsg.make_chunks([], []))
    gs.keep = t
    assert check(gs, side, [], SC.word_list(9), 0, "no chunks", counter=False) == [0] * 9
    lc = xsg.LiteralCounter(0, xsg.literal_list(SC.word_list(9)))
    lc.add(b"")  # len == 0 is fine
    got, nbytes = lc.get()
    lc.close()
    assert got.tolist() == [0] * 9 and nbytes == 0


def test_refusals(gs, side):
    import torch
    blocks = SC.raw_blocks()
    lits = SC.RAW_LIST
    k = len(lits)
    fresh = GpuSearch()
    fresh.bind(blocks)
    with pytest.raises(xsg.XsgError) as e:  # the context holds no pattern
        fresh.shard.count_literals()
    assert e.value.code == xsg.ESTATE
    fresh.ctx.close()
    gs.bind(blocks)
    gs.ctx.set_pattern(b"caf", 0)
    for call in (lambda: gs.shard.count_literals(), lambda: side.run(gs.shard, k)):
        with pytest.raises(xsg.XsgError) as e:  # the pattern is no list
            call()
        assert e.value.code == xsg.ENOTSUP and "xsg_set_literals" in str(e.value)
    gs.ctx.set_literals(xsg.literal_list(lits), xsg.FLAG_INVERT)
    for call in (lambda: gs.shard.count_literals(), lambda: side.run(gs.shard, k)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "XSG_FLAG_INVERT" in str(e.value)
    with pytest.raises(xsg.XsgError) as e:
        xsg.LiteralCounter(0, xsg.literal_list(lits), xsg.FLAG_INVERT)
    assert e.value.code == xsg.ENOTSUP
    with pytest.raises(xsg.XsgError) as e:
        xsg.LiteralCounter(0, b"a\n\nb")
    assert e.value.code == xsg.EINVAL
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    lib, h = gs.shard._lib, gs.shard.h
    out = np.zeros(k + 2, dtype=np.uint64)
    dev = torch.zeros(k + 2, dtype=torch.int64, device="cuda:0")
    assert lib.xsg_count_literals(h, None, k) == xsg.EINVAL
    assert lib.xsg_count_literals(h, C.c_void_p(out.ctypes.data), k - 1) == xsg.EINVAL
    assert lib.xsg_count_literals_async(h, None, None, k) == xsg.EINVAL
    assert lib.xsg_count_literals_async(h, None, C.c_void_p(dev.data_ptr()), k - 1) == xsg.EINVAL
    assert lib.xsg_count_literals(h, C.c_void_p(out.ctypes.data), k + 2) == xsg.OK  # room to spare
    want = LM.counts(blocks, lits)
    assert out.tolist() == want + [0, 0]
    # the CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and change nothing
    for flags in (xsg.FLAG_EXACT_TAIL, xsg.flag_context(2, 3), xsg.FLAG_EXACT_TAIL | xsg.flag_context(4095, 1)):
        gs.ctx.set_literals(xsg.literal_list(lits), flags)
        assert gs.shard.count_literals().tolist() == want
    lc = xsg.LiteralCounter(0, xsg.literal_list(lits))
    assert lib.xsg_literal_counter_get(lc.h, C.c_void_p(out.ctypes.data), k - 1, None) == xsg.EINVAL
    assert lib.xsg_literal_counter_get(lc.h, None, k, None) == xsg.EINVAL
    assert lib.xsg_literal_counter_get(lc.h, C.c_void_p(out.ctypes.data), k, None) == xsg.OK  # (bytes is optional)
    lc.close()


def test_call_order_on_one_binding(gs, side, oracle):
    """the list tags before and after count_literals are unchanged; a plain literal, the list again, and count_literals
    after a rebind"""
    blocks = list(SC.text_blocks())
    lits = SC.word_list(9)
    gs.bind(blocks)
    before = list_all_modes(gs, lits, 0)
    want = LM.counts(blocks, lits)
    assert gs.shard.count_literals().tolist() == want
    assert side.run(gs.shard, len(lits)) == want
    assert list_all_modes(gs, lits, 0) == before
    assert gs.shard.count_literals().tolist() == want
    plain = gs.all_modes(b"Sherlock")
    oracle.set_exact(False)
    assert plain["count_matches"] == sum(oracle.count(b, b"Sherlock", False) for b in blocks)
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    assert gs.shard.count_literals().tolist() == want
    assert list_all_modes(gs, lits, 0) == before
    small = [b[:TILE + 5].copy() for b in blocks[:2]]
    gs.bind(small)
    assert gs.shard.count_literals().tolist() == LM.counts(small, lits)
    assert int(gs.shard.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) == list_all_modes(gs, lits, 0)["count_matches"]
    gs.bind(blocks)
    assert gs.shard.count_literals().tolist() == want
    assert list_all_modes(gs, lits, 0) == before
