"""xsg_count_literals_csr / xsg_result_literals_csr / xsg_count_literals_csr_async: the chunks x literals matrix in CSR form.

Expected values are tests/literal_matrix_model.py's rows turned into CSR by tests/literal_csr_model.py: exact equality
everywhere.  Every case runs the synchronous form, the same with every flush a sweep (XSG_LITMATRIX_TOUCHED=0), and the
stream-ordered form on a side stream into buffers pre-filled with 0xFF that are 8 rows / entries longer than needed.  Every
result is checked for its form (row_ptr non-decreasing, columns strictly ascending within a row, no entry 0) and, densified,
against Shard.count_literals_chunks() on the same binding wherever the dense form serves it."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import literal_csr_model as CM
import literal_matrix_model as MM
import set_cases as SC
import xsg
from gpu_util import GpuSearch
from set_gpu_util import IC, bind_tight

pytestmark = pytest.mark.gpu
TILE = SC.TILE
SPARE = 8
DENSE_LIMIT = 1 << 28


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


class Side:
    """a side stream for the stream-ordered form; the buffers are made per call, SPARE words longer than asked for"""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()

    def run(self, shard, n, cap_entries):
        """-> (row_ptr[n + 1], cols[:cap_entries], vals[:cap_entries], status); asserts that nothing behind them was written"""
        torch = self.torch
        rp = torch.full((n + 1 + SPARE,), -1, dtype=torch.int64, device="cuda:0")  # every byte 0xFF
        cols = torch.full((cap_entries + SPARE,), -1, dtype=torch.int32, device="cuda:0")
        vals = torch.full((cap_entries + SPARE,), -1, dtype=torch.int64, device="cuda:0")
        status = torch.full((1 + SPARE,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        shard.count_literals_csr_async(self.stream.cuda_stream, rp.data_ptr(), n + 1, cols.data_ptr(), vals.data_ptr(), cap_entries,
                                       status.data_ptr())
        self.stream.synchronize()
        grp, gc, gv, gst = rp.cpu().numpy(), cols.cpu().numpy(), vals.cpu().numpy(), status.cpu().numpy()
        assert (grp[n + 1:] == -1).all(), "words behind row_ptr were written"
        assert (gc[cap_entries:] == -1).all() and (gv[cap_entries:] == -1).all(), "entries at or behind cap_entries were written"
        assert (gst[1:] == -1).all(), "words behind the status were written"
        return grp[:n + 1].view(np.uint64).tolist(), gc[:cap_entries].view(np.uint32).tolist(), gv[:cap_entries].view(np.uint64).tolist(), int(gst[0])


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


def sync(gs):
    indptr, indices, data = gs.shard.count_literals_csr()
    assert indptr.dtype == np.uint64 and indices.dtype == np.uint32 and data.dtype == np.uint64
    return indptr.tolist(), indices.tolist(), data.tolist()


def forms(gs, side, n, nnz):
    """every form of the call on the current binding and list -> {name: (indptr, indices, data)}"""
    out = {"synchronous": sync(gs), "every flush a sweep": with_env({"XSG_LITMATRIX_TOUCHED": "0"}, lambda: sync(gs))}
    rp, cols, vals, status = side.run(gs.shard, n, nnz)
    assert status == xsg.STATUS_OK, "stream-ordered: status"
    out["stream-ordered"] = (rp, cols, vals)
    return out


def check(gs, side, blocks, lits, flags, what, want=None, dense=True):
    """every form against the model, its form, and the dense form of the same binding -> the expected (indptr, indices, data)"""
    blocks = list(blocks)
    n, k = len(blocks), len(lits)
    want = CM.csr(blocks, lits, bool(flags & IC)) if want is None else want
    assert CM.well_formed(*want, k)
    gs.ctx.set_literals(xsg.literal_list(lits), flags)
    got = forms(gs, side, n, len(want[1]))
    print(what, "n", n, "k", k, "nnz", len(want[1]), "row_ptr", want[0][:8], "got", got["synchronous"][0][:8])
    rows = None
    if dense and n * k <= DENSE_LIMIT:
        rows = gs.shard.count_literals_chunks(False)[0].tolist()
    for name, g in got.items():
        assert g[0] == want[0], (what, name, "row_ptr")
        assert g[1] == want[1], (what, name, "cols")
        assert g[2] == want[2], (what, name, "vals")
        assert CM.well_formed(*g, k), (what, name, "form")
        if rows is not None:
            assert CM.to_rows(*g, k) == rows, (what, name, "against the dense form")
    return want


# ---- 1. text: about 1 MiB in 5 chunks, lists of 1, 2, 9 and 300 literals ---------------------------------------------------------
@pytest.mark.parametrize("flags", [0, IC], ids=["plain", "icase"])
@pytest.mark.parametrize("k", SC.LIST_SIZES)
def test_text(gs, side, k, flags):
    blocks = SC.text_blocks()
    gs.bind(list(blocks))
    want = check(gs, side, blocks, SC.word_list(k), flags, ("text", k, flags))
    assert len(want[1]) > 0


# ---- 2. seams: 16 KiB tiles, a forced grid, chunks packed at 16-byte alignment ---------------------------------------------------
SEAM_LITS = SC.END_LITS[4]  # (b"kqzw", b"needle")


def seam_chunk(t):
    """a chunk of t tiles that ends 9 bytes in front of a tile edge: both literals in its first bytes, `kqzw` and a
    `needl` that lacks its `e` in its last, and at every tile edge inside it `needle` up to the edge and `kqzw` from it
    (even edges) or `needle` across it and `kqzw` behind (odd edges) -> (chunk, what it lacks)"""
    if t == 0:
        return np.zeros(0, dtype=np.uint8), b""
    short, long_ = SEAM_LITS
    n = t * TILE - 9
    body = bytearray(SC._ending_in(long_[:-1], n).tobytes())
    body[0:len(long_)] = long_
    body[len(long_):len(long_) + len(short)] = short
    body[n - 5 - len(short):n - 5] = short
    for i in range(1, t):
        e = i * TILE
        if i % 2:
            body[e - 3:e + 3] = long_
            body[e + 3:e + 3 + len(short)] = short
        else:
            body[e - len(long_):e] = long_
            body[e:e + len(short)] = short
    return SC.u8(body), long_[-1:]


def seam_fill(plan):
    short, long_ = SEAM_LITS

    def fill(i, n):  # the gap in FRONT of chunk i: what chunk i - 1 lacks, then stale occurrences
        head = plan[i - 1][1] if i > 0 else b""
        return SC.u8((head + (b" " + long_ + b"\n" + short) * (n // 4 + 2))[:n])
    return fill


def grid_of(ntiles, forced):
    """xsg_litmatrix.h: litmatrix_grid for a forced grid far below 2^18 tiles a workgroup -> (grid, tiles per workgroup)"""
    g = min(forced, ntiles)
    per = -(-ntiles // g)
    return -(-ntiles // per), per


def seams_of(lengths, forced):
    """from the byte lengths alone: the chunks whose tiles do not lie in one workgroup's range"""
    tiles = [-(-n // TILE) for n in lengths]
    _, per = grid_of(sum(tiles), forced)
    out, t0 = [], 0
    for c, t in enumerate(tiles):
        if t and t0 // per != (t0 + t - 1) // per:
            out.append(c)
        t0 += t
    return out, per


SEAM_LAYOUTS = {
    # tiles per chunk, XSG_LITMATRIX_GRID, tiles per workgroup, the seam chunks
    "whole-seam-empty": ((1, 3, 2, 5, 0, 1, 4), 4, 4, [3]),
    "one-spans-all": ((1, 14, 1), 4, 4, [1]),
    "every-chunk-a-seam": ((3, 3, 3, 3), 8, 2, [0, 1, 2, 3]),
}


@pytest.mark.parametrize("name", list(SEAM_LAYOUTS))
def test_seams(gs, side, name):
    tiles, forced, per_want, seams_want = SEAM_LAYOUTS[name]
    plan = [seam_chunk(t) for t in tiles]
    blocks = [b for b, _ in plan]
    seams, per = seams_of([b.size for b in blocks], forced)
    assert (seams, per) == (seams_want, per_want), "the layout no longer tests what it is for"
    assert all(b.size % 16 for b in blocks if b.size)  # a pad behind every end: the stale bytes there complete `needle`
    bind_tight(gs, blocks, seam_fill(plan))
    want = CM.csr(blocks, SEAM_LITS)
    assert all(want[0][c + 1] - want[0][c] == (2 if b.size else 0) for c, b in enumerate(blocks))
    for grid in (str(forced), "1", "2", "3", "16", None):
        with_env({"XSG_LITMATRIX_GRID": grid}, lambda: check(gs, side, blocks, SEAM_LITS, 0, ("seams", name, "grid", grid), want=want))
    with_env({"XSG_LITMATRIX_GRID": str(forced)}, lambda: check(gs, side, blocks, SEAM_LITS, IC, ("seams", name, "icase")))


# ---- 3. a boundary at every tile: hundreds of small chunks packed tightly, stale bytes behind every end -------------------------
def boundary_plan(g):
    """-> ((chunk, lack), ...): SC.end_plan(g), then 640 chunks of 0..3000 bytes whose ends are whole occurrences,
    occurrences cut short by one byte (the bytes behind the end complete them: `lack`), or plain text; every 23rd is empty"""
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
        for _ in range(int(rng.integers(0, 4))):
            lit = (short, long_)[int(rng.integers(0, 2))]
            at = int(rng.integers(0, n - len(tail) - len(lit)))
            body[at:at + len(lit)] = lit
        plan.append((SC.u8(body), lack if len(lack) <= -n % 16 else b""))
    return plan


def boundary_fill(g, plan):
    short, long_ = SC.END_LITS[g]

    def fill(i, n):
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
    want = check(gs, side, blocks, SC.END_LITS[g], flags, ("boundaries", g, flags))
    # (by default every workgroup has one tile here) one workgroup and seven flush hundreds of times each
    for grid in ("1", "7"):
        assert with_env({"XSG_LITMATRIX_GRID": grid}, lambda: sync(gs)) == want, ("boundaries", g, flags, "grid", grid)
    assert all(want[0][c] == want[0][c + 1] for c, b in enumerate(blocks) if b.size == 0)
    assert 100 < len(want[1]) < 2 * len(blocks)


# ---- 4. the touched list's edge, in a whole chunk and in a seam chunk ---------------------------------------------------------------
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
    spelled = SC.u8(b" ".join(lits))  # below a tile: every literal occurs in it
    assert spelled.size < TILE
    one = SC.u8(lits[0])  # the neighbours hit one literal each
    # two tiles: every literal in the first, every literal again in the second
    across = SC.u8(spelled.tobytes() + b" " * (TILE + 5 - spelled.size) + spelled.tobytes())
    blocks = [one, spelled, one, across, one]
    seams, per = seams_of([b.size for b in blocks], 3)
    assert (seams, per) == ([3], 2)  # under three workgroups `spelled` is whole and `across` a seam
    gs.bind(blocks)
    want = with_env({"XSG_LITMATRIX_GRID": "3"}, lambda: check(gs, side, blocks, lits, 0, ("touched", k)))
    lens = [want[0][c + 1] - want[0][c] for c in range(5)]
    assert lens == [1, k, 1, k, 1]
    assert want[1][1:1 + k] == list(range(k)) and want[2][lens[0] + k + 1:lens[0] + 2 * k + 1] == [2 * v for v in want[2][1:1 + k]]
    # one workgroup walks all five chunks; the default grid has one per tile: `across` is a seam of two workgroups
    for grid in ("1", None):
        with_env({"XSG_LITMATRIX_GRID": grid}, lambda: check(gs, side, blocks, lits, 0, ("touched", k, "grid", grid), want=want))


# ---- 5. shapes of the list ---------------------------------------------------------------------------------------------------------
LIST_SHAPES = [
    ("one literal", (b"ab",), [b"xabab", b"", b"ab", b"b"]),
    ("duplicates", (b"ab", b"b", b"ab"), [b"xabab", b"", b"ab", b"b"]),
    ("covering", (b"ab", b"abc"), [b"abc ab abcabc", b"ab", b"bc"]),
    ("overlaps", (b"aa",), [b"aaaa", b"a", b"aa"]),
    ("a list no chunk holds", (b"zq", b"qz"), [b"xabab", b"", b"ab"]),
    ("no chunks", (b"ab", b"b"), []),
]


@pytest.mark.parametrize("name,lits,texts", LIST_SHAPES, ids=[c[0] for c in LIST_SHAPES])
def test_shapes_of_the_list(gs, side, name, lits, texts):
    import torch
    blocks = [SC.u8(t) for t in texts]
    if blocks:
        gs.bind(blocks)
    else:
        gs.bind([SC.u8(b"ab")])
        t = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
        gs.shard.rebind(t.data_ptr(), 256, xsg.make_chunks([], []))
        gs.keep = t
    want = check(gs, side, blocks, lits, 0, name)
    if name == "overlaps":
        assert want == ([0, 1, 1, 2], [0, 0], [3, 1])
    if name == "duplicates":
        assert want == ([0, 3, 3, 6, 7], [0, 1, 2, 0, 1, 2, 1], [2, 2, 2, 1, 1, 1, 1])
    if name == "covering":
        assert want[:2] == ([0, 2, 3, 3], [0, 1, 0])
    if name == "a list no chunk holds":
        assert want == ([0, 0, 0, 0], [], [])
    if name == "no chunks":
        assert want == ([0], [], [])


# ---- 6. capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_of_the_stream_ordered_form(gs, side):
    blocks = list(SC.text_blocks())
    lits = SC.word_list(9)
    n = len(blocks)
    want = CM.csr(blocks, lits)
    nnz = len(want[1])
    first = want[0][1]
    assert 0 < first < nnz - 1
    gs.bind(blocks)
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    for cap in (nnz, nnz - 1, first, 0):
        rp, cols, vals, status = side.run(gs.shard, n, cap)  # (asserts that nothing at or behind cap was written)
        assert status == (xsg.STATUS_OK if cap >= nnz else xsg.STATUS_OVERFLOW), ("capacity", cap)
        assert rp == want[0], ("capacity", cap, "row_ptr is complete")
        assert cols == want[1][:cap] and vals == want[2][:cap], ("capacity", cap, "the entries below it")
        # come back with row_ptr[n]
        rp2, cols2, vals2, status2 = side.run(gs.shard, n, rp[n])
        assert status2 == xsg.STATUS_OK and (rp2, cols2, vals2) == want, ("capacity", cap, "the second call")


# ---- 7. refusals and the kept result -------------------------------------------------------------------------------------------------
def test_refusals_and_the_kept_result(gs, side):
    import torch
    blocks = SC.raw_blocks()
    lits = SC.RAW_LIST
    n, k = len(blocks), len(lits)
    want = CM.csr(blocks, lits)
    nnz = len(want[1])
    assert nnz >= 2

    def result(lib, h, rows=n + 1, entries=nnz, with_cols=True, with_vals=True):
        rp = np.full(n + 3, 7, dtype=np.uint64)
        cols = np.full(nnz + 2, 7, dtype=np.uint32)
        vals = np.full(nnz + 2, 7, dtype=np.uint64)
        rc = lib.xsg_result_literals_csr(h, C.c_void_p(rp.ctypes.data), rows, C.c_void_p(cols.ctypes.data) if with_cols else None,
                                         C.c_void_p(vals.ctypes.data) if with_vals else None, entries)
        return rc, rp.tolist(), cols.tolist(), vals.tolist()

    untouched = ([7] * (n + 3), [7] * (nnz + 2), [7] * (nnz + 2))
    fresh = GpuSearch()
    fresh.bind(blocks)
    with pytest.raises(xsg.XsgError) as e:  # the context holds no pattern
        fresh.shard.count_literals_csr()
    assert e.value.code == xsg.ESTATE
    fresh.ctx.set_literals(xsg.literal_list(lits), 0)
    assert result(fresh.shard._lib, fresh.shard.h) == (xsg.ESTATE,) + untouched  # before any pass
    fresh.ctx.close()

    gs.bind(blocks)
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    lib, h = gs.shard._lib, gs.shard.h
    assert sync(gs) == want
    # the kept result: copied out again and again, with room to spare, row_ptr alone
    assert result(lib, h) == (xsg.OK, want[0] + [7, 7], want[1] + [7, 7], want[2] + [7, 7])
    assert result(lib, h, rows=n + 3, entries=nnz + 2) == (xsg.OK, want[0] + [7, 7], want[1] + [7, 7], want[2] + [7, 7])
    assert result(lib, h, entries=0, with_cols=False, with_vals=False) == (xsg.OK, want[0] + [7, 7]) + untouched[1:]
    for kw in ({"rows": n}, {"entries": nnz - 1}, {"with_cols": False}, {"with_vals": False}):
        assert result(lib, h, **kw) == (xsg.EINVAL,) + untouched, kw
    assert lib.xsg_result_literals_csr(h, None, n + 1, None, None, 0) == xsg.EINVAL  # row_ptr is null
    assert lib.xsg_count_literals_csr(h, None) == xsg.EINVAL  # nnz is null
    # ... and it survives other entry points in between
    assert sync(gs) == want
    assert int(gs.shard.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) > 0
    assert gs.shard.count_literals_chunks()[0].tolist() == MM.matrix(blocks, lits)
    assert side.run(gs.shard, n, nnz)[:3] == want
    assert result(lib, h) == (xsg.OK, want[0] + [7, 7], want[1] + [7, 7], want[2] + [7, 7])
    # the stream-ordered form's own refusals: a null output, one row short
    dev = torch.zeros(n + nnz + 8, dtype=torch.int64, device="cuda:0")
    p = C.c_void_p(dev.data_ptr())
    for args in ((None, n + 1, p, p, nnz, p), (p, n + 1, None, p, nnz, p), (p, n + 1, p, None, nnz, p), (p, n + 1, p, p, nnz, None),
                 (p, n, p, p, nnz, p)):
        assert lib.xsg_count_literals_csr_async(h, None, *args) == xsg.EINVAL, args
    assert not dev.any().item()  # a refusal writes nothing
    # a pattern that is no list, an inverted list
    nnz_out = C.c_uint64(0)
    gs.ctx.set_pattern(b"caf", 0)
    for call in (lambda: gs.shard.count_literals_csr(), lambda: side.run(gs.shard, n, nnz)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "xsg_set_literals" in str(e.value)
    gs.ctx.set_literals(xsg.literal_list(lits), xsg.FLAG_INVERT)
    for call in (lambda: gs.shard.count_literals_csr(), lambda: side.run(gs.shard, n, nnz)):
        with pytest.raises(xsg.XsgError) as e:
            call()
        assert e.value.code == xsg.ENOTSUP and "XSG_FLAG_INVERT" in str(e.value)
    assert lib.xsg_count_literals_csr(h, C.byref(nnz_out)) == xsg.ENOTSUP
    # (a refused call ran no pass: the result of the last one that did is still kept)
    assert result(lib, h)[0] == xsg.OK
    # the CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and change nothing
    for flags in (xsg.FLAG_EXACT_TAIL, xsg.flag_context(2, 3), xsg.FLAG_EXACT_TAIL | xsg.flag_context(4095, 1)):
        gs.ctx.set_literals(xsg.literal_list(lits), flags)
        assert sync(gs) == want
    # an invalidate and a rebind drop the kept result
    gs.shard.invalidate()
    assert result(lib, h) == (xsg.ESTATE,) + untouched
    assert sync(gs) == want and result(lib, h)[0] == xsg.OK
    gs.bind(blocks)
    assert result(gs.shard._lib, gs.shard.h) == (xsg.ESTATE,) + untouched
    gs.ctx.set_literals(xsg.literal_list(lits), 0)
    assert sync(gs) == want


# ---- 8. the new ground: more words than the dense synchronous form keeps ----------------------------------------------------------
def code(j):
    """4096 distinct codes of six bytes over [0-9a-f] (multiplying by an odd number is a bijection modulo 2^24)"""
    return b"%06x" % ((j * 2654435761 + 12345) % (1 << 24))


def test_more_words_than_the_dense_form_keeps(gs, side):
    n, k = 65537, xsg.MAX_LITERALS
    assert n * k == 268_439_552 > DENSE_LIMIT
    lits = [code(j) for j in range(k)]
    assert len(set(lits)) == k and len(xsg.literal_list(lits)) == 28_671
    rng = np.random.Generator(np.random.PCG64(65537))
    picks = rng.integers(0, k, size=(n, 3))
    three = rng.integers(0, 2, size=n)
    blocks, rows = [], []
    for c in range(n):
        if c % 97 == 96:
            blocks.append(np.zeros(0, dtype=np.uint8))
            rows.append({})
            continue
        js = [int(j) for j in picks[c][:2 + int(three[c])]]
        if c % 101 == 100:
            js[1] = js[0]  # the same code twice
        text = b"|" + b"|".join(lits[j] for j in js) + b"|"
        blocks.append(SC.u8(text + b"-" * (47 - len(text) + c % 3)))  # (`|` and `-` lie outside the alphabet: nothing occurs by accident)
        rows.append(Counter(js))
    indptr, indices, data = [0], [], []
    for r in rows:
        for j in sorted(r):
            indices.append(j)
            data.append(r[j])
        indptr.append(len(indices))
    want = (indptr, indices, data)
    assert 2 * n < len(indices) < 3 * n and max(data) >= 2 and sum(b.size for b in blocks) < 4 << 20
    sample = [int(c) for c in rng.integers(0, n, size=60)] + [96, 100, 0, n - 1]  # an empty row and a doubled code among them
    assert MM.matrix([blocks[c] for c in sample], lits) == [[rows[c].get(j, 0) for j in range(k)] for c in sample]
    bind_tight(gs, blocks, lambda i, m: np.full(m, ord("0"), dtype=np.uint8))
    check(gs, side, blocks, lits, 0, "new ground", want=want, dense=False)
    # the dense synchronous form refuses this binding (its 2 GiB of zeros are never touched)
    m = np.zeros(n * k, dtype=np.uint64)
    rc = gs.shard._lib.xsg_count_literals_chunks(gs.shard.h, C.c_void_p(m.ctypes.data), m.size, None, 0)
    assert rc == xsg.ENOTSUP
