"""Random and hand-written call orders on ONE context and ONE shard, every result compared with the model of
tests/call_sequences.py (the oracle plus what include/xsg.h promises, no library-internal state).

A binding carries state from call to call -- the clean flags of the per-tile arrays, the epoch of tile_last, the newline
cache, the choices keyed by pattern_serial, the pending result (x-search_amd/csrc/xsg_objects.h; DESIGN.md, "State a binding
carries") -- and a wrong flag returns a count or a list that is off for one call, after one particular predecessor.  The
other GPU suites all go through the call order of gpu_util.GpuSearch.all_modes.

A failure prints the sequence up to the failing call as a literal: paste it into `replay(oracle, [...])`.
"""
import ctypes as C
import os

import numpy as np
import pytest

import call_sequences as cs
import corpus
import xsg
from gpu_util import upload

pytestmark = pytest.mark.gpu
TILE = cs.TILE
TAGS = {"match_byte_offsets": xsg.MATCH_BYTE_OFFSETS, "line_byte_offsets": xsg.LINE_BYTE_OFFSETS, "line_indices": xsg.LINE_INDICES,
        "lines": xsg.LINES, "lines_view": xsg.LINES, "u64_view": xsg.LINE_BYTE_OFFSETS, "result_newlines": xsg.LINE_INDICES}
POISON = (1 << 64) - 1


# x-search_amd/csrc/xsg_shard.cpp: xsg_test_shard_state (XSG_TEST_HOOKS=1; not part of the ABI): the host-side bookkeeping
STATE = ("epoch", "cnt_clean", "sum_clean", "last_valid", "nl_cached", "table_pending", "fast_result", "fast_dense", "overlap_checked",
         "overlap_free", "last_raw_matches", "mask", "dense", "tune", "tune_for_pattern", "tile_cnt_cap", "tile_sum_cap", "stream",
         "tile_last0")


def shard_state(shard, tile_last=False):
    """-> dict of STATE; tile_last=True also waits for the context's stream and reads the first tile's tile_last word"""
    fn = shard._lib.xsg_test_shard_state
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]
    out = (C.c_uint64 * len(STATE))()
    rc = fn(shard.h, out, len(STATE) if tile_last else len(STATE) - 1)
    assert rc == xsg.OK, shard._lib.xsg_last_error()
    return dict(zip(STATE, [int(x) for x in out]))


def _host_image(blocks):
    lengths = [int(b.size) for b in blocks]
    off, _, cap = corpus.chunk_table(lengths)
    host = np.zeros(max(cap, 256), dtype=np.uint8)
    for o, b in zip(off, blocks):
        host[int(o):int(o) + b.size] = b
    return host


class Replay:
    """Runs operations on one context and one shard and compares every result with the model, element by element."""

    def __init__(self, oracle, seed=None, hot=None, probe=False):
        import torch
        self.torch = torch
        self.seed, self.oracle = seed, oracle
        env = {}
        if hot is not None:
            env["XSG_HOT"] = str(hot)  # read when the context is created
        if probe:
            env["XSG_PROBE_MIN_BYTES"] = "0"
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.ctx = xsg.Context(0)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        self.shard = None
        self.tensor = None
        self.model = cs.Model(oracle)
        self.done = []           # the operations so far
        self.counted = set()     # count tags compared since the pattern or the bytes last changed
        self.stream = torch.cuda.Stream()
        self.buf = torch.zeros(xsg.NUM_COUNTERS + 1, dtype=torch.int64, device="cuda:0")
        self.env0 = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for k, v in self.env0.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        self.torch.cuda.synchronize()
        self.ctx.close()

    # -- reporting --------------------------------------------------------------------
    def fail(self, key, what, mode=None):
        name = "-"
        try:
            if mode is not None and self.model.pattern is not None:
                name = self.shard.scan_kernel_name(mode)
        except xsg.XsgError as e:
            name = f"({e})"
        pytest.fail(f"seed={self.seed} op[{len(self.done) - 1}]={self.done[-1]!r} key={key}: {what}\n  kernel: {name}\n"
                    f"  replay(oracle, {self.done!r})", pytrace=False)

    def same_list(self, key, got, want, mode):
        if got == want:
            return
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        self.fail(key, f"{len(got)} entries, want {len(want)}; first difference at [{first}]: got "
                       f"{got[first] if first < len(got) else None!r} want {want[first] if first < len(want) else None!r}", mode)

    # -- the calls ----------------------------------------------------------------------
    def raw_count(self, mode, via):
        """-> ([4 counters], status or None); raises XsgError"""
        s, t = self.shard, self.torch
        if via == "sync":
            return [int(x) for x in s.count(mode)], None
        if via == "begin_end":
            s.count_begin(mode)
            return [int(x) for x in s.count_end()], None
        self.buf.fill_(77)
        t.cuda.synchronize()
        if via == "async":
            s.count_async(mode, 0, self.buf.data_ptr())
            t.cuda.synchronize()
        elif via == "async_stream":
            s.count_async(mode, self.stream.cuda_stream, self.buf.data_ptr())
            self.stream.synchronize()
        else:
            s.count_async_status(mode, self.stream.cuda_stream, self.buf.data_ptr(), self.buf.data_ptr() + 8 * xsg.NUM_COUNTERS)
            self.stream.synchronize()
        got = [int(x) & POISON for x in self.buf.cpu().tolist()]
        return got[:xsg.NUM_COUNTERS], (got[xsg.NUM_COUNTERS] if via == "status" else None)

    def raw_list(self, kind):
        s = self.shard
        if kind in ("match_byte_offsets", "line_byte_offsets", "line_indices"):
            return s.search_u64(TAGS[kind]).tolist()
        if kind == "u64_view":
            return s.search_u64_view(xsg.LINE_BYTE_OFFSETS).tolist()
        if kind == "result_newlines":
            s.search_u64(xsg.LINE_INDICES)
            nl = C.c_uint64(0)
            rc = s._lib.xsg_result_newlines(s.h, C.byref(nl))
            if rc != xsg.OK:
                raise xsg.XsgError(rc, "xsg_result_newlines")
            return int(nl.value)
        if kind == "lines":
            ls, lo = s.search_lines()
            return ls, lo.tolist()
        vl, vb, vo = s.search_lines_view()
        ends = np.cumsum(vl.astype(np.int64)) if vl.size else np.zeros(0, dtype=np.int64)
        raw = vb.tobytes()
        return [raw[int(e) - int(n):int(e)] for e, n in zip(ends, vl)], vo.tolist()

    def bind(self, kind, data, layout):
        blocks = cs.blocks_of(data)
        go, lb = cs.layout_of(data, layout)
        if kind == "same_addr":  # other bytes behind the same address and the same table
            self.torch.cuda.synchronize()
            self.tensor.copy_(self.torch.from_numpy(_host_image(blocks)))
            self.torch.cuda.synchronize()
            self.shard.rebind(self.tensor.data_ptr(), self.tensor.numel(), self.chunks)
            return
        t, chunks = upload(blocks, go, lb)
        self.torch.cuda.synchronize()
        if self.shard is None:
            self.shard = xsg.Shard(self.ctx, t.data_ptr(), t.numel(), chunks)
        else:
            self.shard.rebind(t.data_ptr(), t.numel(), chunks)
        self.tensor, self.chunks = t, chunks  # (the old buffer is released only now)

    def check_count(self, tag, with_nl, via, e):
        mode = (xsg.COUNT_MATCHES if tag == "matches" else xsg.COUNT_LINES) | (xsg.WITH_NEWLINES if with_nl else 0)
        try:
            got, status = self.raw_count(mode, via)
        except xsg.XsgError as err:
            if e.kind != "err" or err.code != e.value:
                self.fail("count_" + tag, f"raised {err}, want {e.kind} {e.value}", mode)
            return
        if e.kind == "err":
            self.fail("count_" + tag, f"returned {got}, want error {e.value} ({e.refusal})", mode)
        if e.kind == "poison":
            if got != [POISON] * xsg.NUM_COUNTERS:
                self.fail("count_" + tag, f"counters {got}, want all UINT64_MAX ({e.refusal})", mode)
            return
        if e.kind == "status":
            if status != e.value or got != [0] * xsg.NUM_COUNTERS:
                self.fail("count_" + tag, f"status {status} counters {got}, want status {e.value} and zero counters ({e.refusal})", mode)
            return
        if status not in (None, xsg.STATUS_OK):
            self.fail("count_" + tag, f"status {status}, want 0", mode)
        names = {xsg.CTR_MATCHES: "matches", xsg.CTR_LINES: "lines", xsg.CTR_NEWLINES: "newlines", xsg.CTR_BYTES: "bytes"}
        for idx, want in e.value.items():
            if got[idx] != want:
                self.fail(f"count_{tag}/{names[idx]} via {via}", f"got {got[idx]} want {want} (counters {got})", mode)
        self.counted.add(tag)

    def step(self, op):
        e = self.model.apply(op)
        self.done.append(op)
        head = op[0]
        if head == "bind":
            self.bind(*op[1:])
            self.counted.clear()
        elif head == "invalidate":
            self.torch.cuda.synchronize()
            self.tensor.copy_(self.torch.from_numpy(_host_image(cs.blocks_of(op[1]))))
            self.torch.cuda.synchronize()
            self.shard.invalidate()
            self.counted.clear()
        elif head == "set_line_base":
            self.shard.set_line_base(op[1])
        elif head == "toggle":
            self.env0.setdefault(op[1], os.environ.get(op[1]))
            os.environ.pop(op[1], None) if op[2] is None else os.environ.__setitem__(op[1], op[2])
        elif head == "set_pattern":
            self.counted.clear()
            try:
                self.ctx.set_pattern(op[1], op[2])
            except xsg.XsgError as err:
                if e.kind != "err" or err.code != e.value:
                    self.fail("set_pattern", f"raised {err}")
                return
            if e.kind == "err":
                self.fail("set_pattern", f"accepted, want error {e.value}")
        elif head in ("tune", "time_scan"):
            try:
                self.shard.tune(op[1]) if head == "tune" else self.shard.time_scan_kernel(op[1], op[2])
            except xsg.XsgError as err:
                if e.kind != "err" or err.code != e.value:
                    self.fail(head, f"raised {err}", op[1])
                return
            if e.kind == "err":
                self.fail(head, f"succeeded, want error {e.value} ({e.refusal})", op[1])
        elif head == "count":
            self.check_count(op[1], op[2], op[3], e)
        elif head == "list":
            self.check_list(op[1], e)
        else:
            raise ValueError(op)

    def check_list(self, kind, e):
        mode = TAGS[kind]
        if e.kind == "value":
            # Count before list: a wrong count must end the sequence here, not be handed to the list kernels as a size (a wrong
            # count once led the list passes to read entries nobody wrote)
            tag = "matches" if kind in cs.MATCH_ONLY_LISTS else "lines"
            if tag not in self.counted:
                probe = cs.Model(self.oracle)
                probe.__dict__.update(self.model.__dict__)
                self.check_count(tag, False, "sync", probe._count(tag, False, "sync"))
        try:
            got = self.raw_list(kind)
        except xsg.XsgError as err:
            if e.kind != "err" or err.code != e.value:
                self.fail(kind, f"raised {err}, want {e.kind} {e.value}", mode)
            return
        if e.kind == "err":
            self.fail(kind, f"returned a result, want error {e.value} ({e.refusal})", mode)
        if kind == "result_newlines":
            if got != e.value:
                self.fail(kind, f"got {got} want {e.value}", mode)
        elif kind in ("lines", "lines_view"):
            self.same_list(kind, got[0], e.value[0], mode)
            self.same_list(kind + "/offsets", got[1], e.value[1], mode)
        else:
            self.same_list(kind, got, e.value, mode)

    def run(self, ops):
        for op in ops:
            self.step(op)
        return self

    def name(self, mode):
        return self.shard.scan_kernel_name(mode)

    def state(self, tile_last=False):
        return shard_state(self.shard, tile_last)


def replay(oracle, ops, seed=None, **ctx):
    with Replay(oracle, seed, **ctx) as r:
        r.run(ops)


# ---------------------------------------------------------------------------
# the generated sequences
# ---------------------------------------------------------------------------
SEEDS = list(range(cs.N_SEQUENCES))


@pytest.mark.parametrize("seed", SEEDS)
def test_generated_sequence(seed, oracle):
    replay(oracle, cs.sequences()[seed], seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_generated_sequence_with_the_probe_choosing(seed, oracle):
    """XSG_PROBE_MIN_BYTES=0: hot filter, filter window and stagger picked by measurements that are noise on shards this small"""
    replay(oracle, cs.sequences()[seed], seed, probe=True)


@pytest.mark.parametrize("seed", SEEDS)
def test_generated_sequence_with_the_aligned_dword_trigger(seed, oracle):
    replay(oracle, cs.sequences()[seed], seed, hot=1)


# ---------------------------------------------------------------------------
# targeted sequences
# ---------------------------------------------------------------------------
def define(name, blocks):
    cs._blocks_memo[name] = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
    return name


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


EVERY_TAG = [("count", "matches", False, "sync"), ("count", "lines", False, "sync"), ("count", "matches", True, "begin_end"),
             ("count", "lines", True, "async_stream"), ("list", "match_byte_offsets"), ("list", "line_byte_offsets"),
             ("list", "line_indices"), ("list", "lines"), ("list", "lines_view"), ("list", "u64_view"), ("list", "result_newlines")]
PASSES_PER_EPOCH_ROUND = 0xffff  # prepare_tiles: epochs 1 .. 0xffff, then the memset and 1 again


def test_tile_last_across_the_epoch_wrap(oracle):
    """tile_last is never cleaned between passes: a word carries the 16-bit epoch of the pass that wrote it, and after 65 535
    more passes that value comes round.  A (`aab`) leaves the end of its last bulk match in the tile's word; B (`ba`, lossy
    tail mode) has no bulk match in that tile and must enter the tail zone from the chunk's start.  One pass of A, then more
    than 0xffff stream-ordered passes of B, each into its own slot, one sync: every slot must hold the oracle's count
    (tests/test_call_sequences.py::test_a_stale_tile_last_word_changes_the_walk shows a stale word would change it).
    Then A and B once more, synchronously, beyond the wrap: A's own word must still be read as this pass's."""
    import torch
    d, a, a_end, b = cs.epoch_wrap_case()
    data = define("epoch_wrap", [d])
    n = PASSES_PER_EPOCH_ROUND + 70
    with Replay(oracle) as r:
        r.run([("bind", "create", data, 0), ("set_pattern", a, 0), ("count", "matches", False, "sync"),
               ("set_pattern", b, 0)])
        assert "k_scan" in r.name(xsg.COUNT_MATCHES)
        st = r.state(tile_last=True)
        epoch_a = st["epoch"]  # (the pattern change launched nothing: A's count was the last pass)
        assert st["last_valid"] and 0 < epoch_a < 100, st
        assert st["tile_last0"] == (epoch_a << 16) | a_end, f"A's pass left {st['tile_last0']:#x}, not its epoch and the end of its last match"
        want_b = oracle.count(d, b, False)
        slots = torch.full((n, xsg.NUM_COUNTERS), 77, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for k in range(n):
            r.shard.count_async(xsg.COUNT_MATCHES, 0, slots.data_ptr() + 8 * xsg.NUM_COUNTERS * k)
        torch.cuda.synchronize()
        got = slots.cpu().numpy()
        bad = np.flatnonzero(got[:, xsg.CTR_MATCHES] != want_b)
        assert bad.size == 0, f"pass {int(bad[0])} of {n} after A's: count {int(got[bad[0], xsg.CTR_MATCHES])}, want {want_b} ({bad.size} passes differ)"
        assert (got[:, xsg.CTR_BYTES] == d.size).all()
        st = r.state(tile_last=True)
        # n passes later the epoch has been through 0xffff and past A's value again; B wrote no word, so what the tile holds
        # is the memset's zero -- A's word would still be there had the wrap not cleared it
        assert st["epoch"] == epoch_a + n - PASSES_PER_EPOCH_ROUND and st["epoch"] > epoch_a, (st, epoch_a)
        assert st["tile_last0"] == 0, f"{st['tile_last0']:#x}"
        r.run([("count", "matches", False, "sync"), ("set_pattern", a, 0), ("count", "matches", False, "sync"),
               ("count", "lines", False, "sync"), ("set_pattern", b, 0), ("count", "matches", True, "status")])


DIRTY_PATTERNS = [(b"the", 0), (b"Sherlock", 0), (b"that", 0), (b"lock", cs.X), (b"She[r ]lock", cs.R), (b"\\w+ing", cs.R),
                  (b"the", cs.V)]


def test_every_tag_after_a_timing_loop(oracle):
    """xsg_time_scan_kernel runs scans with no finish kernel behind them: tile_cnt and tile_sum stay dirty"""
    with Replay(oracle) as r:
        r.run([("bind", "create", "mid", 0)])
        for pat, flags in DIRTY_PATTERNS:
            tags = [t for t in EVERY_TAG if not (flags & cs.V and (t[1] == "matches" or t[1] == "match_byte_offsets"))]
            r.run([("set_pattern", pat, flags), ("count", "lines", False, "sync")] + ([] if flags & cs.V else [("count", "matches", False, "sync")]))
            for mode in cs.MODES:
                for tag in tags:
                    r.run([("time_scan", mode, 2)])
                    st = r.state()
                    assert not st["cnt_clean"] and not st["sum_clean"], (pat, mode, st)
                    r.run([tag])


def test_every_tag_after_the_tuner_on_a_shard_it_measures(oracle):
    """xsg_shard_tune keeps the default below 1 GiB without a launch, so it runs here on 64 chunks of 16 MiB + 1 byte: the
    same text in every chunk, the expected results assembled from one chunk's.  Its timing loops leave tile_cnt and
    tile_sum dirty; every count and list tag must come out right directly behind it."""
    import torch
    from gpu_util import oracle_all_modes
    nchunks, pat = 64, b"Sherlock"
    piece = corpus.text_block(81, 0, (16 << 20) + 1, needle_rate=2e-4)
    one = oracle_all_modes(oracle, [piece], pat)
    size, nl = int(piece.size), one["newlines"]
    stride = (size + 255) // 256 * 256 + 256
    buf = torch.zeros(nchunks * stride, dtype=torch.uint8, device="cuda:0")
    dev = torch.from_numpy(piece).to("cuda:0")
    for k in range(nchunks):
        buf[k * stride:k * stride + size] = dev
    torch.cuda.synchronize()
    want = {"count_matches": one["count_matches"] * nchunks, "count_lines": one["count_lines"] * nchunks, "newlines": nl * nchunks,
            "match_byte_offsets": [x + k * size for k in range(nchunks) for x in one["match_byte_offsets"]],
            "line_byte_offsets": [x + k * size for k in range(nchunks) for x in one["line_byte_offsets"]],
            "line_indices": [x + k * nl for k in range(nchunks) for x in one["line_indices"]], "lines": one["lines"] * nchunks}
    assert nchunks * size >= 1 << 30 and one["count_matches"] > 100
    ctx = xsg.Context(0)
    sh = xsg.Shard(ctx, buf.data_ptr(), buf.numel(), xsg.make_chunks([k * stride for k in range(nchunks)], [size] * nchunks))
    ctx.set_pattern(pat, 0)
    ctr = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")

    def async_lines():
        sh.count_async(xsg.COUNT_LINES | xsg.WITH_NEWLINES, 0, ctr.data_ptr())
        torch.cuda.synchronize()
        c = ctr.cpu().tolist()
        return c[xsg.CTR_LINES], c[xsg.CTR_NEWLINES]
    tags = [("count_matches", lambda: int(sh.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES])),
            ("count_lines", lambda: int(sh.count(xsg.COUNT_LINES)[xsg.CTR_LINES])),
            ("newlines", lambda: int(sh.count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)[xsg.CTR_NEWLINES])),
            ("count_lines+newlines, stream-ordered", async_lines),
            ("match_byte_offsets", lambda: sh.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist()),
            ("line_byte_offsets", lambda: sh.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()),
            ("line_indices", lambda: sh.search_u64(xsg.LINE_INDICES).tolist()),
            ("lines", lambda: sh.search_lines()[0])]
    try:
        assert int(sh.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) == want["count_matches"]  # (count before list)
        assert int(sh.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == want["count_lines"]
        for mode in (xsg.COUNT_LINES, xsg.COUNT_MATCHES | xsg.WITH_NEWLINES):
            for key, call in tags:
                chosen = sh.tune(mode)
                st = shard_state(sh)
                assert chosen is not None and st["tune"] == chosen and st["tune_for_pattern"], ("the tuner did not measure", chosen, st)
                assert not st["cnt_clean"] and not st["sum_clean"], ("the tuner's timing loops leave the arrays dirty", st)
                got = call()
                expect = (want["count_lines"], want["newlines"]) if key.startswith("count_lines+") else want[key]
                assert got == expect, f"{key} behind xsg_shard_tune({mode:#x}): " + (f"got {got} want {expect}" if not isinstance(expect, list) else
                                                                                  f"{len(got)} entries, want {len(expect)}")
        ctx.set_pattern(b"Holmes", 0)  # the stagger was tuned for another pattern
        assert not shard_state(sh)["tune_for_pattern"]
        assert int(sh.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]) == oracle.count(piece, b"Holmes", False) * nchunks
    finally:
        torch.cuda.synchronize()
        sh.close()
        ctx.close()


@pytest.mark.parametrize("name,env", [("one-sync", {}), ("exact", {"XSG_LIST_FAST": "0"}), ("overflow->exact", {"XSG_LIST_CAP": "3"})])
def test_count_lines_after_a_list_pass_on_every_route(oracle, name, env):
    """a list pass leaves the tile counts (and, on some routes, the sums) for its later stages: dirty"""
    with Replay(oracle) as r:
        r.run([("bind", "create", "base", 0)] + [("toggle", k, v) for k, v in env.items()])
        for pat, flags in DIRTY_PATTERNS:
            r.run([("set_pattern", pat, flags), ("count", "lines", False, "sync")] + ([] if flags & cs.V else [("count", "matches", False, "sync")]))
            # the one-sync route serves literals and class sequences that are not inverted (xsg_list.cpp: fast_route_serves)
            one_sync = not flags & cs.V and pat != b"\\w+ing"
            for kind in cs.LIST_KINDS:
                if flags & cs.V and kind in cs.MATCH_ONLY_LISTS:
                    continue
                for after in (("count", "lines", False, "sync"), ("count", "lines", True, "async"), ("count", "lines", False, "status")):
                    r.run([("list", kind)])
                    st = r.state()
                    assert not st["cnt_clean"], ("the list pass left the tile counts in place", pat, kind, st)
                    # (a match list of a pattern that may overlap itself takes the exact route unless the binding knows better)
                    bordered_match = kind in cs.MATCH_ONLY_LISTS and (flags & cs.R or pat == b"that" and not st["overlap_free"])
                    # fast_result tells the routes apart for the u64 lists only (xs::lines moves its result to the pinned mirrors on
                    # either route, and the accessors do so on demand); the remembered overflow shows for every kind
                    u64 = kind in ("match_byte_offsets", "line_byte_offsets", "line_indices")
                    if one_sync and not bordered_match and kind != "result_newlines":
                        if name == "one-sync":
                            assert not st["fast_dense"] and (st["fast_result"] or not u64), (pat, kind, st)
                        elif name == "exact":
                            assert not st["fast_dense"] and not (st["fast_result"] and u64), (pat, kind, st)
                        else:  # (every pattern here has far more than the 3 results XSG_LIST_CAP leaves room for)
                            assert st["fast_dense"] and not (st["fast_result"] and u64), ("the overflow was not met or not remembered", pat, kind, st)
                    r.run([after])
                    assert r.state()["cnt_clean"], (pat, kind, after)
                if not flags & cs.V:
                    r.run([("list", kind), ("count", "matches", False, "async_stream")])
        if "XSG_LIST_CAP" in env:  # the overflow is remembered per pattern serial: a new one takes the one-sync route again
            r.run([("toggle", "XSG_LIST_CAP", None), ("set_pattern", b"the", 0), ("list", "lines")])
            assert not r.state()["fast_dense"], r.state()
            r.run([("list", "line_indices")])
            assert r.state()["fast_result"] and not r.state()["fast_dense"], r.state()
            r.run([("count", "lines", False, "sync")])


def test_count_after_the_bordered_async_count(oracle):
    """xsg_count_async of a pattern that overlaps itself keeps the tile counts for its emit pass (x-search_amd/csrc/xsg_count.cpp:
    enqueue_count_bordered)"""
    with Replay(oracle) as r:
        r.run([("bind", "create", "base", 0)])
        for pat in (b"aa", b"abab", b"that"):
            r.run([("set_pattern", pat, 0)])
            for via in ("async", "async_stream", "status"):
                for after in (("count", "matches", False, "sync"), ("count", "lines", True, "sync"), ("count", "lines", False, "async"),
                              ("list", "line_byte_offsets"), ("count", "matches", False, "begin_end")):
                    # (a fresh serial each time: the synchronous call establishes whether the occurrences overlap, and the
                    # stream-ordered one then takes the plain route)
                    r.run([("set_pattern", pat, 0)])
                    raw0 = r.state()
                    assert not raw0["overlap_checked"], raw0  # nothing established for this serial: the bounded list route it is
                    r.run([("count", "matches", False, via)])
                    st = r.state()
                    assert not st["overlap_checked"] and not st["cnt_clean"], ("the bordered route keeps the tile counts for its emit pass", pat, via, st)
                    r.run([after])
                    if after[:2] == ("count", "matches"):  # the synchronous call settles it for this serial
                        assert r.state()["overlap_checked"], (pat, after, r.state())
        r.run([("set_pattern", b"aa", 0), ("count", "matches", False, "async"), ("set_pattern", b"the", 0)] + EVERY_TAG)


def test_rebind_after_a_list_pass_inside_the_grown_buffers_and_past_them(oracle):
    """a rebind resets neither cnt_clean nor sum_clean: the words beyond the old ntiles must read as clean, inside the allocation
    (a clean-up covers the whole allocation) and past it (a grown buffer is new)"""
    for kind in cs.LIST_KINDS:
        with Replay(oracle) as r:
            r.run([("bind", "create", "small", 0), ("set_pattern", b"the", 0), ("count", "lines", False, "sync"), ("count", "matches", False, "sync"),
                   ("list", kind)])
            assert cs.ntiles_of("small") < cs.ntiles_of("mid") <= 64 < cs.ntiles_of("many")
            r.run([("bind", "larger_fit", "mid", 0), ("count", "lines", True, "sync"), ("count", "matches", False, "async"), ("list", kind),
                   ("bind", "larger_nofit", "many", 0), ("count", "lines", False, "sync"), ("count", "matches", True, "sync"), ("list", kind),
                   ("time_scan", xsg.COUNT_LINES, 2), ("bind", "smaller", "small_alt", 1), ("count", "lines", False, "sync"),
                   ("bind", "larger_fit", "mid_alt", 2), ("count", "lines", False, "sync"), ("count", "matches", False, "sync")])


NL_PRODUCERS = [(b"the", 0, {}), (b"Sherlock", 0, {}), (b"detective street", 0, {}), (b"that", 0, {}), (b"She[r ]lock", cs.R, {}),
                (b"colou?r", cs.R, {"XSG_RX_PRE": "1"}), (b"colou?r", cs.R, {"XSG_RX_PRE": "0"}), (b"\\w+ing", cs.R, {"XSG_RX_FAC": "0"}),
                (b"\\w+ing", cs.R, {"XSG_RX_FAC": "1"}), (b"(?m)^She", cs.R, {}), (b"the", cs.V, {})]


@pytest.mark.parametrize("pat,flags,env", NL_PRODUCERS, ids=[f"{p.decode()}-{f}-{''.join(e.values())}" for p, f, e in NL_PRODUCERS])
def test_newline_cache_whoever_produces_it(oracle, pat, flags, env):
    """the per-tile newline counts are written by whichever kernel family first needs them and reused by every later pattern"""
    others = [(b"Holmes", 0), (b"lock(ed|s)?", cs.R), (b"which", cs.V)]
    with Replay(oracle) as r:
        r.run([("bind", "create", "base", 2), ("set_line_base", 4000)] + [("toggle", k, v) for k, v in env.items()])
        for data, first in (("base", ("count", "lines", True, "sync")), ("base_alt", ("list", "line_indices")), ("base", ("count", "lines", True, "async")),
                            ("base_alt", ("list", "result_newlines"))):
            r.run([("invalidate", data)] if data != r.model.data else [])
            r.run([("set_pattern", pat, flags)])
            if env.get("XSG_RX_FAC") == "1":
                r.run([("count", "lines", False, "sync")])  # the first synchronous call marks the tiles
                assert "tiles marked by the factor prefilter only" in r.name(xsg.COUNT_LINES), r.name(xsg.COUNT_LINES)
            before = r.name(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
            r.run([first])
            after = r.name(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
            if not flags & cs.R:  # the scan kernel's WANT_NL instantiation, then the plain one: the counts are cached
                assert ", true, " in before.split("k_scan<")[1][:12] and ", false, " in after.split("k_scan<")[1][:12], (before, after)
            for p2, f2 in others:
                r.run([("set_pattern", p2, f2), ("list", "line_indices"), ("count", "lines", True, "status"), ("list", "result_newlines")])


def test_choices_keyed_by_the_pattern_serial(oracle):
    dense = define("dense_lock", [_u8(b"lock the lock\nno\n" * 3000), corpus.text_block(51, 0, TILE + 1)])
    sparse = define("sparse_lock", [corpus.text_block(52, 0, 51000, lexicon=corpus.LEXICON_PLAIN), _u8(b"x" * 900 + b" lock\n")])
    flat = define("abab_flat", [_u8(b"abab xx abab\nab ab\n" * 2000)])
    steep = define("abab_steep", [_u8(b"abab xx ababab\nabababab\n" * 1500)])
    assert [b.size for b in cs.blocks_of(flat)] != [b.size for b in cs.blocks_of(steep)]
    steep_same = define("abab_steep_same", [_u8((b"abab xx ababab\nab\n" * 3000)[:cs.blocks_of(flat)[0].size])])
    with Replay(oracle) as r:
        # density: a synchronous count's verdict changes the kernel of the next pass of THIS pattern on THIS binding
        r.run([("bind", "create", dense, 0), ("set_pattern", b"lock", 0)])
        assert "dense" not in r.name(xsg.COUNT_MATCHES)
        r.run([("count", "matches", False, "sync")])
        assert "(dense: byte-parallel)" in r.name(xsg.COUNT_MATCHES)
        r.run([("count", "matches", False, "sync"), ("count", "matches", True, "async"), ("list", "match_byte_offsets"),
               ("set_pattern", b"lock", 0)])
        assert "dense" not in r.name(xsg.COUNT_MATCHES)
        r.run([("count", "matches", False, "async"), ("count", "matches", False, "sync"), ("set_pattern", b"from", 0)])
        assert "dense" not in r.name(xsg.COUNT_MATCHES)
        r.run([("count", "matches", False, "sync"), ("set_pattern", b"lock", 0), ("count", "matches", False, "sync")])
        assert "(dense: byte-parallel)" in r.name(xsg.COUNT_MATCHES)
        r.run([("bind", "other", sparse, 0)])
        assert "dense" not in r.name(xsg.COUNT_MATCHES), "the verdict of the old bytes survived the rebind"
        r.run([("count", "matches", False, "sync"), ("count", "matches", False, "sync")])
        assert "dense" not in r.name(xsg.COUNT_MATCHES)
        r.run([("bind", "other", dense, 0), ("count", "matches", False, "sync"), ("invalidate", dense)])
        assert "dense" not in r.name(xsg.COUNT_MATCHES), "the verdict of the old bytes survived xsg_shard_invalidate"
    with Replay(oracle) as r:
        # `abab` without overlaps is counted in one pass from then on; the verdict belongs to the bytes
        r.run([("bind", "create", flat, 0), ("set_pattern", b"abab", 0), ("count", "matches", False, "sync")])
        # "the exception lapses once a synchronous call on this binding has established that its occurrences do not overlap"
        # (include/xsg.h, xsg_count_async): the newline count next to the match count is served now
        m = cs.expected_modes(oracle, flat, 0, b"abab", 0)
        got, _ = r.raw_count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES, "async")
        assert (got[xsg.CTR_MATCHES], got[xsg.CTR_NEWLINES]) == (m["count_matches"], m["newlines"]), got
        r.run([("bind", "other", steep, 0), ("count", "matches", False, "async"), ("count", "matches", False, "sync"),
               ("list", "match_byte_offsets"), ("bind", "other", flat, 0), ("count", "matches", False, "sync"),
               ("invalidate", steep_same), ("count", "matches", False, "status"), ("count", "matches", False, "begin_end"),
               ("list", "match_byte_offsets")])
    with Replay(oracle) as r:
        # the factor prefilter's tile marks: built once per (binding, pattern); another binding marks other tiles
        ing_late = define("ing_late", cs._text(61, [TILE * 2, TILE])[:1] + [_u8(b"nothing to see\nwalking\n" * 600)])
        ing_early = define("ing_early", [_u8(b"walking along\n" * 2000)] + cs._text(62, [TILE * 2 + 7]))
        r.run([("toggle", "XSG_RX_FAC", "1"), ("bind", "create", ing_late, 0), ("set_pattern", b"\\w+ing", cs.R), ("count", "lines", False, "sync")])
        assert "tiles marked by the factor prefilter only" in r.name(xsg.COUNT_LINES)
        r.run([("count", "lines", True, "async"), ("list", "lines"), ("bind", "other", ing_early, 0), ("count", "lines", False, "async"),
               ("count", "lines", False, "sync"), ("count", "matches", False, "sync"), ("list", "line_indices"),
               ("bind", "other", ing_late, 0), ("list", "line_byte_offsets"), ("count", "lines", True, "begin_end")])
    with Replay(oracle) as r:
        # a pattern that overflowed the one-sync list route is remembered by serial: the next pattern starts afresh
        # (fast_result tells the routes apart for the u64 lists; xs::lines ends in the pinned mirrors on either route)
        r.run([("bind", "create", "mid", 0), ("toggle", "XSG_LIST_CAP", "16"), ("set_pattern", b"the", 0), ("list", "line_byte_offsets")])
        assert r.state()["fast_dense"] and not r.state()["fast_result"], ("16 entries did not overflow", r.state())
        r.run([("list", "lines"), ("toggle", "XSG_LIST_CAP", None), ("list", "line_indices")])
        assert r.state()["fast_dense"] and not r.state()["fast_result"], ("the binding forgot the overflow", r.state())
        r.run([("list", "lines"), ("set_pattern", b"Sherlock", 0)])
        assert not r.state()["fast_dense"]
        r.run([("list", "line_byte_offsets")])
        assert r.state()["fast_result"], ("another pattern inherited the verdict", r.state())
        r.run([("list", "lines"), ("list", "match_byte_offsets"), ("set_pattern", b"the", 0), ("list", "u64_view")])
        assert r.state()["fast_result"] and not r.state()["fast_dense"], r.state()  # (a new serial: the verdict was the old one's)
        r.run([("list", "lines_view")])
        r.run([("bind", "other", "base", 0), ("list", "lines")])


def test_table_upload_is_ordered_before_a_callers_stream(oracle):
    """A one-chunk rebind uploads its table on the context's stream without a host sync (table_pending); a count on a caller's
    stream right behind it must wait for that upload.  The context's stream is kept busy by passes over a 1 GiB shard, so an
    unordered count would run ahead of the upload and scan with the previous binding's table (both buffers have the same
    capacity: a stale length stays inside the allocation)."""
    import torch
    blocks = [corpus.text_block(71, 0, 40_000, needle_rate=2e-2), corpus.text_block(72, 0, 9_000, needle_rate=4e-2)]
    want = [(oracle.count(b, b"Sherlock", False), int(b.size)) for b in blocks]
    assert want[0][0] != want[1][0]
    ups = []
    for b in blocks:
        host = np.zeros(64 << 10, dtype=np.uint8)
        host[:b.size] = b
        ups.append((torch.from_numpy(host).to("cuda:0"), xsg.make_chunks([0], [int(b.size)])))
    piece = torch.from_numpy(corpus.text_block(73, 0, 16 << 20)).to("cuda:0")
    big = piece.repeat(64)
    del piece
    ctx = xsg.Context(0)
    big_shard = xsg.Shard(ctx, big.data_ptr(), big.numel(), xsg.make_chunks([0], [big.numel()]))
    torch.cuda.synchronize()
    shard = xsg.Shard(ctx, ups[1][0].data_ptr(), ups[1][0].numel(), ups[1][1])
    ctx.set_pattern(b"Sherlock", 0)
    st = torch.cuda.Stream()
    ctx_stream = torch.cuda.ExternalStream(shard_state(shard)["stream"])
    n, behind = 60, 0
    slots = torch.zeros((n, xsg.NUM_COUNTERS), dtype=torch.int64, device="cuda:0")
    sink = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    try:
        for k in range(n):
            for _ in range(4):  # about a millisecond of work ahead of the upload
                big_shard.count_async(xsg.COUNT_LINES | xsg.WITH_NEWLINES, 0, sink.data_ptr())
            t, chunks = ups[k % 2]
            shard.rebind(t.data_ptr(), t.numel(), chunks)
            assert shard_state(shard)["table_pending"], "the rebind did not leave its upload to the stream"
            shard.count_async(xsg.COUNT_MATCHES, st.cuda_stream, slots.data_ptr() + 8 * xsg.NUM_COUNTERS * k)
            behind += not ctx_stream.query()  # the context's stream, upload included, had not drained when the count was queued
            st.synchronize()  # (between the rebind and the count there is none)
        torch.cuda.synchronize()
        assert behind >= n // 2, f"the count was queued behind a pending upload in {behind} of {n} rounds only: the test did not meet its state"
        got = slots.cpu().tolist()
        for k in range(n):
            assert (got[k][xsg.CTR_MATCHES], got[k][xsg.CTR_BYTES]) == want[k % 2], f"round {k}: {got[k]}, want {want[k % 2]}"
    finally:
        torch.cuda.synchronize()
        shard.close()
        big_shard.close()
        ctx.close()


def test_every_tag_of_a_clean_pattern_after_each_refusal(oracle):
    clean = [("set_pattern", b"the", 0)] + EVERY_TAG
    with Replay(oracle) as r:
        r.run([("bind", "create", "nonascii", 0)])
        # a match tag under XSG_FLAG_INVERT, by every entry point
        for refused in [("count", "matches", nl, via) for via in cs.COUNT_VIAS for nl in (False, True)] + [("list", "match_byte_offsets")]:
            r.run([("set_pattern", b"that", cs.V), refused, ("count", "lines", True, "sync"), ("list", "lines")] + clean)
        # a pattern xsg_set_pattern refuses: no pattern afterwards
        for bad in cs.REFUSED_PATTERNS:
            for search in (("count", "lines", False, "sync"), ("count", "matches", False, "async"), ("list", "lines"), ("count", "lines", False, "begin_end")):
                r.run([("set_pattern",) + bad, search] + clean)
        # non-ASCII data under an ascii_only expression: every route refuses in its own way
        for expr, flags in ((b"t.e", cs.R), (b"Sher.*k", cs.R), (b"t.e", cs.R | cs.V)):
            for refused in (("count", "lines", False, "sync"), ("count", "lines", True, "begin_end"), ("count", "lines", False, "async"),
                            ("count", "lines", True, "async_stream"), ("count", "lines", True, "status"), ("list", "line_byte_offsets"),
                            ("list", "lines"), ("list", "line_indices")):
                r.run([("set_pattern", expr, flags), refused] + clean)
        # the bounded device-side list of a pattern that overlaps itself runs out
        for via in ("async", "status", "async_stream"):
            r.run([("bind", "other", "runs", 0), ("set_pattern", b"aa", 0), ("count", "matches", False, via), ("count", "lines", False, "sync"),
                   ("set_pattern", b"e", 0), ("count", "matches", True, "sync"), ("set_pattern", b"a", 0), ("count", "lines", True, "async"),
                   ("count", "matches", False, "begin_end"), ("bind", "other", "small", 0)] + clean)  # (no list pass on this set: it would teach the shard a capacity)
