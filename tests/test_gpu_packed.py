"""Every tag on tightly packed chunks with hostile bytes behind every chunk end.

include/xsg.h asks of a binding only offset % 16 == 0, offset + round_up(length, 16) <= capacity and increasing offsets.
tests/packing.py lays the chunks of every pattern kind exactly so -- capacity = sum(round_up16(len)), a guard band on
either side inside the same allocation -- and fills the guards and the pad bytes with zeros (the control), newlines,
0xFF, stale text, or the bytes that complete a witness whose beginning ends the chunk (tests/test_packing.py proves
without a GPU that each of these misleads a reader which looks past a chunk's ends).  The truth comes from the blocks
alone, once per kind (packing.truth_of: the oracle, match_model, invert_model, context_model), so a result that moves
with the fill is wrong by construction.

Then the product's own reuse of one device buffer: a host searcher with a single slot and a file job with a single
worker, fed long and short chunks in turn, so that behind every short chunk's end lies what the long one left there.

Counts are compared before the lists are asked for: a list pass behind a wrong count may read entries that were never
written (tests/test_gpu_rx_spans.py).

Run as a program (`python test_gpu_packed.py child`, XSG_RX_WAVE=0 in the environment) it is the child process of
test_expressions_counted_by_the_tile_kernel: that switch is read once per process."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import match_model
import packing as P
import xsg
from gpu_util import GpuSearch
from test_gpu_list_routes import route
from xs_oracle import UnsupportedRegex

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
KIND_IDS = [k.name for k in P.KINDS]
ROUTE_FILLS = ("complete", "nl")
LIST_ROUTES = ({"XSG_LIST_FAST": "0"}, {"XSG_LIST_CAP": "3"})
RX_ROUTES = ({"XSG_RX_PRE": "0"}, {"XSG_RX_PRE": "1"}, {"XSG_RX_FAC": "0"}, {"XSG_RX_FAC": "1"})
ON_DEMAND = {"XSG_LINES_EAGER": "0"}
HOT = ("hot0", "hot1", "probe")
ASCII_ONLY = [k for k in P.KINDS if k.ascii_only]
RX_KINDS = [k for k in P.KINDS if k.family == "rx"]
LITERALS = [k for k in P.KINDS if k.family == "lit"]

TALLY = {"shard": 0, "single": 0, "offsets": 0, "refused": 0, "list_route": 0, "rx_route": 0, "on_demand": 0, "hot": 0,
         "counts": 0, "rx_wave": 0, "host": 0, "job": 0}
CASES = {}


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


@pytest.fixture(scope="module")
def hot_searches():
    return {"hot0": GpuSearch(hot=0), "hot1": GpuSearch(hot=1), "probe": GpuSearch(probe=True)}


def case_of(oracle, kind):
    """the kind's chunks and every truth about them, computed once whatever fills and routes follow"""
    if kind.name not in CASES:
        case = P.build_case(kind)
        go, lb, lb_bind = P.offsets_and_bases(case.blocks)
        CASES[kind.name] = {"case": case, "shard": P.truth_of(oracle, kind, case.blocks),
                            "single": {n: P.truth_of(oracle, kind, P.single_case(case, n).blocks) for n in P.SINGLES},
                            "offsets": (go, lb_bind, P.truth_of(oracle, kind, case.blocks, go, lb))}
    return CASES[kind.name]


def bind_packed(gs, case, fill, go=None, lb=None):
    """the whole buffer goes up as one tensor; the binding is data_ptr() + guard with the exact capacity"""
    import torch
    pk = P.pack_case(case, fill)
    t = torch.from_numpy(pk.host).to("cuda:0")
    base = t.data_ptr() + pk.base
    assert base % 16 == 0 and pk.base + pk.capacity + P.GUARD == t.numel()
    chunks = xsg.make_chunks(pk.offsets, pk.lengths, go, lb)
    if gs.shard is None:
        gs.shard = xsg.Shard(gs.ctx, base, pk.capacity, chunks)
    else:
        gs.shard.rebind(base, pk.capacity, chunks)
    gs.keep = t


def differ(got, want, where):
    if got == want:
        return
    if isinstance(got, list) and isinstance(want, list):
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        pytest.fail(f"{where}: {len(got)} entries, want {len(want)}; first difference at [{first}]: "
                    f"got {got[first] if first < len(got) else None!r} want {want[first] if first < len(want) else None!r}")
    pytest.fail(f"{where}: got {got!r} want {want!r}")


def check_counts(gs, kind, plain, where):
    s = gs.shard
    gs.ctx.set_pattern(kind.pat, kind.flags)
    c = s.count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)
    differ([int(c[xsg.CTR_MATCHES]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])],
           [plain["count_matches"], plain["newlines"], plain["bytes"]], f"{where}: count_matches, newlines, bytes")
    if kind.lines:
        c = s.count(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
        differ([int(c[xsg.CTR_LINES]), int(c[xsg.CTR_NEWLINES])], [plain["count_lines"], plain["newlines"]], f"{where}: count_lines, newlines")


def check_plain(gs, kind, tr, where, matches=True):
    """both counts, newlines and bytes; then match offsets, line offsets, line indices, lines and their offsets in the
    copy and the view form (GpuSearch.all_modes); then XSG_MATCHES: lengths, bytes, offsets"""
    check_counts(gs, kind, tr.plain, where)
    got = gs.all_modes(kind.pat, kind.flags, lines=kind.lines)
    for k, v in tr.plain.items():
        differ(got[k], v, f"{where}: {k}")
    if matches:
        ms, mo = gs.shard.search_matches()
        differ(mo.tolist(), tr.matches[1], f"{where}: XSG_MATCHES offsets")
        differ(ms, tr.matches[0], f"{where}: XSG_MATCHES bytes")
        vl, vb, vo = gs.shard.search_matches_view()
        differ(vl.tolist(), tr.matches[2], f"{where}: XSG_MATCHES lengths")
        assert vb.tobytes() == b"".join(tr.matches[0]) and vo.tolist() == tr.matches[1], f"{where}: XSG_MATCHES view"


def check_invert(gs, kind, tr, where):
    s = gs.shard
    gs.ctx.set_pattern(kind.pat, kind.flags | xsg.FLAG_INVERT)
    c = s.count(xsg.COUNT_LINES | xsg.WITH_NEWLINES)
    differ([int(c[xsg.CTR_LINES]), int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])],
           [tr.invert["count_lines"], tr.invert["newlines"], tr.invert["bytes"]], f"{where}: invert count_lines, newlines, bytes")
    differ(s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist(), tr.invert["line_byte_offsets"], f"{where}: invert line_byte_offsets")
    differ(s.search_u64(xsg.LINE_INDICES).tolist(), tr.invert["line_indices"], f"{where}: invert line_indices")
    ls, lo = s.search_lines()
    differ(lo.tolist(), tr.invert["lines_offsets"], f"{where}: invert lines_offsets")
    differ(ls, tr.invert["lines"], f"{where}: invert lines")


def check_context(gs, kind, tr, where, pairs=P.CONTEXT_PAIRS):
    from test_gpu_context import context_modes
    for pair in pairs:
        got = context_modes(gs, kind.pat, kind.flags, pair[0], pair[1])
        for k in ("line_byte_offsets", "line_indices", "lines_offsets", "lines"):
            differ(got[k], tr.context[pair][k], f"{where}: context {pair} {k}")
        differ(got["edges"], tr.edges[pair], f"{where}: context {pair} edges")


def check_all(gs, kind, tr, where):
    check_plain(gs, kind, tr, where)
    if kind.invctx:
        check_invert(gs, kind, tr, where)
        check_context(gs, kind, tr, where)


@pytest.mark.parametrize("name", KIND_IDS)
def test_every_tag_under_every_fill(gs, oracle, name):
    """the packed shard of the kind, and four of its chunks bound alone, under each fill: every tag equals the truth"""
    kind = next(k for k in P.KINDS if k.name == name)
    c = case_of(oracle, kind)
    for fill in P.FILLS:
        bind_packed(gs, c["case"], fill)
        check_all(gs, kind, c["shard"], f"{name} fill={fill} shard")
        TALLY["shard"] += 1
        for n in P.SINGLES:
            bind_packed(gs, P.single_case(c["case"], n), fill)
            check_all(gs, kind, c["single"][n], f"{name} fill={fill} single chunk of {n}")
            TALLY["single"] += 1


@pytest.mark.parametrize("name", KIND_IDS)
def test_global_offsets_and_line_bases(gs, oracle, name):
    """every odd chunk far away in the file with a line base of its own, every even one on the running offset with
    XSG_LINE_BASE_AUTO"""
    kind = next(k for k in P.KINDS if k.name == name)
    c = case_of(oracle, kind)
    go, lb_bind, tr = c["offsets"]
    for fill in ROUTE_FILLS:
        bind_packed(gs, c["case"], fill, go, lb_bind)
        check_all(gs, kind, tr, f"{name} fill={fill} offsets and bases")
        TALLY["offsets"] += 1


@pytest.mark.parametrize("name", [k.name for k in ASCII_ONLY])
def test_a_non_ascii_byte_inside_a_chunk_is_still_refused(gs, oracle, name):
    """'.' and negated classes are served on clean chunks whatever lies around them (test_every_tag_under_every_fill binds
    them under `hi` and `stale`); with one byte >= 0x80 INSIDE a chunk -- its last byte, its first -- they are refused"""
    kind = next(k for k in P.KINDS if k.name == name)
    case = case_of(oracle, kind)["case"]
    for fill in ("zero", "hi"):
        for which, at in ((6, -1), (2, -1), (8, 0)):
            blocks = [b.copy() for b in case.blocks]
            assert blocks[which].size > 1000
            blocks[which][at] = 0xC3
            with pytest.raises(UnsupportedRegex):
                P.plain_model(oracle, kind, blocks)
            bind_packed(gs, P.Case(kind, blocks, case.plan, case.stale), fill)
            gs.ctx.set_pattern(kind.pat, kind.flags)
            with pytest.raises(xsg.XsgError) as e:
                gs.shard.count(xsg.COUNT_MATCHES)
            assert e.value.code == xsg.ENOTSUP, (name, fill, which, at, "count")
            for mode in (xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES) + ((xsg.LINE_BYTE_OFFSETS, xsg.LINES) if kind.lines else ()):
                with pytest.raises(xsg.XsgError) as e:
                    gs.shard.search_u64(mode)
                assert e.value.code == xsg.ENOTSUP, (name, fill, which, at, mode)
            TALLY["refused"] += 1
        bind_packed(gs, case, fill)  # clean again: served
        check_counts(gs, kind, case_of(oracle, kind)["shard"].plain, f"{name} fill={fill} clean again")


@pytest.mark.parametrize("name", KIND_IDS)
def test_routes(gs, oracle, name):
    """the kind's own route toggles, the on-demand accessors and the four count entry points, under `complete` and `nl`"""
    from test_gpu_context import counts_everywhere
    kind = next(k for k in P.KINDS if k.name == name)
    c = case_of(oracle, kind)
    tr = c["shard"]
    for fill in ROUTE_FILLS:
        bind_packed(gs, c["case"], fill)
        check_counts(gs, kind, tr.plain, f"{name} fill={fill}")
        # (next to the match count of a literal that can overlap itself only xsg_count takes XSG_WITH_NEWLINES:
        # check_counts above; the newline count of the other entry points rides on the line count)
        modes = [(xsg.COUNT_MATCHES | (0 if kind.lines else xsg.WITH_NEWLINES), xsg.CTR_MATCHES, "count_matches")]
        modes += [(xsg.COUNT_LINES | xsg.WITH_NEWLINES, xsg.CTR_LINES, "count_lines")] if kind.lines else []
        if b"\n" in kind.pat:  # (the line count of a literal that holds a '\n' is xsg_count's alone as well)
            modes = [(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES, xsg.CTR_MATCHES, "count_matches")]
        for mode, ctr, key in modes:  # xsg_count, xsg_count_begin/_end, xsg_count_async, xsg_count_async_status
            for i, got in enumerate(counts_everywhere(gs, mode)):
                want = [tr.plain[key], tr.plain["bytes"]] + ([tr.plain["newlines"]] if mode & xsg.WITH_NEWLINES else [])
                differ([got[ctr], got[xsg.CTR_BYTES]] + ([got[xsg.CTR_NEWLINES]] if mode & xsg.WITH_NEWLINES else []), want,
                       f"{name} fill={fill} count entry point {i} {key}")
        TALLY["counts"] += 1
        for env in RX_ROUTES if kind.family == "rx" else LIST_ROUTES:
            with route(**env):
                check_plain(gs, kind, tr, f"{name} fill={fill} {env}")
                if kind.invctx:
                    check_context(gs, kind, tr, f"{name} fill={fill} {env}", pairs=P.CONTEXT_PAIRS[2:])
            TALLY["rx_route" if kind.family == "rx" else "list_route"] += 1
        with route(**ON_DEMAND):
            check_all(gs, kind, tr, f"{name} fill={fill} {ON_DEMAND}")
        TALLY["on_demand"] += 1


@pytest.mark.parametrize("name", [k.name for k in LITERALS])
def test_literals_with_either_hot_filter_and_a_probing_context(hot_searches, oracle, name):
    kind = next(k for k in P.KINDS if k.name == name)
    c = case_of(oracle, kind)
    for how in HOT:
        for fill in ROUTE_FILLS:
            bind_packed(hot_searches[how], c["case"], fill)
            check_plain(hot_searches[how], kind, c["shard"], f"{name} fill={fill} {how}", matches=False)
            TALLY["hot"] += 1


def test_expressions_counted_by_the_tile_kernel(oracle):
    """XSG_RX_WAVE=0 (counts by k_rx_scan) is read once per process: one fresh child process, started while this one has
    nothing in flight, runs the expressions under `complete` and `nl` against its own oracle"""
    import torch
    torch.cuda.synchronize()
    env = dict(os.environ, XSG_RX_WAVE="0", PYTHONPATH=os.pathsep.join(
        [str(HERE), str(HERE.parent / "x-search_amd"), str(HERE.parent / "oracle")] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), "child"]
    r = subprocess.run(cmd, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"child ok {len(RX_KINDS) * len(ROUTE_FILLS)}" in r.stdout, r.stdout[-2000:]
    TALLY["rx_wave"] += len(RX_KINDS) * len(ROUTE_FILLS)


def child_main():
    from xs_oracle import Oracle
    assert os.environ.get("XSG_RX_WAVE") == "0"
    oracle = Oracle()
    oracle.set_exact(False)
    gs = GpuSearch()
    done = 0
    for kind in RX_KINDS:
        case = P.build_case(kind)
        tr = P.truth_of(oracle, kind, case.blocks)
        for fill in ROUTE_FILLS:
            bind_packed(gs, case, fill)
            try:
                gs.ctx.set_pattern(kind.pat, kind.flags)
                name = gs.shard.scan_kernel_name(xsg.COUNT_MATCHES)
                assert "k_rx_count" not in name, name
                check_plain(gs, kind, tr, f"XSG_RX_WAVE=0 {kind.name} fill={fill}")
            except BaseException as e:  # (pytest.fail raises outside Exception)
                print(f"{kind.name} fill={fill}: {e}")
                return 1
            done += 1
    print(f"child ok {done}")
    return 0


# ---- stale bytes in the pipeline: one device buffer, reused from chunk to chunk
def _take_u64(lib, ptr, n):
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(max(n, 1),))[:n].tolist()
    lib.xsg_free(ptr)
    return out


def _take_strings(lib, lens, raw, n, nb):
    ll = _take_u64(lib, lens, n)
    blob = C.string_at(raw, nb)
    lib.xsg_free(raw)
    ends = np.cumsum(ll).tolist() if ll else []
    return [blob[e - k:e] for e, k in zip(ends, ll)], ll


@pytest.mark.parametrize("name", KIND_IDS)
def test_host_searcher_with_one_slot(oracle, name):
    """xsg_host_searcher_create(max_slots=1): long and short chunks in turn through every entry point; a short chunk ends
    in a witness prefix and the long one before it left the witness's rest (or a '\\n') at that very offset of the slot's
    buffer.  Results are chunk-local.  For '.' and negated classes the long chunk holds a non-ASCII byte there: the
    long chunk is refused, and the short one that follows -- clean, with that byte right behind its end -- is served."""
    kind = next(k for k in P.KINDS if k.name == name)
    lib = xsg.load()
    hs = C.c_void_p()
    assert lib.xsg_host_searcher_create(0, kind.pat, len(kind.pat), kind.flags, 1, C.byref(hs)) == xsg.OK, lib.xsg_last_error()
    try:
        for i, b in enumerate(P.host_sequence(kind)):
            where = f"{name} chunk {i} ({b.size} bytes)"
            try:
                plain = P.plain_model(oracle, kind, [b])
                want_m = match_model.matches(oracle, [b], kind.pat, kind.flags)
                rc = xsg.OK
            except UnsupportedRegex:
                assert kind.ascii_only and not i & 1, where
                rc = xsg.ENOTSUP
            data = np.ascontiguousarray(b)
            n, nb = C.c_uint64(0), C.c_uint64(0)
            assert lib.xsg_host_count(hs, data.ctypes.data, data.size, 0, C.byref(n)) == rc, where
            assert rc != xsg.OK or n.value == plain["count_matches"], (where, n.value, plain["count_matches"])
            if kind.lines:
                assert lib.xsg_host_count(hs, data.ctypes.data, data.size, 1, C.byref(n)) == rc, where
                assert rc != xsg.OK or n.value == plain["count_lines"], (where, n.value, plain["count_lines"])
            modes = [(xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets")]
            modes += [(xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices")] if kind.lines else []
            for mode, key in modes:
                out = C.c_void_p()
                assert lib.xsg_host_offsets(hs, mode, data.ctypes.data, data.size, C.byref(out), C.byref(n)) == rc, (where, key)
                if rc == xsg.OK:
                    differ(_take_u64(lib, out, n.value), plain[key], f"{where}: host {key}")
            lens, raw = C.c_void_p(), C.c_void_p()
            if kind.lines:
                assert lib.xsg_host_lines(hs, data.ctypes.data, data.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == rc, where
                if rc == xsg.OK:
                    differ(_take_strings(lib, lens, raw, n.value, nb.value)[0], plain["lines"], f"{where}: host lines")
            assert lib.xsg_host_matches(hs, data.ctypes.data, data.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == rc, where
            if rc == xsg.OK:
                got, ll = _take_strings(lib, lens, raw, n.value, nb.value)
                differ(ll, want_m[2], f"{where}: host matches lengths")
                differ(got, want_m[0], f"{where}: host matches")
            TALLY["host"] += 1
    finally:
        lib.xsg_host_searcher_destroy(hs)


JOB_TAGS = [("count_matches", xsg.COUNT_MATCHES, False), ("match_byte_offsets", xsg.MATCH_BYTE_OFFSETS, False), ("matches", xsg.MATCHES, False),
            ("count_lines", xsg.COUNT_LINES, True), ("line_byte_offsets", xsg.LINE_BYTE_OFFSETS, True),
            ("line_indices", xsg.LINE_INDICES, True), ("lines", xsg.LINES, True)]


def _job(pat, path, mode, flags, meta=None):
    j = xsg.Job(pat, path, mode, meta_path=meta, num_threads=1, num_max_readers=1, chunk_bytes=P.PIPELINE_CHUNK, flags=flags)
    try:
        r = j.result()
        return r if isinstance(r, int) else list(r) if mode in (xsg.LINES, xsg.MATCHES) else [int(x) for x in r]
    finally:
        j.close()


def test_file_job_with_one_worker(oracle, tmp_path):
    """xsg.Job(num_threads=1, num_max_readers=1, chunk_bytes=4096) over a file whose planned chunks are ~12 KB and
    ~4.1 KB in turn (tests/packing.py: pipeline_chunks says what then lies behind each chunk's end in the worker's device
    buffer): every tag equals the oracle's over the planned chunks, plain and through an LZ4 metafile"""
    chunks = P.pipeline_chunks()
    path = tmp_path / "alternating.txt"
    path.write_bytes(b"".join(chunks))
    plan = xsg.plan_chunks(str(path), P.PIPELINE_CHUNK)
    sizes = [int(c["original_size"]) for c in plan]
    assert sizes == [len(c) for c in chunks], sizes
    assert all(11_000 < n < 13_000 for n in sizes[0::2]) and all(4096 <= n < 4200 for n in sizes[1::2]), sizes
    meta, packed = tmp_path / "alternating.xslz4.meta", tmp_path / "alternating.xslz4"
    xsg.meta_write(str(path), str(meta), str(packed), xsg.COMPRESSION_LZ4, P.PIPELINE_CHUNK, 500)
    assert [int(c["original_size"]) for c in xsg.meta_read(str(meta))[1]] == sizes
    blocks = [P.u8(c) for c in chunks]
    for pat, flags, line_tags in P.PIPELINE_PATTERNS:
        kind = next(k for k in P.KINDS if k.pat == pat and k.flags == flags)
        plain = P.plain_model(oracle, kind, blocks)
        plain["matches"] = match_model.matches(oracle, blocks, pat, flags)[0]
        assert plain["count_matches"] > 20
        for how, args in (("plain", (str(path), None)), ("lz4", (str(packed), str(meta)))):
            for key, mode, needs_lines in JOB_TAGS:
                if needs_lines and not line_tags:
                    continue
                differ(_job(pat, args[0], mode, flags, meta=args[1]), plain[key], f"job {how} {pat!r} {key}")
            TALLY["job"] += 1


def test_zz_no_case_was_left_out():
    """the number of compared cases is the product of the tables: a case that stops running fails the suite"""
    kinds, fills, rf = len(P.KINDS), len(P.FILLS), len(ROUTE_FILLS)
    rx, lit = len(RX_KINDS), len(LITERALS)
    want = {"shard": kinds * fills, "single": kinds * fills * len(P.SINGLES), "offsets": kinds * rf,
            "refused": len(ASCII_ONLY) * 2 * 3, "counts": kinds * rf, "list_route": (kinds - rx) * rf * len(LIST_ROUTES),
            "rx_route": rx * rf * len(RX_ROUTES), "on_demand": kinds * rf, "hot": lit * len(HOT) * rf, "rx_wave": rx * rf,
            "host": kinds * 8, "job": len(P.PIPELINE_PATTERNS) * 2}
    assert len(P.KINDS) == 31 and len(ASCII_ONLY) == 3 and rx == 6 and lit == 22
    assert TALLY == want, {k: (TALLY[k], want[k]) for k in want if TALLY[k] != want[k]}


if __name__ == "__main__":
    sys.exit(child_main() if sys.argv[1:] == ["child"] else 2)
