"""Class-sequence expressions of 9 to 32 positions on every path k_scan can decide them by.

tests/class_paths.py names the five paths (exact, inreg, view, memory:long, memory:before-unit), lists an expression
for each and generates more; tests/test_class_paths.py proves without a GPU that their texts reach every path with a
true match, a filter-passing decoy and (several alternatives) a crossover.  Here the product runs them: every tag of
GpuSearch.all_modes -- the six list and count tags, the second count, the lines view -- must equal
oracle_regex_all_modes, bit for bit, whatever the hot filter (XSG_HOT=0/1, a probing context), the verification
toggles (XSG_CLS_FAST, XSG_CLS_INREG), the list route, the global offsets, or the bytes around a tightly packed chunk.

The closing census counts, from the cases that really ran, the true matches and rejected decoys per path."""
import ctypes as C

import numpy as np
import pytest

import class_paths as CP
import match_model
import packing as P
import xsg
from gpu_util import GpuSearch, oracle_regex_all_modes
from test_gpu_list_routes import ROUTES, route
from test_gpu_packed import JOB_TAGS, _take_strings, _take_u64, bind_packed, check_all, check_plain, differ
from xs_oracle import UnsupportedRegex

pytestmark = pytest.mark.gpu
IC, RX = xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX
K_CLASS, K_CLASS_FAST = 5, 7  # x-search_amd/csrc/xsg_internal.h
DIRECTED_LABELS = [f"directed {d.expr[:40].decode('latin-1')}" for d in CP.DIRECTED]
THREE = [f"directed {e.decode('latin-1')}" for e in (CP.KOFF_POSITIVE, CP.MULTI_ALT, CP.DENSE_OVERLAP)]
PACKED_LABELS = [l for l, d in zip(DIRECTED_LABELS, CP.DIRECTED) if "memory:before-unit" in d.paths]
POISON = (1 << 64) - 1

EXECUTED = {p: {"true": 0, "decoy": 0, "cross": 0} for p in CP.PATHS}
RAN = {"directed": 0, "random": 0, "toggle": 0, "route": 0, "tags": 0, "offsets": 0, "packed": 0, "async": 0, "refused": 0,
       "factor": 0, "job": 0, "host": 0}
_WANT, _CENSUS = {}, {}


@pytest.fixture(scope="module")
def texts():
    return CP.all_texts()


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


@pytest.fixture(scope="module")
def searches(gs):
    return {"default": gs, "hot0": GpuSearch(hot=0), "hot1": GpuSearch(hot=1), "probe": GpuSearch(probe=True)}


def want_of(oracle, label, t, icase):
    if (label, icase) not in _WANT:
        _WANT[(label, icase)] = oracle_regex_all_modes(oracle, t.case.blocks, t.info.expr, icase)
    return _WANT[(label, icase)]


def note(oracle, label, t, icase, env=""):
    """the paths this run took, counted with the fields the compiler chose under the flags and toggles of the run"""
    info = CP.info_or_none(t.info.expr, IC if icase else 0)
    if info is None:  # a literal under ignore_case: not a class sequence any more
        return None
    key = (label, icase, env)
    if key not in _CENSUS:
        _CENSUS[key] = CP.census(info, t.case.blocks, CP.true_starts(oracle, info, t.case.blocks))
    for p, c in _CENSUS[key].items():
        for k in c:
            EXECUTED[p][k] += c[k]
    return info


def run(gs, oracle, label, t, icase, where, how="default", env="", bind=True):
    """bind the text, search it through every tag, compare with the oracle; -> the compiler's fields for the run"""
    flags = RX | (IC if icase else 0)
    want, lines = want_of(oracle, label, t, icase)
    if bind:
        gs.bind(t.case.blocks)
    got = gs.all_modes(t.info.expr, flags, lines=lines)
    for k, v in want.items():
        differ(got[k], v, f"{where}: {k}")
    info = note(oracle, label, t, icase, env)
    if info is not None:  # the kernel that ran is the one the fields call for
        kind, k_icase, aligned = CP.kernel_fields(gs.shard.scan_kernel_name(xsg.COUNT_MATCHES))
        assert k_icase == icase and kind in (K_CLASS, K_CLASS_FAST), (where, kind)
        assert (kind == K_CLASS_FAST) == bool(info.f.cls_fast and not aligned), (where, kind, aligned, info.f)
        if how in ("hot0", "hot1"):
            assert aligned == (how == "hot1"), (where, aligned)
    return info


@pytest.mark.parametrize("label", DIRECTED_LABELS)
def test_directed_expressions(searches, texts, oracle, label):
    """each directed expression on its text, case-sensitive and not, under the window filter, the aligned trigger and a
    probing context: kClassFast against kClass"""
    t = texts[label]
    for icase in (False, True):
        want, _ = want_of(oracle, label, t, icase)
        assert want["count_matches"] > 0, label
        for how, g in searches.items():
            run(g, oracle, label, t, icase, f"{label} icase={icase} {how}", how)
            RAN["directed"] += 1


@pytest.mark.parametrize("seed", CP.SEEDS)
def test_random_expressions(searches, texts, oracle, seed):
    how = "hot1" if seed in CP.SEEDS_HOT1 else "default"
    labels = [l for l in texts if l.startswith(f"seed {seed} ")]
    assert 12 <= len(labels) <= 15
    for label in labels:
        for icase in (False, True):
            run(searches[how], oracle, label, texts[label], icase, f"{label} {texts[label].info.expr!r} icase={icase} {how}", how)
            RAN["random"] += 1


@pytest.mark.parametrize("toggle", ["XSG_CLS_FAST", "XSG_CLS_INREG"])
def test_verification_toggles(gs, texts, oracle, toggle):
    """XSG_CLS_FAST=0: the masked window compare where the 16 + 32 bit filter would run; XSG_CLS_INREG=0: the view where
    the registers would decide.  The fields say that the toggle took; the results do not move."""
    moved = 0
    for label in DIRECTED_LABELS:
        t = texts[label]
        with route(**{toggle: "0"}):
            f = CP.class_fields(t.info.expr)
            assert not (f.cls_fast if toggle == "XSG_CLS_FAST" else (f.cls_inreg or f.cls_exact)), (label, f)
            moved += f != t.info.f
            run(gs, oracle, label, t, False, f"{label} {toggle}=0", env=toggle)
        RAN["toggle"] += 1
    assert moved >= 10, moved


@pytest.mark.parametrize("name,env", ROUTES + [("on-demand", {"XSG_LINES_EAGER": 0})])
def test_list_routes(gs, texts, oracle, name, env):
    for label in THREE:
        gs.bind(texts[label].case.blocks)
        for icase in (False, True):
            with route(**env):
                run(gs, oracle, label, texts[label], icase, f"{label} icase={icase} route {name}", bind=False)
            RAN["route"] += 1


def truth(oracle, t, flags=0, go=None, lb=None):
    kind = t.case.kind._replace(flags=t.case.kind.flags | flags)
    return kind, P.truth_of(oracle, kind, t.case.blocks, go, lb)


@pytest.mark.parametrize("label", THREE)
def test_matched_text_inverted_lines_and_context(gs, texts, oracle, label):
    """XSG_MATCHES (every length is the number of positions), XSG_FLAG_INVERT and XSG_FLAG_CONTEXT"""
    t = texts[label]
    gs.bind(t.case.blocks)
    for flags in (0, IC):
        kind, tr = truth(oracle, t, flags)
        assert tr.matches[2] and set(tr.matches[2]) == {t.info.f.plen} and kind.invctx
        check_all(gs, kind, tr, f"{label} flags={flags}")
        RAN["tags"] += 1


@pytest.mark.parametrize("label", THREE + [DIRECTED_LABELS[0], DIRECTED_LABELS[7]])
def test_global_offsets_and_line_bases(searches, texts, oracle, label):
    """every odd chunk beyond 2^33 in the file with a line base of its own: m_pos = window - koff is added to them"""
    t = texts[label]
    go, lb, lb_bind = P.offsets_and_bases(t.case.blocks)
    assert max(go) >= 1 << 33
    kind, tr = truth(oracle, t, 0, go, lb)
    for how in ("default", "hot1"):
        searches[how].bind(t.case.blocks, go, lb_bind)
        check_all(searches[how], kind, tr, f"{label} offsets and bases {how}")
        RAN["offsets"] += 1


@pytest.mark.parametrize("label", PACKED_LABELS)
def test_tightly_packed_with_stale_and_completing_bytes_around(searches, texts, oracle, label):
    """capacity = sum(round_up16(len)); the chunk in front (or its pad, or the guard) ends with the bytes that complete a
    window lying in the first koff bytes of the next chunk, the pad behind a chunk completes the match that would end
    at L + 1, and `stale` puts old text with the witness there: none of it belongs to a chunk"""
    t = texts[label]
    assert t.info.f.koff > 0
    kind = t.case.kind
    tr = P.Truth(P.plain_model(oracle, kind, t.case.blocks), match_model.matches(oracle, t.case.blocks, kind.pat, kind.flags), None, {}, {})
    for fill in ("zero", "stale", "complete"):
        for how in ("default", "hot1"):
            bind_packed(searches[how], t.case, fill)
            check_plain(searches[how], kind, tr, f"{label} fill={fill} {how}")
            RAN["packed"] += 1
    note(oracle, label, t, False)


def async_counts(gs, mode):
    """xsg_count_async and xsg_count_async_status -> (counters, counters, status)"""
    import torch
    buf = torch.full((xsg.NUM_COUNTERS + 1,), 77, dtype=torch.int64, device="cuda:0")
    gs.shard.count_async(mode, 0, buf.data_ptr())
    torch.cuda.synchronize()
    plain = buf.cpu().numpy().astype(np.uint64).tolist()[:xsg.NUM_COUNTERS]
    st = torch.cuda.Stream()
    gs.shard.count_async_status(mode, st.cuda_stream, buf.data_ptr(), buf.data_ptr() + 8 * xsg.NUM_COUNTERS)
    st.synchronize()
    c = buf.cpu().numpy().astype(np.uint64).tolist()
    return plain, c[:xsg.NUM_COUNTERS], c[xsg.NUM_COUNTERS]


def test_stream_ordered_counts(gs, texts, oracle):
    """xsg_count_async / xsg_count_async_status: the plain pass for an expression that cannot overlap itself, the bounded
    list and its greedy walk on the device for one that can -- the oracle's counts either way"""
    overlapping = 0
    for label in DIRECTED_LABELS:
        t = texts[label]
        want, lines = want_of(oracle, label, t, False)
        gs.bind(t.case.blocks)
        gs.ctx.set_pattern(t.info.expr, RX)
        modes = [(xsg.COUNT_MATCHES, xsg.CTR_MATCHES, "count_matches")] + ([(xsg.COUNT_LINES | xsg.WITH_NEWLINES, xsg.CTR_LINES, "count_lines")] if lines else [])
        for mode, ctr, key in modes:
            for _ in range(2):  # twice: the pass leaves the shard as it found it
                plain, counters, status = async_counts(gs, mode)
                assert status == xsg.STATUS_OK, (label, key)
                for got in (plain, counters):
                    differ([got[ctr], got[xsg.CTR_BYTES]], [want[key], want["bytes"]], f"{label}: stream-ordered {key}")
                    if mode & xsg.WITH_NEWLINES:
                        assert got[xsg.CTR_NEWLINES] == want["newlines"], label
        raw = sum(int(CP.events(t.info, b).accept.sum()) for b in t.case.blocks)
        overlapping += raw > want["count_matches"]
        RAN["async"] += 1
    assert overlapping >= 4, overlapping  # the dense ones: more raw occurrences than the greedy walk keeps


def test_a_non_ascii_byte_inside_a_long_match_is_refused_and_clean_data_served_again(gs, texts, oracle):
    """`x.{12}y`, 14 positions: one byte >= 0x80 at position 10 of a planted member -- beyond the window, where of the
    verification paths only the memory walk reads.  Refused on every entry point (UINT64_MAX counters,
    XSG_STATUS_NONASCII), then served again on clean data.  The verdict is gathered from every byte of the chunk as it is
    loaded, whoever reads it later, so this checks the refusal and the recovery for a long expression; it does not tell
    the paths apart."""
    label = "directed x.{12}y"
    t = texts[label]
    assert t.info.f.ascii_only and t.info.f.plen == 14 and t.info.f.koff == 0
    want, lines = want_of(oracle, label, t, False)
    for c, pos, what in [p for p in t.plants if p[2] == "member"][:3]:
        blocks = [b.copy() for b in t.case.blocks]
        blocks[c][pos + 10] = 0xC3
        with pytest.raises(UnsupportedRegex):
            oracle_regex_all_modes(oracle, blocks, t.info.expr, False)
        gs.bind(blocks)
        gs.ctx.set_pattern(t.info.expr, RX)
        for mode in (xsg.COUNT_MATCHES, xsg.COUNT_LINES):
            plain, counters, status = async_counts(gs, mode)
            assert plain == [POISON] * xsg.NUM_COUNTERS, (c, pos, mode, plain)
            assert status == xsg.STATUS_NONASCII and counters == [0] * xsg.NUM_COUNTERS, (c, pos, mode, status, counters)
            with pytest.raises(xsg.XsgError) as e:
                gs.shard.count(mode)
            assert e.value.code == xsg.ENOTSUP
        for mode in (xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES, xsg.LINES):
            with pytest.raises(xsg.XsgError) as e:
                gs.shard.search_u64(mode)
            assert e.value.code == xsg.ENOTSUP
        RAN["refused"] += 1
        gs.bind(t.case.blocks)
        gs.ctx.set_pattern(t.info.expr, RX)
        plain, counters, status = async_counts(gs, xsg.COUNT_MATCHES)
        assert status == xsg.STATUS_OK and plain[xsg.CTR_MATCHES] == counters[xsg.CTR_MATCHES] == want["count_matches"]
    run(gs, oracle, label, t, False, f"{label} clean again")


def test_the_factor_prefilter_runs_the_same_matcher(gs, oracle):
    """`\\w+ing of the [a-z]{4}` goes to the automaton route; its 16-position factor marks the tiles through k_scan's
    class-sequence matcher (the memory walk): with the prefilter forced on and switched off, the same results"""
    d = CP.Directed(CP.FACTOR_EXPR, set(), None, "")
    t = CP.directed_text(d)
    assert t.info.expr == CP.FACTOR_OF and t.info.f.plen == 16
    gs.bind(t.case.blocks)
    for icase in (False, True):
        want, lines = oracle_regex_all_modes(oracle, t.case.blocks, CP.FACTOR_EXPR, icase)
        assert lines and want["count_matches"] >= 20
        for fac in ("0", "1"):
            with route(XSG_RX_FAC=fac):
                got = gs.all_modes(CP.FACTOR_EXPR, RX | (IC if icase else 0))
                name = gs.shard.scan_kernel_name(xsg.COUNT_MATCHES)
                assert ("factor prefilter" in name) == (fac == "1"), name
            for k, v in want.items():
                differ(got[k], v, f"factor route XSG_RX_FAC={fac} icase={icase}: {k}")
            RAN["factor"] += 1


def test_a_file_job_and_a_host_searcher(texts, oracle, tmp_path):
    """the same matcher behind the file pipeline (chunk_bytes = 65536, two workers) and behind a host searcher"""
    label = THREE[0]
    t = texts[label]
    expr = t.info.expr
    data = b"".join(b.tobytes() for b in t.case.blocks) + b"\n"
    path = tmp_path / "long_expression.txt"
    path.write_bytes(data)
    plan = xsg.plan_chunks(str(path), 65536)
    blocks, at = [], 0
    for c in plan:
        blocks.append(P.u8(data[at:at + int(c["original_size"])]))
        at += int(c["original_size"])
    assert at == len(data) and len(blocks) >= 2
    want, _ = oracle_regex_all_modes(oracle, blocks, expr, False)
    want["matches"] = match_model.matches(oracle, blocks, expr, RX)[0]
    assert want["count_matches"] > 20
    for key, mode, _ in JOB_TAGS:
        j = xsg.Job(expr, str(path), mode, num_threads=2, num_max_readers=2, chunk_bytes=65536, flags=RX)
        try:
            r = j.result()
        finally:
            j.close()
        got = r if isinstance(r, int) else list(r) if mode in (xsg.LINES, xsg.MATCHES) else [int(x) for x in r]
        differ(got, want[key], f"job {key}")
        RAN["job"] += 1
    lib = xsg.load()
    hs = C.c_void_p()
    assert lib.xsg_host_searcher_create(0, expr, len(expr), RX, 2, C.byref(hs)) == xsg.OK, lib.xsg_last_error()
    try:
        for i, b in enumerate(t.case.blocks):
            one, _ = oracle_regex_all_modes(oracle, [b], expr, False)
            data_b = np.ascontiguousarray(b)
            n, nb = C.c_uint64(0), C.c_uint64(0)
            for lines_mode, key in ((0, "count_matches"), (1, "count_lines")):
                assert lib.xsg_host_count(hs, data_b.ctypes.data, data_b.size, lines_mode, C.byref(n)) == xsg.OK, lib.xsg_last_error()
                assert n.value == one[key], (i, key, n.value, one[key])
            for mode, key in ((xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"), (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices")):
                out = C.c_void_p()
                assert lib.xsg_host_offsets(hs, mode, data_b.ctypes.data, data_b.size, C.byref(out), C.byref(n)) == xsg.OK, lib.xsg_last_error()
                differ(_take_u64(lib, out, n.value), one[key], f"host chunk {i} {key}")
            lens, raw = C.c_void_p(), C.c_void_p()
            assert lib.xsg_host_matches(hs, data_b.ctypes.data, data_b.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == xsg.OK
            got, ll = _take_strings(lib, lens, raw, n.value, nb.value)
            differ(got, match_model.matches(oracle, [b], expr, RX)[0], f"host chunk {i} matches")
            RAN["host"] += 1
    finally:
        lib.xsg_host_searcher_destroy(hs)


def test_zz_every_path_was_executed():
    """counted from the cases that ran: every path saw true matches and (but for `exact`, whose filter is the decision:
    nothing passes it and is rejected) rejected decoys; the paths that serve several alternatives saw crossovers.
    (test_directed_expressions feeds all of it: run at least that one before this.)"""
    for p in CP.PATHS:
        assert EXECUTED[p]["true"] >= 1 and (p == "exact" or EXECUTED[p]["decoy"] >= 1), (p, EXECUTED[p])
    for p in ("view", "memory:long", "memory:before-unit"):
        assert EXECUTED[p]["cross"] >= 1, (p, EXECUTED[p])


def test_zz_no_case_was_left_out(texts):
    """the number of compared cases is the product of the tables, as in tests/test_gpu_packed.py: a case that stops
    running fails the suite.  (It also fails when only a part of this file was run, or after a failure further up.)"""
    nseed = sum(1 for l in texts if l.startswith("seed "))
    want = {"directed": len(CP.DIRECTED) * 2 * 4, "random": nseed * 2, "toggle": len(CP.DIRECTED) * 2, "route": 5 * 3 * 2, "tags": 3 * 2,
            "offsets": 5 * 2, "packed": len(PACKED_LABELS) * 3 * 2, "async": len(CP.DIRECTED), "refused": 3, "factor": 4,
            "job": len(JOB_TAGS), "host": len(texts[THREE[0]].case.blocks)}
    assert RAN == want, {k: (RAN[k], want[k]) for k in want if RAN[k] != want[k]}
