"""A literal LIST as the pattern on the GPU (include/xsg.h: xsg_set_literals; kernels k_set_scan / k_set_verify).

Expected values: the oracle's independent regex reader on E(S) = esc(l1)|...|esc(lk) (set_cases.expected); lists with
bytes >= 0x80 that are no UTF-8, which that reader refuses, from tests/set_model.py, which tests/test_set_host.py pins to
the oracle.  XSG_MATCHES, XSG_FLAG_INVERT and XSG_FLAG_CONTEXT come from set_model.matches, invert_model and context_model on
top of those.  Shapes: a tile is 16 KiB, a wave-load 1 KiB, a lane's unit 16 B."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import context_model
import corpus
import invert_model
import set_cases as SC
import set_model
import xsg
from gpu_util import GpuSearch, oracle_regex_all_modes
from set_gpu_util import bind_tight, check, check_matches, list_all_modes

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
IC = xsg.FLAG_IGNORE_CASE
LINE_KEYS = ("count_lines", "line_byte_offsets", "line_indices", "lines", "lines_offsets")


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


# ---- all seven tags against the oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_bound(gs):
    blocks = list(SC.text_blocks())
    gs.bind(blocks)
    return blocks


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
@pytest.mark.parametrize("k", SC.LIST_SIZES)
def test_all_tags_against_the_oracle(gs, oracle, text_bound, k, icase):
    """lists of 1, 2, 9 (past the class route's 8 alternatives) and 300 (past the automaton's table cap) literals"""
    blocks, lits, flags = text_bound, SC.word_list(k), IC if icase else 0
    gs.bind(blocks)
    want = SC.expected(oracle, blocks, lits, icase)
    assert want["count_matches"] > 0 and want["count_lines"] > 0
    got = list_all_modes(gs, lits, flags)
    check(got, want, (k, icase))
    check_matches(gs, blocks, lits, flags, (k, icase))
    if k <= 8:  # the product's own regex route accepts E(S): the definition, taken literally
        rx = gs.all_modes(set_model.expression(lits), xsg.FLAG_REGEX | flags)
        check(got, rx, (k, icase, "XSG_FLAG_REGEX"), keys=[key for key in want if key in rx])


def test_the_regex_route_refuses_what_the_list_route_serves(gs, oracle, text_bound):
    """E(S) of the 300 literals is over XSG_MAX_REGEX bytes, and 60 of them, which fit, are past the automaton's table
    cap: the capability is new, not only the speed"""
    assert len(set_model.expression(SC.word_list(300))) > xsg.MAX_REGEX
    sixty = tuple(l for l in SC.word_list(300) if len(l) >= 5)[:60]
    assert len(set_model.expression(sixty)) <= xsg.MAX_REGEX
    with pytest.raises(xsg.XsgError) as e:
        gs.ctx.set_pattern(set_model.expression(sixty), xsg.FLAG_REGEX)
    assert e.value.code == xsg.ENOTSUP
    gs.bind(text_bound)
    gs.ctx.set_literals(xsg.literal_list(sixty))
    want = SC.expected(oracle, text_bound, sixty)
    assert int(gs.shard.count(xsg.COUNT_LINES)[xsg.CTR_LINES]) == want["count_lines"] > 0


# ---- order and overlap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lits,blocks", SC.ORDER_CASES, ids=[c[0] for c in SC.ORDER_CASES])
def test_order_and_overlap(gs, oracle, name, lits, blocks):
    gs.bind(blocks)
    want = SC.expected(oracle, blocks, lits)
    got = list_all_modes(gs, lits)
    check(got, want, name)
    check_matches(gs, blocks, lits, 0, name)


def test_first_listed_wins_and_the_walk_resumes_at_its_end(gs):
    """the definition on the issue's own strings, spelled out"""
    gs.bind([SC.u8(b"abcd")])
    for lits, want in (((b"ab", b"abc"), [b"ab"]), ((b"abc", b"ab"), [b"abc"]), ((b"b", b"abc"), [b"abc"]), ((b"ab", b"bcd"), [b"ab"])):
        gs.ctx.set_literals(xsg.literal_list(lits))
        assert gs.shard.search_matches()[0] == want, lits
    gs.bind([SC.u8(b"ba a a")])
    gs.ctx.set_literals(b"a a\n")
    assert gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist() == [1]


# ---- every alignment ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_every_alignment(gs, oracle, g):
    """a 5-byte and a 255-byte literal starting at every offset around a tile edge, a wave-load edge and the lane edges in
    between, in chunks of 32 KiB + 16 B; a second shortest literal sets g"""
    blocks, lits = list(SC.align_blocks()), SC.align_list(g)
    assert xsg.literals_info(xsg.literal_list(lits))["gram"] == g
    gs.bind(blocks)
    want = SC.expected(oracle, blocks, lits)
    assert want["count_matches"] == 2 * len(blocks)
    got = list_all_modes(gs, lits)
    check(got, want, g)
    check_matches(gs, blocks, lits, 0, g)


# ---- chunk ends ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_chunk_ends(gs, oracle, g, icase):
    """an occurrence that ends exactly at the chunk's end is reported; one whose last bytes lie behind it is not, although
    the bytes that complete it are there, in the pad or at the start of the next chunk (set_cases.end_plan;
    test_set_host.py::test_the_chunk_end_layout_is_hostile shows that a reader past the end would report it); a gram that
    straddles the end is no candidate; stale matches in the padding; chunks of 1, g - 1, g, 15, 16 and 17 bytes"""
    blocks, lits, flags = SC.end_blocks(g), SC.END_LITS[g], IC if icase else 0
    assert len(SC.end_cut_chunks(g)) >= 6
    bind_tight(gs, blocks, SC.end_fill(g))
    want = SC.expected(oracle, blocks, lits, icase)
    got = list_all_modes(gs, lits, flags)
    check(got, want, (g, icase))
    check_matches(gs, blocks, lits, flags, (g, icase))


def test_bytes_that_are_no_utf8(gs, oracle):
    """a literal is bytes: the oracle's reader refuses such a list, the model answers"""
    blocks = SC.raw_blocks()
    gs.bind(blocks)
    for flags in (0, IC):
        want = set_model.all_modes(blocks, SC.RAW_LIST, bool(flags))
        assert want == SC.expected(oracle, blocks, SC.RAW_LIST, bool(flags)) and want["count_matches"] >= 9
        check(list_all_modes(gs, SC.RAW_LIST, flags), want, flags)
        check_matches(gs, blocks, SC.RAW_LIST, flags, flags)


# ---- a candidate-dense list -------------------------------------------------------------------------------------------------------------------
def test_dense_list(gs, oracle):
    """`e` and `th` make every eighth position a candidate: no bail-out, slow but exact"""
    blocks = list(SC.dense_blocks())
    gs.bind(blocks)
    want = SC.expected(oracle, blocks, SC.DENSE_LIST)
    assert want["count_matches"] * 16 > want["bytes"]
    check(list_all_modes(gs, SC.DENSE_LIST), want, "dense")
    check_matches(gs, blocks, SC.DENSE_LIST, 0, "dense")


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flag_case(oracle):
    blocks = [corpus.text_block(21, i, n, needle_rate=2e-3) for i, n in enumerate((40_000, 16_384, 70_001))]
    blocks[2] = np.concatenate([blocks[2][:-1], SC.u8(b" Holmes")])  # a last line without its newline, with a match
    lits = (b"Sherlock", b"Holmes", b"Watson said")
    return blocks, lits, SC.expected(oracle, blocks, lits)


def test_invert(gs, flag_case):
    blocks, lits, plain = flag_case
    gs.bind(blocks)
    want = invert_model.invert_all_modes(plain, blocks)
    got = list_all_modes(gs, lits, xsg.FLAG_INVERT, matches=False)
    check(got, want, "invert", keys=LINE_KEYS)
    for mode in (xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES):  # a non-match has no offset
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.search_u64(mode)
        assert e.value.code == xsg.ENOTSUP
    with pytest.raises(xsg.XsgError) as e:
        gs.shard.count(xsg.COUNT_MATCHES)
    assert e.value.code == xsg.ENOTSUP


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "invert"])
def test_context(gs, flag_case, invert):
    blocks, lits, plain = flag_case
    gs.bind(blocks)
    base = invert_model.invert_all_modes(plain, blocks) if invert else plain
    want = context_model.context_all_modes(base, blocks, 2, 3)
    flags = xsg.flag_context(2, 3) | (xsg.FLAG_INVERT if invert else 0)
    got = list_all_modes(gs, lits, flags, matches=not invert)
    check(got, want, ("context", invert), keys=[k for k in want if k in got])
    gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS)
    edges = gs.shard.context_edges()
    assert [tuple(int(x) for x in e) for e in edges] == context_model.edges(base, blocks, 2, 3)
    if not invert:
        check_matches(gs, blocks, lits, flags, "context")  # XSG_MATCHES ignores the bits


def test_refusals(gs, flag_case):
    import torch
    blocks, lits, _ = flag_case
    gs.bind(blocks)
    gs.ctx.set_literals(xsg.literal_list(lits))
    d = torch.zeros(xsg.NUM_COUNTERS + 1, dtype=torch.int64, device="cuda:0")
    for mode in (xsg.COUNT_MATCHES, xsg.COUNT_LINES):  # both stream-ordered counts: the route fetches sizes from the device
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.count_async(mode, 0, d.data_ptr())
        assert e.value.code == xsg.ENOTSUP
        with pytest.raises(xsg.XsgError) as e:
            gs.shard.count_async_status(mode, 0, d.data_ptr(), d.data_ptr() + 8 * xsg.NUM_COUNTERS)
        assert e.value.code == xsg.ENOTSUP
    for bad, flags in ((b"", 0), (b"a\n\nb", 0), (b"\na", 0), (b"a", xsg.FLAG_REGEX), (b"a", 0x10), (b"x" * 256, 0)):
        with pytest.raises(xsg.XsgError) as e:
            gs.ctx.set_literals(bad, flags)
        assert e.value.code == xsg.EINVAL
        with pytest.raises(xsg.XsgError) as e:  # a failed call leaves the context without a pattern
            gs.shard.count(xsg.COUNT_MATCHES)
        assert e.value.code == xsg.ESTATE
    gs.ctx.set_literals(xsg.literal_list(lits), xsg.FLAG_EXACT_TAIL)  # accepted, changes nothing
    name = gs.shard.scan_kernel_name(xsg.COUNT_LINES)
    assert "k_set_scan" in name and "k_set_verify" in name
    # (a binding this small keeps the default for every pattern kind: this pins the call on a list, not the kind's own
    # clause in xsg_shard_tune, which only a binding of 1 GiB and more reaches)
    assert gs.shard.tune(xsg.COUNT_MATCHES) is None
    assert gs.shard.time_scan_kernel(xsg.COUNT_LINES, 2) > 0


# ---- call order on one binding ------------------------------------------------------------------------------------------------------------------
def test_call_order_on_one_binding(gs, oracle, flag_case):
    """list -> literal -> regex -> list -> rebind -> list: nothing a pattern of one kind leaves behind reaches the next"""
    from gpu_util import oracle_all_modes
    blocks, lits, want_list = flag_case
    gs.bind(blocks)
    check(list_all_modes(gs, lits), want_list, "list 1")
    check(gs.all_modes(b"Sherlock"), oracle_all_modes(oracle, blocks, b"Sherlock"), "literal")
    rx, _ = oracle_regex_all_modes(oracle, blocks, b"Sher(lock|wood)?")
    check(gs.all_modes(b"Sher(lock|wood)?", xsg.FLAG_REGEX), rx, "regex")
    check(list_all_modes(gs, lits), want_list, "list 2")
    other = [corpus.text_block(22, i, n, needle_rate=1e-3) for i, n in enumerate((20_000, 50_000))]
    gs.bind(other)
    check(list_all_modes(gs, lits, IC), SC.expected(oracle, other, lits, True), "list after rebind")


# ---- the file pipeline, the host seam, the command line ------------------------------------------------------------------------------------------
FILE_LITS = (b"Sherlock", b"Holmes", b"Watson said", b"street of")


@pytest.fixture(scope="module")
def textfile(tmp_path_factory):
    path = tmp_path_factory.mktemp("set") / "text.txt"
    data = np.concatenate([corpus.text_block(31, i, 1 << 20, needle_rate=5e-4) for i in range(3)])
    data.tofile(path)
    return str(path), data


def job_result(path, lits, mode, chunk_bytes, flags=0):
    j = xsg.Job(xsg.literal_list(lits), path, mode, chunk_bytes=chunk_bytes, flags=flags, num_threads=2, num_max_readers=2,
                pattern_is_list=True)
    try:
        r = j.result()
        return r.tolist() if isinstance(r, np.ndarray) else r
    finally:
        j.close()


def test_file_pipeline_all_tags(textfile, oracle):
    path, data = textfile
    chunks = [data[int(c["original_offset"]):int(c["original_offset"] + c["original_size"])] for c in xsg.plan_chunks(path, 256 << 10)]
    assert len(chunks) > 8
    want = SC.expected(oracle, chunks, FILE_LITS)
    strings, _, _ = set_model.matches(chunks, FILE_LITS)
    for mode, key in ((xsg.COUNT_MATCHES, "count_matches"), (xsg.COUNT_LINES, "count_lines"),
                      (xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"), (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"),
                      (xsg.LINE_INDICES, "line_indices"), (xsg.LINES, "lines")):
        assert job_result(path, FILE_LITS, mode, 256 << 10) == want[key], key
    assert job_result(path, FILE_LITS, xsg.MATCHES, 256 << 10) == strings
    with pytest.raises(xsg.XsgError) as e:  # a bad list is refused at the start, not in a worker
        job_result(path, (b"a", b"", b"b"), xsg.COUNT_LINES, 256 << 10)
    assert e.value.code == xsg.EINVAL


def test_file_pipeline_context_is_independent_of_the_chunk_size(textfile, oracle):
    path, data = textfile
    plain = SC.expected(oracle, [data], FILE_LITS)
    want = context_model.context_all_modes(plain, [data], 3, 3)
    for cb in (256 << 10, 1 << 20):
        for mode, key in ((xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices"), (xsg.LINES, "lines")):
            assert job_result(path, FILE_LITS, mode, cb, xsg.flag_context(3, 3)) == want[key], (cb, key)


def test_host_searcher_create_list(textfile, oracle):
    """xsg_host_*: what the Gpu*Searcher functors call, chunk-local, on a searcher made from a list"""
    _, data = textfile
    lib = xsg.load()
    lst = xsg.literal_list(FILE_LITS)
    hs = C.c_void_p()
    assert lib.xsg_host_searcher_create_list(0, b"a\n\nb", 4, 0, 2, C.byref(hs)) == xsg.EINVAL
    assert lib.xsg_host_searcher_create_list(0, lst, len(lst), 0, 2, C.byref(hs)) == xsg.OK, lib.xsg_last_error()
    try:
        for lo, hi in ((0, 300_000), (300_000, 300_017), (1 << 20, 3 << 20)):
            blk = np.ascontiguousarray(data[lo:hi])
            want = SC.expected(oracle, [blk], FILE_LITS)
            n = C.c_uint64(0)
            assert lib.xsg_host_count(hs, blk.ctypes.data, blk.size, 0, C.byref(n)) == xsg.OK
            assert n.value == want["count_matches"]
            assert lib.xsg_host_count(hs, blk.ctypes.data, blk.size, 1, C.byref(n)) == xsg.OK
            assert n.value == want["count_lines"]
            for mode, key in ((xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"), (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"),
                              (xsg.LINE_INDICES, "line_indices")):
                out = C.c_void_p()
                assert lib.xsg_host_offsets(hs, mode, blk.ctypes.data, blk.size, C.byref(out), C.byref(n)) == xsg.OK
                got = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
                lib.xsg_free(out)
                assert got == want[key], (lo, key)
            for fn, strings in ((lib.xsg_host_lines, want["lines"]), (lib.xsg_host_matches, set_model.matches([blk], FILE_LITS)[0])):
                lens, raw, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
                assert fn(hs, blk.ctypes.data, blk.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == xsg.OK
                ln = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].copy()
                buf = C.string_at(raw, nb.value)
                lib.xsg_free(lens)
                lib.xsg_free(raw)
                ends = np.cumsum(ln.astype(np.int64))
                assert [buf[int(e) - int(k):int(e)] for e, k in zip(ends, ln)] == strings, lo
    finally:
        lib.xsg_host_searcher_destroy(hs)


CLI_LITS = (b"Sherlock", b"Holmes", b"watson SAID")


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """a 300 KB file, the word list as a grep -f file, and what the model says xsgrep prints for every option"""
    d = tmp_path_factory.mktemp("setcli")
    raw = corpus.text_block(33, 0, 300_000, needle_rate=2e-3).tobytes()
    (d / "text.txt").write_bytes(raw)
    (d / "words.txt").write_bytes(b"\n".join(CLI_LITS) + b"\n")
    arr = [np.frombuffer(raw, dtype=np.uint8)]
    plain = set_model.all_modes([raw], CLI_LITS)
    icase = set_model.all_modes([raw], CLI_LITS, True)
    assert icase["count_lines"] > plain["count_lines"] > 0

    def text(lines):
        return b"".join(l + b"\n" for l in lines)
    head = raw[:100_003]  # (ends inside a line: the pipe's last line lacks its newline and is not printed)
    want = {
        "default": text(plain["lines"]),
        "stdin": text(set_model.all_modes([head], CLI_LITS)["lines"]),
        "-c": b"%d\n" % plain["count_lines"],
        "-v": text(invert_model.invert_all_modes(plain, arr)["lines"]),
        "-o": text(set_model.matches([raw], CLI_LITS)[0]),
        "-i": text(icase["lines"]),
        "-C": text(context_model.context_all_modes(plain, arr, 1, 1)["lines"]),
    }
    return str(d / "text.txt"), str(d / "words.txt"), head, want


def xsgrep(*args, stdin=None):
    r = subprocess.run([str(ROOT / "tools" / "build" / "xsgrep"), *args], input=stdin, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


AS_E = [x for l in CLI_LITS for x in ("-e", l.decode())]


@pytest.mark.parametrize("name,args", [
    ("default", ["-F", "-f", "WORDS", "FILE"]),
    ("default", ["-F", *AS_E, "FILE"]),
    ("stdin", ["-F", *AS_E, "-"]),
    ("-c", ["-F", "-c", "-f", "WORDS", "FILE"]),
    ("-v", ["-F", "-v", "-f", "WORDS", "FILE"]),
    ("-o", ["-F", "-o", *AS_E, "FILE"]),
    ("-i", ["-F", "-i", "-f", "WORDS", "FILE"]),
    ("-C", ["-F", "-C", "1", "-f", "WORDS", "FILE"]),
], ids=["-f", "-e", "stdin", "-c", "-v", "-o", "-i", "-C1"])
def test_xsgrep_with_several_patterns(cli_case, name, args):
    """xsgrep -F -f / -e ... -e against the model; -o is leftmost-first in listing order"""
    path, words, head, want = cli_case
    args = [path if a == "FILE" else words if a == "WORDS" else a for a in args]
    assert xsgrep(*args, stdin=head if name == "stdin" else None) == want[name]


def test_xsgrep_a_single_e_equals_the_positional_pattern(cli_case):
    path = cli_case[0]
    out = xsgrep("-F", "-e", "Sherlock", path)
    assert out == xsgrep("-F", "Sherlock", path) and out.count(b"Sherlock") > 0
