"""XSG_MATCHES on the GPU: lengths, bytes and offsets element by element against tests/match_model.py (the oracle's
match list plus a length), on every route, at the edges of the tile / span / output-unit geometry, on the on-demand
result path, through the job layer, the host-searcher seam and xsgrep -o; the refusals; call orders.

Without the feature every case fails at the first search ("mode 6 is not a list mode") or, for the job, at its start."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import corpus
import match_model
import xsg
from gpu_util import GpuSearch, oracle_all_modes, oracle_regex_all_modes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TILE = 16384   # a workgroup's tile (k_scan, k_rx_scan)
KBLOCK = 256   # entries per workgroup of the span / gather kernels
R, I, X = xsg.FLAG_REGEX, xsg.FLAG_IGNORE_CASE, xsg.FLAG_EXACT_TAIL

WORDS = corpus.LEXICON + [b"Sherlock", b"Sherwood", b"colour", b"color", b"COLOUR", b"running", b"locking", b"ing", b"abc1", b"x9",
                          b"aab", b"aaab", b"end.", b"bc", b"abca", b"abab", b"abababab", b"She lock", b"line\nbreak", b"tab\t\n  gap"]


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


def make_text():
    """three tiles of words, every needle of this file among them, occurrences of `Sherlock` inside the last plen + 31
    bytes and no final newline.  The end is lossy by construction: fewer than 32 + plen bytes follow the last but one
    `Sherlock`, so the reference searches them byte by byte, and in `SheSherlock` it resumes behind the second `S`
    (the byte that ended the partial match) and misses the last occurrence; XSG_FLAG_EXACT_TAIL finds it."""
    t = corpus.text_block(61, 0, 3 * TILE - 40, needle=b"Sherlock", needle_rate=1e-2, lexicon=WORDS)
    return np.concatenate([t[:-1], _u8(b" colour Sherlock and SheSherlock")])


@pytest.fixture(scope="module")
def text():
    return make_text()


def cuts(text):
    """the text as 1, 2 and 5 chunks (cut anywhere: inside words, inside matches) with non-trivial global offsets"""
    n = text.size
    out = [([text], [12345])]
    out.append(([text[:TILE + 63], text[TILE + 63:]], [7, 1 << 33]))
    e = [0, 4097, TILE - 1, TILE + 4096 + 65, 2 * TILE + 15, n]
    out.append(([text[a:b] for a, b in zip(e[:-1], e[1:])], [3, 100_000, 1 << 20, (1 << 40) + 5, (1 << 41)]))
    return out


def check(gs, oracle, blocks, pat, flags, go=None, view=False, nonempty=False, what=""):
    want_s, want_o, want_n = match_model.matches(oracle, blocks, pat, flags, go)
    gs.ctx.set_pattern(pat, flags)
    got_s, got_o = gs.shard.search_matches()
    ctx = f"{what} pattern={pat!r} flags={flags} sizes={[int(b.size) for b in blocks]}"
    assert len(got_s) == len(want_s), ctx
    assert got_o.tolist() == want_o, ctx
    assert [len(s) for s in got_s] == want_n, ctx
    assert got_s == want_s, ctx
    if view:
        vl, vb, vo = gs.shard.search_matches_view()
        assert vl.tolist() == want_n and vo.tolist() == want_o and vb.tobytes() == b"".join(want_s), ctx + " (view)"
    if nonempty:
        assert want_s, "the case holds no match: " + ctx
    return want_s


# (pattern, flags, toggles that put it on each of its routes)
PRE = [{"XSG_RX_PRE": "0"}, {"XSG_RX_PRE": "1"}]
FAC = [{"XSG_RX_FAC": "0"}, {"XSG_RX_FAC": "1"}]
ROUTES = [
    (b"Sherlock", 0, [{}]),                      # literal, the reference's lossy end of chunk
    (b"Sherlock", X, [{}]),
    (b"sherLOCK", I | X, [{}]),                  # the text keeps its case
    (b"colour", I, [{}]),
    (b"abab", X, [{}]),                          # bordered: the greedy walk (abababab holds two)
    (b"abab", 0, [{}]),
    (b"line\nbreak", X, [{}]),                   # a literal that contains '\n'
    (b"She[r ]lock", R, [{}]),                   # class sequence
    (b"she[r ]lock", R | I, [{}]),
    (b"Holmes|Watson", R, [{}]),                 # alternation of one length
    (b"colou?r", R, PRE),                        # automaton with a prefix
    (b"colou?r", R | I, PRE),
    (b"Sher(lock|wood)", R, PRE),
    (b"\\w+ing", R, FAC),                        # automaton with a factor
    (b"[a-z]+[0-9]", R, [{}]),                   # automaton with neither
    (b"a+?b", R, PRE),                           # lazy
    (b"\\s+", R, [{}]),                          # matches across lines: k_rx_chunk
    (b"(?m)^[A-Z][a-z]+", R, [{}]),              # the anchored forms: line walk only (no prefilter), the factor mask applies
    (b"(?m)[a-z]+\\.$", R, FAC),
    (b"(?m)^(?:a|bc)+$", R, [{}]),
]


@pytest.mark.parametrize("pat,flags,envs", ROUTES, ids=[f"{p.decode()!r}/{f}" for p, f, _ in ROUTES])
def test_every_route(gs, oracle, text, monkeypatch, pat, flags, envs):
    for blocks, go in cuts(text):
        gs.bind(blocks, go)
        for env in envs:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            check(gs, oracle, blocks, pat, flags, go, view=len(blocks) == 2, nonempty=True, what=str(env))
            for k in env:
                monkeypatch.delenv(k)


def test_occurrences_in_the_lossy_tail_zone(gs, oracle, text):
    """the last plen + 31 bytes hold occurrences: EXACT_TAIL reports more than the default, both as the oracle does"""
    gs.bind([text], [0])
    lossy = check(gs, oracle, [text], b"Sherlock", 0)
    exact = check(gs, oracle, [text], b"Sherlock", X)
    assert len(exact) == len(lossy) + 1 and exact[:-1] == lossy


# ---- edges, placed by construction ---------------------------------------------------------------------------------
def _one(gs, oracle, chunk: bytes, pat, flags, expect, env=None, monkeypatch=None, go=999):
    blocks = [_u8(chunk)]
    gs.bind(blocks, [go])
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    got = check(gs, oracle, blocks, pat, flags, [go], view=True)
    for k in (env or {}):
        monkeypatch.delenv(k)
    assert got == expect, (pat, flags)


@pytest.mark.parametrize("pat,flags", [(b"Sherlock", X), (b"She[r ]lock", R), (b"Sher(lock|wood)", R), (b"(?m)^Sher[a-z]+", R)])
def test_a_match_from_the_last_byte_of_a_tile_into_the_next(gs, oracle, pat, flags):
    chunk = b"x" * (TILE - 2) + b"\n" + b"Sherlock Holmes\n" + b"y" * 100 + b"\n"
    assert chunk.index(b"Sherlock") == TILE - 1
    _one(gs, oracle, chunk, pat, flags, [b"Sherlock"])


@pytest.mark.parametrize("pat,flags", [(b"colour", X), (b"colo[u]r", R), (b"colou?r", R), (b"(?m)colou?r$", R), (b"\\s*colou?r", R)])
def test_a_match_that_ends_the_chunk_without_a_newline(gs, oracle, pat, flags):
    _one(gs, oracle, b"a line\nsome text colour", pat, flags, [b" colour" if pat.startswith(b"\\s") else b"colour"])


@pytest.mark.parametrize("pat,flags", [(b"colour", X), (b"colou?r", R), (b"(?m)^colou?r$", R), (b"[a-z]{6}", R)])
def test_a_match_that_is_the_whole_chunk(gs, oracle, pat, flags):
    _one(gs, oracle, b"colour", pat, flags, [b"colour"])


@pytest.mark.parametrize("pat,flags", [(b"a", X), (b"a+", R), (b"[ab]", R)])
def test_chunks_of_0_1_and_15_bytes(gs, oracle, pat, flags):
    blocks = [_u8(b""), _u8(b"a"), _u8(b"aaaaaaaaaaaaaab"), _u8(b""), _u8(b"b")]
    go = [0, 10, 20, 40, 50]
    gs.bind(blocks, go)
    got = check(gs, oracle, blocks, pat, flags, go, view=True)
    assert b"".join(got).count(b"a") == 15


@pytest.mark.parametrize("pat,flags", [(b"ab", X), (b"ab", R), (b"(?m)^ab", R), (b"ab+?", R)])
def test_two_matches_that_touch(gs, oracle, pat, flags):
    _one(gs, oracle, b"abab", pat, flags, [b"ab", b"ab"])


@pytest.mark.parametrize("env", [{}, {"XSG_RX_PRE": "1"}], ids=["line-walk", "prefilter-over-its-budget"])
def test_a_run_of_5000_over_a_span_and_a_tile(gs, oracle, monkeypatch, env):
    """`a+` over 5 000 `a`: longer than the 4 KiB verification budget (the prefilter route gives way to the line walk),
    across a tile boundary, and far over the 256 bytes above which a string is no lane's own copy"""
    head = b"b\n" * ((TILE - 2000) // 2)
    chunk = head + b"a" * 5000 + b"\nbaab\n"
    assert len(head) < TILE < len(head) + 5000
    _one(gs, oracle, chunk, b"a+", R, [b"a" * 5000, b"aa"], env, monkeypatch)


def test_300_matches_of_lengths_1_to_17(gs, oracle):
    """output units start at every alignment: lengths 1..17 cycle, so the packed offsets run through all residues mod 16"""
    chunk = b"".join(b"a" * (1 + k % 17) + (b"b\n" if k % 5 == 0 else b"b") for k in range(300))
    blocks = [_u8(chunk)]
    gs.bind(blocks, [5])
    got = check(gs, oracle, blocks, b"a+", R, [5], view=True)
    assert [len(s) for s in got] == [1 + k % 17 for k in range(300)]
    starts = np.cumsum([0] + [len(s) for s in got[:-1]])
    assert set(int(x) % 16 for x in starts) == set(range(16))


@pytest.mark.parametrize("n", [0, KBLOCK - 1, KBLOCK, KBLOCK + 1, 2 * KBLOCK])
@pytest.mark.parametrize("pat,flags", [(b"ab", X), (b"ab?", R)])
def test_results_around_one_workgroup_of_entries(gs, oracle, n, pat, flags):
    blocks = [_u8(b"ab " * n + b"xx\n")]
    gs.bind(blocks, [0])
    got = check(gs, oracle, blocks, pat, flags, [0], view=True)
    assert len(got) == n


# ---- the on-demand result path ---------------------------------------------------------------------------------------
ON_DEMAND = [(b"Sherlock", X, {}), (b"She[r ]lock", R, {}), (b"colou?r", R, {"XSG_RX_PRE": "0"}), (b"colou?r", R, {"XSG_RX_PRE": "1"}),
             (b"\\w+ing", R, {"XSG_RX_FAC": "1"}), (b"\\s+", R, {}), (b"(?m)^[A-Z][a-z]+", R, {})]


@pytest.mark.parametrize("pat,flags,env", ON_DEMAND, ids=[f"{p.decode()!r}/{e}" for p, _, e in ON_DEMAND])
def test_results_fetched_on_demand(gs, oracle, text, monkeypatch, pat, flags, env):
    """XSG_LINES_EAGER=0: lengths, offsets and bytes stay on the device until an accessor asks"""
    blocks, go = cuts(text)[2]
    gs.bind(blocks, go)
    monkeypatch.setenv("XSG_LINES_EAGER", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check(gs, oracle, blocks, pat, flags, go, view=True, nonempty=True, what="on demand")
    monkeypatch.delenv("XSG_LINES_EAGER")
    check(gs, oracle, blocks, pat, flags, go, view=True, what="mirrors again")


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(xsg.XsgError) as e:
        call()
    return e.value


def test_refusals_leave_no_state_behind(gs, oracle, text):
    blocks, go = cuts(text)[1]
    gs.bind(blocks, go)
    gs.ctx.set_pattern(b"Sherlock", xsg.FLAG_INVERT)
    e = _refused(gs.shard.search_matches)
    assert e.code == xsg.ENOTSUP and "invert" in str(e).lower()
    gs.ctx.set_pattern(b"Sherlock", 0)
    for mode in (xsg.MATCHES, xsg.MATCHES | xsg.WITH_NEWLINES):
        assert _refused(lambda: gs.shard.count(mode)).code == xsg.EINVAL
    assert _refused(lambda: gs.shard.count_begin(xsg.MATCHES)).code == xsg.EINVAL
    check(gs, oracle, blocks, b"colou?r", R, go, nonempty=True)
    # the u64 accessors behave as after an XSG_LINES search
    out = np.empty(4, dtype=np.uint64)
    assert gs.shard._lib.xsg_result_u64(gs.shard.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 4) == xsg.ESTATE
    nl = C.c_uint64(0)
    assert gs.shard._lib.xsg_result_newlines(gs.shard.h, C.byref(nl)) == xsg.ESTATE
    # any other tag afterwards on the same binding equals the oracle
    for pat, flags in ((b"colou?r", R), (b"Sherlock", 0), (b"She[r ]lock", R)):
        got = gs.all_modes(pat, flags)
        want = (oracle_regex_all_modes(oracle, blocks, pat, False, go)[0] if flags & R else oracle_all_modes(oracle, blocks, pat, global_offsets=go))
        for k, v in want.items():
            assert got[k] == v, (pat, k)
        check(gs, oracle, blocks, pat, flags, go, nonempty=True, what="after all tags")


@pytest.mark.parametrize("pat", [b"a.c", b"a.+c", b"a[^b]c"])
def test_dot_refuses_bytes_from_0x80(gs, oracle, pat):
    blocks = [_u8(b"abc a\xc3\xa9c abbc\n")]
    gs.bind(blocks, [0])
    gs.ctx.set_pattern(pat, R)
    assert _refused(gs.shard.search_matches).code == xsg.ENOTSUP
    ascii_blocks = [_u8(b"abc axc abbc\n")]
    gs.bind(ascii_blocks, [0])
    check(gs, oracle, ascii_blocks, pat, R, [0], nonempty=True)


def test_a_chunk_of_4_gib_refuses_lengths_that_vary(oracle):
    """the automaton routes carry a match's length as uint32: on a binding with a chunk of 4 GiB an expression whose
    matches vary in length is refused before anything runs (the buffer is never read, so it is left unwritten)"""
    import torch
    n = 1 << 32
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    ctx = xsg.Context(0)
    shard = xsg.Shard(ctx, buf.data_ptr(), buf.numel(), xsg.make_chunks([0], [n]))
    ctx.set_pattern(b"colou?r", R)
    e = _refused(shard.search_matches)
    assert e.code == xsg.ENOTSUP and "4 GiB" in str(e)
    shard.close()
    ctx.close()


# ---- call order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pat,flags", [(b"Sherlock", X), (b"colou?r", R), (b"She[r ]lock", R), (b"\\s+", R)])
def test_first_call_of_a_fresh_context(oracle, text, pat, flags):
    blocks, go = cuts(text)[1]
    fresh = GpuSearch()
    fresh.bind(blocks, go)
    check(fresh, oracle, blocks, pat, flags, go, view=True, nonempty=True, what="first call")
    fresh.shard.close()
    fresh.ctx.close()


def test_between_two_line_searches_of_another_pattern(gs, oracle, text):
    blocks, go = cuts(text)[2]
    gs.bind(blocks, go)
    lines_want = oracle_all_modes(oracle, blocks, b"Holmes", global_offsets=go)
    for pat, flags in ((b"colou?r", R), (b"Sherlock", 0), (b"\\w+ing", R)):
        gs.ctx.set_pattern(b"Holmes", 0)
        ls, lo = gs.shard.search_lines()
        assert (ls, lo.tolist()) == (lines_want["lines"], lines_want["lines_offsets"])
        check(gs, oracle, blocks, pat, flags, go, nonempty=True, what="between two XSG_LINES")
        gs.ctx.set_pattern(b"Holmes", 0)
        ls, lo = gs.shard.search_lines()
        assert (ls, lo.tolist()) == (lines_want["lines"], lines_want["lines_offsets"])


# ---- the job layer, the seam, the command line ------------------------------------------------------------------------------
CHUNK = 16 << 10


@pytest.fixture(scope="module")
def textfile(tmp_path_factory):
    d = tmp_path_factory.mktemp("xsmatches")
    data = corpus.text_block(62, 0, 200_000, needle=b"Sherlock", needle_rate=1e-2, lexicon=WORDS)
    data = np.concatenate([data[:-1], _u8(b" Sherlock or SheSherlock")])  # the lossy end of `text`, no final newline
    p = d / "t.txt"
    data.tofile(p)
    plan = xsg.plan_chunks(str(p), CHUNK)
    chunks = [data[int(c["original_offset"]):int(c["original_offset"] + c["original_size"])] for c in plan]
    go = [int(c["original_offset"]) for c in plan]
    assert len(chunks) > 8
    return str(p), chunks, go


@pytest.mark.parametrize("pat,flags", [(b"Sherlock", 0), (b"\\w+ing", R), (b"(?m)^[A-Z][a-z]+", R)])
def test_job_over_a_file(textfile, oracle, pat, flags):
    path, chunks, go = textfile
    want_s, want_o, _ = match_model.matches(oracle, chunks, pat, flags, go)
    assert want_s
    j = xsg.Job(pat, path, xsg.MATCHES, num_threads=2, num_max_readers=2, chunk_bytes=CHUNK, flags=flags)
    got = j.result()
    assert j.total() == len(want_s)
    v = C.c_uint64(0)
    assert j._lib.xsg_job_get_u64(j.h, 0, 1, C.byref(v)) == xsg.ESTATE  # strings, as for XSG_LINES
    j.close()
    assert got == want_s
    live = xsg.Job(pat, path, xsg.MATCHES, chunk_bytes=CHUNK, flags=flags)
    assert list(live) == want_s
    live.close()


def test_host_searcher_seam(textfile, oracle):
    """xsg_host_matches: what xs::GpuMatchSearcher calls, chunk-local"""
    _, chunks, _ = textfile
    lib = xsg.load()
    for pat, flags in ((b"Sherlock", X), (b"colou?r", R)):
        hs = C.c_void_p()
        assert lib.xsg_host_searcher_create(0, pat, len(pat), flags, 2, C.byref(hs)) == xsg.OK
        try:
            for i, b in enumerate(chunks[:2] + [chunks[-1], _u8(b"")]):
                want_s, _, want_n = match_model.matches(oracle, [b], pat, flags)
                data = np.ascontiguousarray(b)
                lens, raw, n, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
                assert lib.xsg_host_matches(hs, data.ctypes.data, data.size, C.byref(lens), C.byref(raw), C.byref(n), C.byref(nb)) == xsg.OK
                ll = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].tolist()
                blob = C.string_at(raw, nb.value)
                lib.xsg_free(lens)
                lib.xsg_free(raw)
                assert ll == want_n and blob == b"".join(want_s), (pat, i)
        finally:
            lib.xsg_host_searcher_destroy(hs)


def test_xsgrep_only_matching(textfile, oracle):
    """xsgrep -o over a file, -o over stdin (GpuMatchSearcher), and -oc: the count stays the count of matching lines"""
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    path, chunks, _ = textfile
    env = dict(os.environ, XS_CHUNK_BYTES=str(CHUNK))
    want = match_model.matches(oracle, chunks, b"colou?r", R)[0]
    r = subprocess.run([str(exe), "-oE", "colou?r", path], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.split(b"\n")[:-1] == want, r.stderr.decode()
    want_i = match_model.matches(oracle, chunks, b"sherlock", I)[0]
    r = subprocess.run([str(exe), "-o", "-i", "-F", "sherlock", path], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.split(b"\n")[:-1] == want_i, r.stderr.decode()
    whole = np.concatenate(chunks)  # stdin is read as one newline-aligned chunk of up to 16 MiB
    want_stdin = match_model.matches(oracle, [whole], b"colou?r", R)[0]
    r = subprocess.run([str(exe), "-o", "-E", "colou?r", "-"], input=whole.tobytes(), capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.split(b"\n")[:-1] == want_stdin, r.stderr.decode()
    lines = oracle_regex_all_modes(oracle, chunks, b"colou?r", False)[0]["count_lines"]
    r = subprocess.run([str(exe), "-oc", "-E", "colou?r", path], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and int(r.stdout) == lines, r.stderr.decode()


# ---- a random sweep ------------------------------------------------------------------------------------------------------
def sweep_cases(seed, n=36):
    """n cases of (blocks, global offsets, pattern, flags): literals and substrings as tests/test_gpu_fuzz.py draws them,
    and expressions put together from a few pieces"""
    from test_gpu_fuzz import SIZES, rand_pattern
    rng = np.random.default_rng(4200 + seed)
    alphabets = [_u8(b"ab"), _u8(b"ab\n"), _u8(b"abcAB \n\n"), _u8(b"Sherlock Holmes\n"), _u8(b"ab01 \n")]
    atoms = [b"a", b"b", b"[ab]", b"[a-c]", b"\\w", b"[0-9]", b"o", b"(ab|b)", b"(?:l|lo)", b"e", b" "]
    ops = [b"", b"", b"+", b"*", b"?", b"+?", b"{2}", b"{1,3}"]
    for _ in range(n):
        alphabet = alphabets[int(rng.integers(0, len(alphabets)))]
        literal = rng.random() < 0.5
        # (an expression's chunks stay small: the model's backtracking engine is quadratic on some of them; the tile
        # and span edges of the automaton routes have their own cases above)
        top = 40000 if literal else 3000
        blocks = []
        for _k in range(int(rng.integers(1, 5))):
            size = int(rng.choice([v for v in SIZES if v <= top])) if rng.random() < 0.6 else int(rng.integers(0, top))
            b = alphabet[rng.integers(0, len(alphabet), size=size)].copy()
            if size and rng.random() < 0.5:
                b[-1] = 10
            blocks.append(b)
        go = (np.cumsum([0] + [int(b.size) + int(rng.integers(0, 1000)) for b in blocks[:-1]]) + int(rng.integers(0, 1 << 35))).tolist()
        flags = (X if rng.random() < 0.5 else 0) | (I if rng.random() < 0.3 else 0)
        if literal:
            pat = rand_pattern(rng, max(blocks, key=lambda x: x.size), alphabet)[:64]
        else:
            pat = b"".join(atoms[int(rng.integers(0, len(atoms)))] + ops[int(rng.integers(0, len(ops)))] for _k in range(int(rng.integers(1, 4))))
            if rng.random() < 0.2:
                pat = b"(?m)^" + pat
            flags = (flags & I) | R
        yield blocks, go, pat, flags


SWEEP_SEEDS = [1, 2]
MAX_SKIPPED = 0.25


def sweep_skips(oracle, seed):
    """-> (cases, those the oracle's expression reader refuses): needs no GPU"""
    from xs_oracle import UnsupportedRegex
    cases, skipped = [], 0
    for blocks, go, pat, flags in sweep_cases(seed):
        try:
            want = match_model.matches(oracle, blocks, pat, flags, go)
        except (UnsupportedRegex, xsg.XsgError):
            skipped += 1
            continue
        cases.append((blocks, go, pat, flags, want))
    return cases, skipped


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_random_sweep(gs, oracle, seed):
    cases, skipped = sweep_skips(oracle, seed)
    assert len(cases) + skipped <= 40
    assert skipped <= MAX_SKIPPED * (len(cases) + skipped), f"{skipped} of {len(cases) + skipped} cases drawn are refused"
    for blocks, go, pat, flags, want in cases:
        gs.bind(blocks, go)
        try:
            gs.ctx.set_pattern(pat, flags)
        except xsg.XsgError as e:  # the product's reader refuses what the oracle's accepts: counted with the skipped
            assert e.code == xsg.ENOTSUP, (pat, str(e))
            skipped += 1
            continue
        got_s, got_o = gs.shard.search_matches()
        ctx = f"seed={seed} pattern={pat!r} flags={flags} sizes={[int(b.size) for b in blocks]}"
        assert got_o.tolist() == want[1], ctx
        assert got_s == want[0], ctx
    assert skipped <= MAX_SKIPPED * (len(cases) + skipped), f"{skipped} cases were refused by one reader or the other"
