"""Line anchors, (?m) [^] BODY [$], on the GPU: every case through all six tags (GpuSearch.all_modes) against the
restated walks of tests/anchor_oracle.py, and through the stream-ordered count, the file pipeline, the C++ surface
and xsgrep."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import anchor_oracle
import corpus
import xsg
from gpu_util import GpuSearch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

CLASS_BODIES = [b"(?m)^Sherlock", b"(?m)^She[r ]lock", b"(?m)Holmes[.,]$", b"(?m)^[A-Z][a-z]{3}$", b"(?m)^(?:ab|cd)",
                b"(?m)abc"]
AUTOMATON = [b"(?m)^Sher.*mes", b"(?m)^\\w+ing", b"(?m)colou?r$", b"(?m)\\w+ing$", b"(?m)^[A-Z][a-z]+ [A-Z][a-z]+$",
             b"(?m)^a{40}", b"(?m)^a+?$"]
SMALL = [b"(?m)^ab", b"(?m)ab$", b"(?m)^ab$", b"(?m)^aa", b"(?m)^(?:ab|ba)", b"(?m)^a+", b"(?m)a+?$", b"(?m)^a+b$",
         b"(?m)^[ab]{3}"]


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8)


def check(gs, blocks, expr, icase=False, ctx="", **kw):
    flags = xsg.FLAG_REGEX | (xsg.FLAG_IGNORE_CASE if icase else 0)
    want = anchor_oracle.all_modes(blocks, expr, icase, **kw)
    got = gs.all_modes(expr, flags)
    for k in want:
        assert got[k] == want[k], f"{ctx} expr={expr!r} icase={icase}: {k}: got {str(got[k])[:200]} want {str(want[k])[:200]}"
    return want


def _route(gs, expr):
    gs.ctx.set_pattern(expr, xsg.FLAG_REGEX)
    return gs.shard.scan_kernel_name(xsg.COUNT_MATCHES)


KNOWN = [
    (b"(?m)^ab", b"abab\nxab\nab"), (b"(?m)^ab", b"xxab"), (b"(?m)ab$", b"abab\nab"), (b"(?m)ab$", b"abyy\n"),
    (b"(?m)^aa", b"aaaaa\n"), (b"(?m)^(?:ab|cd)", b"abcdab cd\ncd\n"), (b"(?m)^a+", b"aaab aa\n"),
    (b"(?m)^[A-Z][a-z]+$", b"Holmes\nHolmes.\nWatson"), (b"(?m)[a-z]+ing$", b"king sing\nringing\n"),
]


def test_known_answers(gs):
    for expr, chunk in KNOWN:
        blocks = [_u8(chunk)]
        gs.bind(blocks)
        want = check(gs, blocks, expr, ctx="known")
        assert want["count_matches"] == len(anchor_oracle.AnchorProgram(expr).match_starts(chunk))


def test_anchored_expressions_run_their_kernels(gs):
    gs.bind([corpus.text_block(3, 0, 100_000)])
    for expr in CLASS_BODIES + AUTOMATON:
        name = _route(gs, expr)
        _, bol, eol = anchor_oracle.split(expr)
        if bol or eol:  # the line walks of the automaton route, naming their anchors
            assert "k_rx_" in name and "anchored=" + ("^" if bol else "") + ("$" if eol else "") in name, (expr, name)
        else:  # (?m) without an anchor: BODY's own search
            assert "k_rx_" not in name and "anchored" not in name, (expr, name)


@pytest.mark.parametrize("variant", ["hot0", "hot1", "probe"])
def test_must_serve_on_text(variant):
    gs = GpuSearch(hot=0) if variant == "hot0" else GpuSearch(hot=1) if variant == "hot1" else GpuSearch(probe=True)
    blocks = [corpus.text_block(50 + i, i, 150_000 + 997 * i, needle_rate=2e-3) for i in range(3)]
    # lines that start and end with the bodies, so that each expression has something to find
    extra = (b"Sherlock Holmes was here\nShe lock\nHolmes.\nHolmes,\nThat colour\nSher and Holmes\nrunning\nAbcd\n"
             b"Sherlock Holmes\nab\ncdab\nabc abc\n" + b"a" * 45 + b"\n" + b"aaa\n" + b"a" * 40)
    blocks.append(_u8(extra))
    gs.bind(blocks)
    for expr in CLASS_BODIES + AUTOMATON:
        for icase in (False, True):
            check(gs, blocks, expr, icase, ctx=variant)


@pytest.mark.parametrize("seed", range(3))
def test_must_serve_on_small_alphabet(gs, seed):
    blocks = [corpus.small_alphabet(seed * 7 + i, 30_000 + 4099 * i) for i in range(3)]
    blocks[1] = np.concatenate([blocks[1], _u8(b"a" * 50)])  # a chain that runs to the chunk's end
    gs.bind(blocks)
    for expr in SMALL + [b"(?m)^a{40}", b"(?m)^a+?$"]:
        for icase in (False, True):
            check(gs, blocks, expr, icase, ctx=f"small{seed}")


def test_chunk_edges_in_mid_line(gs):
    """chunk k ends with BODY's tail, chunk k+1 starts with BODY's head: the edge is a line edge, nothing is read across"""
    for expr, a, b in [(b"(?m)ab$", b"xxab\nqqa", b"bzz\n"), (b"(?m)^ab", b"zz\nxa", b"bab\n"),
                       (b"(?m)^Sherlock$", b"Sher", b"lock\nSherlock"), (b"(?m)^\\w+ing$", b"go sing", b"ing\nking")]:
        for pad in (0, 1, 5, 15, 16, 17):
            blocks = [_u8(a + b"q" * pad), _u8(b"ab" * pad + b)]
            gs.bind(blocks)
            check(gs, blocks, expr, ctx=f"edge{pad}")


def test_line_edges_around_tile_boundaries(gs):
    """line starts and ends at every offset from -40 to +40 around multiples of 4 KiB and 16 KiB: one chunk per offset
    d, in which a line STARTS with `ab` at 4096 + d, 16384 + d and 32768 + d and a line ENDS with `ab` at 8192 + d,
    20480 + d and 49152 + d (the k_rx_count spans are 4 KiB, the k_rx_scan tiles 16 KiB)"""
    rng = np.random.default_rng(5)
    base = rng.choice(_u8(b"xyz "), size=53_000).astype(np.uint8)
    blocks = []
    for d in range(-40, 41):
        c = base.copy()
        for m in (4096, 16384, 32768):
            c[m + d - 1] = 10
            c[m + d:m + d + 2] = _u8(b"ab")
        for m in (8192, 20480, 49152):
            c[m + d - 2:m + d] = _u8(b"ab")
            c[m + d] = 10
        blocks.append(c)
    blocks.append(base[:16384 + 2].copy())  # and a chunk that ends 2 bytes behind a tile
    gs.bind(blocks)
    for expr in (b"(?m)^ab", b"(?m)ab$", b"(?m)^ab[^\\n]*ab$", b"(?m)^a+b", b"(?m)[xyz ]ab$"):
        want = check(gs, blocks, expr, ctx="tiles")
        if expr in (b"(?m)^ab", b"(?m)ab$"):
            assert want["count_matches"] >= 3 * 81, expr


def test_fixed_length_bodies_whose_unanchored_automaton_is_too_big(gs):
    """`a[ab]{12}` is served by the class route; before the `(?m)` forms, its unanchored automaton (2^13 states) was
    never needed.  The anchored forms do not build it: what xsg_regex_check accepts, xsg_set_pattern serves."""
    blocks = [corpus.small_alphabet(11 + i, 40_000, alphabet=b"ab\n" + b"ab" * 6) for i in range(2)]
    gs.bind(blocks)
    for expr in (b"(?m)^a[ab]{12}", b"(?m)a[ab]{12}$", b"(?m)^a[ab]{12}$", b"(?m)^[ab]{20}b$"):
        assert xsg.regex_check(expr)[0] > 0
        check(gs, blocks, expr, ctx="big")


def test_a_one_mib_chain(gs):
    chain = b"ab" * 2 ** 19 + b"\n"
    for blocks, n in (([_u8(chain)], 2 ** 19), ([_u8(b"x" + chain)], 0)):
        gs.bind(blocks)
        want = check(gs, blocks, b"(?m)^ab", ctx="chain")
        assert want["count_matches"] == n and want["count_lines"] == (1 if n else 0)


def test_count_async_status(gs):
    import torch
    blocks = [corpus.text_block(9, i, 1 << 20, needle_rate=1e-3) for i in range(3)]
    gs.bind(blocks)
    buf = torch.full((xsg.NUM_COUNTERS + 1,), 77, dtype=torch.int64, device="cuda:0")
    st = torch.cuda.Stream()
    for expr in (b"(?m)^Sherlock", b"(?m)\\w+ing$"):
        want = anchor_oracle.all_modes(blocks, expr)
        for mode, key, ctr in ((xsg.COUNT_MATCHES, "count_matches", xsg.CTR_MATCHES),
                               (xsg.COUNT_LINES, "count_lines", xsg.CTR_LINES)):
            gs.ctx.set_pattern(expr, xsg.FLAG_REGEX)
            gs.shard.count_async_status(mode, st.cuda_stream, buf.data_ptr(), buf.data_ptr() + 8 * xsg.NUM_COUNTERS)
            st.synchronize()
            got = buf.cpu().numpy().astype(np.uint64)
            assert int(got[xsg.NUM_COUNTERS]) == xsg.STATUS_OK
            assert int(got[ctr]) == want[key], (expr, key)


def test_job_over_a_planned_file(tmp_path):
    blocks = [corpus.text_block(77, i, 200_000, needle_rate=2e-3) for i in range(3)]
    data = np.concatenate(blocks)
    path = tmp_path / "t.txt"
    data.tofile(path)
    for expr in (b"(?m)^Sherlock", b"(?m)Holmes[.,]$", b"(?m)^Sher.*mes"):
        # chunks are newline-aligned, so the walks of the chunks concatenate to the walk of the file
        want = anchor_oracle.all_modes([data], expr)
        for mode, key in ((xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"), (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets")):
            j = xsg.Job(expr, str(path), mode=mode, flags=xsg.FLAG_REGEX, chunk_bytes=65536, num_threads=2,
                        num_max_readers=2)
            assert j.result().tolist() == want[key], (expr, key)


def test_extern_search_with_force_regex(tmp_path):
    cli = ROOT / "tests" / "cpp" / "build" / "extern_search_cli"
    if not cli.exists():
        pytest.fail(f"{cli} not built (make -C tests/cpp)")
    data = np.concatenate([corpus.text_block(31, i, 300_000, needle_rate=2e-3) for i in range(2)])
    p = tmp_path / "x.txt"
    data.tofile(p)
    expr = b"(?m)^Sherlock"
    want = anchor_oracle.all_modes([data], expr)
    env = dict(os.environ, XS_CHUNK_BYTES=str(1 << 30), XS_FORCE_REGEX="1")
    r = subprocess.run([str(cli), "count", "join", expr.decode(), str(p), "-", "2"], capture_output=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert int(r.stdout.split(b"\n")[0]) == want["count_matches"]
    r = subprocess.run([str(cli), "match_byte_offsets", "join", expr.decode(), str(p), "-", "2"], capture_output=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert [int(x) for x in r.stdout.split(b"\n")[:-1]] == want["match_byte_offsets"]
    # both set: XS_FORCE_LITERAL wins (the bytes "(?m)^Sherlock" do not occur)
    env["XS_FORCE_LITERAL"] = "1"
    r = subprocess.run([str(cli), "count", "join", expr.decode(), str(p), "-", "2"], capture_output=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and int(r.stdout.split(b"\n")[0]) == 0


def test_xsgrep_against_gnu_grep(tmp_path):
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    if not shutil.which("grep"):
        pytest.fail("no GNU grep on this host")
    data = np.concatenate([corpus.text_block(404, i, 1_500_000, needle_rate=3e-4) for i in range(2)])
    text = (b"Sherlock\nSherlock Holmes\nHolmes.\nShe\nShelter\nSher.lock\n1887\n12a\n" * 50)
    data = np.concatenate([data, _u8(text)])
    p = tmp_path / "g.txt"
    data.tofile(p)
    env = dict(os.environ, XS_CHUNK_BYTES=str(1 << 30), LC_ALL="C")
    cases = [(["-x", "-E", "Sherlock( Holmes)?"], ["-x", "-E", "Sherlock( Holmes)?"]),
             (["-x", "-F", "Sher.lock"], ["-x", "-F", "Sher.lock"]),
             (["-x", "-E", "[0-9]{4}"], ["-x", "-E", "[0-9]{4}"]),
             (["-c", "-x", "-E", "[A-Z][a-z]+"], ["-c", "-x", "-E", "[A-Z][a-z]+"]),
             (["-i", "-x", "-F", "holmes."], ["-i", "-x", "-F", "holmes."]),
             (["-E", "(?m)^She"], ["-E", "^She"]),
             (["-c", "-E", "(?m)Holmes[.,]$"], ["-c", "-E", "Holmes[.,]$"])]
    for ours, theirs in cases:
        want = subprocess.run(["grep", *theirs, str(p)], capture_output=True, env=env).stdout
        got = subprocess.run([str(exe), "-j", "2", *ours, str(p)], capture_output=True, env=env, timeout=120)
        assert got.returncode == 0, (ours, got.stderr.decode())
        assert got.stdout == want, ours
        with open(p, "rb") as f:  # and from stdin
            got = subprocess.run([str(exe), *ours, "-"], stdin=f, capture_output=True, env=env, timeout=120)
        assert got.returncode == 0 and got.stdout == want, ("stdin", ours)
    r = subprocess.run([str(exe), "^She", str(p)], capture_output=True, env=env, timeout=120)
    assert r.returncode != 0 and b"not supported" in r.stderr
