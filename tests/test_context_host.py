"""XSG_FLAG_CONTEXT without a GPU: the model of tests/context_model.py against an independent brute force over line lists
and against GNU grep -A/-B/-C, the flag macros, the refusals a job decides before it needs a device, and the seam
stitcher of the file pipeline (x-search_amd/csrc/xsg_context.h) under the CPU sanitizers, as a program of its own."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import context_model
import corpus
import invert_model
import xsg
from gpu_util import oracle_all_modes

ROOT = Path(__file__).resolve().parent.parent
PAIRS = [(0, 0), (1, 0), (0, 1), (2, 3), (5, 1), (4095, 4095)]


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8)


def _brute(data: bytes, hit, before, after, g=0, lb=0):
    """(offsets, indices, terminated lines) of the lines within `before` behind / `after` ahead of a line for which
    hit(line) holds: every line against every hit line, by bytes.split"""
    parts = data.split(b"\n")
    terminated = data.endswith(b"\n")
    if terminated or not data:
        parts = parts[:-1]
    hits = [k for k, ln in enumerate(parts) if hit(ln)]
    offs, idx, out, at = [], [], [], 0
    for k, ln in enumerate(parts):
        if any(r - before <= k <= r + after for r in hits):
            offs.append(g + at)
            idx.append(lb + k)
            if terminated or k + 1 < len(parts):
                out.append(ln)
        at += len(ln) + 1
    return offs, idx, out, hits, len(parts)


def test_known_answers():
    assert context_model.chunk_context(10, [5], 1, 2) == [4, 5, 6, 7]
    assert context_model.chunk_context(10, [0, 9], 3, 3) == [0, 1, 2, 3, 6, 7, 8, 9]
    assert context_model.chunk_context(10, [2, 4], 1, 1) == [1, 2, 3, 4, 5]      # the spans touch
    assert context_model.chunk_context(10, [2, 5], 1, 1) == [1, 2, 3, 4, 5, 6]   # merge: A + B + 1 apart
    assert context_model.chunk_context(10, [2, 6], 1, 1) == [1, 2, 3, 5, 6, 7]   # a gap
    assert context_model.chunk_context(3, [1], 4095, 4095) == [0, 1, 2]
    assert context_model.chunk_context(3, [], 2, 2) == []
    assert context_model.chunk_context(4, [0, 1, 2, 3], 2, 2) == [0, 1, 2, 3]


def test_the_model_against_a_brute_force(oracle):
    """exact mode: a line is in R iff it contains the needle; also around the NON-matching lines (XSG_FLAG_INVERT)"""
    n = 0
    for seed in range(4):
        for term in (True, False):
            b = corpus.text_block(1500 + seed, 0, 4000 + 13 * seed, needle_rate=2e-2)
            if not term:
                b = b[:-1]
            for pat in (b"Sherlock", b"that", b"e", b"q"):
                plain = oracle_all_modes(oracle, [b], pat, exact=True, global_offsets=[777], line_bases=[31])
                inv = invert_model.invert_all_modes(plain, [b], [777], [31])
                for before, after in PAIRS:
                    for src, hit in ((plain, lambda ln: pat in ln), (inv, lambda ln: pat not in ln)):
                        got = context_model.context_all_modes(src, [b], before, after, [777], [31])
                        offs, idx, ls, hits, nlines = _brute(b.tobytes(), hit, before, after, 777, 31)
                        assert (got["line_byte_offsets"], got["line_indices"], got["lines"]) == (offs, idx, ls), (seed, term, pat, before, after)
                        assert got["lines_offsets"] == offs[:len(ls)]
                        (e,) = context_model.edges(src, [b], before, after, [777])
                        if hits:
                            want = (nlines, idx[0] - 31, idx[-1] - 31, max(0, before - hits[0]), max(0, after - (nlines - 1 - hits[-1])))
                        else:
                            want = (nlines, context_model.NONE, context_model.NONE, 0, 0)
                        assert e == want, (seed, term, pat, before, after)
                        n += 1
                assert context_model.context_all_modes(plain, [b], 0, 0, [777], [31])["lines"] == plain["lines"]
    for seed in range(30):  # many short lines, several chunks, the empty and the one-byte chunk among them
        blocks = [corpus.small_alphabet(seed * 7 + i, k) for i, k in enumerate((0, 1, 2, 40 + seed, 129 + seed))]
        for pat in (b"a", b"ab", b"aa"):
            plain = oracle_all_modes(oracle, blocks, pat, exact=True)
            for before, after in PAIRS:
                got = context_model.context_all_modes(plain, blocks, before, after)
                offs, idx, ls, g, lb = [], [], [], 0, 0
                for b in blocks:
                    o, i, l, _, _ = _brute(b.tobytes(), lambda ln: pat in ln, before, after, g, lb)
                    offs, idx, ls = offs + o, idx + i, ls + l
                    g, lb = g + b.size, lb + int((b == 10).sum())
                assert (got["line_byte_offsets"], got["line_indices"], got["lines"]) == (offs, idx, ls), (seed, pat, before, after)
                n += 1
    assert n > 500


def test_whole_file_form_and_the_refusal_rule(oracle):
    """chunks that are pieces of one text: whole_file is the context of their concatenation; job_refuses restates the
    one-neighbour rule"""
    text = b"".join(b"row %d %s\n" % (i, b"that" if i in (0, 7, 8, 30, 59) else b"-") for i in range(60))
    rows = text.split(b"\n")[:-1]
    cuts = [0, 5, 6, 7, 20, 45, 60]
    chunks = [_u8(b"".join(r + b"\n" for r in rows[a:b])) for a, b in zip(cuts, cuts[1:])]
    plain = oracle_all_modes(oracle, chunks, b"that", exact=True)
    for before, after in PAIRS:
        got = context_model.whole_file(plain, chunks, before, after)
        offs, idx, ls, _, _ = _brute(text, lambda ln: b"that" in ln, before, after)
        assert (got["line_byte_offsets"], got["line_indices"], got["lines"]) == (offs, idx, ls)
    assert not context_model.job_refuses(plain, chunks, 1, 1)
    assert context_model.job_refuses(plain, chunks, 2, 0)      # row 7's two lines before it cross the one-line chunk [6, 7)
    assert not context_model.job_refuses(plain, chunks, 0, 5)  # row 0's fifth line after it is the one-line chunk [5, 6) itself
    assert context_model.job_refuses(plain, chunks, 0, 6)      # ... its sixth lies behind that chunk


def test_the_model_against_gnu_grep(oracle, tmp_path):
    """grep -A/-B/-C --no-group-separator on terminated files, literals in exact mode (grep has no end-of-chunk quirk)"""
    if not shutil.which("grep"):
        pytest.skip("no GNU grep on this host")
    env = {"LC_ALL": "C", "PATH": "/usr/bin:/bin"}
    for seed in range(3):
        b = corpus.text_block(1600 + seed, 0, 20_000 + 7 * seed, needle_rate=1e-2)
        p = tmp_path / f"g{seed}.txt"
        b.tofile(p)
        for pat in (b"Sherlock", b"that", b"e"):
            plain = oracle_all_modes(oracle, [b], pat, exact=True)
            for args, (before, after) in ((["-A", "2"], (0, 2)), (["-B", "3"], (3, 0)), (["-C", "1"], (1, 1)), (["-B", "2", "-A", "5"], (2, 5))):
                want = context_model.context_all_modes(plain, [b], before, after)
                out = subprocess.run(["grep", "-F", "--no-group-separator", *args, pat.decode(), str(p)], capture_output=True, env=env)
                assert out.returncode == 0, out.stderr
                assert out.stdout.split(b"\n")[:-1] == want["lines"], (seed, pat, args)
            inv = invert_model.invert_all_modes(plain, [b])
            out = subprocess.run(["grep", "-F", "-v", "--no-group-separator", "-C", "2", pat.decode(), str(p)], capture_output=True, env=env)
            assert out.stdout.split(b"\n")[:-1] == context_model.context_all_modes(inv, [b], 2, 2)["lines"], (seed, pat, "-v -C 2")


def test_the_flag_macros_round_trip(tmp_path):
    text = (ROOT / "include" / "xsg.h").read_text()
    assert re.search(r"^#define XSG_CONTEXT_MAX 4095u$", text, re.M)
    assert re.search(r"^#define XSG_ABI_VERSION 4$", text, re.M)
    assert "xsg_result_context_edges" in xsg.EXPORTS
    assert xsg.flag_context(0, 0) == 0
    assert xsg.flag_context(1, 0) == 0x100 and xsg.flag_context(0, 1) == 0x100000
    assert xsg.flag_context(4095, 4095) == 0xffffff00
    for before, after in ((0, 1), (7, 0), (2, 3), (4095, 1), (4095, 4095)):
        f = xsg.flag_context(before, after) | xsg.FLAG_INVERT | xsg.FLAG_EXACT_TAIL
        assert (xsg.context_before(f), xsg.context_after(f)) == (before, after)
        assert f & 0xff == xsg.FLAG_INVERT | xsg.FLAG_EXACT_TAIL
    for bad in ((4096, 0), (0, 4096), (-1, 0), (0, 1 << 20)):
        with pytest.raises(ValueError):
            xsg.flag_context(*bad)
    assert xsg.CONTEXT_EDGE_DTYPE.itemsize == 32
    # the macros of the header, compiled: the same numbers
    src = tmp_path / "macros.c"
    src.write_text('#include <xsg.h>\n#include <stdio.h>\nint main(void) { unsigned f = XSG_FLAG_CONTEXT(2, 3) | XSG_FLAG_INVERT;'
                   ' printf("%u %u %u %u %u %u", XSG_FLAG_CONTEXT(4095, 4095), XSG_FLAG_CONTEXT(0, 0), XSG_CONTEXT_BEFORE(f), XSG_CONTEXT_AFTER(f),'
                   ' XSG_FLAG_CONTEXT(4096, 1), (unsigned)sizeof(xsg_context_edge)); return 0; }\n')
    r = subprocess.run(["gcc", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "macros")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    out = subprocess.run([str(tmp_path / "macros")], capture_output=True).stdout.split()
    assert [int(x) for x in out] == [0xffffff00, 0, 2, 3, xsg.flag_context(0, 1), 32]  # (the macro masks: 4096 -> 0)


def test_the_inspection_calls_ignore_the_bits():
    f = xsg.flag_context(3, 4)
    assert xsg.regex_check(b"She[r ]lock", f)[0] == xsg.regex_check(b"She[r ]lock", 0)[0] == 8
    assert xsg.regex_info(b"colou?r", f)[:3] == xsg.regex_info(b"colou?r", 0)[:3]
    assert xsg.regex_dfa(b"colou?r", f)[0].ncls == xsg.regex_dfa(b"colou?r", 0)[0].ncls
    assert xsg.regex_prefix(b"colou?r", f)[0] == xsg.regex_prefix(b"colou?r", 0)[0]
    assert xsg.regex_factor(b"\\w+ing", f)[0] == xsg.regex_factor(b"\\w+ing", 0)[0]


def test_job_refuses_a_newline_pattern_before_it_needs_a_device(tmp_path):
    """context + a pattern that can match '\\n' is a property of the request: XSG_ENOTSUP on any host"""
    p = tmp_path / "t.txt"
    p.write_bytes(b"one\ntwo\n")
    for mode in (xsg.LINES, xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.COUNT_LINES, xsg.MATCH_BYTE_OFFSETS):
        for pat, flags in ((b"one\ntwo", 0), (b"one\\stwo", xsg.FLAG_REGEX), (b"o[^x]+o", xsg.FLAG_REGEX)):
            with pytest.raises(xsg.XsgError) as e:
                xsg.Job(pat, str(p), mode, flags=flags | xsg.flag_context(1, 0))
            assert e.value.code == xsg.ENOTSUP and "'\\n'" in str(e.value), (mode, pat)


def test_the_seam_stitcher_under_the_sanitizers(tmp_path):
    """tests/cpp/context_stitch.cpp: xsg_context.h alone over random texts, cuts, match sets and (B, A) against whole-range
    context, and the refusal cases -- a program of its own, built like tests/cpp's lz4_selftest"""
    exe = tmp_path / "context_stitch"
    src = ROOT / "tests" / "cpp" / "context_stitch.cpp"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(src), "-o", str(exe)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"context_stitch ok" in r.stdout, (r.stdout + r.stderr).decode()


def test_xsgrep_usage_and_argument_checks():
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    r = subprocess.run([str(exe), "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and all(x in r.stdout for x in (b"-A N", b"-B N", b"-C N"))
    for args in (["-A", "4096", "x", "f"], ["-C", "-1", "x", "f"], ["-B", "two", "x", "f"]):
        r = subprocess.run([str(exe), *args], capture_output=True, timeout=60)
        assert r.returncode == 2 and b"4095" in r.stderr, args
    r = subprocess.run([str(exe), "-C", "2", "x", "-"], capture_output=True, stdin=subprocess.DEVNULL, timeout=60)
    assert r.returncode == 2 and b"stdin" in r.stderr
