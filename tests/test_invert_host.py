"""XSG_FLAG_INVERT without a GPU: the model of tests/invert_model.py against independent restatements (bytes.split / re,
GNU grep -v), the facts the complement rests on, and the surfaces that can be checked on any host."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import corpus
import invert_model
import xsg
from gpu_util import oracle_all_modes

ROOT = Path(__file__).resolve().parent.parent
TEXT_NEEDLES = [b"Sherlock", b"e", b"the", b"that", b" ", b"aa"]
SMALL_NEEDLES = [b"a", b"ab", b"aa", b"aba", b"b"]


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8)


def test_lines_of_a_chunk():
    assert invert_model.lines(b"a\nb") == [0, 2]
    assert invert_model.lines(b"a\n") == [0]
    assert invert_model.lines(b"a\n\n") == [0, 2]
    assert invert_model.lines(b"") == []
    assert invert_model.lines(b"\n") == [0]
    assert invert_model.lines(b"x") == [0]
    assert invert_model.lines(b"\n\n\nx") == [0, 1, 2, 3]


def _cases():
    for seed in range(6):
        yield [corpus.text_block(900 + seed, i, 3000 + 411 * i + seed, needle_rate=2e-2) for i in range(3)], TEXT_NEEDLES
    for seed in range(40):
        blocks = [corpus.small_alphabet(seed * 7 + i, n) for i, n in enumerate((0, 1, 2, 17 + seed, 64, 129 + seed))]
        yield blocks, SMALL_NEEDLES


def test_the_complement_is_well_defined(oracle):
    """every start the oracle reports is a line start, none twice, count(skip_to_nl) == len(byte_offsets_line) -- both
    tail modes; and the model's count is |lines| - count_lines"""
    n = both = 0
    for blocks, needles in _cases():
        for pat in needles:
            for exact in (False, True):
                plain = oracle_all_modes(oracle, blocks, pat, exact=exact)
                invert_model.properties(plain, blocks)
                inv = invert_model.invert_all_modes(plain, blocks)
                total = sum(len(invert_model.lines(b)) for b in blocks)
                assert inv["count_lines"] == total - plain["count_lines"] == len(inv["line_byte_offsets"])
                assert len(inv["line_indices"]) == inv["count_lines"] and len(inv["lines"]) == len(inv["lines_offsets"])
                n += 1
                both += bool(plain["count_lines"]) and bool(inv["count_lines"])
    assert 2 * both >= n, (both, n)


def test_the_model_honours_offsets_and_line_bases(oracle):
    blocks = [_u8(b"ab\ncd\nab"), _u8(b""), _u8(b"\nab\n\nzz\n")]
    go, lb = [1000, 5000, 70], [10, 99, 500]
    plain = oracle_all_modes(oracle, blocks, b"ab", exact=True, global_offsets=go, line_bases=lb)
    inv = invert_model.invert_all_modes(plain, blocks, go, lb)
    assert inv["line_byte_offsets"] == [1003, 70, 74, 75]
    assert inv["line_indices"] == [11, 500, 502, 503]
    assert inv["lines"] == [b"cd", b"", b"", b"zz"] and inv["lines_offsets"] == [1003, 70, 74, 75]
    assert inv["count_lines"] == 4
    auto = invert_model.invert_all_modes(oracle_all_modes(oracle, blocks, b"ab", exact=True), blocks)
    assert auto["line_byte_offsets"] == [3, 8, 12, 13] and auto["line_indices"] == [1, 2, 4, 5]


def _split_restatement(data: bytes, keep):
    """(offsets, indices, terminated lines) of the lines for which keep(line) holds, by bytes.split"""
    parts = data.split(b"\n")
    terminated = data.endswith(b"\n")
    if terminated or not data:
        parts = parts[:-1]
    offs, idx, out, at = [], [], [], 0
    for k, ln in enumerate(parts):
        if keep(ln):
            offs.append(at)
            idx.append(k)
            if terminated or k + 1 < len(parts):
                out.append(ln)
        at += len(ln) + 1
    return offs, idx, out


def test_the_model_against_split_and_re(oracle):
    """exact mode, ASCII: a line is in R iff it contains the needle (bytes `in`) or matches the expression (re)"""
    from gpu_util import oracle_regex_all_modes
    for seed in range(4):
        for term in (True, False):
            b = corpus.text_block(1200 + seed, 0, 5000 + seed, needle_rate=2e-2)
            if not term:
                b = b[:-1]
            data = b.tobytes()
            for pat in TEXT_NEEDLES:
                inv = invert_model.invert_all_modes(oracle_all_modes(oracle, [b], pat, exact=True), [b])
                offs, idx, ls = _split_restatement(data, lambda ln: pat not in ln)
                assert (inv["line_byte_offsets"], inv["line_indices"], inv["lines"]) == (offs, idx, ls), (seed, term, pat)
            for expr in (b"She[r ]lock", b"colou?r|lock(ed|s)?", b"\\w+ing"):
                plain, with_lines = oracle_regex_all_modes(oracle, [b], expr)
                assert with_lines
                inv = invert_model.invert_all_modes(plain, [b])
                rx = re.compile(expr)
                offs, idx, ls = _split_restatement(data, lambda ln: rx.search(ln) is None)
                assert (inv["line_byte_offsets"], inv["line_indices"], inv["lines"]) == (offs, idx, ls), (seed, term, expr)
    for seed in range(30):
        b = corpus.small_alphabet(seed, 200 + seed)
        for pat in SMALL_NEEDLES:
            inv = invert_model.invert_all_modes(oracle_all_modes(oracle, [b], pat, exact=True), [b])
            offs, idx, ls = _split_restatement(b.tobytes(), lambda ln: pat not in ln)
            assert (inv["line_byte_offsets"], inv["line_indices"], inv["lines"]) == (offs, idx, ls), (seed, pat)


def test_the_model_against_gnu_grep(oracle, tmp_path):
    """grep -v -c / grep -v -n on terminated files, exact mode (grep has no end-of-chunk quirk)"""
    if not shutil.which("grep"):
        pytest.skip("no GNU grep on this host")
    env = {"LC_ALL": "C", "PATH": "/usr/bin:/bin"}
    for seed in range(3):
        b = corpus.text_block(1300 + seed, 0, 20_000 + 7 * seed, needle_rate=1e-2)
        p = tmp_path / f"g{seed}.txt"
        b.tofile(p)
        for pat in (b"Sherlock", b"the", b"e", b"that"):
            inv = invert_model.invert_all_modes(oracle_all_modes(oracle, [b], pat, exact=True), [b])
            c = subprocess.run(["grep", "-F", "-v", "-c", pat.decode(), str(p)], capture_output=True, env=env).stdout
            assert int(c) == inv["count_lines"], (seed, pat)
            out = subprocess.run(["grep", "-F", "-v", "-n", pat.decode(), str(p)], capture_output=True, env=env).stdout
            rows = [r.split(b":", 1) for r in out.split(b"\n")[:-1]]
            assert [int(r[0]) - 1 for r in rows] == inv["line_indices"], (seed, pat)
            assert [r[1] for r in rows] == inv["lines"], (seed, pat)


def test_the_flag_in_the_header_and_in_python():
    text = (ROOT / "include" / "xsg.h").read_text()
    assert re.search(r"^#define XSG_FLAG_INVERT 0x8u$", text, re.M)
    assert re.search(r"^#define XSG_ABI_VERSION 4$", text, re.M)
    assert xsg.FLAG_INVERT == 8


def test_job_refuses_the_match_tags_before_it_opens_anything(tmp_path):
    """flag + match tag is a property of the request: refused with ENOTSUP on any host, before the file or a device"""
    p = tmp_path / "t.txt"
    p.write_bytes(b"one\ntwo\n")
    for mode in (xsg.MATCH_BYTE_OFFSETS, xsg.COUNT_MATCHES):
        for path in (str(p), str(tmp_path / "missing.txt")):
            with pytest.raises(xsg.XsgError) as e:
                xsg.Job(b"one", path, mode, flags=xsg.FLAG_INVERT)
            assert e.value.code == xsg.ENOTSUP and "invert" in str(e.value).lower()
    with pytest.raises(xsg.XsgError) as e:  # a literal that can match '\n'
        xsg.Job(b"one\ntwo", str(p), xsg.COUNT_LINES, flags=xsg.FLAG_INVERT)
    assert e.value.code == xsg.ENOTSUP and "invert" in str(e.value).lower()


def test_xsgrep_usage_lists_invert():
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    r = subprocess.run([str(exe), "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"-v" in r.stdout and b"--invert-match" in r.stdout
