"""xsgrep -F [-i] --count-each: the keyword table of a FILE and of stdin against tests/literal_counts_model.py, and the
option combinations it refuses (those need no GPU: the arguments are checked before a device is touched)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import corpus
import literal_counts_model as LM
import set_cases as SC

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
LITS = (b"Sherlock", b"She", b"lock", b"e", b"Holmes", b"the ", b"She", b"detective street", b"\tTab", b"zzzq")


def run(args, stdin=None, chunk_bytes=None):
    env = dict(os.environ)
    if chunk_bytes:
        env["XSGREP_CHUNK_BYTES"] = str(chunk_bytes)
    return subprocess.run([str(XSGREP)] + [os.fsencode(a) if isinstance(a, str) else a for a in args], input=stdin,
                          capture_output=True, timeout=300, env=env)


def table(out: bytes):
    rows = [l.split(b"\t", 1) for l in out.split(b"\n") if l]
    return [int(c) for c, _ in rows], [l for _, l in rows]


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    """3 MiB of text; with XSGREP_CHUNK_BYTES = 300 000 it is read in about ten newline-aligned chunks"""
    t = corpus.text_block(21, 0, 3 << 20, needle_rate=4e-4).tobytes()
    t = t[:1000] + b"\tTab\tTab SHERLOCK hOLMES\n" + t[1000:]
    assert b"\n" in t[-300_000:] and not t.endswith(b"\n\n")
    p = tmp_path_factory.mktemp("count_each") / "text.txt"
    p.write_bytes(t)
    return p, t


@pytest.mark.gpu
@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
def test_file_in_several_chunks_with_e_and_f(text, tmp_path, icase):
    path, t = text
    pf = tmp_path / "patterns.txt"
    pf.write_bytes(b"\n".join(LITS[3:7]) + b"\n")
    args = ["-F"] + (["-i"] if icase else []) + ["--count-each"]
    for l in LITS[:3]:
        args += ["-e", l]
    args += ["-f", str(pf)]
    for l in LITS[7:]:
        args += ["-e", l]
    order = LITS[:3] + LITS[3:7] + LITS[7:]
    want = LM.counts([np.frombuffer(t, dtype=np.uint8)], order, icase)
    assert want[0] > 100 and want[-1] == 0 and want[1] == want[6] and want[8] == 2
    r = run(args + [str(path)], chunk_bytes=300_000)
    assert r.returncode == 0, r.stderr.decode()
    assert table(r.stdout) == (want, list(order))
    one = run(args + [str(path)])  # one chunk of 16 MiB holds it all: the same table
    assert one.returncode == 0 and one.stdout == r.stdout


@pytest.mark.gpu
def test_stdin_and_a_single_pattern(text):
    path, t = text
    arr = [np.frombuffer(t, dtype=np.uint8)]
    r = run(["-F", "--count-each", "-e", "lock", "-e", "She", "-"], stdin=t, chunk_bytes=250_000)
    assert r.returncode == 0, r.stderr.decode()
    assert table(r.stdout) == (LM.counts(arr, (b"lock", b"She")), [b"lock", b"She"])
    for args in (["-F", "--count-each", "Sherlock", str(path)], ["-F", "--count-each", "-e", "Sherlock", str(path)]):  # a list of one
        r = run(args)
        assert r.returncode == 0, r.stderr.decode()
        assert table(r.stdout) == (LM.counts(arr, (b"Sherlock",)), [b"Sherlock"])
    r = run(["-Fi", "--count-each", "-e", "aa", "-"], stdin=b"aAaa\naa")  # overlapping occurrences, an open last line
    assert r.returncode == 0 and r.stdout == b"4\taa\n"
    r = run(["-F", "--count-each", "-e", "x", "-"], stdin=b"")
    assert r.returncode == 0 and r.stdout == b"0\tx\n"


@pytest.mark.parametrize("extra", [["-c"], ["-o"], ["-v"], ["-x"], ["-A", "1"], ["-B", "2"], ["-C", "0"], ["-m", "some.meta"], ["-E"]],
                         ids=lambda e: e[0])
def test_excluded_options_exit_2(tmp_path, extra):
    f = tmp_path / "t.txt"
    f.write_bytes(b"a line\n")
    r = run(["-F", "--count-each"] + extra + ["-e", "a", "-e", "b", str(f)])
    assert r.returncode == 2 and b"--count-each excludes" in r.stderr and extra[0].encode() in r.stderr, r.stderr
    assert r.stdout == b""


def test_count_each_needs_F_and_patterns_without_newlines(tmp_path):
    f = tmp_path / "t.txt"
    f.write_bytes(b"a line\n")
    r = run(["--count-each", "-e", "a", "-e", "b", str(f)])
    assert r.returncode == 2 and b"needs -F" in r.stderr
    r = run(["-F", "--count-each", "-e", "a", "-e", "", str(f)])
    assert r.returncode == 2 and b"empty pattern" in r.stderr
    r = run(["-F", "--count-each", "-e", "a", str(tmp_path / "missing.txt")])
    assert r.returncode == 2 and b"cannot read" in r.stderr
    h = run(["--help"])
    assert h.returncode == 0 and b"--count-each" in h.stdout
