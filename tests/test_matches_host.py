"""XSG_MATCHES without a GPU: the model (tests/match_model.py) on hand-written vectors, the tag's value in the header
and in xsg.py, the job layer's mode check, the C++ call sites and xsgrep's option handling."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import match_model
import xsg

ROOT = Path(__file__).resolve().parent.parent
R, I, X = xsg.FLAG_REGEX, xsg.FLAG_IGNORE_CASE, xsg.FLAG_EXACT_TAIL


def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


VECTORS = [
    # (pattern, flags, chunk, strings, chunk-relative starts)
    (b"Sher|Sherlock", R, b"Sherlock\n", [b"Sher"], [0]),            # leftmost-first, not longest
    (b"Sherlock|Sher", R, b"Sherlock\n", [b"Sherlock"], [0]),
    (b"a+", R, b"aaa\n", [b"aaa"], [0]),                               # greedy
    (b"a+?", R, b"aaa\n", [b"a", b"a", b"a"], [0, 1, 2]),              # lazy
    (b"(?m)^ab", R, b"abab", [b"ab", b"ab"], [0, 2]),                  # `^` holds at the walk's resume point
    (b"(?m)b$", R, b"ab\n", [b"b"], [1]),                              # the '\n' is not part of the match
    (b"(?m)^(?:a|bc)+$", R, b"abca\nbcx\nbc", [b"abca", b"bc"], [0, 9]),
    (b"sherlock", I | X, b"SHERlock sherLOCK\n", [b"SHERlock", b"sherLOCK"], [0, 9]),  # the text keeps its case
    (b"colou?r", R | I, b"COLOR Colour\n", [b"COLOR", b"Colour"], [0, 6]),
    (b"She[r ]lock", R, b"Sherlock She lock\n", [b"Sherlock", b"She lock"], [0, 9]),  # a class sequence: its positions
    (b"ab", X, b"abab\n", [b"ab", b"ab"], [0, 2]),                     # two matches that touch
    (b"abab", X, b"abababab\n", [b"abab", b"abab"], [0, 4]),           # bordered: the greedy walk
    (b"a\nb", X, b"a\nb a\nb\n", [b"a\nb", b"a\nb"], [0, 4]),          # a literal that contains '\n'
    (b"\\s+", R, b"a \n b\n", [b" \n ", b"\n"], [1, 5]),               # an expression that matches across lines
]


@pytest.mark.parametrize("pat,flags,chunk,strings,starts", VECTORS, ids=[v[0].decode().replace("\n", "\\n") + f"/{v[1]}" for v in VECTORS])
def test_model_on_hand_written_vectors(oracle, pat, flags, chunk, strings, starts):
    got = match_model.matches(oracle, [_u8(chunk)], pat, flags, global_offsets=[1000])
    assert got[0] == strings
    assert got[1] == [1000 + s for s in starts]
    assert got[2] == [len(s) for s in strings]


def test_model_concatenates_chunks_with_their_global_offsets(oracle):
    blocks = [_u8(b"colour color\n"), _u8(b""), _u8(b"x color")]
    s, o, n = match_model.matches(oracle, blocks, b"colou?r", R, global_offsets=[100, 500, 7])
    assert (s, o, n) == ([b"colour", b"color", b"color"], [100, 107, 9], [6, 5, 5])
    s, o, _ = match_model.matches(oracle, blocks, b"colou?r", R)
    assert o == [0, 7, 15]


def test_the_lossy_tail_is_the_oracle_s(oracle):
    """the default end-of-chunk behaviour belongs to M: a model that reported more than the oracle would be wrong"""
    blk = _u8(b"x" * 100 + b" SheSherlock")
    lossy = match_model.matches(oracle, [blk], b"Sherlock", 0)
    exact = match_model.matches(oracle, [blk], b"Sherlock", X)
    assert exact[0] == [b"Sherlock"] and exact[1] == [104]
    assert lossy[1] == [int(v) for v in oracle.byte_offsets_match(blk, b"Sherlock")]


def test_the_gpu_cases_text_ends_in_the_lossy_zone(oracle):
    """the text of tests/test_gpu_matches.py loses exactly its last occurrence to the default end-of-chunk behaviour,
    whole and as the last chunk of every cut"""
    import test_gpu_matches as g
    text = g.make_text()
    for blocks, go in g.cuts(text):
        lossy = match_model.matches(oracle, blocks, b"Sherlock", 0, go)
        exact = match_model.matches(oracle, blocks, b"Sherlock", X, go)
        assert len(exact[0]) > len(lossy[0]) and exact[1][-1] not in lossy[1]
        assert exact[1][-1] - go[-1] == blocks[-1].size - 8
    assert len(match_model.matches(oracle, [text], b"Sherlock", X)[0]) == len(match_model.matches(oracle, [text], b"Sherlock", 0)[0]) + 1


def test_the_tag_is_six():
    header = (ROOT / "include" / "xsg.h").read_text()
    m = re.search(r"\bXSG_MATCHES\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 6
    assert xsg.MATCHES == 6
    assert re.search(r"#define\s+XSG_ABI_VERSION\s+4\b", header)
    assert "xsg_host_matches" in xsg.EXPORTS and "xsg_host_matches(" in header


def test_the_job_layer_accepts_the_mode(tmp_path):
    """the mode check comes before the file is opened: XSG_EINVAL there, XSG_EIO here"""
    missing = str(tmp_path / "no such file")
    with pytest.raises(xsg.XsgError) as e:
        xsg.Job(b"x", missing, xsg.MATCHES)
    assert e.value.code == xsg.EIO, str(e.value)
    with pytest.raises(xsg.XsgError) as e:  # one past the last tag stays a bad mode
        xsg.Job(b"x", missing, xsg.MATCHES + 1)
    assert e.value.code == xsg.EINVAL
    with pytest.raises(xsg.XsgError) as e:  # an inverted search has no match tags
        xsg.Job(b"x", missing, xsg.MATCHES, flags=xsg.FLAG_INVERT)
    assert e.value.code == xsg.ENOTSUP and "invert" in str(e.value).lower()


def test_cpp_call_sites_compile():
    src = ROOT / "tests" / "cpp" / "matches_callsites.cpp"
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_xsgrep_names_the_option_and_refuses_it_with_invert(tmp_path):
    exe = ROOT / "tools" / "build" / "xsgrep"
    if not exe.exists():
        pytest.fail(f"{exe} not built (make -C tools)")
    r = subprocess.run([str(exe), "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"-o" in r.stdout and b"--only-matching" in r.stdout
    f = tmp_path / "t.txt"
    f.write_bytes(b"x\n")
    for args in (["-o", "-v"], ["-ov"], ["--only-matching", "--invert-match"]):
        r = subprocess.run([str(exe), *args, "x", str(f)], capture_output=True, timeout=60)  # refused before any device is touched
        assert r.returncode == 2 and b"-o" in r.stderr and r.stdout == b"", (args, r.stderr)
