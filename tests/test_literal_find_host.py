"""xsg_find_literals without a GPU: tests/literal_find_model.py pinned to the count models and to bytes.find, the binding's
declarations, xsgrep's refusals for --find-each, and the host side of k_set_find_literals -- the index arithmetic of
x-search_amd/csrc/xsg_litfind.h with count pass, prefix sum and fill pass replayed -- under the sanitizers as a stand-alone
program."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import literal_counts_model as LM
import literal_find_model as FM
import literal_matrix_model as MM
import set_cases as SC
import words_model as WM
import xsg

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"


def test_model_on_small_cases():
    u8 = SC.u8
    assert FM.find([u8(b"aaaa")], [b"aa"]) == ([0, 3], [0, 1, 2], [0, 0, 0])  # overlapping occurrences
    assert FM.find([u8(b"abc")], [b"ab", b"abc"]) == ([0, 2], [0, 0], [0, 1])  # a covered one: two entries at one position
    assert FM.find([u8(b"xab")], [b"ab", b"b", b"ab"]) == ([0, 3], [1, 1, 2], [0, 2, 1])  # a duplicate: adjacent, ascending j
    assert FM.find([u8(b"xa"), u8(b"b")], [b"ab"]) == ([0, 0, 0], [], [])  # no occurrence straddles two chunks
    assert FM.find([], [b"a", b"b"]) == ([0], [], [])
    assert FM.find([u8(b"ab"), u8(b""), u8(b"ab")], [b"b"]) == ([0, 1, 1, 2], [1, 3], [0, 0])  # the running global offset
    assert FM.find([u8(b"ab"), u8(b"ab")], [b"b"], global_offsets=[100, 50]) == ([0, 1, 2], [101, 51], [0, 0])
    assert FM.find([u8(b"AbaB")], [b"aB"], icase=True) == ([0, 2], [0, 2], [0, 0])
    assert FM.find([u8(b"art party art")], [b"art"], words=True) == ([0, 2], [0, 10], [0, 0])
    assert FM.find([u8(b"xart"), u8(b"art")], [b"art"], words=True) == ([0, 0, 1], [4], [0])  # a chunk's edges are boundaries
    assert FM.well_formed([0, 2], [0, 0], [0, 1], 2) and not FM.well_formed([0, 2], [0, 0], [1, 0], 2)
    assert not FM.well_formed([0, 2], [0, 0], [1, 1], 2) and not FM.well_formed([0, 2], [3, 1], [0, 0], 2)
    assert not FM.well_formed([0, 1], [0], [2], 2) and not FM.well_formed([1, 1], [0], [0], 1)


def random_case(rng):
    alphabet = (b"ab", b"abAB _", b"etaoinETA ,\n")[int(rng.integers(0, 3))]
    pick = lambda n: bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n))
    lits = [pick(int(rng.integers(1, 5))).replace(b"\n", b"e") for _ in range(int(rng.integers(1, 7)))]
    if len(lits) > 2:
        lits[1] = lits[-1]  # a duplicate
    blocks = [SC.u8(pick(int(rng.integers(0, 120)))) for _ in range(int(rng.integers(0, 5)))]
    return blocks, lits


def test_model_agrees_with_the_count_models_and_bytes_find():
    rng = np.random.Generator(np.random.PCG64(1620))
    total = 0
    for _ in range(300):
        blocks, lits = random_case(rng)
        k = len(lits)
        lengths = [b.size for b in blocks]
        starts = [sum(lengths[:c]) for c in range(len(blocks))]
        for icase in (False, True):
            cp, pos, lit = FM.find(blocks, lits, icase)
            assert FM.well_formed(cp, pos, lit, k, starts, lengths)
            assert FM.bincount(lit, k) == LM.counts(blocks, lits, icase)
            assert FM.rows(cp, lit, k) == MM.matrix(blocks, lits, icase)
            total += len(pos)
            cpw, posw, litw = FM.find(blocks, lits, icase, words=True)
            assert FM.well_formed(cpw, posw, litw, k, starts, lengths)
            assert FM.bincount(litw, k) == WM.counts(blocks, lits, icase)
            assert FM.rows(cpw, litw, k) == WM.matrix(blocks, lits, icase)
            assert set(zip(posw, litw)) <= set(zip(pos, lit))  # admissible occurrences are occurrences
        # a list of one literal without a border: the positions bytes.find steps through without overlap
        for l in {l for l in lits if LM.borderless(l)}:
            want, base = [], 0
            for b in blocks:
                t, at = b.tobytes(), 0
                while (at := t.find(l, at)) >= 0:
                    want.append(base + at)
                    at += len(l)
                base += len(t)
            assert FM.find(blocks, [l])[1] == want
    assert total > 5000


def test_binding_declares_the_entry_points():
    names = {"xsg_find_literals", "xsg_result_literal_hits", "xsg_find_literals_async", "xsg_literal_finder_create_opts",
             "xsg_literal_finder_find", "xsg_literal_finder_destroy"}
    assert names <= set(xsg.EXPORTS)
    assert hasattr(xsg.Shard, "find_literals") and hasattr(xsg.Shard, "find_literals_async") and hasattr(xsg, "LiteralFinder")
    header = (ROOT / "include" / "xsg.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert names <= set(re.findall(r"\b(xsg_[a-z0-9_]+)\s*\(", code))
    assert "sorted ascending by (c, p, j)" in header  # the contract


def test_the_finder_refuses_a_bad_list_before_a_device_is_touched():
    import ctypes as C
    lib = xsg.load()
    h = C.c_void_p()
    assert lib.xsg_literal_finder_create_opts(0, b"", 0, 0, 0, C.byref(h)) == xsg.EINVAL and not h.value  # an empty list
    assert lib.xsg_literal_finder_create_opts(0, b"a", 1, 0, 2, C.byref(h)) == xsg.EINVAL  # unknown list flags
    assert lib.xsg_literal_finder_create_opts(0, b"a", 1, xsg.FLAG_INVERT, 0, C.byref(h)) == xsg.ENOTSUP
    assert lib.xsg_literal_finder_create_opts(0, b"a", 1, 0, 0, None) == xsg.EINVAL
    lib.xsg_literal_finder_destroy(None)


def test_span_words_ranks_and_the_clip_under_the_sanitizers(tmp_path):
    """tests/cpp/literal_find_selftest.cpp includes csrc/xsg_set.h (through xsg_set.cpp) and csrc/xsg_litfind.h: a stand-alone
    program, nothing is loaded into Python.  Random chunk tables (empty chunks, chunks around the load, span and tile
    edges) and lists with g = 1..4, both fold modes, with and without whole words; tiles taken in the order of grids of 1, 3
    and ntiles workgroups and shuffled; count pass, prefix sum, chunk_ptr and fill pass against a brute-force list under
    full capacity, total - 1 and 0, with guard words behind every array."""
    exe = tmp_path / "literal_find_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "literal_find_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "literal_find_selftest ok" in r.stdout


def run_xsgrep(args):
    return subprocess.run([str(XSGREP)] + args, capture_output=True, timeout=120)


@pytest.mark.parametrize("extra", [["--count-each"], ["-c"], ["-o"], ["-v"], ["-x"], ["-A", "1"], ["-B", "2"], ["-C", "0"], ["-m", "some.meta"], ["-E"]],
                         ids=lambda e: e[0])
def test_xsgrep_find_each_excluded_options_exit_2(tmp_path, extra):
    f = tmp_path / "t.txt"
    f.write_bytes(b"a line\n")
    r = run_xsgrep(["-F", "--find-each"] + extra + ["-e", "a", "-e", "b", str(f)])
    assert r.returncode == 2 and b"--find-each excludes" in r.stderr and extra[0].encode() in r.stderr, r.stderr
    assert r.stdout == b""


def test_xsgrep_find_each_needs_F_and_patterns_without_newlines(tmp_path):
    f = tmp_path / "t.txt"
    f.write_bytes(b"a line\n")
    r = run_xsgrep(["--find-each", "-e", "a", "-e", "b", str(f)])
    assert r.returncode == 2 and b"--find-each needs -F" in r.stderr
    r = run_xsgrep(["-F", "--find-each", "-e", "a", "-e", "", str(f)])
    assert r.returncode == 2 and b"empty pattern" in r.stderr
    r = run_xsgrep(["-F", "--find-each", "-e", "a", str(tmp_path / "missing.txt")])
    assert r.returncode == 2 and b"cannot read" in r.stderr
    r = run_xsgrep(["-F", "-w", "-x", "--find-each", "-e", "a", str(f)])
    assert r.returncode == 2 and b"-w" in r.stderr
    h = run_xsgrep(["--help"])
    assert h.returncode == 0 and b"--find-each" in h.stdout and b"OFFSET:LITERAL" in h.stdout
