"""xsg_count_literals_csr without a GPU: tests/literal_csr_model.py on hand-written cases, the binding's declarations, and
the host side of k_set_count_literals_csr / k_set_csr_seam -- the whole / seam predicates of
x-search_amd/csrc/xsg_litmatrix.h and the five stages of a call replayed -- under the sanitizers as a stand-alone program."""
import subprocess
from pathlib import Path

import literal_csr_model as CM
import literal_matrix_model as MM
import set_cases as SC
import xsg

ROOT = Path(__file__).resolve().parents[1]


def test_model_on_small_cases():
    u8 = SC.u8
    blocks = [u8(b"xabab"), u8(b""), u8(b"ab"), u8(b"b")]
    lits = [b"ab", b"b", b"ab", b"zz"]
    # rows [2, 2, 2, 0], [0, 0, 0, 0], [1, 1, 1, 0], [0, 1, 0, 0]: duplicates get an entry each, the empty chunk an empty row
    assert CM.csr(blocks, lits) == ([0, 3, 3, 6, 7], [0, 1, 2, 0, 1, 2, 1], [2, 2, 2, 1, 1, 1, 1])
    assert CM.to_rows(*CM.csr(blocks, lits), 4) == MM.matrix(blocks, lits)
    assert CM.well_formed(*CM.csr(blocks, lits), 4)
    assert CM.csr([], [b"a", b"b"]) == ([0], [], [])  # no chunks
    assert CM.csr([u8(b"abc")], [b"a", b"b", b"c", b"bc"]) == ([0, 4], [0, 1, 2, 3], [1, 1, 1, 1])  # every literal present
    assert CM.csr([u8(b"aa"), u8(b"q")], [b"a", b"a", b"a"]) == ([0, 3, 3], [0, 1, 2], [2, 2, 2])  # duplicates: an entry each
    assert CM.csr([u8(b"xa"), u8(b"b")], [b"ab"]) == ([0, 0, 0], [], [])  # no occurrence straddles two chunks
    assert CM.csr([u8(b"Ab")], [b"ab"], icase=True) == ([0, 1], [0], [1])


def test_model_refuses_what_is_no_csr():
    assert not CM.well_formed([0, 2], [1, 0], [1, 1], 2)  # columns descend
    assert not CM.well_formed([0, 2], [0, 0], [1, 1], 2)  # a column twice
    assert not CM.well_formed([0, 1], [0], [0], 2)  # an entry of 0
    assert not CM.well_formed([0, 1], [2], [1], 2)  # a column beyond the list
    assert not CM.well_formed([0, 2, 1], [0, 1], [1, 1], 2)  # row_ptr descends
    assert not CM.well_formed([1, 1], [0], [1], 2)  # row_ptr does not begin at 0


def test_binding_declares_the_entry_points():
    assert {"xsg_count_literals_csr", "xsg_result_literals_csr", "xsg_count_literals_csr_async"} <= set(xsg.EXPORTS)
    assert hasattr(xsg.Shard, "count_literals_csr") and hasattr(xsg.Shard, "count_literals_csr_async")


def test_seams_and_the_five_stages_under_the_sanitizers(tmp_path):
    """tests/cpp/literal_csr_selftest.cpp includes csrc/xsg_litmatrix.h: a stand-alone program, nothing is loaded into
    Python.  Random tile -> chunk sequences with empty chunks and lists around the touched list's capacity, split over 1,
    2, 3, 7 and ntiles workgroups: the whole / seam predicate, then count, seam count, prefix, fill and seam fill replayed
    against the dense replay's non-zeros under full capacity, nnz - 1 and 0."""
    exe = tmp_path / "literal_csr_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(ROOT / "tests" / "cpp" / "literal_csr_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "literal_csr_selftest ok" in r.stdout
