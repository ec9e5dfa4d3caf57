"""xsg_count_literals_chunks without a GPU: tests/literal_matrix_model.py pinned to tests/literal_counts_model.py, and the
host side of k_set_count_literals_chunks -- the tile partition and the flush rule of x-search_amd/csrc/xsg_litmatrix.h --
under the sanitizers as a stand-alone program."""
import subprocess
from pathlib import Path

import literal_counts_model as LM
import literal_matrix_model as MM
import set_cases as SC
import xsg

ROOT = Path(__file__).resolve().parents[1]


def test_model_rows_sum_to_the_counts_of_the_binding():
    blocks = SC.text_blocks()
    lits = SC.word_list(9)
    rows = MM.matrix(blocks, lits)
    assert len(rows) == len(blocks) and all(len(r) == len(lits) for r in rows)
    for c, b in enumerate(blocks):
        assert rows[c] == LM.counts([b], lits)
    total = LM.counts(blocks, lits)
    assert [sum(r[j] for r in rows) for j in range(len(lits))] == total and sum(total) > 0
    folded = MM.matrix(blocks, lits, icase=True)
    assert [sum(r[j] for r in folded) for j in range(len(lits))] == LM.counts(blocks, lits, icase=True)
    assert folded != rows
    with_ = MM.chunks_with(rows, len(lits))
    assert all(0 <= w <= len(blocks) for w in with_) and max(with_) == len(blocks)
    assert [w > 0 for w in with_] == [t > 0 for t in total]


def test_model_on_small_cases():
    u8 = SC.u8
    blocks = [u8(b"xabab"), u8(b""), u8(b"ab"), u8(b"b")]
    rows = MM.matrix(blocks, [b"ab", b"b", b"ab", b"zz"])
    assert rows == [[2, 2, 2, 0], [0, 0, 0, 0], [1, 1, 1, 0], [0, 1, 0, 0]]
    assert MM.chunks_with(rows, 4) == [2, 3, 2, 0]  # duplicates get the same number each
    assert MM.matrix([u8(b"xa"), u8(b"b")], [b"ab"]) == [[0], [0]]  # no occurrence straddles two chunks
    assert MM.matrix([], [b"a", b"b"]) == [] and MM.chunks_with([], 2) == [0, 0]


def test_binding_declares_the_entry_points():
    assert {"xsg_count_literals_chunks", "xsg_count_literals_chunks_async", "xsg_literals_chunks_touched_capacity"} <= set(xsg.EXPORTS)
    assert hasattr(xsg.Shard, "count_literals_chunks") and hasattr(xsg.Shard, "count_literals_chunks_async")


def test_partition_and_flush_rule_under_the_sanitizers(tmp_path):
    """tests/cpp/literal_matrix_selftest.cpp includes csrc/xsg_litmatrix.h: a stand-alone program, nothing is loaded into
    Python.  Tile counts 0 .. 3 * 2^18 + 1 under grids 1 .. ntiles + 5; the flush replayed over random tile -> chunk
    sequences split over 1, 2, 3 and 7 workgroups, with lists around the touched list's capacity."""
    exe = tmp_path / "literal_matrix_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(ROOT / "tests" / "cpp" / "literal_matrix_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "literal_matrix_selftest ok" in r.stdout
