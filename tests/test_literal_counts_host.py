"""xsg_count_literals without a GPU: tests/literal_counts_model.py pinned to the oracle through the relation include/xsg.h
states, and set_count_at -- the function k_set_count_literals runs at every candidate -- under the sanitizers as a
stand-alone program."""
import subprocess
from pathlib import Path

import literal_counts_model as LM
import set_cases as SC

ROOT = Path(__file__).resolve().parents[1]


def exact_count(oracle, blocks, lit):
    """XSG_CTR_MATCHES of xsg_count(XSG_COUNT_MATCHES) under XSG_FLAG_EXACT_TAIL with `lit` as the only pattern"""
    oracle.set_exact(True)
    try:
        return sum(oracle.count(b, lit, False) for b in blocks)
    finally:
        oracle.set_exact(False)


def test_model_equals_the_exact_tail_match_count_of_every_borderless_literal(oracle):
    blocks = SC.text_blocks()
    lits = SC.word_list(300)
    free = [l for l in lits if LM.borderless(l)]
    assert len(free) >= 250 and len(free) < len(lits)  # (the list also holds literals with a border)
    want = dict(zip(lits, LM.counts(blocks, lits)))
    assert sum(want[l] for l in free) > 10_000
    for lit in sorted(set(free)):
        assert exact_count(oracle, blocks, lit) == want[lit], lit
    # and where occurrences do not overlap in the data, a literal with a border agrees as well
    for lit in sorted(set(lits) - set(free)):
        texts = [b.tobytes() for b in blocks]
        overlap = any(t.find(lit, at + 1, at + 2 * len(lit) - 1) >= 0 for t in texts for at in _starts(t, lit))
        if not overlap:
            assert exact_count(oracle, blocks, lit) == want[lit], lit


def _starts(text, lit):
    at = text.find(lit)
    while at >= 0:
        yield at
        at = text.find(lit, at + 1)


def test_model_counts_occurrences_where_the_match_walk_skips_overlaps(oracle):
    u8 = SC.u8
    assert LM.counts([u8(b"aaaa")], [b"aa"]) == [3] and exact_count(oracle, [u8(b"aaaa")], b"aa") == 2
    assert LM.counts([u8(b"ababab")], [b"abab"]) == [2] and exact_count(oracle, [u8(b"ababab")], b"abab") == 1
    assert not LM.borderless(b"aa") and not LM.borderless(b"abab") and LM.borderless(b"ab")
    # covered literals, duplicates, chunk ends, ignore-case
    assert LM.counts([u8(b"abc")], [b"ab", b"abc"]) == [1, 1]
    assert LM.counts([u8(b"xabab"), u8(b"ab")], [b"ab", b"b", b"ab"]) == [3, 3, 3]
    assert LM.counts([u8(b"xa"), u8(b"b")], [b"ab"]) == [0]  # no occurrence straddles two chunks
    assert LM.counts([u8(b"AbaB caf\xc9")], [b"ab", b"caf\xe9", b"CAF\xc9"], icase=True) == [2, 0, 1]
    assert LM.counts([], [b"a", b"b"]) == [0, 0]


def test_set_count_at_under_the_sanitizers(tmp_path):
    """tests/cpp/literal_counts_selftest.cpp includes csrc/xsg_set.h/.cpp: a stand-alone program, nothing is loaded into
    Python.  The 4096-literal shared-gram list, a 255-byte literal, NUL literals, bytes >= 0x80, both fold modes,
    room = len and room = len - 1, against a naive double loop."""
    exe = tmp_path / "literal_counts_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "literal_counts_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "literal_counts_selftest ok" in r.stdout
