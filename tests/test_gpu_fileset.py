"""xsg_fileset_* / xsg.FileSet: a list of files searched as the chunks of a few bindings.

File f's result must be what a search of that file ALONE reports.  Expected values come from the CPU oracle per file taken
as one chunk (tests/per_chunk_model.py: file_results), and for the one file larger than chunk_bytes -- the delegated path --
from the oracle per chunk of xsg_plan_chunks, which is host-only.  The path list holds the tree of tests/fileset_tree.py
plus a path that does not exist, a directory, and one path a second time.

Without the feature every test fails: xsg.FileSet does not exist."""
import os

import numpy as np
import pytest

import fileset_tree as T
import xsg
from per_chunk_model import CTX, IC, INV, RX, X

pytestmark = pytest.mark.gpu

TAGS = [(xsg.COUNT_MATCHES, "count_matches"), (xsg.COUNT_LINES, "count_lines"), (xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"),
        (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices"), (xsg.LINES, "lines"), (xsg.MATCHES, "matches")]
FLAGS = [(0, "none"), (IC, "icase"), (X, "exact"), (INV, "invert"), (CTX, "context"), (INV | CTX, "invert+context")]
PATTERNS = [
    ("literal", "lit", b"that", 0),
    ("regex", "rx", b"colou?r", RX),
    ("any_of", "anyof", (b"that", b"colour", b"zebra"), 0),
    ("all_of", "allof", (b"that", b"ing"), 0),
]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("fileset")
    files = T.build(str(root))
    rels = list(files)
    paths = [str(root / r) for r in rels]
    data = [files[r] for r in rels]
    # a missing path, a directory and a second mention, in the middle of the list and at its end
    paths[10:10] = [str(root / "missing.txt")]
    data[10:10] = [None]
    paths[30:30] = [str(root / "d1")]
    data[30:30] = [None]
    paths.append(paths[3])
    data.append(data[3])
    assert sum(d is not None and len(d) > T.CHUNK_BYTES for d in data) == 1
    return paths, data


def run(tree, pat, mode, flags=0, kind="lit", batch_bytes=T.BATCH_BYTES, num_readers=4):
    paths, _ = tree
    is_list = kind in ("anyof", "allof")
    fs = xsg.FileSet(b"\n".join(pat) if is_list else pat, paths, mode, flags=flags, num_readers=num_readers, batch_bytes=batch_bytes,
                     chunk_bytes=T.CHUNK_BYTES, pattern_is_list=is_list, list_flags=xsg.LIST_ALL_OF if kind == "allof" else 0)
    fs.join()
    status, counts = fs.status().tolist(), fs.counts().tolist()
    if mode in (xsg.COUNT_MATCHES, xsg.COUNT_LINES):
        results = counts
    else:
        fp = fs.file_ptr().tolist()
        assert fp[0] == 0 and [b - a for a, b in zip(fp, fp[1:])] == counts
        flat = fs._entries(0, fp[-1])
        flat = flat if isinstance(flat, list) else flat.tolist()
        results = [flat[a:b] for a, b in zip(fp, fp[1:])]
    fs.close()
    return status, results


def served(kind, flags, mode):
    if mode in (xsg.COUNT_MATCHES, xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES):
        return kind != "allof" and not flags & INV
    return True


def want_all(oracle, tree, kind, pat, pflags, flags):
    paths, data = tree
    return [None if d is None else T.want_file(oracle, kind, pat, pflags, flags, p, d) for p, d in zip(paths, data)]


def compare(status, results, want, key, where):
    for f, w in enumerate(want):
        if w is None:
            assert status[f] == xsg.EIO, (where, f, "status of a path that cannot be read")
            assert results[f] in (0, []), (where, f, "its row is empty")
            continue
        assert status[f] == xsg.OK, (where, f, status[f])
        assert results[f] == w[key], (where, f, key)


@pytest.mark.parametrize("pid,kind,pat,pflags", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_every_tag_and_flag(oracle, tree, pid, kind, pat, pflags):
    for flags, fname in FLAGS:
        want = want_all(oracle, tree, kind, pat, pflags, flags)
        for mode, key in TAGS:
            if not served(kind, flags, mode):
                with pytest.raises(xsg.XsgError) as e:  # refused where the set is started
                    run(tree, pat, mode, pflags | flags, kind)
                assert e.value.code == xsg.ENOTSUP, (pid, fname, key)
                continue
            status, results = run(tree, pat, mode, pflags | flags, kind)
            compare(status, results, want, key, (pid, fname, key))
    # the cases tell something: the delegated file and the small ones report lines, and the duplicate equals its first mention
    paths, data = tree
    big = next(f for f, d in enumerate(data) if d is not None and len(d) > T.CHUNK_BYTES)
    assert want[big]["line_byte_offsets"] and len(results[big]) > 100
    assert results[-1] == results[3]


@pytest.mark.parametrize("mode,key", TAGS, ids=[k for _, k in TAGS])
def test_identical_for_every_batch_size_and_reader_count(oracle, tree, mode, key):
    for kind, pat, pflags, flags in (("lit", b"that", 0, 0), ("rx", b"colou?r", RX, CTX)):
        want = want_all(oracle, tree, kind, pat, pflags, flags)
        got = {}
        for batch_bytes in (T.BATCH_BYTES, 0):  # several batches with cuts between files; the default: one batch
            for readers in (1, 4):
                got[batch_bytes, readers] = run(tree, pat, mode, pflags | flags, kind, batch_bytes, readers)
                compare(*got[batch_bytes, readers], want, key, (key, pat, batch_bytes, readers))
        assert len({repr(v) for v in got.values()}) == 1


def test_only_the_non_ascii_file_is_refused(oracle, tree):
    """`Sher.ock`: `.` is ASCII-only, and a binding that holds a byte >= 0x80 is refused as a whole -- the set searches such a
    batch again file by file, and the other files of it keep their results"""
    paths, data = tree
    dirty = [f for f, d in enumerate(data) if d is not None and any(c >= 0x80 for c in d)]
    assert len(dirty) == 1
    for mode, key in ((xsg.COUNT_LINES, "count_lines"), (xsg.LINES, "lines"), (xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets")):
        status, results = run(tree, b"Sher.ock", mode, RX, "rx")
        hits = 0
        for f, d in enumerate(data):
            if d is None:
                assert status[f] == xsg.EIO
            elif f in dirty:
                assert status[f] == xsg.ENOTSUP and results[f] in (0, [])
            else:
                assert status[f] == xsg.OK
                w = T.want_file(oracle, "rx", b"Sher.ock", RX, 0, paths[f], d)[key]
                assert results[f] == w, (key, f)
                hits += bool(w)
        assert hits > 5


def test_wait_publishes_in_path_order(oracle, tree):
    """the contract of xsg_fileset_wait, not its timing: when wait(i) returns, files 0..i have their final results, whatever
    is still pending behind them"""
    paths, data = tree
    want = want_all(oracle, tree, "lit", b"that", 0, 0)
    fs = xsg.FileSet(b"that", paths, xsg.LINES, batch_bytes=T.BATCH_BYTES, chunk_bytes=T.CHUNK_BYTES, num_readers=2)
    seen = 0
    for i in (0, 5, 10, 11, 40, len(paths) - 1):
        done, finished = fs.wait(i)
        assert done > i and done >= seen and (not finished or done == len(paths))
        seen = done
        st, fp = fs.status().tolist(), fs.file_ptr().tolist()
        for f in range(done):
            got = fs._entries(fp[f], fp[f + 1])
            assert got == ([] if want[f] is None else want[f]["lines"]), (i, f)
            assert st[f] == (xsg.EIO if want[f] is None else xsg.OK)
    early = [fs.result(f) for f in range(12)]
    fs.join()
    assert [fs.result(f) for f in range(12)] == early and fs.wait(0) == (len(paths), True)
    it = list(xsg.FileSet(b"that", paths[:6], xsg.COUNT_LINES, chunk_bytes=T.CHUNK_BYTES))
    assert [p for p, _, _ in it] == paths[:6] and [r for _, _, r in it] == [w["count_lines"] for w in want[:6]]
    fs.close()


def test_nothing_to_search_and_sets_without_a_batch(oracle, tmp_path):
    fs = xsg.FileSet(b"that", [], xsg.LINES)
    fs.join()
    assert fs.counts().size == 0 and fs.file_ptr().tolist() == [0] and fs.wait(0) == (0, True)
    fs.close()
    # only files that cannot be read, and only a large one: no batch holds an item
    big = tmp_path / "big.txt"
    big.write_bytes(b"x that\n" * 20_000)
    fs = xsg.FileSet(b"that", [str(tmp_path / "nope"), str(big), str(tmp_path)], xsg.COUNT_LINES, chunk_bytes=T.CHUNK_BYTES).join()
    assert fs.status().tolist() == [xsg.EIO, xsg.OK, xsg.EIO] and fs.counts().tolist() == [0, 20_000, 0]
    fs.close()
    with pytest.raises(xsg.XsgError) as e:
        xsg.FileSet(b"that", [str(big)], xsg.LINES, batch_bytes=1 << 10, chunk_bytes=1 << 12)
    assert e.value.code == xsg.EINVAL
