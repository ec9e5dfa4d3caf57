"""The row limit per FILE (include/xsg.h: xsg_job_start_max_count, xsg_fileset_start_max_count, xsg_host_searcher_set_max_count;
xsgrep --max-count, -q): a job's, a file set's and the command line's results against the same call without the limit, cut,
and against tests/limit_model.py's whole-file form over the oracle.

Without the feature every test fails: xsg.Job and xsg.FileSet take no max_count, xsg.HostSearcher does not exist and xsgrep
knows neither option."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fileset_tree as T
import limit_model
import xsg
from test_gpu_max_count import plain_of

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
INV, RX = xsg.FLAG_INVERT, xsg.FLAG_REGEX
JOB_CHUNK = 4096

TAGS = [(xsg.COUNT_MATCHES, "count_matches"), (xsg.COUNT_LINES, "count_lines"), (xsg.MATCH_BYTE_OFFSETS, "match_byte_offsets"),
        (xsg.LINE_BYTE_OFFSETS, "line_byte_offsets"), (xsg.LINE_INDICES, "line_indices"), (xsg.LINES, "lines"), (xsg.MATCHES, "matches")]
MATCH_TAGS = (xsg.COUNT_MATCHES, xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES)
# (id, kind, pattern, list flags, invert)
JOB_CASES = [
    ("literal", "lit", b"that", 0, False),
    ("literal_inverted", "lit", b"that", 0, True),
    ("any_of", "anyof", (b"that", b"colour", b"zebra"), 0, False),
    ("any_of_inverted", "anyof", (b"that", b"colour", b"zebra"), 0, True),
    ("all_of", "allof", (b"that", b"ing"), xsg.LIST_ALL_OF, False),
    ("all_of_inverted", "allof", (b"that", b"ing"), xsg.LIST_ALL_OF, True),
]


def blocks_of(path, data: bytes, chunk_bytes: int):
    """the chunks a job over this file searches (xsg_plan_chunks is host only)"""
    plan = xsg.plan_chunks(str(path), chunk_bytes)
    blocks = [np.frombuffer(data[int(c["original_offset"]):int(c["original_offset"]) + int(c["original_size"])], dtype=np.uint8) for c in plan]
    assert sum(b.size for b in blocks) == len(data)
    return blocks


def whole_file(oracle, kind, pat, invert, blocks, n, cache=None):
    """limit_model's whole-file form over the chunk-wise oracle dict -> {tag key: expected result}; cache: a dict that keeps
    the oracle's answer between calls with the same pattern and blocks"""
    if cache is None or "plain" not in cache:
        plain, matches = plain_of(oracle, kind, pat, RX if kind == "rx" else 0, invert, blocks, None, None)
        if cache is not None:
            cache["plain"] = (plain, matches)
    else:
        plain, matches = cache["plain"]
    w = limit_model.limit_whole_file(plain, n, matches)
    return {k: w[k] for k in ("count_matches", "count_lines", "match_byte_offsets", "line_byte_offsets", "line_indices", "lines", "matches") if k in w}


def run_job(path, kind, pat, lflags, invert, mode, threads, n):
    is_list = kind in ("anyof", "allof")
    j = xsg.Job(b"\n".join(pat) if is_list else pat, str(path), mode, num_threads=threads, num_max_readers=threads, chunk_bytes=JOB_CHUNK,
                flags=INV if invert else 0, pattern_is_list=is_list, list_flags=lflags, max_count=n)
    r = j.result()
    st = j.stats()
    j.close()
    return (r if isinstance(r, (int, list)) else r.tolist()), st


@pytest.fixture(scope="module")
def job_file(tmp_path_factory):
    rng = np.random.default_rng(77)
    data = T.words_text(rng, 300 << 10, terminated=False) + b" that colour running"  # the last line lacks its newline
    path = tmp_path_factory.mktemp("max_count_job") / "corpus.txt"
    path.write_bytes(data)
    blocks = blocks_of(path, data, JOB_CHUNK)
    assert len(blocks) >= 64
    return path, data, blocks


@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("cid,kind,pat,lflags,invert", JOB_CASES, ids=[c[0] for c in JOB_CASES])
def test_a_job_reports_the_first_n_entries(oracle, job_file, cid, kind, pat, lflags, invert, threads):
    path, data, blocks = job_file
    cache = {}
    for mode, key in TAGS:
        if mode in MATCH_TAGS and (invert or kind == "allof"):
            continue
        full, st_full = run_job(path, kind, pat, lflags, invert, mode, threads, 0)
        assert full == whole_file(oracle, kind, pat, invert, blocks, 0, cache)[key], (cid, key, "the job without a limit")
        counting = isinstance(full, int)
        total = full if counting else len(full)
        assert total > 40
        # the cut in the chunk of the first entry, in a middle one, in the last one (the file's last line is selected), beyond the total
        for n in (1, total // 2, total - 1, total + 7):
            got, st = run_job(path, kind, pat, lflags, invert, mode, threads, n)
            assert got == (min(full, n) if counting else full[:n]), (cid, key, n, "the first n of the job without a limit")
            assert got == whole_file(oracle, kind, pat, invert, blocks, n, cache)[key], (cid, key, n, "the whole-file model")
            assert st["chunks"] <= st["plan_chunks"] == len(blocks)
            if n > total:
                assert st["chunks"] == len(blocks)


@pytest.mark.parametrize("threads", [1, 2])
def test_a_job_stops_reading_behind_the_budget(tmp_path, threads):
    """the only hits lie in chunk k; with N = 1 no more than k + 1 + R chunks are searched, R = 2 x workers + 3 pinned buffers
    in circulation, on a file more than four times as long as that bound"""
    k, ring = 6, 2 * threads + 3
    nchunks = 4 * (k + 1 + ring) + 8
    line = b"plain words and nothing of interest here\n"
    per_chunk = JOB_CHUNK // len(line) + 1
    chunks = [line * per_chunk for _ in range(nchunks)]
    chunks[k] = line * 10 + b"x that colour\n" * 3 + line * (per_chunk - 13)
    path = tmp_path / "sparse.txt"
    path.write_bytes(b"".join(chunks))
    plan = xsg.plan_chunks(str(path), JOB_CHUNK)
    hit = sum(len(c) for c in chunks[:k]) + len(line) * 10
    at = [i for i, c in enumerate(plan) if int(c["original_offset"]) <= hit < int(c["original_offset"]) + int(c["original_size"])]
    assert len(plan) >= 4 * (k + 1 + ring) and len(at) == 1
    k_plan = at[0]
    for mode, want in ((xsg.LINE_BYTE_OFFSETS, [hit]), (xsg.COUNT_LINES, 1), (xsg.LINES, [b"x that colour"])):
        j = xsg.Job(b"that", str(path), mode, num_threads=threads, num_max_readers=threads, chunk_bytes=JOB_CHUNK, max_count=1)
        got = j.result()
        st = j.stats()
        j.close()
        assert (got if isinstance(got, (int, list)) else got.tolist()) == want
        print(f"early stop: {st['chunks']} of {st['plan_chunks']} chunks searched, first hit in chunk {k_plan}, bound {k_plan + 1 + ring}")
        assert k_plan + 1 <= st["chunks"] <= k_plan + 1 + ring, (mode, st)


def test_context_with_a_limit_is_refused_by_both_start_calls(job_file):
    path, _, _ = job_file
    for mode in (xsg.LINES, xsg.COUNT_LINES):
        with pytest.raises(xsg.XsgError) as e:
            xsg.Job(b"that", str(path), mode, chunk_bytes=JOB_CHUNK, flags=xsg.flag_context(1, 2), max_count=3)
        assert e.value.code == xsg.ENOTSUP and "XSG_FLAG_CONTEXT" in str(e.value)
        with pytest.raises(xsg.XsgError) as e:
            xsg.FileSet(b"that", [str(path)], mode, flags=xsg.flag_context(0, 1), max_count=3)
        assert e.value.code == xsg.ENOTSUP and "XSG_FLAG_CONTEXT" in str(e.value)
    j = xsg.Job(b"that", str(path), xsg.LINES, chunk_bytes=JOB_CHUNK, flags=xsg.flag_context(1, 2))  # served without a limit
    assert len(j.result()) > 40
    j.close()


# ---- file sets ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("max_count_fileset")
    files = T.build(str(root))
    paths = [str(root / r) for r in files]
    data = list(files.values())
    assert sum(len(d) > T.CHUNK_BYTES for d in data) == 1
    return paths, data


def run_set(tree, kind, pat, lflags, mode, flags, n, batch_bytes, readers):
    paths, _ = tree
    is_list = kind in ("anyof", "allof")
    fs = xsg.FileSet(b"\n".join(pat) if is_list else pat, paths, mode, flags=flags, num_readers=readers, batch_bytes=batch_bytes,
                     chunk_bytes=T.CHUNK_BYTES, pattern_is_list=is_list, list_flags=lflags, max_count=n)
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


SET_CASES = [("literal", "lit", b"that", 0, False), ("literal_inverted", "lit", b"that", 0, True),
             ("all_of", "allof", (b"that", b"ing"), xsg.LIST_ALL_OF, False)]


@pytest.mark.parametrize("cid,kind,pat,lflags,invert", SET_CASES, ids=[c[0] for c in SET_CASES])
def test_every_file_of_a_set_has_its_own_limit(oracle, tree, cid, kind, pat, lflags, invert):
    paths, data = tree
    blocks = [T.chunks_of(p, d) for p, d in zip(paths, data)]
    caches = [{} for _ in blocks]
    for n in (1, 3):
        want = [whole_file(oracle, kind, pat, invert, b, n, c) for b, c in zip(blocks, caches)]
        cut = 0
        for mode, key in TAGS:
            if mode in MATCH_TAGS and (invert or kind == "allof"):
                continue
            got = {}
            for batch_bytes in (T.BATCH_BYTES, 0):
                for readers in (1, 4):
                    status, results = run_set(tree, kind, pat, lflags, mode, INV if invert else 0, n, batch_bytes, readers)
                    got[batch_bytes, readers] = results
                    assert all(s == xsg.OK for s in status)
                    for f, w in enumerate(want):
                        assert results[f] == w[key], (cid, key, n, batch_bytes, readers, paths[f])
            assert len({repr(v) for v in got.values()}) == 1
            full = run_set(tree, kind, pat, lflags, mode, INV if invert else 0, 0, T.BATCH_BYTES, 4)[1]
            cut += sum(r != f for r, f in zip(results, full))
        assert cut > 20, "the limit cut next to nothing: the tree does not exercise it"


def test_the_search_behind_a_refusal_carries_the_limit(oracle, tree):
    """`Sher.ock` accepts no byte >= 0x80: the batch with such a file is searched again file by file, under the same limit"""
    paths, data = tree
    dirty = [f for f, d in enumerate(data) if any(c >= 0x80 for c in d)]
    assert len(dirty) == 1
    status, limited = run_set(tree, "rx", b"Sher.ock", 0, xsg.COUNT_LINES, RX, 1, T.BATCH_BYTES, 2)
    _, full = run_set(tree, "rx", b"Sher.ock", 0, xsg.COUNT_LINES, RX, 0, T.BATCH_BYTES, 2)
    assert status[dirty[0]] == xsg.ENOTSUP and all(s == xsg.OK for f, s in enumerate(status) if f not in dirty)
    assert limited == [min(c, 1) for c in full] and sum(full) > sum(limited) > 5


# ---- the host searcher --------------------------------------------------------------------------------------------------------------
def test_the_host_searcher_takes_a_limit_between_calls(oracle):
    """chunk-local results under the limit of the moment, against limit_model on the chunk alone; 4: the fourth selected line
    lacks its newline -- cut in, then not handed out"""
    chunk = b"x that one\nplain\nthat two that\nthat three\nplain words to keep the end of the chunk away\nthat four"
    block = [np.frombuffer(chunk, dtype=np.uint8)]
    plain, matches = plain_of(oracle, "lit", b"that", 0, False, block, None, None)
    assert (plain["count_lines"], plain["count_matches"], len(plain["lines"])) == (4, 5, 3)
    hs = xsg.HostSearcher(0, b"that", max_slots=2, max_count=2)
    for n in (2, 4, 1, 0, 3):
        if n != 2:
            hs.set_max_count(n)
        w = limit_model.limit_all_modes(plain, block, n, matches=matches)
        assert hs.count(chunk, skip_to_nl=True) == w["count_lines"] and hs.count(chunk) == w["count_matches"], n
        assert hs.offsets(xsg.LINE_BYTE_OFFSETS, chunk).tolist() == w["line_byte_offsets"], n
        assert hs.offsets(xsg.LINE_INDICES, chunk).tolist() == w["line_indices"], n
        assert hs.offsets(xsg.MATCH_BYTE_OFFSETS, chunk).tolist() == w["match_byte_offsets"], n
        assert hs.lines(chunk) == w["lines"] and hs.matches(chunk) == w["matches"], n
    hs.close()


# ---- xsgrep -----------------------------------------------------------------------------------------------------------------------------
def xsgrep(*args, cwd=None, stdin=None, env=None):
    e = dict(os.environ, XS_CHUNK_BYTES=str(T.CHUNK_BYTES), XS_BATCH_BYTES=str(T.BATCH_BYTES), **(env or {}))
    r = subprocess.run([str(XSGREP), *args], capture_output=True, timeout=120, env=e, cwd=cwd, input=stdin,
                       stdin=subprocess.DEVNULL if stdin is None else None)
    return r.returncode, r.stdout, r.stderr


def cut_per_file(stdout: bytes, n: int) -> bytes:
    """the first n lines of every PATH: prefix, in the order they were printed"""
    seen, out = {}, []
    for line in stdout.splitlines(keepends=True):
        p = line.split(b":", 1)[0]
        seen[p] = seen.get(p, 0) + 1
        if seen[p] <= n:
            out.append(line)
    return b"".join(out)


@pytest.fixture(scope="module")
def cli_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("max_count_cli")
    return str(root), T.build(str(root))


@pytest.mark.parametrize("opts", [[], ["-v"], ["-i"], ["-F", "-w"], ["-x", "-E"]], ids=["default", "-v", "-i", "-F -w", "-x -E"])
def test_xsgrep_max_count_on_one_file(cli_tree, opts):
    """the same command without the option, cut; the single-file form's exit status stays 0 without -q"""
    root, files = cli_tree
    pat = "x that colour a" if "-x" in opts else "that"
    for rel in ("a_len16.txt" if "-x" in opts else "c_large.txt", "b_no_final_newline.txt"):
        rc, full, err = xsgrep(*opts, pat, rel, cwd=root)
        assert rc == 0 and err == b""
        lines = full.splitlines(keepends=True)
        for n in (1, 3):
            rc, out, err = xsgrep(f"--max-count={n}", *opts, pat, rel, cwd=root)
            assert (rc, err) == (0, b"") and out == b"".join(lines[:n]), (rel, n)
        rc, out, err = xsgrep("--max-count", "3", "-c", *opts, pat, rel, cwd=root)
        count = int(xsgrep("-c", *opts, pat, rel, cwd=root)[1])
        assert (rc, err, out) == (0, b"", b"%d\n" % min(count, 3)), rel
        assert xsgrep("-q", *opts, pat, rel, cwd=root) == (0 if count else 1, b"", b"")


def test_xsgrep_q_exit_statuses_on_one_file(cli_tree):
    root, _ = cli_tree
    assert xsgrep("-q", "qqqqzz", "c_large.txt", cwd=root) == (1, b"", b"")
    assert xsgrep("-qi", "THAT", "c_large.txt", cwd=root) == (0, b"", b"")
    rc, out, err = xsgrep("-q", "that", "missing.txt", cwd=root)
    assert rc == 2 and out == b"" and err.startswith(b"xsgrep: ")
    assert xsgrep("--max-count=1000000", "that", "c_large.txt", cwd=root) == xsgrep("that", "c_large.txt", cwd=root)


SEVERAL = [[], ["-v"], ["-F", "--all-of", "-e", "that", "-e", "ing"]]


@pytest.mark.parametrize("opts", SEVERAL, ids=["default", "-v", "--all-of -r"])
def test_xsgrep_max_count_on_several_files_and_recursively(cli_tree, opts):
    root, files = cli_tree
    pattern = [] if "--all-of" in opts else ["that"]
    operands = ["-r", "."] if not pattern else list(files)  # (-e / -f keep their one FILE operand: a tree through -r)
    rc, full, err = xsgrep(*opts, *pattern, *operands, cwd=root)
    assert rc == 0 and err == b""
    _, counts, _ = xsgrep("-c", *opts, *pattern, *operands, cwd=root)
    for n in (1, 2):
        rc, out, err = xsgrep(f"--max-count={n}", *opts, *pattern, *operands, cwd=root)
        assert (rc, err) == (0, b"") and out == cut_per_file(full, n) and out != full, (opts, n)
    rc, out, err = xsgrep("-c", "--max-count", "2", *opts, *pattern, *operands, cwd=root)
    want = b"".join(p + b":%d\n" % min(int(c), 2) for p, c in (l.rsplit(b":", 1) for l in counts.splitlines()))
    assert (rc, err, out) == (0, b"", want), opts
    if pattern:  # -r with the positional pattern too
        rc, out, _ = xsgrep("-r", "--max-count=2", *opts, "that", ".", cwd=root)
        assert rc == 0 and out == cut_per_file(xsgrep("-r", *opts, "that", ".", cwd=root)[1], 2)


def test_xsgrep_exit_statuses_on_several_files(cli_tree):
    """0 selected, 1 nothing, 2 a file failed; -q prints nothing in every case; -H on one file"""
    root, files = cli_tree
    rels = list(files)
    assert xsgrep("-H", "--max-count=2", "that", "c_large.txt", cwd=root)[1] == cut_per_file(xsgrep("-H", "that", "c_large.txt", cwd=root)[1], 2)
    assert xsgrep("--max-count=1", "qqqqzz", *rels[:8], cwd=root) == (1, b"", b"")
    assert xsgrep("-q", "that", *rels, cwd=root) == (0, b"", b"")
    assert xsgrep("-q", "-r", "that", ".", cwd=root) == (0, b"", b"")
    assert xsgrep("-q", "qqqqzz", *rels[:8], cwd=root) == (1, b"", b"")
    rc, out, err = xsgrep("-q", "that", rels[2], "missing.txt", cwd=root)
    assert rc == 2 and out == b"" and err.startswith(b"xsgrep: missing.txt: ")


def test_xsgrep_l_and_L_print_what_they_printed(cli_tree):
    root, files = cli_tree
    rels = list(files)
    _, counts, _ = xsgrep("-c", "that", *rels, cwd=root)
    with_, without = [], []
    for l in counts.splitlines():
        p, c = l.rsplit(b":", 1)
        (with_ if int(c) else without).append(p + b"\n")
    assert xsgrep("-l", "that", *rels, cwd=root) == (0, b"".join(with_), b"")
    assert xsgrep("-L", "that", *rels, cwd=root) == (0, b"".join(without), b"")
    assert xsgrep("-l", "--max-count=5", "that", *rels, cwd=root) == (0, b"".join(with_), b"")
    assert xsgrep("-rl", "that", ".", cwd=root)[1] == b"".join(b"./" + p for p in with_)
    assert b"c_large.txt\n" in with_ and without


@pytest.mark.parametrize("opts", [[], ["-v"], ["-F", "-e", "that", "-e", "zebra"]], ids=["default", "-v", "-F -e -e"])
def test_xsgrep_max_count_on_stdin(cli_tree, opts):
    root, files = cli_tree
    data = files["c_large.txt"]
    env = {"XSGREP_CHUNK_BYTES": "8192"}  # the pipe is read as two dozen chunks: the budget crosses their seams
    pattern = [] if "-e" in opts else ["that"]
    rc, full, err = xsgrep(*opts, *pattern, "-", stdin=data, env=env)
    lines = full.splitlines(keepends=True)
    first = len([l for l in data[:8192].splitlines() if (b"that" in l or b"zebra" in l and "-e" in opts) != ("-v" in opts)])
    assert rc == 0 and err == b"" and 5 < first < len(lines) // 4  # (about what the first chunk selects)
    for n in (1, first + 20, len(lines) + 3):
        rc, out, err = xsgrep(f"--max-count={n}", *opts, *pattern, "-", stdin=data, env=env)
        assert (rc, err) == (0, b"") and out == b"".join(lines[:n]), (opts, n)
    rc, out, err = xsgrep("-c", f"--max-count={first + 20}", *opts, *pattern, "-", stdin=data, env=env)
    assert (rc, err, out) == (0, b"", b"%d\n" % (first + 20)), opts
    assert xsgrep("-q", *opts, *pattern, "-", stdin=data, env=env) == (0, b"", b"")
    if not opts:
        assert xsgrep("-q", "qqqqzz", "-", stdin=data, env=env) == (1, b"", b"")
