"""xsgrep FILE FILE... / -r: stdout byte for byte against a model built from the CPU oracle (tests/per_chunk_model.py:
file_results per file), the exit statuses, the order of the walk, and the single-FILE path left as it was.

Without the feature every test fails: a second FILE is "unexpected argument"."""
import os
import subprocess
from pathlib import Path

import pytest

import fileset_tree as T
from per_chunk_model import CTX, IC, INV

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("fileset_cli")
    return str(root), T.build(str(root))


def xsgrep(*args, cwd=None):
    env = dict(os.environ, XS_CHUNK_BYTES=str(T.CHUNK_BYTES), XS_BATCH_BYTES=str(T.BATCH_BYTES))
    r = subprocess.run([str(XSGREP), *args], capture_output=True, timeout=120, env=env, cwd=cwd)
    return r.returncode, r.stdout, r.stderr


def model(oracle, root, rels, files, kind, pat, flags, out, prefix=True):
    """-> (stdout, anything selected) for the files `rels` (relative to root, printed as given)"""
    text, selected = b"", False
    for rel in rels:
        w = T.want_file(oracle, kind, pat, 0, flags, os.path.join(root, rel), files[rel])
        p = rel.encode() + b":" if prefix else b""
        if out == "count":
            text += p + str(w["count_lines"]).encode() + b"\n"
            selected |= w["count_lines"] != 0
        elif out in ("with", "without"):
            if (w["count_lines"] != 0) == (out == "with"):
                text += rel.encode() + b"\n"
                selected = True
        else:
            for line in w["matches" if out == "only" else "lines"]:
                text += p + line + b"\n"
                selected = True
    return text, selected


CASES = [
    ([], "lit", b"that", 0, "lines"),
    (["-c"], "lit", b"that", 0, "count"),
    (["-l"], "lit", b"that", 0, "with"),
    (["-L"], "lit", b"that", 0, "without"),
    (["-o"], "lit", b"that", 0, "only"),
    (["-v"], "lit", b"that", INV, "lines"),
    (["-i", "-c"], "lit", b"that", IC, "count"),
    (["-F", "-e", "that", "-e", "zebra"], "anyof", (b"that", b"zebra"), 0, "lines"),
    (["-F", "--all-of", "-e", "that", "-e", "ing"], "allof", (b"that", b"ing"), 0, "lines"),
    (["-F", "--all-of", "-l", "-e", "that", "-e", "ing"], "allof", (b"that", b"ing"), 0, "with"),
]


@pytest.mark.parametrize("opts,kind,pat,flags,out", CASES, ids=[" ".join(c[0]) or "default" for c in CASES])
def test_recursive_and_explicit_files(oracle, tree, opts, kind, pat, flags, out):
    root, files = tree
    rels = list(files)
    pattern = [] if kind in ("anyof", "allof") else [pat.decode()]
    want, selected = model(oracle, root, rels, files, kind, pat, flags, out)
    # explicit operands, relative to the tree's root (with the positional PATTERN: -e / -f keep their one FILE operand) ...
    if pattern:
        rc, stdout, stderr = xsgrep(*opts, *pattern, *rels, cwd=root)
        assert (rc, stderr) == (0 if selected else 1, b""), stderr
        assert stdout == want
    else:
        rc, stdout, stderr = xsgrep(*opts, rels[2], rels[3], cwd=root)
        assert (rc, stdout, stderr) == (2, b"", b"unexpected argument '%s'\n" % rels[3].encode())
    # ... and -r over the directory: the same files in the order of the sorted walk, printed as DIR/relative
    rc, stdout, stderr = xsgrep("-r", *opts, *pattern, ".", cwd=root)
    want_r, _ = model(oracle, root, ["./" + r for r in rels], {"./" + r: files[r] for r in rels}, kind, pat, flags, out)
    assert (rc, stderr) == (0 if selected else 1, b""), stderr
    assert stdout == want_r
    if out in ("lines", "only", "count"):
        rc, stdout, _ = xsgrep("-r", "--no-filename", *opts, *pattern, ".", cwd=root)
        assert stdout == model(oracle, root, rels, files, kind, pat, flags, out, prefix=False)[0] and rc == (0 if selected else 1)


def test_context_lines_carry_the_path(oracle, tree):
    root, files = tree
    rels = [r for r in files if not r.startswith("c_large")]  # (context across the delegated file's seams: test_gpu_fileset.py)
    rc, stdout, stderr = xsgrep("-C", "1", "-A", "2", "zebra", *rels, cwd=root)
    want, selected = model(oracle, root, rels, files, "lit", b"zebra", CTX, "lines")
    assert (rc, stderr) == (0, b"") and selected and stdout == want
    assert b"--\n" not in stdout and not any(l.split(b":")[0].endswith(b"-") for l in stdout.splitlines())


def test_exit_statuses(oracle, tree):
    root, files = tree
    rels = list(files)[:8]
    assert xsgrep("-c", "qqqqzz", *rels, cwd=root)[0] == 1
    assert xsgrep("-l", "qqqqzz", *rels, cwd=root)[::2] == (1, b"")
    rc, stdout, _ = xsgrep("-L", "qqqqzz", *rels, cwd=root)
    assert rc == 0 and stdout == b"".join(r.encode() + b"\n" for r in rels)
    # a file that fails: status 2, its line on stderr, the others still printed
    rc, stdout, stderr = xsgrep("that", rels[2], "missing.txt", "d1", rels[3], cwd=root)
    want, _ = model(oracle, root, [rels[2], rels[3]], files, "lit", b"that", 0, "lines")
    assert rc == 2 and stdout == want
    assert stderr.startswith(b"xsgrep: missing.txt: ") and b"\nxsgrep: d1: " in stderr and stderr.count(b"\n") == 2
    # `.` accepts no byte >= 0x80: only that file fails
    rc, stdout, stderr = xsgrep("-E", "-c", "Sher.ock", "b_non_ascii.txt", "b_no_final_newline.txt", cwd=root)
    assert rc == 2 and stderr.startswith(b"xsgrep: b_non_ascii.txt: ") and stdout.startswith(b"b_no_final_newline.txt:")


def test_a_single_file_prints_what_it_always_printed(oracle, tree):
    root, files = tree
    for rel, opts in (("b_no_final_newline.txt", []), ("c_large.txt", []), ("c_large.txt", ["-c"]), ("c_large.txt", ["-o"]), ("d2/no_match.txt", ["-v"])):
        single = xsgrep(*opts, "that", rel, cwd=root)
        listed = xsgrep("--no-filename", *opts, "that", rel, cwd=root)
        assert single[0] == 0 and single[2] == b"" and single[1]  # (the single-FILE path has always exited 0)
        assert listed[1] == single[1], (rel, opts)
    single = xsgrep("that", "c_large.txt", cwd=root)[1]
    assert xsgrep("-H", "that", "c_large.txt", cwd=root)[1] == b"".join(b"c_large.txt:" + l + b"\n" for l in single.splitlines())
