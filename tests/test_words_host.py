"""The host side of XSG_LIST_WHOLE_WORDS (include/xsg.h: xsg_set_literals_opts) -- no GPU: tests/words_model.py pinned to
Python's re and, where there is one, to grep -w -F; the verify step under the sanitizers as a stand-alone program; what the
four new entry points refuse before they need a device; xsgrep's argument handling."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import literal_counts_model as LM
import set_model
import words_model as WM
import xsg

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
WW = xsg.LIST_WHOLE_WORDS


# ---- the model against Python's re ---------------------------------------------------------------------------------------------
class ReOccurrences(set_model.Occurrences):
    """set_model's walks over re.search: a backtracking leftmost-first engine on the expression of words_model.regex"""

    def __init__(self, data, literals, icase=False):
        self.d = set_model._bytes(data)
        self.rx = re.compile(WM.regex(literals), re.IGNORECASE if icase else 0)  # (bytes: ASCII letters only)

    def search(self, start):
        m = self.rx.search(self.d, start)  # (pos does not cut the text: the look-behind sees the byte in front of it)
        return None if m is None else m.span()


def re_counts(text: bytes, literals, icase):
    """admissible occurrences of every literal by itself, overlapping ones included: a zero-width match per position"""
    out = []
    for lit in literals:
        rx = re.compile(b"(?<![0-9A-Za-z_])(?=" + set_model.esc(lit) + b"(?![0-9A-Za-z_]))", re.IGNORECASE if icase else 0)
        out.append(sum(1 for _ in rx.finditer(text)))
    return out


def generated_case(seed: int):
    """-> (literals, text): a list with prefix pairs, a duplicate and literals with non-word edge bytes over an alphabet of
    word bytes, non-word bytes, both letter cases and bytes >= 0x80, and a text with the literals planted next to every
    kind of neighbour, at the chunk's first byte and as its last"""
    rng = np.random.Generator(np.random.PCG64(seed))
    alpha = [b"a", b"b", b"A", b"_", b"7", b" ", b"-", b".", b"\n", b"\xe9", b"\xc1"]
    lit_alpha = [a for a in alpha if a != b"\n"]
    n = int(rng.integers(2, 9))
    lits = []
    for _ in range(n):
        lits.append(b"".join(lit_alpha[int(k)] for k in rng.integers(0, len(lit_alpha), int(rng.integers(1, 5)))))
    lits.append(lits[0] + b"b")       # a prefix pair, the short one first ...
    lits.insert(0, lits[1] + b"a")    # ... and the long one first
    lits.append(lits[2])              # a duplicate
    lits.append(b"-" + lits[0][:2] + b".")  # non-word bytes at both of the literal's own edges
    pieces = []
    for _ in range(int(rng.integers(20, 60))):
        pieces.append(alpha[int(rng.integers(0, len(alpha)))] if rng.random() < 0.6 else lits[int(rng.integers(0, len(lits)))])
    text = lits[int(rng.integers(0, len(lits)))] + b"".join(pieces) + lits[int(rng.integers(0, len(lits)))]
    return lits, text


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
def test_the_model_is_a_backtracking_leftmost_first_engine(icase):
    hits = 0
    for seed in range(300):
        lits, text = generated_case(seed)
        model, engine = WM.Occurrences(text, lits, icase), ReOccurrences(text, lits, icase)
        assert model.spans() == engine.spans(), (seed, lits, text)
        assert model.line_walk() == engine.line_walk(), (seed, lits, text)
        assert model.lines_spans() == engine.lines_spans(), (seed, lits, text)
        assert WM.counts([text], lits, icase) == re_counts(text, lits, icase), (seed, lits, text)
        hits += len(model.spans())
        assert len(model.spans()) <= len(set_model.Occurrences(text, lits, icase).pos)
    assert hits > 600


def test_the_model_on_the_strings_of_the_header():
    assert WM.matches([b"abc ab abcd"], (b"ab", b"abc")) == ([b"abc", b"ab"], [0, 4], [3, 2])
    assert WM.matches([b"abc ab abcd"], (b"abc", b"ab")) == ([b"abc", b"ab"], [0, 4], [3, 2])
    assert WM.matches([b"a-x-b -x- -x-"], (b"-x-",))[1] == [6, 10]  # the neighbours decide, not the literal's own edges
    assert WM.counts([b"party art art", b"art"], (b"art", b"he", b"art")) == [3, 0, 3]
    assert LM.counts([b"party art art", b"art"], (b"art", b"he", b"art")) == [4, 0, 4]
    # a chunk's edges are word boundaries: the same bytes as one chunk and cut in two
    assert WM.counts([b"the", b"the"], (b"the",)) == [2] and WM.counts([b"thethe"], (b"the",)) == [0]
    # every byte >= 0x80 and '\n' are no word bytes; ignore-case does not change the set
    assert WM.counts([b"\xe9the\xc1 K\nthe\n_the the_ THE"], (b"the",), True) == [3]
    rows = WM.matrix([b"a b", b"ab", b""], (b"a", b"b", b"ab"))
    assert rows == [[1, 1, 0], [0, 0, 1], [0, 0, 0]] and WM.chunks_with(rows, 3) == [1, 1, 1]
    assert WM.csr([b"a b", b"ab", b""], (b"a", b"b", b"ab")) == ([0, 2, 3, 3], [0, 1, 2], [1, 1, 1])


# ---- grep -w -F ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
def test_line_selection_is_that_of_grep(tmp_path, icase):
    """LC_ALL=C grep -a -w -F -f: the selected lines and -c.  (GNU grep retries a shorter or later match of a line when the
    one it found fails the word test, so the SET OF LINES is the one the definition gives; no case disagreed.)"""
    grep = shutil.which("grep")
    if grep is None:
        pytest.skip("no grep on this machine")
    for seed in range(60):
        lits, text = generated_case(1000 + seed)
        lits = [l for l in lits if b"\0" not in l]
        text = text.replace(b"\0", b" ") + b"\n"
        (tmp_path / "words.txt").write_bytes(b"\n".join(lits) + b"\n")
        (tmp_path / "text.txt").write_bytes(text)
        args = [grep, "-a", "-w", "-F"] + (["-i"] if icase else []) + ["-f", str(tmp_path / "words.txt")]
        env = {"LC_ALL": "C", "PATH": "/usr/bin:/bin"}
        r = subprocess.run(args + [str(tmp_path / "text.txt")], capture_output=True, env=env, timeout=60)
        assert r.returncode in (0, 1), r.stderr
        want = WM.all_modes([text], lits, icase)
        assert r.stdout == b"".join(l + b"\n" for l in want["lines"]), (seed, lits, text)
        c = subprocess.run(args + ["-c", str(tmp_path / "text.txt")], capture_output=True, env=env, timeout=60)
        assert int(c.stdout) == want["count_lines"] == len(want["lines"]), (seed, lits, text)


# ---- the verify step under the sanitizers ----------------------------------------------------------------------------------------
def test_the_word_test_under_the_sanitizers(tmp_path):
    """tests/cpp/words_selftest.cpp includes csrc/xsg_set.h/.cpp: a stand-alone program on chunks of exactly L heap bytes,
    p == 0 and p + len == L included -- a read outside the chunk is a report; nothing is loaded into Python"""
    exe = tmp_path / "words_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "words_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "words_selftest ok" in r.stdout


# ---- refusals that need no device -----------------------------------------------------------------------------------------------
NEW = ("xsg_set_literals_opts", "xsg_host_searcher_create_list_opts", "xsg_literal_counter_create_opts", "xsg_job_start_list")


def test_the_binding_and_the_header_agree():
    header = (ROOT / "include" / "xsg.h").read_text()
    for name in NEW:
        assert name in xsg.EXPORTS and name + "(" in header
    assert "#define XSG_LIST_WHOLE_WORDS 0x1u" in header and WW == 1
    assert xsg.load().xsg_abi_version() == 4
    assert C.sizeof(xsg.JobOpts) == 56  # xsg_job_opts did not grow: the option has an entry point of its own


def last_error():
    return xsg.load().xsg_last_error().decode()


def job_opts(**kw):
    o = xsg.JobOpts()
    xsg.load().xsg_job_opts_init(C.byref(o))
    o.mode = xsg.COUNT_LINES
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("bad", [0x2, 0x3, 0x80, 0x80000000])
def test_an_unknown_list_flag_is_refused_by_every_new_entry_point(tmp_path, bad):
    lib, lst, h = xsg.load(), b"art\nparty", C.c_void_p()
    (tmp_path / "t.txt").write_bytes(b"art\n")
    path = str(tmp_path / "t.txt").encode()
    calls = {
        "xsg_set_literals_opts": lambda: lib.xsg_set_literals_opts(None, lst, len(lst), 0, bad),
        "xsg_host_searcher_create_list_opts": lambda: lib.xsg_host_searcher_create_list_opts(0, lst, len(lst), 0, bad, 1, C.byref(h)),
        "xsg_literal_counter_create_opts": lambda: lib.xsg_literal_counter_create_opts(0, lst, len(lst), 0, bad, C.byref(h)),
        "xsg_job_start_list": lambda: lib.xsg_job_start_list(lst, len(lst), bad, path, None, C.byref(job_opts()), C.byref(h)),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() == xsg.EINVAL, name
        assert "unknown list flags" in last_error() and not h.value, (name, last_error())


def test_job_start_list_reads_struct_size_as_job_start_does(tmp_path):
    """both take the 56-byte structure and the 48-byte one of a program built before pattern_is_list, and refuse every other
    size; behind that check a file that does not exist is XSG_EIO from both (no device is needed to get there)"""
    lib, lst, h = xsg.load(), b"art\nparty", C.c_void_p()
    missing = str(tmp_path / "missing.txt").encode()
    for size, want, word in ((56, xsg.EIO, "missing.txt"), (48, xsg.EIO, "missing.txt"), (0, xsg.EINVAL, "struct_size"),
                             (40, xsg.EINVAL, "struct_size"), (52, xsg.EINVAL, "struct_size"), (64, xsg.EINVAL, "struct_size")):
        for flags in (0, WW):
            o = job_opts(struct_size=size)
            assert lib.xsg_job_start_list(lst, len(lst), flags, missing, None, C.byref(o), C.byref(h)) == want, (size, flags)
            assert word in last_error() and not h.value, (size, last_error())
        o = job_opts(struct_size=size, pattern_is_list=1)
        assert lib.xsg_job_start(lst, len(lst), missing, None, C.byref(o), C.byref(h)) == want, size
        assert word in last_error() and not h.value, (size, last_error())
    assert lib.xsg_job_start_list(lst, len(lst), WW, missing, None, None, C.byref(h)) == xsg.EINVAL


def test_job_start_list_forces_the_list_reading(tmp_path):
    lib, h = xsg.load(), C.c_void_p()
    missing = str(tmp_path / "missing.txt").encode()
    for is_list in (0, 1):  # whatever pattern_is_list says: an empty literal is refused as one, XSG_FLAG_REGEX as for any list
        o = job_opts(pattern_is_list=is_list)
        assert lib.xsg_job_start_list(b"a\n\nb", 4, WW, missing, None, C.byref(o), C.byref(h)) == xsg.EINVAL
        assert "empty literal" in last_error()
        o = job_opts(pattern_is_list=is_list, pattern_flags=xsg.FLAG_REGEX)
        assert lib.xsg_job_start_list(b"a|b", 3, WW, missing, None, C.byref(o), C.byref(h)) == xsg.EINVAL
        assert "XSG_FLAG_REGEX" in last_error()
        assert o.pattern_is_list == is_list  # the caller's structure is read, never written
    o = job_opts()
    assert lib.xsg_job_start(b"a\n\nb", 4, missing, None, C.byref(o), C.byref(h)) == xsg.EIO  # (a literal with newlines: accepted)


# ---- xsgrep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [
    (["-w", "art", "FILE"], "needs -F"),
    (["-w", "-e", "art", "-e", "he", "FILE"], "needs -F"),
    (["-E", "-w", "a.t", "FILE"], "needs -F"),
    (["-wc", "art", "FILE"], "needs -F"),
    (["--word-regexp", "art", "-"], "needs -F"),
    (["-F", "-w", "-x", "art", "FILE"], "excludes -x"),
    (["-F", "-w", "--count-each", "-x", "art", "FILE"], "excludes -x"),
    (["-F", "-w", "", "FILE"], "empty pattern"),
])
def test_xsgrep_w_is_refused_before_a_device_is_needed(args, word):
    """never a silent substring search: one line on stderr, exit status 2"""
    r = subprocess.run([str(XSGREP), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert r.stderr.count("\n") == 1


def test_xsgrep_documents_w():
    r = subprocess.run([str(XSGREP), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-w, --word-regexp" in r.stdout and "[-w]" in r.stdout
