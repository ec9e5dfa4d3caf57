"""The host side of XSG_LIST_ALL_OF (include/xsg.h) -- no GPU: tests/all_of_model.py pinned two ways, to the intersection
of the line lists of the k lists of one (set_model / words_model, the identity the header states) and to Python's re, one
lookup per literal per line; set_mask_at under the sanitizers as a stand-alone program; what the entry points refuse before
they need a device; xsgrep's argument handling."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import all_of_model as AM
import set_model
import words_model as WM
import xsg

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
WW, ALL = xsg.LIST_WHOLE_WORDS, xsg.LIST_ALL_OF


def generated_case(seed: int):
    """-> (literals, blocks): 2 to 5 literals with a covered pair, an overlapping pair and a duplicate over a small alphabet
    (both letter cases, word and non-word bytes, a byte >= 0x80), and 1 to 4 chunks of short lines in which every literal is
    planted often enough for conjunctions to hold -- empty lines, empty chunks and an unterminated last line among them"""
    rng = np.random.Generator(np.random.PCG64(seed))
    alpha = [b"a", b"b", b"A", b"_", b" ", b"-", b"\xe9"]
    lits = [b"".join(alpha[int(k)] for k in rng.integers(0, len(alpha), int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 4)))]
    lits.append(lits[0] + b"b")          # lits[0] is covered by it
    if rng.random() < 0.5:
        lits.append(lits[0][-1:] + b"a")  # overlaps the end of lits[0]
    if rng.random() < 0.5:
        lits.append(lits[0])             # a duplicate: one requirement
    blocks = []
    for _ in range(int(rng.integers(1, 5))):
        if rng.random() < 0.15:
            blocks.append(b"")
            continue
        lines = []
        for _ in range(int(rng.integers(1, 12))):
            pieces = []
            for _ in range(int(rng.integers(0, 12))):
                pieces.append(alpha[int(rng.integers(0, len(alpha)))] if rng.random() < 0.3 else lits[int(rng.integers(0, len(lits)))])
            lines.append((b"", b" ", b"-")[int(rng.integers(0, 3))].join(pieces))  # (apart, so that whole words occur too)
        text = b"\n".join(lines)
        blocks.append(text if rng.random() < 0.4 else text + b"\n")
    return lits, blocks


def intersection(blocks, lits, icase, words):
    """the header's identity: the lines every list of one reports, as sorted global line starts"""
    model = WM if words else set_model
    sets = [set(model.all_modes(blocks, (l,), icase)["line_byte_offsets"]) for l in lits]
    return sorted(set.intersection(*sets))


def by_re(blocks, lits, icase, words):
    """Python's re, one lookup per literal per line.  The line is searched INSIDE its chunk (pos / endpos), so that the
    look-behind sees the byte in front of the line -- a newline or nothing -- and the look-ahead is cut at the line's end,
    which is a newline or the chunk's end: both are word boundaries"""
    out, goff = [], 0
    for b in blocks:
        for lo, hi, _ in AM.chunk_lines(b):
            ok = True
            for l in lits:
                body = set_model.esc(l)
                rx = re.compile(b"(?<![0-9A-Za-z_])(?:" + body + b")(?![0-9A-Za-z_])" if words else body, re.IGNORECASE if icase else 0)
                ok = ok and rx.search(b, lo, hi) is not None
            if ok:
                out.append(goff + lo)
        goff += len(b)
    return out


@pytest.mark.parametrize("words", [False, True], ids=["substrings", "words"])
@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
def test_the_model_is_the_intersection_and_what_re_finds(icase, words):
    selected = total = 0
    for seed in range(250):
        lits, blocks = generated_case(seed)
        got = AM.all_modes(blocks, lits, icase, words)
        assert got["line_byte_offsets"] == intersection(blocks, lits, icase, words), (seed, lits, blocks)
        assert got["line_byte_offsets"] == by_re(blocks, lits, icase, words), (seed, lits, blocks)
        assert got["count_lines"] == len(got["line_byte_offsets"]) == sum(got["chunk_counts"])
        inv = AM.all_modes(blocks, lits, icase, words, invert=True)
        nlines = sum(len(AM.chunk_lines(b)) for b in blocks)
        assert sorted(got["line_byte_offsets"] + inv["line_byte_offsets"]) == sorted(
            sum(([g + lo for lo, _, _ in AM.chunk_lines(b)] for g, b in zip(np.cumsum([0] + [len(b) for b in blocks[:-1]]).tolist(), blocks)), []))
        assert got["count_lines"] + inv["count_lines"] == nlines
        selected += got["count_lines"]
        total += nlines
    assert 100 < selected < total - 100, (selected, total)  # the cases select some lines and leave some


def test_the_model_on_the_strings_of_the_header():
    sel = lambda text, lits, **kw: AM.all_modes([text], lits, **kw)["line_byte_offsets"]
    assert sel(b"abc\nab\n", (b"ab", b"abc")) == [0]               # covered occurrences serve different literals
    assert sel(b"aaa\naa\n", (b"aa", b"aaa")) == [0]
    assert sel(b"abcd\nab cd\nbc\n", (b"abc", b"bcd")) == [0]      # overlapping ones too
    assert sel(b"a\nb\nab\n", (b"a", b"b", b"a")) == [4]           # duplicates are one requirement
    assert sel(b"x\n\ny", (b"x",)) == [0] and sel(b"x\n\ny", (b"y",)) == [3]  # a list of one; an unterminated last line
    assert AM.all_modes([b"x\n\ny"], (b"y",))["lines"] == []       # ... which xs::lines does not hand out
    assert AM.all_modes([b"a", b"b\n"], (b"a", b"b"))["count_lines"] == 0  # a chunk's edges are line edges
    assert sel(b"the he\nthe\n", (b"he", b"the"), words=True) == [0]
    assert AM.all_modes([b"he", b"the"], (b"he",), words=True)["chunk_counts"] == [1, 0]  # `he` at a chunk's edges, inside `the`
    assert sel(b"ERROR timeout\nerror TIMEOUT db01\n", (b"error", b"db01", b"Timeout"), icase=True) == [14]
    assert AM.all_modes([b"", b"\n", b"a\n"], (b"a",), invert=True)["chunk_counts"] == [0, 1, 0]
    got = AM.all_modes([b"a b\nb\n", b"b a\n"], (b"a", b"b"), global_offsets=[100, 1000], line_bases=[7, 70])
    assert (got["line_byte_offsets"], got["line_indices"], got["lines"]) == ([100, 1000], [7, 70], [b"a b", b"b a"])


# ---- set_mask_at under the sanitizers -----------------------------------------------------------------------------------------------
def test_set_mask_at_under_the_sanitizers(tmp_path):
    """tests/cpp/all_of_selftest.cpp includes csrc/xsg_set.h/.cpp: a stand-alone program on chunks of exactly L heap bytes
    -- a read outside the chunk is a report; nothing is loaded into Python"""
    exe = tmp_path / "all_of_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "all_of_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "all_of_selftest ok" in r.stdout


# ---- what needs no device ------------------------------------------------------------------------------------------------------------
def last_error():
    return xsg.load().xsg_last_error().decode()


def job_opts(**kw):
    o = xsg.JobOpts()
    xsg.load().xsg_job_opts_init(C.byref(o))
    o.mode = xsg.COUNT_LINES
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_the_binding_and_the_header_agree():
    header = (ROOT / "include" / "xsg.h").read_text()
    assert "#define XSG_LIST_ALL_OF 0x4u" in header and ALL == 4
    assert "#define XSG_MAX_ALL_OF_LITERALS 64u" in header and xsg.MAX_ALL_OF_LITERALS == 64
    assert "#define XSG_LIST_WHOLE_WORDS 0x1u" in header and WW == 1
    assert xsg.load().xsg_abi_version() == 4
    assert C.sizeof(xsg.JobOpts) == 56  # xsg_job_opts did not grow


@pytest.mark.parametrize("flags", [ALL, ALL | WW])
def test_the_bit_is_known_where_whole_words_is(tmp_path, flags):
    """past the list-flag check: a null context and a missing file are what is refused, not the flag"""
    lib, lst, h = xsg.load(), b"art\nparty", C.c_void_p()
    assert lib.xsg_set_literals_opts(None, lst, len(lst), 0, flags) == xsg.EINVAL and "ctx is null" in last_error()
    missing = str(tmp_path / "missing.txt").encode()
    assert lib.xsg_job_start_list(lst, len(lst), flags, missing, None, C.byref(job_opts()), C.byref(h)) == xsg.EIO
    assert "missing.txt" in last_error() and not h.value
    for bad in (0x2, 0x3, 0x8, ALL | 0x2, ALL | 0x80000000):  # (0x2 stays unknown: tests/test_words_host.py)
        assert lib.xsg_set_literals_opts(None, lst, len(lst), 0, bad) == xsg.EINVAL and "unknown list flags" in last_error()
        assert lib.xsg_job_start_list(lst, len(lst), bad, missing, None, C.byref(job_opts()), C.byref(h)) == xsg.EINVAL
        assert "unknown list flags" in last_error()


@pytest.mark.parametrize("flags", [ALL, ALL | WW])
def test_counter_and_finder_keep_refusing_the_bit(flags):
    lib, h = xsg.load(), C.c_void_p()
    assert lib.xsg_literal_counter_create_opts(0, b"a\nb", 3, 0, flags, C.byref(h)) == xsg.EINVAL
    assert "unknown list flags" in last_error() and not h.value
    assert lib.xsg_literal_finder_create_opts(0, b"a\nb", 3, 0, flags, C.byref(h)) == xsg.EINVAL
    assert "unknown list flags" in last_error() and not h.value


def test_a_job_refuses_the_match_tags_and_a_long_list_at_its_start(tmp_path):
    lib, h = xsg.load(), C.c_void_p()
    missing = str(tmp_path / "missing.txt").encode()  # (the refusals come before the file is opened)
    for mode in (xsg.COUNT_MATCHES, xsg.MATCH_BYTE_OFFSETS, xsg.MATCHES):
        o = job_opts(mode=mode)
        assert lib.xsg_job_start_list(b"a\nb", 3, ALL, missing, None, C.byref(o), C.byref(h)) == xsg.ENOTSUP, mode
        assert "XSG_LIST_ALL_OF" in last_error() and not h.value
        assert lib.xsg_job_start_list(b"a\nb", 3, WW, missing, None, C.byref(o), C.byref(h)) == xsg.EIO, mode
    for mode in (xsg.COUNT_LINES, xsg.LINE_BYTE_OFFSETS, xsg.LINE_INDICES, xsg.LINES):
        assert lib.xsg_job_start_list(b"a\nb", 3, ALL, missing, None, C.byref(job_opts(mode=mode)), C.byref(h)) == xsg.EIO, mode
    lst64 = b"\n".join(b"w%02d" % j for j in range(64))
    lst65 = lst64 + b"\nw64"
    assert lib.xsg_job_start_list(lst64, len(lst64), ALL, missing, None, C.byref(job_opts()), C.byref(h)) == xsg.EIO
    assert lib.xsg_job_start_list(lst65, len(lst65), ALL, missing, None, C.byref(job_opts()), C.byref(h)) == xsg.EINVAL
    assert "at most 64" in last_error() and not h.value
    assert lib.xsg_job_start_list(lst65, len(lst65), WW, missing, None, C.byref(job_opts()), C.byref(h)) == xsg.EIO


# ---- xsgrep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [
    (["--all-of", "-e", "a", "-e", "b", "FILE"], "needs -F"),
    (["--all-of", "a", "FILE"], "needs -F"),
    (["-E", "--all-of", "a.b", "FILE"], "needs -F"),
    (["-F", "--all-of", "-o", "-e", "a", "-e", "b", "FILE"], "excludes -o"),
    (["-F", "--all-of", "-x", "a", "FILE"], "excludes -x"),
    (["-F", "--all-of", "--count-each", "-e", "a", "-e", "b", "FILE"], "excludes --count-each"),
    (["-F", "--all-of", "--find-each", "-e", "a", "-e", "b", "-"], "excludes --find-each"),
    (["-F", "--all-of", "", "FILE"], "empty pattern"),
    (["-F", "--all-of"] + sum((["-e", "w%02d" % j] for j in range(65)), []) + ["FILE"], "at most 64"),
])
def test_xsgrep_all_of_is_refused_before_a_device_is_needed(args, word):
    """never a silent any-of search: one line on stderr, exit status 2"""
    r = subprocess.run([str(XSGREP), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert r.stderr.count("\n") == 1


def test_xsgrep_documents_all_of():
    r = subprocess.run([str(XSGREP), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--all-of" in r.stdout and "-F --all-of [-c]" in r.stdout
