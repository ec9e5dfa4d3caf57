"""File sets without a GPU: the HIP-free planner under the sanitizers, and what xsg_fileset_start and xsgrep refuse
before a device is touched.  What a file set reports is tests/test_gpu_fileset.py's business.

Without the feature every test here fails: on the missing header, the missing symbol, or "unexpected argument"."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

import xsg

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"


def test_the_planner_under_the_sanitizers(tmp_path):
    """tests/cpp/fileset_selftest.cpp includes csrc/xsg_fileset.h: random size lists against a brute-force plan, 16-byte
    packing, no file split across batches, the batch_bytes and 2^20 caps, files over chunk_bytes set aside, the attribution
    of rows across batch cuts.  A stand-alone program; nothing is loaded into Python."""
    exe = tmp_path / "fileset_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(ROOT / "tests" / "cpp" / "fileset_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "fileset_selftest ok" in r.stdout


def start(pattern=b"that", paths=(b"/nonexistent/a",), npaths=None, **fields):
    lib = xsg.load()
    o = xsg.FileSetOpts()
    lib.xsg_fileset_opts_init(C.byref(o))
    for k, v in fields.items():
        setattr(o, k, v)
    arr = (C.c_char_p * max(len(paths), 1))(*paths) if paths is not None else None
    h = C.c_void_p()
    rc = lib.xsg_fileset_start(pattern, len(pattern), arr, len(paths) if npaths is None else npaths, C.byref(o), C.byref(h))
    assert not h.value or rc == xsg.OK
    if h.value:
        lib.xsg_fileset_destroy(h)
    return rc, lib.xsg_last_error().decode()


def test_opts_init_and_layout():
    o = xsg.FileSetOpts()
    xsg.load().xsg_fileset_opts_init(C.byref(o))
    assert C.sizeof(o) == 48 and o.struct_size == 48
    assert (o.mode, o.pattern_flags, o.pattern_is_list, o.list_flags, o.device, o.num_readers, o.batch_bytes, o.chunk_bytes) == \
        (xsg.COUNT_LINES, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("kw,word", [
    (dict(paths=None, npaths=3), "paths is null"),
    (dict(struct_size=40), "struct_size"),
    (dict(mode=7), "mode"),
    (dict(batch_bytes=1 << 20, chunk_bytes=2 << 20), "batch_bytes"),
    (dict(batch_bytes=1 << 20), "batch_bytes"),  # (below the default chunk_bytes of 16 MiB)
    (dict(pattern=b""), "pattern"),
    (dict(list_flags=0x2, pattern_is_list=1), "unknown list flags"),
    (dict(list_flags=xsg.LIST_ALL_OF | 0x80, pattern_is_list=1), "unknown list flags"),
    (dict(list_flags=xsg.LIST_WHOLE_WORDS), "pattern_is_list"),
    (dict(num_readers=-1), "num_readers"),
])
def test_start_refusals_that_need_no_device(kw, word):
    rc, msg = start(**kw)
    assert rc == xsg.EINVAL and word in msg, (rc, msg)


def test_start_refuses_what_the_searches_would():
    assert start(mode=xsg.MATCH_BYTE_OFFSETS, pattern_flags=xsg.FLAG_INVERT)[0] == xsg.ENOTSUP
    assert start(pattern=b"a\nb", pattern_is_list=1, list_flags=xsg.LIST_ALL_OF, mode=xsg.MATCHES)[0] == xsg.ENOTSUP
    assert start(pattern=b"a\\sb", pattern_flags=xsg.FLAG_REGEX, mode=xsg.LINES)[0] == xsg.ENOTSUP
    assert start(pattern=b"a(b", pattern_flags=xsg.FLAG_REGEX)[0] != xsg.OK


@pytest.mark.parametrize("args,word", [
    (["-r", "that", "-"], "stdin"),
    (["that", "a.txt", "-"], "stdin"),
    (["-F", "--count-each", "that", "a.txt", "b.txt"], "--count-each"),
    (["-F", "--find-each", "that", "a.txt", "b.txt"], "--find-each"),
    (["-m", "a.meta", "that", "a.txt", "b.txt"], "-m"),
    (["-r", "-m", "a.meta", "that", "a.txt"], "-m"),
    (["-r", "-F", "-e", "a", "-e", "b", "DIR", "MORE"], "unexpected argument 'MORE'"),  # -e / -f: one FILE operand, as ever
    (["-lL", "that", "a.txt"], "-l and -L"),                     # the bundle was read as -l -L ...
    (["-rH", "--no-filename", "that", "a.txt"], "--no-filename"),  # ... and this one as -r -H
])
def test_xsgrep_refusals_before_a_device_is_needed(args, word):
    r = subprocess.run([str(XSGREP), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert r.stderr.count("\n") == 1


def test_xsgrep_documents_the_mode():
    r = subprocess.run([str(XSGREP), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for word in ("--recursive", "FILE FILE...", "--no-filename", "PATH-"):
        assert word in r.stdout, word
    src = (ROOT / "tools" / "xsgrep.cpp").read_text()
    assert "-rl" in src and "PATH-" in src
