"""The host side of the row limit (include/xsg.h: xsg_set_max_count, xsg_job_start_max_count, xsg_fileset_start_max_count,
xsg_host_searcher_set_max_count) -- no GPU: the header's new names against the binding, the structures that did not grow, the
ordered publisher's budget in tests/cpp/max_count_pipeline.cpp (built here, once plainly and once under ThreadSanitizer as
a program of its own, against tests/cpp/device_double.cpp), what the start calls refuse before they need a device, and
xsgrep's argument handling.

Without the feature every test fails: the library exports none of the four names and xsgrep knows neither option."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import pytest

import xsg
from test_sanitizers import _no_aslr_prefix

ROOT = Path(__file__).resolve().parents[1]
XSGREP = ROOT / "tools" / "build" / "xsgrep"
CSRC = ROOT / "x-search_amd" / "csrc"
NEW = ("xsg_set_max_count", "xsg_job_start_max_count", "xsg_fileset_start_max_count", "xsg_host_searcher_set_max_count")
# tests/cpp/Makefile: SAN_FLAGS, SAN_SRCS with this file's driver in the place of pipeline_sanitize.cpp
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             f"-I{ROOT / 'include'}"]
SOURCES = [ROOT / "tests" / "cpp" / "max_count_pipeline.cpp", ROOT / "tests" / "cpp" / "device_double.cpp", CSRC / "xsg_meta.cpp",
           CSRC / "xsg_job.cpp", CSRC / "xsg_hostsearch.cpp"]


def test_the_header_the_exports_and_the_binding_agree():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "xsg.h").read_text(), flags=re.S)
    lib = C.CDLL(str(xsg.lib_path()))
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in xsg.EXPORTS and hasattr(lib, name), name
    assert re.search(r"int xsg_set_max_count\(xsg_ctx\* ctx, uint64_t max_count\);", header)
    assert re.search(r"int xsg_host_searcher_set_max_count\(xsg_host_searcher\* hs, uint64_t max_count\);", header)
    assert xsg.load().xsg_abi_version() == 4
    # the structures did not grow: the number travels through entry points of its own
    assert C.sizeof(xsg.JobOpts) == 56 and C.sizeof(xsg.FileSetOpts) == 48
    o, f = xsg.JobOpts(), xsg.FileSetOpts()
    xsg.load().xsg_job_opts_init(C.byref(o))
    xsg.load().xsg_fileset_opts_init(C.byref(f))
    assert (o.struct_size, f.struct_size) == (56, 48)


def last_error():
    return xsg.load().xsg_last_error().decode()


def test_a_limit_without_a_context_or_a_searcher_is_an_argument_error():
    lib = xsg.load()
    assert lib.xsg_set_max_count(None, 3) == xsg.EINVAL
    assert lib.xsg_host_searcher_set_max_count(None, 3) == xsg.EINVAL


def test_the_start_calls_refuse_before_they_need_a_device(tmp_path):
    lib, h = xsg.load(), C.c_void_p()
    (tmp_path / "t.txt").write_bytes(b"art\n")
    path = str(tmp_path / "t.txt").encode()
    o = xsg.JobOpts()
    lib.xsg_job_opts_init(C.byref(o))
    o.mode = xsg.LINES
    # list flags belong to a list
    assert lib.xsg_job_start_max_count(b"art", 3, xsg.LIST_WHOLE_WORDS, 2, path, None, C.byref(o), C.byref(h)) == xsg.EINVAL
    assert "pattern_is_list" in last_error() and not h.value
    assert lib.xsg_job_start_max_count(b"art", 3, 0x2, 2, path, None, C.byref(o), C.byref(h)) == xsg.EINVAL
    assert lib.xsg_job_start_max_count(b"art", 3, 0, 2, path, None, None, C.byref(h)) == xsg.EINVAL
    # context with a limit: refused from both start calls, and the message says why
    o.pattern_flags = xsg.flag_context(1, 2)
    assert lib.xsg_job_start_max_count(b"art", 3, 0, 2, path, None, C.byref(o), C.byref(h)) == xsg.ENOTSUP
    assert "XSG_FLAG_CONTEXT" in last_error() and "file order" in last_error() and not h.value
    f = xsg.FileSetOpts()
    lib.xsg_fileset_opts_init(C.byref(f))
    f.mode, f.pattern_flags = xsg.LINES, xsg.flag_context(0, 1)
    arr = (C.c_char_p * 1)(path)
    assert lib.xsg_fileset_start_max_count(b"art", 3, arr, 1, C.byref(f), 2, C.byref(h)) == xsg.ENOTSUP
    assert "XSG_FLAG_CONTEXT" in last_error() and not h.value
    f.struct_size = 40
    assert lib.xsg_fileset_start_max_count(b"art", 3, arr, 1, C.byref(f), 2, C.byref(h)) == xsg.EINVAL


@pytest.fixture(scope="module")
def oracle_objects(tmp_path_factory):
    d = tmp_path_factory.mktemp("max_count_build")
    out = {}
    for name, extra in (("plain", []), ("tsan", ["-fsanitize=thread"])):
        obj = d / f"oracle_{name}.o"
        subprocess.check_call(["gcc", "-O1", "-g", "-mavx2", *extra, "-c", str(ROOT / "oracle" / "xs_oracle.c"), "-o", str(obj)])
        out[name] = obj
    return d, out


@pytest.mark.parametrize("name,extra", [("plain", []), ("tsan", ["-fsanitize=thread"])])
def test_the_publishers_budget_in_a_program_of_its_own(oracle_objects, tmp_path, name, extra):
    """the cut, the clamped count sequence, the early stop and 200 joins and destroys while readers run; nothing is loaded
    into Python, and the ThreadSanitizer build is its own executable"""
    d, objs = oracle_objects
    exe = d / f"max_count_pipeline_{name}"
    subprocess.check_call(["g++", *SAN_FLAGS, *extra, *map(str, SOURCES), str(objs[name]), "-o", str(exe), "-ldl"])
    e = dict(os.environ)
    e["TSAN_OPTIONS"] = "halt_on_error=1 second_deadlock_stack=1"
    e["XSG_READ_PIECE"] = "65536"
    e.pop("XS_DEVICES", None)
    prefix = _no_aslr_prefix() if name == "tsan" else []
    r = subprocess.run(prefix + [str(exe), str(tmp_path)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ThreadSanitizer" not in r.stderr and "CHECK failed" not in r.stderr, r.stderr[-4000:]
    assert "max count pipeline: ok" in r.stdout


# ---- xsgrep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,word", [
    (["--max-count=x", "art", "FILE"], "in digits"),
    (["--max-count=", "art", "FILE"], "in digits"),
    (["--max-count=-1", "art", "FILE"], "in digits"),
    (["--max-count", "1e3", "art", "FILE"], "in digits"),
    (["--max-count=2", "-o", "art", "FILE"], "excludes -o"),
    (["--max-count=2", "-A", "1", "art", "FILE"], "excludes -A, -B and -C"),
    (["--max-count=2", "-B", "1", "art", "FILE"], "excludes -A, -B and -C"),
    (["--max-count", "2", "-C", "1", "-c", "art", "FILE"], "excludes -A, -B and -C"),
    (["-F", "--max-count=2", "--count-each", "art", "FILE"], "excludes --count-each"),
    (["-F", "--max-count=2", "--find-each", "art", "FILE"], "excludes --find-each"),
    (["-F", "-q", "--count-each", "art", "FILE"], "-q excludes"),
    (["-F", "--quiet", "--find-each", "art", "-"], "-q excludes"),
    (["--max-count=2", "-o", "art", "A", "B"], "excludes -o"),
    (["-r", "--max-count=2", "-C", "3", "art", "DIR"], "excludes -A, -B and -C"),
])
def test_xsgrep_refuses_before_a_device_is_needed(args, word):
    r = subprocess.run([str(XSGREP), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert r.stderr.count("\n") == 1


@pytest.mark.parametrize("args", [["--max-count=0", "art", "FILE"], ["--max-count", "0", "-c", "art", "-"],
                                  ["-r", "-l", "--max-count=0", "art", "DIR"], ["-q", "--max-count=0", "art", "A", "B"]])
def test_xsgrep_max_count_zero_selects_nothing_and_touches_no_device(args):
    r = subprocess.run([str(XSGREP), *args], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "")


def test_xsgrep_documents_the_options():
    r = subprocess.run([str(XSGREP), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--max-count=N" in r.stdout and "-q, --quiet" in r.stdout
    assert "-m METAFILE" in r.stdout  # -m stays the metafile
