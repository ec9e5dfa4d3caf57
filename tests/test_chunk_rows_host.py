"""xsg_result_chunk_ptr without a GPU: the declaration, the export, the Python binding and the one refusal that needs no
shard.  What the rows hold is tests/test_gpu_chunk_rows.py's business.

Without the feature every test here fails on the missing symbol."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import xsg

ROOT = Path(__file__).resolve().parents[1]


def test_declared_exported_and_bound():
    header = (ROOT / "include" / "xsg.h").read_text()
    assert re.search(r"^int xsg_result_chunk_ptr\(xsg_shard\* shard, uint64_t\* chunk_ptr, uint64_t cap_rows, uint64_t\* byte_ptr\);$",
                     header, re.M)
    assert re.search(r"^#define XSG_ABI_VERSION 4$", header, re.M), "the accessor joined: the version stays"
    assert re.search(r"xsg_result_chunk_ptr[^;]* joined;", header), "the list of what joined version 4"
    assert "xsg_result_chunk_ptr" in xsg.EXPORTS
    lib = C.CDLL(str(xsg.lib_path()))
    assert hasattr(lib, "xsg_result_chunk_ptr")
    assert callable(getattr(xsg.Shard, "result_chunk_ptr"))


def test_a_null_shard_is_refused():
    lib = xsg.load()
    rows = np.zeros(1, dtype=np.uint64)
    assert lib.xsg_result_chunk_ptr(None, C.c_void_p(rows.ctypes.data), 1, None) == xsg.EINVAL
    assert b"shard" in lib.xsg_last_error()
