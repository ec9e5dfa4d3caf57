"""Where the words of the per-tile sketch live (x-search_amd/csrc/xsg_sketch.h: sketch_index, sketch_alloc_words): the one
definition that k_sketch_build, k_sketch_sample and k_sketch_select index through, compiled here with g++ as
tests/sketch_model.py compiles the rest of the header.  Word-major inside groups of 64 tiles, whole groups allocated."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
WORDS = 128
GROUP = 64

HELPER = r"""
#include "xsg_sketch.h"
using namespace xsg;
extern "C" {
uint32_t skl_words() { return kSketchWords; }
uint32_t skl_group() { return kSketchGroup; }
uint64_t skl_alloc(uint64_t ntiles) { return sketch_alloc_words(ntiles); }
uint64_t skl_index(uint64_t tile, uint32_t word) { return sketch_index(tile, word); }
void skl_all(uint64_t ntiles, uint64_t* out) {
  for (uint64_t t = 0; t < ntiles; ++t)
    for (uint32_t w = 0; w < kSketchWords; ++w) out[t * kSketchWords + w] = sketch_index(t, w);
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("sketch_layout")
    src = d / "sketch_layout.cpp"
    src.write_text(HELPER)
    so = d / "libsketch_layout.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                        f"-I{ROOT / 'x-search_amd' / 'csrc'}", str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    lib.skl_words.restype = lib.skl_group.restype = C.c_uint32
    lib.skl_alloc.restype = lib.skl_index.restype = C.c_uint64
    lib.skl_alloc.argtypes = [C.c_uint64]
    lib.skl_index.argtypes = [C.c_uint64, C.c_uint32]
    lib.skl_all.argtypes = [C.c_uint64, C.c_void_p]
    assert (lib.skl_words(), lib.skl_group()) == (WORDS, GROUP)
    return lib


def slots(lib, ntiles):
    out = np.zeros((ntiles, WORDS), dtype=np.uint64)
    lib.skl_all(ntiles, out.ctypes.data)
    return out


@pytest.mark.parametrize("ntiles", (1, 63, 64, 65, 127, 128, 129, 1000))
def test_index_is_a_bijection_below_the_allocation(lib, ntiles):
    alloc = lib.skl_alloc(ntiles)
    groups = (ntiles + GROUP - 1) // GROUP
    assert alloc == groups * GROUP * WORDS  # whole groups, nothing more
    s = slots(lib, ntiles)
    assert int(s.max()) < alloc
    assert np.unique(s).size == ntiles * WORDS  # (tile, word) -> distinct slots
    # the tiles that do not exist in the last group take exactly the slots that are left
    full = slots(lib, groups * GROUP)
    assert np.array_equal(np.sort(full.ravel()), np.arange(alloc, dtype=np.uint64))
    assert np.array_equal(full[:ntiles], s)


@pytest.mark.parametrize("ntiles", (1, 63, 64, 65, 127, 128, 129, 1000))
def test_a_word_of_64_consecutive_tiles_is_64_consecutive_dwords(lib, ntiles):
    s = slots(lib, ntiles)
    for k in range((ntiles + GROUP - 1) // GROUP):
        g = s[k * GROUP:(k + 1) * GROUP]  # the last group may be short
        for w in range(WORDS):
            assert np.array_equal(g[:, w], g[0, w] + np.arange(g.shape[0], dtype=np.uint64)), (k, w)
        assert int(g[0, 0]) % GROUP == 0  # a wave's 256-byte load is aligned (the allocation is)
        assert int(g[0, 0]) == k * GROUP * WORDS  # a group is one contiguous 32 KiB record


def test_single_calls_agree_with_the_formula(lib):
    for t, w in ((0, 0), (0, 127), (63, 5), (64, 0), (65, 127), (1 << 32, 3), ((1 << 32) - 2, 127)):
        assert lib.skl_index(t, w) == (t // 64) * 128 * 64 + w * 64 + (t % 64)
