"""Where the words of the sketch's bit planes live (x-search_amd/csrc/xsg_sketch.h: plane_stride, plane_alloc_words,
plane_index): the one definition that k_sketch_planes writes through and the wave form of the finishing pass reads
through, compiled here with g++ as tests/test_sketch_layout.py compiles the sketch's.  Plane-major, one 64-bit word per
(plane, group), the plane stride padded to whole 128-byte lines; and the transposition sketch_index -> plane_index itself,
done on the host, gives back every (tile, bit)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
BITS = 4096
WORDS = 128
GROUP = 64
LINE = 16  # 64-bit words in a 128-byte line
NTILES = (1, 63, 64, 65, 1023, 1024, 1025)

HELPER = r"""
#include "xsg_sketch.h"
using namespace xsg;
extern "C" {
uint32_t pll_bits() { return kSketchBits; }
uint32_t pll_line() { return kPlaneLineGroups; }
uint64_t pll_stride(uint64_t ntiles) { return plane_stride(ntiles); }
uint64_t pll_alloc(uint64_t ntiles) { return plane_alloc_words(ntiles); }
uint64_t pll_index(uint32_t bit, uint64_t group, uint64_t stride) { return plane_index(bit, group, stride); }
// out[bit * groups + group], groups = the plane stride: every word of the allocation
void pll_all(uint64_t ntiles, uint64_t* out) {
  const uint64_t stride = plane_stride(ntiles);
  for (uint32_t b = 0; b < kSketchBits; ++b)
    for (uint64_t g = 0; g < stride; ++g) out[b * stride + g] = plane_index(b, g, stride);
}
// what k_sketch_planes computes, on the host: planes (plane_alloc_words, zeroed by the caller) from sketch words
void pll_transpose(const uint32_t* sketch, uint64_t ntiles, uint64_t* planes) {
  const uint64_t stride = plane_stride(ntiles), groups = (ntiles + kSketchGroup - 1) / kSketchGroup;
  for (uint64_t g = 0; g < groups; ++g)
    for (uint32_t w = 0; w < kSketchWords; ++w)
      for (uint32_t l = 0; l < kSketchGroup; ++l) {
        const uint32_t v = sketch[sketch_index(g * kSketchGroup + l, w)];
        for (uint32_t b = 0; b < 32; ++b)
          if ((v >> b) & 1u) planes[plane_index(w * 32 + b, g, stride)] |= 1ull << l;
      }
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("plane_layout")
    src = d / "plane_layout.cpp"
    src.write_text(HELPER)
    so = d / "libplane_layout.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                        f"-I{ROOT / 'x-search_amd' / 'csrc'}", str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    lib.pll_bits.restype = lib.pll_line.restype = C.c_uint32
    lib.pll_stride.restype = lib.pll_alloc.restype = lib.pll_index.restype = C.c_uint64
    lib.pll_stride.argtypes = lib.pll_alloc.argtypes = [C.c_uint64]
    lib.pll_index.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    lib.pll_all.argtypes = [C.c_uint64, C.c_void_p]
    lib.pll_transpose.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    assert (lib.pll_bits(), lib.pll_line()) == (BITS, LINE)
    return lib


def sketch_alloc(ntiles):
    return (ntiles + GROUP - 1) // GROUP * GROUP * WORDS


def sketch_slot(tile, word):  # sketch_index, pinned by tests/test_sketch_layout.py
    return tile // GROUP * GROUP * WORDS + word * GROUP + tile % GROUP


@pytest.mark.parametrize("ntiles", NTILES)
def test_index_is_a_bijection_below_the_allocation(lib, ntiles):
    groups = (ntiles + GROUP - 1) // GROUP
    stride = lib.pll_stride(ntiles)
    assert stride == (groups + LINE - 1) // LINE * LINE  # whole lines, nothing more
    alloc = lib.pll_alloc(ntiles)
    assert alloc == stride * BITS
    assert alloc * 8 == stride * GROUP * 512  # the sketch's own size: 512 B per tile of the padded groups
    s = np.zeros((BITS, stride), dtype=np.uint64)
    lib.pll_all(ntiles, s.ctypes.data)
    assert np.array_equal(np.sort(s.ravel()), np.arange(alloc, dtype=np.uint64))  # onto, hence one-to-one
    assert int(s[:, :groups].max()) < alloc


@pytest.mark.parametrize("ntiles", NTILES)
def test_the_16_groups_of_a_line_are_consecutive(lib, ntiles):
    stride = lib.pll_stride(ntiles)
    s = np.zeros((BITS, stride), dtype=np.uint64)
    lib.pll_all(ntiles, s.ctypes.data)
    assert np.all(s[:, 0] % LINE == 0)  # a plane starts on a line (the allocation is aligned)
    assert np.array_equal(s, s[:, :1] + np.arange(stride, dtype=np.uint64)[None, :])  # a plane is contiguous over the groups
    line = s // LINE
    for g in range(0, stride, LINE):
        assert np.all(line[:, g:g + LINE] == line[:, g:g + 1])  # 16 consecutive groups share a line
    if stride > LINE:
        assert np.all(line[:, LINE:] != line[:, :-LINE])  # groups 16 apart share none
    assert np.unique(line[:, 0]).size == BITS  # nor do two planes


def test_single_calls_agree_with_the_formula(lib):
    for b, g, st in ((0, 0, 16), (4095, 15, 16), (7, 51199, 51200), (4095, (1 << 31) + 5, 1 << 32)):
        assert lib.pll_index(b, g, st) == b * st + g


@pytest.mark.parametrize("ntiles", NTILES)
def test_host_transposition_gives_back_every_tile_and_bit(lib, ntiles):
    rng = np.random.default_rng(ntiles)
    bits = rng.integers(0, 2, size=(ntiles, BITS), dtype=np.uint8)  # [tile][bit]
    words = np.packbits(bits.reshape(ntiles, WORDS, 32), axis=2, bitorder="little").view(np.uint32).reshape(ntiles, WORDS)
    sketch = np.zeros(sketch_alloc(ntiles), dtype=np.uint32)  # tiles behind ntiles: zero, as k_sketch_build leaves them
    t, w = np.meshgrid(np.arange(ntiles), np.arange(WORDS), indexing="ij")
    sketch[sketch_slot(t, w)] = words
    stride = lib.pll_stride(ntiles)
    planes = np.zeros(lib.pll_alloc(ntiles), dtype=np.uint64)
    lib.pll_transpose(sketch.ctypes.data, ntiles, planes.ctypes.data)
    p = planes.reshape(BITS, stride)
    back = np.unpackbits(p.view(np.uint8).reshape(BITS, stride, 8), axis=2, bitorder="little").reshape(BITS, stride * GROUP)
    assert np.array_equal(back[:, :ntiles].T, bits)  # bit l of plane b's word of group g = bit b of tile g * 64 + l
    assert not back[:, ntiles:].any()  # tiles behind the last one and the padding groups hold no bit
