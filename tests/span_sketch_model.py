"""The span locator on the CPU: x-search_amd/csrc/xsg_sketch.h compiled into a small host helper (g++), as
tests/sketch_model.py does for the tile sketch.  The locator of a chunk built by the header's definition -- span s of a
tile holds the bit of every gram that starts in [S0, S0 + 4096 + reach] inside the chunk -- and the finishing count's test
of one tile: the pattern's span entries (span_entries, at most kSpanRegs words) against the tile's four spans (span_mask).
Shared by tests/test_span_sketch_model.py and tests/test_gpu_gate_spans.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TILE = 16384
SPAN = 4096
SPANS = 4
REACH = 28

HELPER = r"""
#include "xsg_sketch.h"
using namespace xsg;
extern "C" {
uint32_t spm_bits() { return kSpanBits; }
uint32_t spm_words() { return kSpanWords; }
uint32_t spm_spans() { return kSpansPerTile; }
uint32_t spm_span_bytes() { return kSpanBytes; }
uint32_t spm_regs() { return kSpanRegs; }
uint32_t spm_hash(uint32_t g) { return span_hash(g); }
uint32_t spm_tile_hash(uint32_t g) { return sketch_hash(g); }
uint32_t spm_mix(uint32_t g) { return sketch_mix(g); }
uint64_t spm_alloc(uint64_t ntiles) { return span_alloc_words(ntiles); }
uint64_t spm_index(uint64_t tile, uint32_t word, uint32_t span) { return span_index(tile, word, span); }
void spm_all(uint64_t ntiles, uint64_t* out) {
  for (uint64_t t = 0; t < ntiles; ++t)
    for (uint32_t w = 0; w < kSpanWords; ++w)
      for (uint32_t s = 0; s < kSpansPerTile; ++s) out[(t * kSpanWords + w) * kSpansPerTile + s] = span_index(t, w, s);
}
// the definition: span s of tile T holds the bit of every gram that starts in [S0, S0 + span + reach] and lies inside the chunk
void spm_build(const uint8_t* d, uint64_t len, uint32_t* out) {
  const uint64_t ntiles = (len + kSketchTileBytes - 1) / kSketchTileBytes;
  for (uint64_t i = 0; i < span_alloc_words(ntiles); ++i) out[i] = 0;
  for (uint64_t t = 0; t < ntiles; ++t)
    for (uint32_t s = 0; s < kSpansPerTile; ++s) {
      const uint64_t s0 = t * kSketchTileBytes + (uint64_t)s * kSpanBytes;
      for (uint64_t p = s0; p <= s0 + kSpanBytes + kSketchReach && p + 4 <= len; ++p) {
        const uint32_t h = span_hash(sketch_gram(d + p));
        out[span_index(t, h >> 5, s)] |= 1u << (h & 31u);
      }
    }
}
// the finishing count's test of one tile (`words`: its kSpanWords * 4 words): the spans that pass, bit s = span s
int spm_mask(const uint32_t* words, const uint8_t* pat, uint32_t plen, uint32_t first) {
  const uint32_t n = sketch_pattern_grams(plen, first);
  if (n == 0) return -1;
  uint16_t h[kSketchMaxGrams];
  for (uint32_t g = 0; g < n; ++g) h[g] = (uint16_t)span_hash(sketch_gram(pat + first + g));
  uint32_t word[kSpanRegs], mask[kSpanRegs];
  const uint32_t used = span_entries(h, n, word, mask);
  return (int)span_mask(words, word, mask, used);
}
}
"""


def load(workdir):
    """compile the helper into `workdir` and load it"""
    d = Path(workdir)
    src = d / "span_sketch_model.cpp"
    src.write_text(HELPER)
    so = d / "libspan_sketch_model.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                        f"-I{ROOT / 'x-search_amd' / 'csrc'}", str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    for f in (lib.spm_bits, lib.spm_words, lib.spm_spans, lib.spm_span_bytes, lib.spm_regs):
        f.restype = C.c_uint32
    for f in (lib.spm_hash, lib.spm_tile_hash, lib.spm_mix):
        f.restype = C.c_uint32
        f.argtypes = [C.c_uint32]
    lib.spm_alloc.restype = lib.spm_index.restype = C.c_uint64
    lib.spm_alloc.argtypes = [C.c_uint64]
    lib.spm_index.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    lib.spm_all.argtypes = [C.c_uint64, C.c_void_p]
    lib.spm_build.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.spm_mask.restype = C.c_int
    lib.spm_mask.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32]
    assert (lib.spm_spans(), lib.spm_span_bytes()) == (SPANS, SPAN)
    return lib


def build(lib, data: np.ndarray) -> np.ndarray:
    """-> (tiles, words, 4) uint32: the locator of every tile of one chunk, as it is stored"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    ntiles = (data.size + TILE - 1) // TILE
    out = np.zeros((ntiles, lib.spm_words(), SPANS), dtype=np.uint32)
    lib.spm_build(data.ctypes.data, data.size, out.ctypes.data)
    return out


def mask(lib, sp: np.ndarray, tile: int, pat: bytes, first: int = 0) -> int:
    """the spans of `tile` that the entries of `pat` (filter window at `first`) let through: bit s = span s"""
    r = lib.spm_mask(sp[tile].ctypes.data, pat, len(pat), first)
    assert r >= 0
    return r


def occurrences(data: np.ndarray, pat: bytes):
    """every start of `pat` in `data`, overlapping ones included"""
    raw, out, o = data.tobytes(), [], 0
    while True:
        o = raw.find(pat, o)
        if o < 0:
            return out
        out.append(o)
        o += 1


def spans_per_holding_tile(lib, data: np.ndarray, pat: bytes, first: int = 0):
    """-> (spans that pass, tiles that hold a window start of an occurrence): over those tiles only"""
    sp = build(lib, data)
    tiles = sorted({(o + first) // TILE for o in occurrences(data, pat)})
    return sum(bin(mask(lib, sp, t, pat, first)).count("1") for t in tiles), len(tiles)
