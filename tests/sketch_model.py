"""The per-tile 4-gram sketch on the CPU: x-search_amd/csrc/xsg_sketch.h compiled into a small host helper (g++), the
sketch of a chunk built by the header's definition, and the gate's test of one tile.  Shared by tests/test_sketch_model.py
(the properties the gate rests on) and tests/test_gpu_sketch.py (what verdict the library should reach on a shard)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TILE = 16384
REACH = 28

HELPER = r"""
#include "xsg_sketch.h"
using namespace xsg;
extern "C" {
uint32_t skm_bits() { return kSketchBits; }
uint32_t skm_tile() { return kSketchTileBytes; }
uint32_t skm_reach() { return kSketchReach; }
uint32_t skm_hash(uint32_t g) { return sketch_hash(g); }
uint32_t skm_grams(uint32_t plen, uint32_t first) { return sketch_pattern_grams(plen, first); }
// the definition: tile T holds the bit of every gram that starts in [T0, T0 + tile + reach] and lies inside the chunk
void skm_build(const uint8_t* d, uint64_t len, uint32_t* out) {
  const uint64_t ntiles = (len + kSketchTileBytes - 1) / kSketchTileBytes;
  for (uint64_t i = 0; i < ntiles * kSketchWords; ++i) out[i] = 0;
  for (uint64_t t = 0; t < ntiles; ++t) {
    const uint64_t t0 = t * kSketchTileBytes;
    for (uint64_t p = t0; p <= t0 + kSketchTileBytes + kSketchReach && p + 4 <= len; ++p) {
      const uint32_t h = sketch_hash(sketch_gram(d + p));
      out[t * kSketchWords + (h >> 5)] |= 1u << (h & 31u);
    }
  }
}
// the gate's test of one tile: the grams at the pattern offsets first .. first + grams - 1
int skm_pass(const uint32_t* words, const uint8_t* pat, uint32_t plen, uint32_t first) {
  const uint32_t n = sketch_pattern_grams(plen, first);
  if (n == 0) return -1;
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t h = sketch_hash(sketch_gram(pat + first + g));
    if (!((words[h >> 5] >> (h & 31u)) & 1u)) return 0;
  }
  return 1;
}
}
"""



def load(workdir):
    """compile the helper into `workdir` and load it"""
    d = Path(workdir)
    src = d / "sketch_model.cpp"
    src.write_text(HELPER)
    so = d / "libsketch_model.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                        f"-I{ROOT / 'x-search_amd' / 'csrc'}", str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    for f in (lib.skm_bits, lib.skm_tile, lib.skm_reach):
        f.restype = C.c_uint32
    lib.skm_hash.restype = C.c_uint32
    lib.skm_hash.argtypes = [C.c_uint32]
    lib.skm_grams.restype = C.c_uint32
    lib.skm_grams.argtypes = [C.c_uint32, C.c_uint32]
    lib.skm_build.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.skm_pass.restype = C.c_int
    lib.skm_pass.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32]
    assert (lib.skm_bits(), lib.skm_tile(), lib.skm_reach()) == (4096, TILE, REACH)
    return lib


def build(lib, data: np.ndarray) -> np.ndarray:
    """-> (tiles, 128) uint32: the sketch of every tile of one chunk"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    ntiles = (data.size + TILE - 1) // TILE
    out = np.zeros((ntiles, 128), dtype=np.uint32)
    lib.skm_build(data.ctypes.data, data.size, out.ctypes.data)
    return out


def passes(lib, sk: np.ndarray, tile: int, pat: bytes, first: int = 0) -> bool:
    r = lib.skm_pass(sk[tile].ctypes.data, pat, len(pat), first)
    assert r >= 0
    return r == 1


def pass_share(lib, blocks, pat: bytes, first: int = 0) -> float:
    """the share of the tiles of these chunks that the gate of `pat` (filter window at `first`) lets through"""
    tiles = ok = 0
    for b in blocks:
        sk = build(lib, b)
        tiles += sk.shape[0]
        ok += sum(1 for t in range(sk.shape[0]) if passes(lib, sk, t, pat, first))
    return ok / max(tiles, 1)
