// xsg_sketch.h -- the per-tile 4-gram sketch of a binding: what is shared by the kernel that builds it (k_sketch_build),
// the kernels that test it (k_scan<..., GATED>: gated_pass, k_sketch_sample), the host code that turns a pattern into the bits they test
// (xsg_set_pattern, scan_args) and the CPU models of the tests (tests/sketch_model.py and tests/test_sketch_layout.py
// compile this header into host helpers).  Plain C++, host and device.
//
// Tile T of a chunk (16 KiB, k_scan's tile) owns kSketchBits bits.  Bit sketch_hash(g) is set for every 4-gram g -- four
// consecutive bytes, read as a little-endian dword -- that STARTS at a chunk-relative position in
// [T0, T0 + kSketchTileBytes + kSketchReach] and lies wholly inside the chunk.  A pattern of 4 bytes or more is tested
// with its grams at the pattern offsets first .. min(plen - 4, first + kSketchReach), first = the offset of the filter
// window (PatternDev::koff: the position k_scan counts an occurrence at, 0 for all kinds but kLong): an occurrence whose
// window starts in tile T has every one of them in T's OWN sketch, so the test reads one tile's words and a tile in which
// a bit is missing cannot hold one.  The sketch is a superset summary: extra bits cost speed, never a result.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XSG_SKETCH_HD __host__ __device__ inline
#else
#define XSG_SKETCH_HD inline
#endif

namespace xsg {

constexpr uint32_t kSketchBits = 4096;                   // per tile: 512 B, 3.1 % of the text
constexpr uint32_t kSketchWords = kSketchBits / 32;      // 128
constexpr uint32_t kSketchTileBytes = 16384;             // the tile of k_scan
constexpr uint32_t kSketchReach = 28;                    // gram starts this far behind the tile's last byte still belong to it
constexpr uint32_t kSketchMaxGrams = kSketchReach + 1;   // grams of a pattern that are tested, at most

// 32 -> 12 bits: multiply, xor-shift, multiply, xor-shift, the top bits.  (A bare multiplicative hash leaves the grams of
// English text in clumps: half the tiles of the bench corpus stayed candidates for `Sherlock`.)
XSG_SKETCH_HD uint32_t sketch_hash(uint32_t g) {
  g *= 0x9E3779B1u;
  g ^= g >> 15;
  g *= 0x85EBCA77u;
  g ^= g >> 13;
  return g >> 20;
}

// Where the words live.  The sketch is stored word-major inside groups of kSketchGroup consecutive tiles: word w of the
// 64 tiles of a group are 64 consecutive dwords, so a wave that holds one tile per lane (gated_pass) reads one word
// of 64 tiles as one 256-byte load.  The allocation covers whole groups; the words of tiles behind the last one are zero.
constexpr uint32_t kSketchGroup = 64;
XSG_SKETCH_HD uint64_t sketch_alloc_words(uint64_t ntiles) {
  return (ntiles + kSketchGroup - 1) / kSketchGroup * kSketchGroup * kSketchWords;
}
XSG_SKETCH_HD uint64_t sketch_index(uint64_t tile, uint32_t word) {
  return tile / kSketchGroup * ((uint64_t)kSketchGroup * kSketchWords) + (uint64_t)word * kSketchGroup + tile % kSketchGroup;
}

// the grams of a pattern that the gate tests: pattern offsets [first, first + n)
XSG_SKETCH_HD uint32_t sketch_pattern_grams(uint32_t plen, uint32_t first) {
  if (plen < 4u || first + 4u > plen) return 0u;
  const uint32_t last = plen - 4u < first + kSketchReach ? plen - 4u : first + kSketchReach;
  return last - first + 1u;
}

XSG_SKETCH_HD uint32_t sketch_gram(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace xsg
