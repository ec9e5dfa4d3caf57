// xsg_sketch.h -- the per-tile 4-gram sketch of a binding and the span locator beside it: what is shared by the kernel that
// builds them (k_sketch_build), the kernels that test them (k_scan<..., GATED> and k_scan_fin: gated_pass, k_sketch_sample),
// the host code that turns a pattern into the bits they test (xsg_set_pattern, scan_args, fin_args) and the CPU models of
// the tests (tests/sketch_model.py, tests/span_sketch_model.py and tests/test_sketch_layout.py compile this header into
// host helpers).  Plain C++, host and device.
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
XSG_SKETCH_HD uint32_t sketch_mix(uint32_t g) {
  g *= 0x9E3779B1u;
  g ^= g >> 15;
  g *= 0x85EBCA77u;
  g ^= g >> 13;
  return g;
}
XSG_SKETCH_HD uint32_t sketch_hash(uint32_t g) { return sketch_mix(g) >> 20; }

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

// ---- the bit planes: the same bits, transposed ---------------------------------------------------------------------------
// A second array derived from the finished sketch (k_sketch_planes), for the one reader that asks "which of a group's 64
// tiles hold bit b": plane b (0 .. kSketchBits - 1) holds one 64-bit word per sketch group, bit l of it = bit b of tile
// group * 64 + l.  Plane-major: a plane is contiguous over the binding's groups, its stride padded to whole 128-byte lines
// (16 groups), so a plane starts on a line, 16 consecutive groups share one and groups 16 apart share none.  The size is
// the sketch's own: 512 B per tile.  A pattern's test of a group is the AND of one word per gram (its sketch_hash is the
// plane); the reader fetches them one word a lane and brings them together by readlane (gated_pass_waves).  The bits of
// tiles behind the last one are zero like their sketch words.  plane_index takes the stride (plane_stride(ntiles)), which
// the host computes once and hands to the kernel (GateFinArgs::pl_stride).
constexpr uint32_t kPlaneLineGroups = 16;  // 64-bit words in a 128-byte line
XSG_SKETCH_HD uint64_t plane_stride(uint64_t ntiles) {  // words from one plane to the next
  const uint64_t groups = (ntiles + kSketchGroup - 1) / kSketchGroup;
  return (groups + kPlaneLineGroups - 1) / kPlaneLineGroups * kPlaneLineGroups;
}
XSG_SKETCH_HD uint64_t plane_alloc_words(uint64_t ntiles) { return plane_stride(ntiles) * kSketchBits; }  // of 64 bits
XSG_SKETCH_HD uint64_t plane_index(uint32_t bit, uint64_t group, uint64_t stride) { return (uint64_t)bit * stride + group; }

// the grams of a pattern that the gate tests: pattern offsets [first, first + n)
XSG_SKETCH_HD uint32_t sketch_pattern_grams(uint32_t plen, uint32_t first) {
  if (plen < 4u || first + 4u > plen) return 0u;
  const uint32_t last = plen - 4u < first + kSketchReach ? plen - 4u : first + kSketchReach;
  return last - first + 1u;
}

XSG_SKETCH_HD uint32_t sketch_gram(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ---- the span locator: the tile sketch's rule one level down ------------------------------------------------------------
// A tile is scanned by four waves, wave s owning the contiguous span [T0 + s * kSpanBytes, + kSpanBytes).  Span s of a tile
// owns kSpanBits bits of its own: bit span_hash(g) is set for every 4-gram g that starts at a chunk-relative position in
// [S0, S0 + kSpanBytes + kSketchReach] and lies inside the chunk.  An occurrence whose filter window starts in span s has
// every tested gram (the same pattern offsets as above) in span s's OWN bits: a span in which a bit is missing holds no
// window start, and the finishing form of the gated count (gated_pass<..., FIN>) does not read its text.  A superset
// summary like the tile sketch; testing fewer of the pattern's grams only lets more spans through.
// The bit index is taken from bits of the mixed value that sketch_hash does not use (it keeps the top 12).
#ifndef XSG_SPAN_BITS
#define XSG_SPAN_BITS 2048
#endif
// (1024 bits per span measured 10 % slower on the bench shard than 2048 -- 1.29 / 1.53 spans pass per tile that holds an
// occurrence against 1.00 / 1.00 -- DESIGN.md section 5; -DXSG_SPAN_BITS=1024 builds that variant)
constexpr uint32_t kSpanBits = XSG_SPAN_BITS;            // per span: 256 B; four spans: 1 KiB per tile, another 6.2 % of the text
constexpr uint32_t kSpanWords = kSpanBits / 32;          // 64
constexpr uint32_t kSpanBytes = 4096;                    // a wave's share of a tile in k_scan
constexpr uint32_t kSpansPerTile = kSketchTileBytes / kSpanBytes;  // 4
static_assert(kSpanBits >= 32 && (kSpanBits & (kSpanBits - 1)) == 0 && kSpanBits <= (1u << 20), "span bits: a power of two below the tile sketch's bits");
constexpr uint32_t span_log2(uint32_t v) { return v <= 1u ? 0u : 1u + span_log2(v >> 1); }
constexpr uint32_t kSpanShift = 20u - span_log2(kSpanBits);  // the field ends below sketch_hash's: bits 9 .. 19 for 2048
XSG_SKETCH_HD uint32_t span_hash_of_mix(uint32_t m) { return (m >> kSpanShift) & (kSpanBits - 1u); }
XSG_SKETCH_HD uint32_t span_hash(uint32_t g) { return span_hash_of_mix(sketch_mix(g)); }

// Where the locator's words live: tile-major, [tile][word 0 .. kSpanWords)[span 0 .. 4).  Word k of a tile's four spans is
// one aligned 16-byte group, and a tile's words are contiguous: only the few lanes whose tile passes the sketch read them.
XSG_SKETCH_HD uint64_t span_alloc_words(uint64_t ntiles) { return ntiles * (uint64_t)(kSpanWords * kSpansPerTile); }
XSG_SKETCH_HD uint64_t span_index(uint64_t tile, uint32_t word, uint32_t span) {
  return (tile * kSpanWords + word) * kSpansPerTile + span;
}

// What k_scan_fin tests of a pattern: the span hashes of its tested grams (span_hash of the grams at the pattern offsets
// first .. first + sketch_pattern_grams - 1) as (word, mask) pairs, one per distinct word of a span's kSpanWords, at most
// kSpanRegs of them -- a gram whose word does not fit any more is left out: fewer grams, still a superset.  -> entries
#ifndef XSG_SPAN_REGS
#define XSG_SPAN_REGS 6
#endif
constexpr uint32_t kSpanRegs = XSG_SPAN_REGS;  // a 16-byte load each (word k of the tile's four spans)
XSG_SKETCH_HD uint32_t span_entries(const uint16_t* hashes, uint32_t n, uint32_t* word, uint32_t* mask) {
  uint32_t used = 0;
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t w = hashes[g] >> 5, bit = 1u << (hashes[g] & 31u);
    uint32_t k = 0;
    while (k < used && word[k] != w) ++k;
    if (k == used) {
      if (used == kSpanRegs) continue;
      word[used] = w, mask[used] = 0u, ++used;
    }
    mask[k] |= bit;
  }
  return used;
}
// the spans of one tile that hold every bit of the entries: bit s = span s; `words` = the tile's kSpanWords * 4 words
XSG_SKETCH_HD uint32_t span_mask(const uint32_t* words, const uint32_t* word, const uint32_t* mask, uint32_t n) {
  uint32_t m = 0;
  for (uint32_t s = 0; s < kSpansPerTile; ++s) {
    uint32_t miss = 0;
    for (uint32_t k = 0; k < n; ++k) miss |= ~words[word[k] * kSpansPerTile + s] & mask[k];
    m |= miss == 0 ? 1u << s : 0u;
  }
  return m;
}

}  // namespace xsg
