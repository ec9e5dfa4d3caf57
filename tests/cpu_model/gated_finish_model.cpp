// Host model of the finishing form of the gated count pass (x-search_amd/csrc/xsg_kernels.hip: gated_pass<..., FIN>),
// built from the product's own headers (xsg_tail.h, xsg_sketch.h).  Driven by tests/test_gated_finish_model.py.
//
//   gf_check_zero_walk   the fact the form rests on: the end-of-chunk walk reports only positions >= Z at which the whole
//                        needle matches, so a zone without an occurrence contributes 0 from EVERY entry -- and where the
//                        zone holds one, the result does depend on the entry
//   gf_count             the pass itself on one chunk: per tile that passes the model sketch, the occurrences below Z
//                        whose filter window starts in it; per such tile that is the home of a position of the zone, a
//                        look at the zone; in the home of the zone's first occurrence, the walk from an entry found by
//                        walking the tiles backwards and searching only those that pass
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../x-search_amd/csrc/xsg_sketch.h"
#include "../../x-search_amd/csrc/xsg_tail.h"

using namespace xsg;

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

constexpr uint64_t kTile = kSketchTileBytes;

std::vector<uint32_t> build_sketch(const uint8_t* d, uint64_t len) {
  const uint64_t ntiles = (len + kTile - 1) / kTile;
  std::vector<uint32_t> out(ntiles * kSketchWords, 0u);
  for (uint64_t t = 0; t < ntiles; ++t)
    for (uint64_t p = t * kTile; p <= t * kTile + kTile + kSketchReach && p + 4 <= len; ++p) {
      const uint32_t h = sketch_hash(sketch_gram(d + p));
      out[t * kSketchWords + (h >> 5)] |= 1u << (h & 31u);
    }
  return out;
}

bool tile_passes(const std::vector<uint32_t>& sk, uint64_t t, const uint8_t* pat, uint32_t plen, uint32_t koff) {
  const uint32_t n = sketch_pattern_grams(plen, koff);
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t h = sketch_hash(sketch_gram(pat + koff + g));
    if (!((sk[t * kSketchWords + (h >> 5)] >> (h & 31u)) & 1u)) return false;
  }
  return true;
}

// fin_last_in_tile: the last occurrence o < Z whose window (o + koff) starts in tile trel; o + 1, or 0
uint64_t last_in_tile(const uint8_t* d, uint64_t Z, uint64_t trel, const uint8_t* pat, uint32_t plen, uint32_t koff) {
  const uint64_t w_lo = trel * kTile > koff ? trel * kTile : koff;
  const uint64_t w_hi = (trel + 1) * kTile < Z + koff ? (trel + 1) * kTile : Z + koff;
  for (uint64_t w = w_hi; w > w_lo; --w)
    if (occurs_at(d, w - 1 - koff, pat, plen, false)) return w - 1 - koff + 1;
  return 0;
}

}  // namespace

extern "C" {

// -> violations (0 is a pass).  *dependent: cases (chunk, needle) whose zone holds an occurrence and whose result differs
// between two entries; *cases: (chunk, needle, entry) triples tried.  alphabet 0: random bytes of a 5-letter alphabet
// that includes '\n'; 1: "ab\n" only.
uint64_t gf_check_zero_walk(uint64_t seed, uint64_t iters, uint32_t alphabet, uint64_t* dependent, uint64_t* cases) {
  Rng r{seed * 2654435761ull + 17};
  uint64_t bad = 0, dep = 0, n_cases = 0;
  const char* alph = alphabet ? "ab\n" : "abc\n ";
  const uint32_t na = (uint32_t)strlen(alph);
  std::vector<uint8_t> d;
  uint64_t out[80];
  for (uint64_t it = 0; it < iters; ++it) {
    const uint32_t plen = 2 + r.below(7);  // 2..8
    uint8_t pat[8];
    for (uint32_t k = 0; k < plen; ++k) pat[k] = (uint8_t)alph[r.below(na)];
    const uint64_t L = 1 + r.below(120);
    d.resize(L);
    for (uint64_t i = 0; i < L; ++i) d[i] = (uint8_t)alph[r.below(na)];
    if (r.below(3) == 0 && L >= plen) memcpy(d.data() + (L - plen - r.below((uint32_t)(L - plen + 1))), pat, plen);
    const uint64_t Z = tail_zone_begin(L, plen);
    bool zone_has = false;
    for (uint64_t o = Z; o + plen <= L; ++o) zone_has |= occurs_at(d.data(), o, pat, plen, false);
    uint32_t lo = UINT32_MAX, hi = 0;
    // every admissible entry: 0, and the end of an occurrence that starts below Z -- and every other value up to L too
    for (uint64_t e = 0; e <= L; ++e) {
      const uint32_t n = tail_walk(d.data(), L, pat, plen, e, false, out, 80, false);
      ++n_cases;
      if (!zone_has && n != 0) ++bad;
      for (uint32_t i = 0; i < n && i < 80; ++i)
        if (out[i] < Z || out[i] + plen > L || !occurs_at(d.data(), out[i], pat, plen, false)) ++bad;
      const bool admissible = e == 0 || (e >= plen && e - plen < Z && occurs_at(d.data(), e - plen, pat, plen, false));
      if (admissible) lo = n < lo ? n : lo, hi = n > hi ? n : hi;
    }
    if (zone_has && lo != hi) ++dep;
  }
  if (dependent) *dependent = dep;
  if (cases) *cases = n_cases;
  return bad;
}

// The finishing pass on one chunk.  -> its match count; *entry: the walk's entry as found (UINT64_MAX: no walk ran);
// *searched: tiles the look-back searched byte by byte; *walks: tiles that ran the walk (must be 0 or 1)
uint64_t gf_count(const uint8_t* d, uint64_t L, const uint8_t* pat, uint32_t plen, uint32_t koff, uint64_t* entry,
                  uint64_t* searched, uint64_t* walks) {
  const std::vector<uint32_t> sk = build_sketch(d, L);
  const uint64_t ntiles = (L + kTile - 1) / kTile;
  const uint64_t Z = tail_zone_begin(L, plen);
  uint64_t total = 0, n_search = 0, n_walks = 0, ent = UINT64_MAX;
  for (uint64_t t = 0; t < ntiles; ++t) {
    if (!tile_passes(sk, t, pat, plen, koff)) continue;
    // the bulk part of a candidate tile: occurrences o < Z whose window starts in it
    for (uint64_t w = t * kTile; w < (t + 1) * kTile; ++w)
      if (w >= koff && w - koff < Z && occurs_at(d, w - koff, pat, plen, false)) ++total;
    if (L < plen || t < (Z + koff) / kTile || t > (L - plen + koff) / kTile) continue;
    // a home of the zone: the first occurrence of the zone names the owner
    uint64_t first = UINT64_MAX;
    for (uint64_t o = Z; o + plen <= L && first == UINT64_MAX; ++o)
      if (occurs_at(d, o, pat, plen, false)) first = o;
    if (first == UINT64_MAX || (first + koff) / kTile != t) continue;
    uint64_t e = 0;
    if (Z) {
      for (uint64_t tt = (Z - 1 + koff) / kTile + 1; tt > 0 && e == 0; --tt) {
        if (!tile_passes(sk, tt - 1, pat, plen, koff)) continue;
        ++n_search;
        const uint64_t r = last_in_tile(d, Z, tt - 1, pat, plen, koff);
        if (r) e = r - 1 + plen;
      }
    }
    ent = e;
    ++n_walks;
    total += tail_walk(d, L, pat, plen, e, false, nullptr, 0, false);
  }
  if (entry) *entry = ent;
  if (searched) *searched = n_search;
  if (walks) *walks = n_walks;
  return total;
}

// the zone's count for a given entry (the test shows that its cases depend on it)
uint32_t gf_tail_walk(const uint8_t* d, uint64_t L, const uint8_t* pat, uint32_t plen, uint64_t entry) {
  return tail_walk(d, L, pat, plen, entry, false, nullptr, 0, false);
}
uint64_t gf_zone_begin(uint64_t L, uint32_t plen) { return tail_zone_begin(L, plen); }
}
