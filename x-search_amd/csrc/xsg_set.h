// xsg_set.h -- a list of literals as ONE pattern (xsg_set_literals, include/xsg.h): the host-side compiler and the pieces
// the kernels share with it (xsg_set_kernels.hip).  Plain C++ when compiled without hipcc: tests/cpp/set_selftest.cpp
// drives the compiler, the filter and the verify step on the host, under the sanitizers.
//
// The search is leftmost-first over the literals in listing order: at the leftmost position where any literal occurs,
// the first-listed literal that occurs there is the match, and the walk resumes at its end.
//   FILTER  Let m be the shortest literal and g = min(m, 4).  Every literal starts with a g-gram; the filter holds one
//           bit per hashed g-gram (65 536 bits = 8 KiB, the hash is the identity for g <= 2).  A position whose g-gram
//           has no bit cannot start a literal: k_set_scan tests every position of the text against the filter in LDS.
//   VERIFY  The distinct g-grams, sorted, each with the literals that start with it IN LISTING ORDER.  k_set_verify
//           looks a candidate's gram up and compares those literals against the chunk bytes until one fits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define XSG_SET_HD __host__ __device__ inline
#else
#define XSG_SET_HD inline
#endif

#include <string>
#include <vector>

namespace xsg {

constexpr uint32_t kSetFilterBits = 65536;
constexpr uint32_t kSetFilterBytes = kSetFilterBits / 8;
constexpr uint32_t kSetFilterWords = kSetFilterBits / 32;

// The filter bit of a gram: `v` holds the gram's g bytes, first byte lowest, upper bytes zero.  One function for the
// compiler, the scan kernel and the host copies the tests drive.
XSG_SET_HD uint32_t set_gram_hash(uint32_t v, uint32_t g) { return g <= 2u ? v : (v * 0x9E3779B1u) >> 16; }
XSG_SET_HD uint32_t set_gram_mask(uint32_t g) { return g >= 4u ? 0xffffffffu : (1u << (8u * g)) - 1u; }
XSG_SET_HD uint8_t set_fold(uint8_t b, bool icase) { return (icase && b >= 'A' && b <= 'Z') ? (uint8_t)(b + 32) : b; }
// the gram that starts at d[0] (g readable bytes), folded under icase
XSG_SET_HD uint32_t set_gram_at(const uint8_t* d, uint32_t g, bool icase) {
  uint32_t v = 0;
  for (uint32_t k = 0; k < g; ++k) v |= (uint32_t)set_fold(d[k], icase) << (8u * k);
  return v;
}
XSG_SET_HD bool set_filter_has(const uint32_t* filter, uint32_t v, uint32_t g) {
  const uint32_t h = set_gram_hash(v, g);
  return (filter[h >> 5] >> (h & 31u)) & 1u;
}

// The verify table as the kernel reads it (all inside one blob; offsets in bytes from its start, multiples of 4):
//   keys[ngrams]       the distinct grams, ascending
//   first[ngrams + 1]  entries of gram k: ent[first[k] .. first[k + 1])
//   ent[nlits]         (offset of the literal's bytes in `bytes`) << 8 | its length, listing order inside a gram
//   bytes              the literals back to back (folded under ignore-case)
//   idx[nlits]         the LISTING index of every entry of `ent`, uint16 (xsg_count_literals: set_count_at; an all-of
//                      list: set_mask_at; the other search routes never read it, and a table built without it leaves
//                      it null)
// words: XSG_LIST_WHOLE_WORDS (include/xsg.h) -- an occurrence stands only between two bytes that are no word bytes, the
// chunk's edges counting as such (set_entry_at).
struct SetTable {
  const uint32_t* keys;
  const uint32_t* first;
  const uint32_t* ent;
  const uint8_t* bytes;
  uint32_t ngrams;
  uint32_t g;
  const uint16_t* idx = nullptr;
  uint32_t words = 0;
};

// A word byte: 0-9 A-Z a-z _ (63 values; GNU grep -w in the C locale).  Ignore-case does not change the set.
XSG_SET_HD bool set_word_byte(uint8_t b) {
  return (uint8_t)((b | 0x20u) - 'a') < 26u || (uint8_t)(b - '0') < 10u || b == '_';
}

// The two steps of a verify.  set_gram_find: is gram v one of the sorted keys[0 .. ngrams)?  *k receives the index of
// the first key >= v (binary search), the gram's own when it is found.  set_entry_at: do the bytes of entry e's literal
// fit the `room` left in the chunk at `at` and equal the chunk's there (folded under icase)?  *len receives the literal's
// length; no byte at or beyond at + room is read.  `p`: the bytes of the chunk in front of `at`.  Under T.words a literal that
// compared equal still has to stand between two bytes that are no word bytes: at[-1] is read only if p > 0, at[n] only if
// n < room -- the chunk's edges are word boundaries, and no byte outside the chunk decides anything.
XSG_SET_HD bool set_gram_find(const uint32_t* keys, uint32_t ngrams, uint32_t v, uint32_t* k) {
  uint32_t lo = 0, hi = ngrams;
  while (lo < hi) {  // first key >= v
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < v)
      lo = mid + 1u;
    else
      hi = mid;
  }
  *k = lo;
  return lo != ngrams && keys[lo] == v;
}
XSG_SET_HD bool set_entry_at(const SetTable& T, uint32_t e, const uint8_t* at, uint64_t p, uint64_t room, bool icase,
                             uint32_t* len) {
  const uint32_t n = *len = T.ent[e] & 0xffu;
  if (n > room) return false;
  const uint8_t* lit = T.bytes + (T.ent[e] >> 8);
  uint32_t k = T.g;  // (the gram is the literal's start: already compared)
  while (k < n && set_fold(at[k], icase) == lit[k]) ++k;
  if (k != n) return false;
  if (T.words) {  // (the same for every lane; behind a compare that succeeded)
    if (p > 0u && set_word_byte(at[-1])) return false;
    if (n < room && set_word_byte(at[n])) return false;
  }
  return true;
}

// Length of the first-listed literal that occurs (under T.words: admissibly) at d[p] of a chunk of L bytes, or 0.
// p + g <= L is the caller's to ensure (the scan reports no other position); nothing at or beyond L is read.
XSG_SET_HD uint32_t set_verify_at(const SetTable& T, const uint8_t* d, uint64_t p, uint64_t L, bool icase) {
  uint32_t k, len;
  if (!set_gram_find(T.keys, T.ngrams, set_gram_at(d + p, T.g, icase), &k)) return 0u;
  for (uint32_t e = T.first[k]; e < T.first[k + 1u]; ++e)
    if (set_entry_at(T, e, d + p, p, L - p, icase, &len)) return len;
  return 0u;
}

// EVERY literal that occurs (under T.words: admissibly) at d[p] of a chunk of L bytes: visit(listing index) once per
// literal whose len bytes fit the room L - p and equal the chunk's (folded under icase) -- prefixes, infixes and
// duplicates of one another included, which is what xsg_count_literals counts.  p + g <= L is the caller's to ensure, as
// for set_verify_at; nothing at or beyond L is read.  `keys`: T.keys, or a copy of them that is cheaper to reach (the
// kernel's lies in LDS).
template <typename Visit>
XSG_SET_HD void set_count_at(const SetTable& T, const uint8_t* d, uint64_t p, uint64_t L, bool icase, Visit&& visit,
                             const uint32_t* keys) {
  uint32_t k, len;
  if (!set_gram_find(keys, T.ngrams, set_gram_at(d + p, T.g, icase), &k)) return;
  for (uint32_t e = T.first[k]; e < T.first[k + 1u]; ++e)
    if (set_entry_at(T, e, d + p, p, L - p, icase, &len)) visit((uint32_t)T.idx[e]);
}

template <typename Visit>
XSG_SET_HD void set_count_at(const SetTable& T, const uint8_t* d, uint64_t p, uint64_t L, bool icase, Visit&& visit) {
  set_count_at(T, d, p, L, icase, visit, T.keys);
}

// XSG_LIST_ALL_OF: set_count_at's visit as a mask -- bit j set <=> the literal of listing index j occurs (under T.words:
// admissibly) at d[p].  The list holds at most 64 literals (xsg_set_literals_opts refuses more under the option), so j < 64.
// Same contract: p + g <= L is the caller's to ensure, nothing at or beyond L is read, and T.idx must be set.
XSG_SET_HD uint64_t set_mask_at(const SetTable& T, const uint8_t* d, uint64_t p, uint64_t L, bool icase) {
  uint64_t mask = 0;
  set_count_at(T, d, p, L, icase, [&](uint32_t j) { mask |= 1ull << (j & 63u); });
  return mask;
}

// What the host compiles a list into.
struct SetProgram {
  uint32_t count = 0, min_len = 0, max_len = 0, g = 0, filter_bits_set = 0;
  bool icase = false;
  std::vector<uint32_t> filter;  // kSetFilterWords
  std::vector<uint32_t> keys, first, ent;
  std::vector<uint8_t> bytes;
  std::vector<uint16_t> idx;  // listing index of every entry of `ent`
  SetTable table() const {
    return SetTable{keys.data(), first.data(), ent.data(), bytes.data(), (uint32_t)keys.size(), g, idx.data()};
  }
  // the device image: filter, keys, first, ent, bytes, idx (+ padding); *off receives the byte offsets of keys, first,
  // ent and bytes; idx lies behind bytes, at idx_offset()
  std::vector<uint8_t> blob(uint32_t off[4]) const;
  uint32_t idx_offset() const;
};
// Parses `list` (literals separated by '\n', one final '\n' allowed) and compiles it.  False with *err set for: an empty
// list, an empty literal, more than XSG_MAX_LITERALS literals, a literal over XSG_MAX_LITERAL_BYTES.
bool compile_literal_set(const uint8_t* list, size_t n, bool icase, SetProgram* out, std::string* err);

}  // namespace xsg
