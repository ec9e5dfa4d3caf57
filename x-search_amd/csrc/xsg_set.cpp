// xsg_set.cpp -- the host-side compiler of a literal list (xsg_set.h).  No device code and no HIP call: it also builds
// with a plain C++ compiler (tests/cpp/set_selftest.cpp).
#include "xsg_set.h"

#include <algorithm>
#include <cstring>

#include "../../include/xsg.h"

namespace xsg {

static_assert(XSG_MAX_LITERALS <= 65536, "SetProgram::idx holds listing indices as uint16");

bool compile_literal_set(const uint8_t* list, size_t n, bool icase, SetProgram* out, std::string* err) {
  *out = SetProgram{};
  out->icase = icase;
  if (!list || n == 0) return *err = "empty literal list", false;
  if (list[n - 1] == '\n') --n;  // one final '\n', as in a grep -f file
  if (n == 0) return *err = "the list holds an empty literal (grep lets it match every line: not served)", false;
  struct Lit {
    uint32_t off, len;
  };
  std::vector<Lit> lits;
  out->bytes.assign(list, list + n);
  if (icase)
    for (uint8_t& b : out->bytes) b = set_fold(b, true);
  for (size_t p = 0; p <= n;) {
    const uint8_t* nl = p < n ? static_cast<const uint8_t*>(memchr(list + p, '\n', n - p)) : nullptr;
    const size_t e = nl ? (size_t)(nl - list) : n;
    if (e == p) return *err = "the list holds an empty literal (grep lets it match every line: not served)", false;
    if (e - p > XSG_MAX_LITERAL_BYTES) {
      *err = "literal " + std::to_string(lits.size() + 1) + " is longer than " + std::to_string(XSG_MAX_LITERAL_BYTES) + " bytes";
      return false;
    }
    if (lits.size() == XSG_MAX_LITERALS) return *err = "more than " + std::to_string(XSG_MAX_LITERALS) + " literals", false;
    lits.push_back(Lit{(uint32_t)p, (uint32_t)(e - p)});
    p = e + 1;
  }
  out->count = (uint32_t)lits.size();
  out->min_len = out->max_len = lits[0].len;
  for (const Lit& l : lits) {
    out->min_len = std::min(out->min_len, l.len);
    out->max_len = std::max(out->max_len, l.len);
  }
  const uint32_t g = out->g = std::min(out->min_len, 4u);
  // every literal under its gram; a stable sort by gram keeps the listing order inside one
  std::vector<std::pair<uint32_t, uint32_t>> by_gram(lits.size());  // (gram, literal)
  for (size_t i = 0; i < lits.size(); ++i) by_gram[i] = {set_gram_at(out->bytes.data() + lits[i].off, g, false), (uint32_t)i};
  std::stable_sort(by_gram.begin(), by_gram.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  out->filter.assign(kSetFilterWords, 0u);
  for (size_t i = 0; i < by_gram.size(); ++i) {
    if (i == 0 || by_gram[i].first != by_gram[i - 1].first) {
      out->keys.push_back(by_gram[i].first);
      out->first.push_back((uint32_t)i);
      const uint32_t h = set_gram_hash(by_gram[i].first, g);
      out->filter[h >> 5] |= 1u << (h & 31u);
    }
    const Lit& l = lits[by_gram[i].second];
    out->ent.push_back(l.off << 8 | l.len);
    out->idx.push_back((uint16_t)by_gram[i].second);  // (XSG_MAX_LITERALS <= 65 536)
  }
  out->first.push_back((uint32_t)by_gram.size());
  for (uint32_t w : out->filter) out->filter_bits_set += (uint32_t)__builtin_popcount(w);
  return true;
}

// where the arrays lie in the device image: off[0..3] as blob hands them out, off[4] = idx, off[5] = the end
static void set_layout(const SetProgram& p, uint32_t off[6]) {
  size_t at = kSetFilterBytes;
  auto place = [&](size_t bytes_) {
    const size_t o = at;
    at = (at + bytes_ + 15) & ~(size_t)15;
    return (uint32_t)o;
  };
  off[0] = place(4 * p.keys.size());
  off[1] = place(4 * p.first.size());
  off[2] = place(4 * p.ent.size());
  off[3] = place(p.bytes.size());
  off[4] = place(2 * p.idx.size());
  off[5] = (uint32_t)at;
}

uint32_t SetProgram::idx_offset() const {
  uint32_t o[6];
  set_layout(*this, o);
  return o[4];
}

std::vector<uint8_t> SetProgram::blob(uint32_t off[4]) const {
  uint32_t o[6];
  set_layout(*this, o);
  memcpy(off, o, 4 * sizeof(uint32_t));
  std::vector<uint8_t> b((size_t)o[5] + 16, 0);
  memcpy(b.data(), filter.data(), kSetFilterBytes);
  memcpy(b.data() + off[0], keys.data(), 4 * keys.size());
  memcpy(b.data() + off[1], first.data(), 4 * first.size());
  memcpy(b.data() + off[2], ent.data(), 4 * ent.size());
  memcpy(b.data() + off[3], bytes.data(), bytes.size());
  memcpy(b.data() + o[4], idx.data(), 2 * idx.size());
  return b;
}

}  // namespace xsg
