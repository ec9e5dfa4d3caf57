// set_selftest.cpp -- the host side of a literal list (x-search_amd/csrc/xsg_set.h/.cpp) on its own, built with
// -fsanitize=address,undefined by tests/test_set_host.py and run as a process: no GPU, no library, nothing loaded.
//   1. no false negative: at every position where a literal truly occurs, the host copy of the filter test passes;
//   2. the host copy of the verify step (set_verify_at, the function k_set_verify runs) equals a brute-force model --
//      the first-listed literal that occurs at the position, bounded by the chunk length -- at EVERY position with room
//      for a gram, and the blob the device receives holds the same table.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../x-search_amd/csrc/xsg_set.cpp"

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
      if (++failures > 10) std::exit(1); \
    }                                    \
  } while (0)

static uint8_t lower(uint8_t b) { return b >= 'A' && b <= 'Z' ? (uint8_t)(b + 32) : b; }

// the model: length of the first-listed literal that occurs at text[p], or 0
static uint32_t model_at(const std::vector<std::string>& lits, const std::vector<uint8_t>& text, size_t p, bool icase) {
  for (const std::string& l : lits) {
    if (l.size() > text.size() - p) continue;
    size_t k = 0;
    while (k < l.size() && (icase ? lower(text[p + k]) == lower((uint8_t)l[k]) : text[p + k] == (uint8_t)l[k])) ++k;
    if (k == l.size()) return (uint32_t)l.size();
  }
  return 0;
}

static void one_case(std::mt19937& rng, const std::string& alphabet, size_t nlits, size_t min_len, size_t max_len, bool icase) {
  std::vector<std::string> lits;
  for (size_t i = 0; i < nlits; ++i) {
    std::string l(min_len + rng() % (max_len - min_len + 1), ' ');
    for (char& c : l) c = alphabet[rng() % alphabet.size()];
    lits.push_back(l);
  }
  lits[rng() % nlits].resize(min_len);  // the shortest literal is min_len bytes: g = min(min_len, 4)
  std::string list;
  for (size_t i = 0; i < nlits; ++i) list += (i ? "\n" : "") + lits[i];
  if (rng() & 1) list += "\n";
  xsg::SetProgram prog;
  std::string err;
  const bool ok = xsg::compile_literal_set((const uint8_t*)list.data(), list.size(), icase, &prog, &err);
  CHECK(ok, "compile failed: %s", err.c_str());
  if (!ok) return;
  CHECK(prog.count == nlits && prog.min_len == min_len && prog.g == std::min<size_t>(min_len, 4), "wrong numbers");
  // the text: random bytes of the alphabet with literals pasted in, exactly sized (the sanitizer sees every byte past it)
  std::vector<uint8_t> text(200 + rng() % 3000);
  for (uint8_t& b : text) b = (uint8_t)alphabet[rng() % alphabet.size()];
  for (int k = 0; k < 40; ++k) {
    const std::string& l = lits[rng() % nlits];
    if (l.size() > text.size()) continue;
    const size_t at = k == 0 ? text.size() - l.size() : rng() % (text.size() - l.size() + 1);  // one ends exactly at the end
    memcpy(text.data() + at, l.data(), l.size());
  }
  uint32_t off[4];
  const std::vector<uint8_t> blob = prog.blob(off);
  xsg::SetTable dev;  // the table as the kernel builds it from the device image
  dev.keys = reinterpret_cast<const uint32_t*>(blob.data() + off[0]);
  dev.first = reinterpret_cast<const uint32_t*>(blob.data() + off[1]);
  dev.ent = reinterpret_cast<const uint32_t*>(blob.data() + off[2]);
  dev.bytes = blob.data() + off[3];
  dev.ngrams = (uint32_t)prog.keys.size();
  dev.g = prog.g;
  const uint32_t* filter = reinterpret_cast<const uint32_t*>(blob.data());
  const xsg::SetTable host = prog.table();
  for (size_t p = 0; p + prog.g <= text.size(); ++p) {
    const uint32_t want = model_at(lits, text, p, icase);
    const bool candidate = xsg::set_filter_has(filter, xsg::set_gram_at(text.data() + p, prog.g, icase), prog.g);
    CHECK(!want || candidate, "false negative of the filter at %zu", p);
    const uint32_t got = xsg::set_verify_at(host, text.data(), p, text.size(), icase);
    CHECK(got == want, "verify at %zu: %u, model %u", p, got, want);
    CHECK(xsg::set_verify_at(dev, text.data(), p, text.size(), icase) == want, "verify from the device image at %zu", p);
  }
  for (size_t p = text.size() - std::min<size_t>(text.size(), prog.g) + 1; p < text.size(); ++p)  // no room for a gram: no literal fits either
    CHECK(model_at(lits, text, p, icase) == 0, "a literal shorter than the gram?");
}

int main() {
  std::mt19937 rng(12345);
  const std::string alphabets[] = {"ab", "abcAB \n", "etaoinshrETAOIN ", std::string("\x00\x01\x7f\x80\xfe\xff z", 8)};
  int cases = 0;
  for (const std::string& alpha : alphabets) {
    std::string a = alpha;
    a.erase(std::remove(a.begin(), a.end(), '\n'), a.end());  // (literals hold no newline; the text may)
    for (size_t min_len : {1, 2, 3, 4, 9})
      for (size_t nlits : {1, 2, 9, 300})
        for (bool icase : {false, true}) {
          one_case(rng, a, nlits, min_len, std::max<size_t>(min_len, nlits == 300 ? 12 : 255), icase);
          ++cases;
        }
  }
  // the limits of the list itself
  xsg::SetProgram prog;
  std::string err;
  CHECK(!xsg::compile_literal_set((const uint8_t*)"", 0, false, &prog, &err), "empty list accepted");
  CHECK(!xsg::compile_literal_set((const uint8_t*)"a\n\nb", 4, false, &prog, &err), "empty literal accepted");
  CHECK(!xsg::compile_literal_set((const uint8_t*)"\na", 2, false, &prog, &err), "leading newline accepted");
  const std::string long_lit(256, 'x');
  CHECK(!xsg::compile_literal_set((const uint8_t*)long_lit.data(), 256, false, &prog, &err), "256 bytes accepted");
  CHECK(xsg::compile_literal_set((const uint8_t*)long_lit.data(), 255, false, &prog, &err) && prog.max_len == 255, "255 bytes refused");
  if (failures) return 1;
  std::printf("set_selftest ok: %d cases\n", cases);
  return 0;
}
