// literal_counts_selftest.cpp -- set_count_at (x-search_amd/csrc/xsg_set.h), the function k_set_count_literals runs at
// every candidate, on its own: built with -fsanitize=address,undefined by tests/test_literal_counts_host.py and run as a
// process -- no GPU, no library, nothing loaded.  The table is rebuilt from the device image (SetProgram::blob and
// idx_offset), as the kernel builds it; the histogram it fills by visiting EVERY position with room for a gram must equal
// a naive double loop over literals and positions.  Texts are exactly sized, so the sanitizer sees a compare that reads
// behind a chunk's end.
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

// the model: for every literal, every position at which it occurs with its whole length inside the text
static std::vector<uint64_t> naive(const std::vector<std::string>& lits, const std::vector<uint8_t>& text, bool icase) {
  std::vector<uint64_t> n(lits.size(), 0);
  for (size_t j = 0; j < lits.size(); ++j) {
    const std::string& l = lits[j];
    for (size_t p = 0; p + l.size() <= text.size(); ++p) {
      size_t k = 0;
      while (k < l.size() && (icase ? lower(text[p + k]) == lower((uint8_t)l[k]) : text[p + k] == (uint8_t)l[k])) ++k;
      n[j] += k == l.size();
    }
  }
  return n;
}

// the histogram of set_count_at over the text, with the table of the device image
static std::vector<uint64_t> counted(const std::vector<std::string>& lits, const std::vector<uint8_t>& text, bool icase,
                                     const char* what, uint32_t want_g = 0) {
  std::string list;
  for (size_t i = 0; i < lits.size(); ++i) list += (i ? "\n" : "") + lits[i];
  xsg::SetProgram prog;
  std::string err;
  std::vector<uint64_t> n(lits.size(), 0);
  const bool ok = xsg::compile_literal_set((const uint8_t*)list.data(), list.size(), icase, &prog, &err);
  CHECK(ok, "%s: compile failed: %s", what, err.c_str());
  if (!ok) return n;
  CHECK(prog.count == lits.size() && prog.idx.size() == lits.size() && prog.ent.size() == lits.size(), "%s: wrong sizes", what);
  CHECK(!want_g || prog.g == want_g, "%s: gram length %u", what, prog.g);
  uint32_t off[4];
  const std::vector<uint8_t> blob = prog.blob(off);
  const uint32_t idx_off = prog.idx_offset();
  CHECK(idx_off % 16 == 0 && idx_off >= off[3] + prog.bytes.size() && idx_off + 2 * lits.size() <= blob.size(), "%s: idx lies at %u", what, idx_off);
  xsg::SetTable dev;
  dev.keys = reinterpret_cast<const uint32_t*>(blob.data() + off[0]);
  dev.first = reinterpret_cast<const uint32_t*>(blob.data() + off[1]);
  dev.ent = reinterpret_cast<const uint32_t*>(blob.data() + off[2]);
  dev.bytes = blob.data() + off[3];
  dev.ngrams = (uint32_t)prog.keys.size();
  dev.g = prog.g;
  dev.idx = reinterpret_cast<const uint16_t*>(blob.data() + idx_off);
  std::vector<uint8_t> seen(lits.size(), 0);  // every listing index is some entry's, once
  for (size_t e = 0; e < lits.size(); ++e) {
    CHECK(dev.idx[e] < lits.size() && !seen[dev.idx[e]], "%s: idx[%zu] = %u", what, e, dev.idx[e]);
    if (dev.idx[e] < lits.size()) seen[dev.idx[e]] = 1;
  }
  const std::vector<uint32_t> keys_copy(prog.keys);  // (the kernel searches a copy of the keys in LDS)
  for (size_t p = 0; p + prog.g <= text.size(); ++p) {
    uint32_t last = UINT32_MAX, visits = 0;
    xsg::set_count_at(dev, text.data(), p, text.size(), icase, [&](uint32_t i) {
      CHECK(i < lits.size(), "%s: visit(%u)", what, i);
      if (i < lits.size()) ++n[i];
      last = i, ++visits;
    }, (p & 1) ? keys_copy.data() : dev.keys);
    (void)last;
    CHECK(visits <= lits.size(), "%s: %u visits at %zu", what, visits, p);
  }
  return n;
}

static void compare(const std::vector<std::string>& lits, const std::vector<uint8_t>& text, bool icase, const char* what,
                    uint32_t want_g = 0, uint64_t want_total_at_least = 0) {
  const std::vector<uint64_t> want = naive(lits, text, icase), got = counted(lits, text, icase, what, want_g);
  uint64_t total = 0;
  for (size_t j = 0; j < lits.size(); ++j) {
    CHECK(got[j] == want[j], "%s (icase %d): literal %zu: %llu, naive %llu", what, (int)icase, j, (unsigned long long)got[j],
          (unsigned long long)want[j]);
    total += want[j];
  }
  CHECK(total >= want_total_at_least, "%s: the case holds %llu occurrences, built for %llu", what, (unsigned long long)total,
        (unsigned long long)want_total_at_least);
}

static std::vector<uint8_t> bytes_of(const std::string& s) { return std::vector<uint8_t>(s.begin(), s.end()); }
#define S(lit) std::string(lit, sizeof(lit) - 1)  // a string literal with NUL bytes inside it

static void fixed_cases() {
  for (bool icase : {false, true}) {
    // occurrences, not matches: overlaps, covered literals, duplicates
    compare({"aa"}, bytes_of("aaaa"), icase, "aa in aaaa", 2, 3);
    compare({"abab"}, bytes_of("ababab"), icase, "abab in ababab", 4, 2);
    compare({"ab", "abc"}, bytes_of("abc"), icase, "ab, abc on abc", 2, 2);
    compare({"abc", "ab", "b", "abc", "bc"}, bytes_of("xabcabxbcABC"), icase, "prefix, infix, duplicate", 1, icase ? 13 : 9);
    // 4096 literals under ONE gram (tests/set_edge_cases.py: limit_shared), the short one listed late
    const std::string a16 = "abcdefghijklmnop";
    std::vector<std::string> shared;
    for (int i = 0; i < 4096; ++i) shared.push_back(std::string("abcd") + a16[i >> 8] + a16[(i >> 4) & 15] + a16[i & 15]);
    shared[3000] = "abcdb";
    // room = len (`abcdb` as the last bytes) and room = len - 1 (`abcdba` lacks one byte of `abcdbaa`, listed first)
    compare(shared, bytes_of("abcdbaa abcdbaq abcdqaa ABCDAAA\nabcdppp abcdlli abcdb"), icase, "shared gram, room = len", 4, icase ? 6 : 5);
    compare(shared, bytes_of("abcdppp abcdbaa abcdba"), icase, "shared gram, room = len - 1", 4, 4);
    compare(shared, bytes_of("abcd"), icase, "shared gram, a gram and nothing else", 4, 0);
    // a 255-byte literal: whole, cut one byte short, and ending exactly at the end
    std::string long_lit;
    for (int i = 0; i < 255; ++i) long_lit += (char)('A' + (i * 7 + i / 26) % 26);
    const std::vector<std::string> longs = {long_lit, long_lit.substr(0, 4), long_lit.substr(1, 40)};
    compare(longs, bytes_of("x" + long_lit + "y" + long_lit.substr(0, 254) + " " + long_lit), icase, "255 bytes", 4, 8);
    compare(longs, bytes_of(long_lit.substr(0, 254)), icase, "255 bytes, room = len - 1", 4, 2);
    // NUL literals
    const std::string z1(1, '\0'), z2(2, '\0'), z4(4, '\0');
    const std::string nul_text = S("a\0b a\0\0b\n\0\0\0\0\0 a\0B\n") + std::string(30, 'x') + S("\0\0\0\0a\0b\0");
    compare({z1}, bytes_of(nul_text), icase, "NUL", 1, 15);
    compare({z2, z1}, bytes_of(nul_text), icase, "NUL NUL, NUL", 1, 20);
    compare({S("a\0b"), z4}, bytes_of(nul_text), icase, "a NUL b, four NULs", 3, icase ? 6 : 5);
    // bytes >= 0x80: nothing folds there
    const std::vector<std::string> raw = {"\xff\xfe", "caf\xe9", "\x80", "\xc1\xe1"};
    compare(raw, bytes_of("caf\xe9 CAF\xe9 caf\xc9 \xff\xfe\xff\xfe \x80\x80 \xc1\xe1 \xe1\xc1 \xc1\xc1 \xff"), icase, "raw bytes", 1, icase ? 7 : 6);
  }
}

static void random_cases() {
  std::mt19937 rng(4711);
  const std::string alphabets[] = {"ab", "abcAB ", "etaoinshrETAOIN ", std::string("\x00\x01\x7f\x80\xfe\xff z", 8)};
  for (const std::string& alpha : alphabets)
    for (size_t min_len : {1, 2, 3, 4, 9})
      for (size_t nlits : {1, 2, 9, 300})
        for (bool icase : {false, true}) {
          std::vector<std::string> lits;
          const size_t max_len = std::max<size_t>(min_len, nlits == 300 ? 12 : 60);
          for (size_t i = 0; i < nlits; ++i) {
            std::string l(min_len + rng() % (max_len - min_len + 1), ' ');
            for (char& c : l) c = alpha[rng() % alpha.size()];
            lits.push_back(l);
          }
          if (nlits > 2) lits[1] = lits[nlits - 1];  // a duplicate
          lits[rng() % nlits].resize(min_len);       // the shortest literal is min_len bytes: g = min(min_len, 4)
          std::vector<uint8_t> text(100 + rng() % 1500);
          for (uint8_t& b : text) b = (uint8_t)alpha[rng() % alpha.size()];
          for (int k = 0; k < 30; ++k) {
            const std::string& l = lits[rng() % nlits];
            if (l.size() > text.size()) continue;
            const size_t at = k == 0 ? text.size() - l.size() : rng() % (text.size() - l.size() + 1);  // one ends exactly at the end
            memcpy(text.data() + at, l.data(), l.size());
          }
          compare(lits, text, icase, "random", (uint32_t)std::min<size_t>(min_len, 4));
        }
}

int main() {
  fixed_cases();
  random_cases();
  if (failures) return 1;
  std::printf("literal_counts_selftest ok\n");
  return 0;
}
