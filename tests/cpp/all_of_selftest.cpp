// all_of_selftest.cpp -- set_mask_at (x-search_amd/csrc/xsg_set.h), the verify step of XSG_LIST_ALL_OF, on its own: built with
// -fsanitize=address,undefined by tests/test_all_of_host.py and run as a process: no GPU, no library.  Every chunk is a heap
// block of EXACTLY L bytes, so a read of chunk[-1] or chunk[L] is a sanitizer report.
//   1. the strings of the header: covered and overlapping occurrences serve different literals, duplicates set both bits;
//   2. the last possible position: every literal of a list ending exactly at L, starting at L - g, and one byte too long;
//   3. g = 1..4, with and without ignore-case and whole words, at EVERY position with room for a gram against a brute-force
//      model, on random texts over an alphabet of word and non-word bytes;
//   4. a list of 64 literals: listing index 63 is bit 63 (no shift by 64, no bit lost), alone and with all the others.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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
static bool word_byte(uint8_t b) { return b != 0 && std::strchr("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_", b) != nullptr; }

// a chunk of exactly n heap bytes
struct Chunk {
  std::unique_ptr<uint8_t[]> p;
  size_t n;
  explicit Chunk(const std::string& s) : p(new uint8_t[s.size() ? s.size() : 1]), n(s.size()) { memcpy(p.get(), s.data(), s.size()); }
  const uint8_t* data() const { return p.get(); }
};

static bool occurs(const std::string& l, const Chunk& c, size_t p, bool icase, bool words) {
  if (l.size() > c.n - p) return false;
  for (size_t k = 0; k < l.size(); ++k)
    if (icase ? lower(c.p[p + k]) != lower((uint8_t)l[k]) : c.p[p + k] != (uint8_t)l[k]) return false;
  if (!words) return true;
  return (p == 0 || !word_byte(c.p[p - 1])) && (p + l.size() == c.n || !word_byte(c.p[p + l.size()]));
}

static xsg::SetProgram compile(const std::vector<std::string>& lits, bool icase) {
  std::string list;
  for (size_t i = 0; i < lits.size(); ++i) list += (i ? "\n" : "") + lits[i];
  xsg::SetProgram prog;
  std::string err;
  CHECK(xsg::compile_literal_set((const uint8_t*)list.data(), list.size(), icase, &prog, &err), "compile failed: %s", err.c_str());
  CHECK(prog.count == lits.size(), "wrong count");
  return prog;
}

// set_mask_at at EVERY position with room for a gram against the model; -> the OR of all masks
static uint64_t check_chunk(const xsg::SetProgram& prog, const std::vector<std::string>& lits, const Chunk& c, bool icase, bool words,
                            const char* what) {
  xsg::SetTable T = prog.table();
  T.words = words ? 1u : 0u;
  uint64_t all = 0;
  for (size_t p = 0; p + prog.g <= c.n; ++p) {
    uint64_t want = 0;
    for (size_t j = 0; j < lits.size(); ++j)
      if (occurs(lits[j], c, p, icase, words)) want |= 1ull << j;
    const uint64_t got = xsg::set_mask_at(T, c.data(), p, c.n, icase);
    CHECK(got == want, "%s: mask at %zu of %zu: %llx, model %llx", what, p, c.n, (unsigned long long)got, (unsigned long long)want);
    all |= got;
  }
  return all;
}

static void header_strings() {
  {
    const std::vector<std::string> lits = {"ab", "abc"};
    const xsg::SetProgram prog = compile(lits, false);
    const Chunk c("abc");
    CHECK(xsg::set_mask_at(prog.table(), c.data(), 0, c.n, false) == 3ull, "ab + abc on abc: both at 0");
    CHECK(check_chunk(prog, lits, c, false, false, "ab+abc") == 3ull, "ab + abc on abc");
    const Chunk d("ab");  // the longer literal does not fit the room: no byte behind the chunk is read
    CHECK(check_chunk(prog, lits, d, false, false, "ab+abc on ab") == 1ull, "ab + abc on ab");
  }
  {
    const std::vector<std::string> lits = {"aa", "aaa"};
    const xsg::SetProgram prog = compile(lits, false);
    const Chunk c("aaa");
    CHECK(xsg::set_mask_at(prog.table(), c.data(), 0, c.n, false) == 3ull, "aa + aaa on aaa at 0");
    CHECK(xsg::set_mask_at(prog.table(), c.data(), 1, c.n, false) == 1ull, "aa + aaa on aaa at 1");
  }
  {
    const std::vector<std::string> lits = {"he", "the", "he"};  // a duplicate: both bits, one requirement for the host
    const xsg::SetProgram prog = compile(lits, false);
    const Chunk c("the he");
    CHECK(check_chunk(prog, lits, c, false, false, "dup") == 7ull, "duplicates");
    CHECK(check_chunk(prog, lits, c, false, true, "dup words") == 7ull, "duplicates, whole words");
    const Chunk e("the");  // `he` inside `the` is no word; `the` between the chunk's edges is
    CHECK(check_chunk(prog, lits, e, false, true, "he in the") == 2ull, "he inside the");
    const Chunk f("he");   // at both edges of the chunk
    CHECK(check_chunk(prog, lits, f, false, true, "he at the edges") == 5ull, "he at the chunk's edges");
  }
}

static void last_position() {
  for (uint32_t g = 1; g <= 4; ++g) {
    std::vector<std::string> lits;
    for (uint32_t n = g; n <= g + 5; ++n) lits.push_back(std::string("wxyz").substr(0, g) + std::string(n - g, 'q'));
    for (bool icase : {false, true}) {
      const xsg::SetProgram prog = compile(lits, icase);
      CHECK(prog.g == g, "last position: gram %u, not %u", prog.g, g);
      for (size_t j = 0; j < lits.size(); ++j)
        for (size_t pad : {(size_t)0, (size_t)1, (size_t)17}) {
          // literal j ends exactly at L: the longer ones lack room, the shorter ones are its prefixes
          const Chunk c(std::string(pad, '.') + (icase ? std::string("WXYZ").substr(0, g) + std::string(lits[j].size() - g, 'Q') : lits[j]));
          xsg::SetTable T = prog.table();
          const uint64_t got = xsg::set_mask_at(T, c.data(), pad, c.n, icase);
          CHECK(got == (2ull << j) - 1ull, "last position: g %u literal %zu pad %zu: %llx", g, j, pad, (unsigned long long)got);
          check_chunk(prog, lits, c, icase, false, "last position");
          check_chunk(prog, lits, c, icase, true, "last position, words");
          // the gram alone as the chunk's last g bytes: p = L - g, the last position the scan reports
          const Chunk tail(std::string(pad, '.') + lits[0]);
          CHECK(xsg::set_mask_at(T, tail.data(), tail.n - g, tail.n, icase) == 1ull, "last position: the gram at L - g");
        }
    }
  }
}

static void random_lists() {
  std::mt19937 rng(20260101u);
  const std::string alpha = "abAB_7 -.\n\xe9";
  size_t hits = 0;
  for (int round = 0; round < 400; ++round) {
    const uint32_t g = 1 + round % 4;
    std::vector<std::string> lits;
    const size_t k = 1 + rng() % 8;
    while (lits.size() < k) {
      std::string l;
      const size_t n = g + rng() % 4;
      while (l.size() < n) {
        const char ch = alpha[rng() % alpha.size()];
        if (ch != '\n') l += ch;
      }
      lits.push_back(l);
    }
    lits.push_back(lits[0] + "b");
    lits.push_back(lits[0]);  // a duplicate
    std::string text;
    const size_t pieces = 5 + rng() % 40;
    for (size_t i = 0; i < pieces; ++i) text += rng() % 2 ? std::string(1, alpha[rng() % alpha.size()]) : lits[rng() % lits.size()];
    text += lits[rng() % lits.size()];  // (a literal as the chunk's last bytes)
    const Chunk c(text);
    for (bool icase : {false, true}) {
      const xsg::SetProgram prog = compile(lits, icase);
      for (bool words : {false, true}) hits += check_chunk(prog, lits, c, icase, words, "random") != 0;
    }
  }
  CHECK(hits > 1000, "random lists: only %zu chunks with an occurrence", hits);
}

static void index_63() {
  for (uint32_t g = 1; g <= 4; ++g) {
    // 64 literals under one gram: the gram itself, then the gram and j spelled with two letters; the 64th is listing index 63
    std::vector<std::string> lits;
    const std::string gram = std::string("kwxy").substr(0, g);
    for (int j = 0; j < 64; ++j) lits.push_back(gram + std::string(1, (char)('a' + j / 8)) + std::string(1, (char)('a' + j % 8)));
    lits[0] = gram;  // (the shortest literal sets the gram's length; it is a prefix of all the others: bit 0 everywhere)
    const xsg::SetProgram prog = compile(lits, false);
    CHECK(prog.g == g && prog.count == 64, "index 63: gram %u count %u", prog.g, prog.count);
    const Chunk last(lits[63]);
    const uint64_t got = xsg::set_mask_at(prog.table(), last.data(), 0, last.n, false);
    CHECK((got >> 63) == 1ull, "index 63: bit 63 missing in %llx (g %u)", (unsigned long long)got, g);
    CHECK((got & ~((1ull << 63) | 1ull)) == 0ull && (got & 1ull), "index 63: stray bits in %llx (g %u)", (unsigned long long)got, g);
    std::string text;
    for (const std::string& l : lits) text += l + " ";
    text.pop_back();
    const Chunk c(text);
    CHECK(check_chunk(prog, lits, c, false, false, "index 63") == ~0ull, "index 63: the OR over all 64 is not full (g %u)", g);
    CHECK(check_chunk(prog, lits, c, false, true, "index 63, words") == ~0ull, "index 63, words: not full (g %u)", g);
    // 64 times the same literal: every bit from one position
    const std::vector<std::string> same(64, gram + "zz");
    const xsg::SetProgram dup = compile(same, false);
    const Chunk one(gram + "zz");
    CHECK(xsg::set_mask_at(dup.table(), one.data(), 0, one.n, false) == ~0ull, "index 63: 64 duplicates (g %u)", g);
  }
}

int main() {
  header_strings();
  last_position();
  random_lists();
  index_63();
  if (failures) {
    std::fprintf(stderr, "all_of_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("all_of_selftest ok\n");
  return 0;
}
