// words_selftest.cpp -- XSG_LIST_WHOLE_WORDS in the verify step (x-search_amd/csrc/xsg_set.h: SetTable::words, set_entry_at)
// on its own, built with -fsanitize=address,undefined by tests/test_words_host.py and run as a process: no GPU, no library.
// Every chunk is a heap block of EXACTLY L bytes, so a read of chunk[-1] or chunk[L] is a sanitizer report.
//   1. neighbours: one literal with each of the 256 byte values in front of it and behind it -- set_verify_at and
//      set_count_at against the 63-byte set, g = 1..4, with and without ignore-case, and with words off;
//   2. edges: the literal at p == 0, ending at p + len == L, and as the whole chunk (a chunk of one byte too);
//   3. the walk's rule on the issue's strings: the first-listed ADMISSIBLE literal at a position, and a short literal that
//      is admissible only where the long one is not;
//   4. random lists and texts over an alphabet of word and non-word bytes against a brute-force model, at every position.
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
// the 63-byte set, spelled out
static bool word_byte(uint8_t b) { return b != 0 && std::strchr("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_", b) != nullptr; }

// a chunk of exactly n heap bytes
struct Chunk {
  std::unique_ptr<uint8_t[]> p;
  size_t n;
  explicit Chunk(const std::string& s) : p(new uint8_t[s.size() ? s.size() : 1]), n(s.size()) { memcpy(p.get(), s.data(), s.size()); }
  const uint8_t* data() const { return p.get(); }
};

static bool occurs(const std::string& l, const Chunk& c, size_t p, bool icase) {
  if (l.size() > c.n - p) return false;
  for (size_t k = 0; k < l.size(); ++k)
    if (icase ? lower(c.p[p + k]) != lower((uint8_t)l[k]) : c.p[p + k] != (uint8_t)l[k]) return false;
  return true;
}
static bool admissible(const std::string& l, const Chunk& c, size_t p, bool words) {
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

// verify and count at EVERY position with room for a gram against the model; -> matches of set_verify_at
static size_t check_chunk(const xsg::SetProgram& prog, const std::vector<std::string>& lits, const Chunk& c, bool icase, bool words,
                          const char* what) {
  xsg::SetTable T = prog.table();
  T.words = words ? 1u : 0u;
  size_t found = 0;
  for (size_t p = 0; p + prog.g <= c.n; ++p) {
    uint32_t want_len = 0;
    std::vector<uint32_t> want(lits.size(), 0), got(lits.size(), 0);
    for (size_t j = 0; j < lits.size(); ++j)
      if (occurs(lits[j], c, p, icase) && admissible(lits[j], c, p, words)) {
        want[j] = 1;
        if (!want_len) want_len = (uint32_t)lits[j].size();
      }
    const uint32_t len = xsg::set_verify_at(T, c.data(), p, c.n, icase);
    CHECK(len == want_len, "%s: verify at %zu of %zu: %u, model %u", what, p, c.n, len, want_len);
    xsg::set_count_at(T, c.data(), p, c.n, icase, [&](uint32_t j) { ++got[j]; });
    CHECK(got == want, "%s: count at %zu of %zu differs from the model", what, p, c.n);
    found += len != 0;
  }
  return found;
}

static void neighbours() {
  const std::string lits_by_g[] = {"x", "Zq", "a-b", "wOrd", "Sherlock"};
  for (const std::string& lit : lits_by_g)
    for (bool icase : {false, true}) {
      const xsg::SetProgram prog = compile({lit}, icase);
      CHECK(prog.g == std::min<size_t>(lit.size(), 4), "neighbours: wrong gram");
      for (int b = 0; b < 256; ++b) {
        const std::string byte(1, (char)b);
        // in front, behind, on both sides; the other side is the chunk's edge or a blank
        const std::string texts[] = {byte + lit, lit + byte, byte + lit + byte, byte + lit + " ", " " + lit + byte};
        for (const std::string& t : texts) {
          const Chunk c(t);
          const size_t with = check_chunk(prog, {lit}, c, icase, true, "neighbours");
          check_chunk(prog, {lit}, c, icase, false, "neighbours, words off");
          // (one occurrence per text unless the neighbour byte makes a second one: the model has decided, this pins the set)
          if (lit.size() > 1) {
            const bool blocked = word_byte((uint8_t)b);
            CHECK(with == (blocked ? 0u : 1u), "neighbours: byte %d around `%s`: %zu matches", b, lit.c_str(), with);
          }
        }
      }
    }
  int nword = 0;
  for (int b = 0; b < 256; ++b) {
    CHECK(xsg::set_word_byte((uint8_t)b) == word_byte((uint8_t)b), "set_word_byte(%d)", b);
    nword += xsg::set_word_byte((uint8_t)b);
  }
  CHECK(nword == 63, "the set holds %d bytes", nword);
}

static void edges() {
  for (bool icase : {false, true}) {
    const std::vector<std::string> lits = {"ab", "a", "abc"};
    const xsg::SetProgram prog = compile(lits, icase);
    struct {
      const char* text;
      size_t matches;
    } rows[] = {{"a", 1},          // a 1-byte chunk holding a 1-byte literal
                {"ab", 1},         // the whole chunk
                {"abc", 1},        // `ab` and `a` are not admissible at 0, `abc` is
                {"ab cd", 1},      // p == 0
                {"cd ab", 1},      // p + len == L
                {"xab", 0},        // the word byte inside the chunk, in front
                {"abx", 0},        // ... and behind
                {"a a", 2},
                {"-a-ab-abc-", 3},
                {"_a_", 0},
                {"9a", 0},
                {"a\nab\nabc", 3},
                {"a\xc3\xa9 \xe9" "ab", 2}};  // bytes >= 0x80 are no word bytes
    for (const auto& r : rows) {
      const Chunk c(r.text);
      const size_t got = check_chunk(prog, lits, c, icase, true, r.text);
      CHECK(got == r.matches, "edges: `%s`: %zu matches, expected %zu", r.text, got, r.matches);
      check_chunk(prog, lits, c, icase, false, r.text);
    }
  }
  // the literal's own edge bytes do not matter: `-x-` in `a-x-b` has word bytes as neighbours
  const xsg::SetProgram pd = compile({"-x-"}, false);
  CHECK(check_chunk(pd, {"-x-"}, Chunk("a-x-b"), false, true, "a-x-b") == 0, "`-x-` in `a-x-b` is admissible");
  CHECK(check_chunk(pd, {"-x-"}, Chunk(" -x- "), false, true, " -x- ") == 1, "`-x-` between blanks is not admissible");
  CHECK(check_chunk(pd, {"-x-"}, Chunk("-x-"), false, true, "-x-") == 1, "`-x-` as the whole chunk is not admissible");
}

static void walk_rule() {
  // (ab, abc) on `abc ab abcd`: abc@0 (ab is not admissible there), ab@4, nothing at 7
  for (int order = 0; order < 2; ++order) {
    const std::vector<std::string> lits = order ? std::vector<std::string>{"abc", "ab"} : std::vector<std::string>{"ab", "abc"};
    const xsg::SetProgram prog = compile(lits, false);
    xsg::SetTable T = prog.table();
    T.words = 1u;
    const Chunk c("abc ab abcd");
    CHECK(xsg::set_verify_at(T, c.data(), 0, c.n, false) == 3, "abc at 0");
    CHECK(xsg::set_verify_at(T, c.data(), 4, c.n, false) == 2, "ab at 4");
    CHECK(xsg::set_verify_at(T, c.data(), 7, c.n, false) == 0, "nothing at 7");
    check_chunk(prog, lits, c, false, true, "walk");
  }
  // duplicates get the same count each
  const std::vector<std::string> dup = {"the", "cat", "the"};
  const xsg::SetProgram prog = compile(dup, true);
  check_chunk(prog, dup, Chunk("The cat, the other and THE\nthen"), true, true, "duplicates");
}

static void random_cases() {
  std::mt19937 rng(777);
  const std::string alphabets[] = {"ab ", "ab_-", "abAB9 .\n", std::string("a\x00\x80\xff z_", 7)};
  int cases = 0;
  for (const std::string& alpha : alphabets) {
    std::string a = alpha;
    a.erase(std::remove(a.begin(), a.end(), '\n'), a.end());
    for (size_t min_len : {1, 2, 3, 4, 6})
      for (size_t nlits : {1, 3, 40})
        for (bool icase : {false, true}) {
          std::vector<std::string> lits;
          for (size_t i = 0; i < nlits; ++i) {
            std::string l(min_len + rng() % 3, ' ');
            for (char& ch : l) ch = a[rng() % a.size()];
            lits.push_back(l);
          }
          lits[rng() % nlits].resize(min_len);
          if (nlits > 1) lits[nlits - 1] = lits[0];  // a duplicate
          const xsg::SetProgram prog = compile(lits, icase);
          std::string text(1 + rng() % 400, ' ');
          for (char& ch : text) ch = alpha[rng() % alpha.size()];
          for (int k = 0; k < 12; ++k) {
            const std::string& l = lits[rng() % nlits];
            if (l.size() > text.size()) continue;
            const size_t at = k == 0 ? 0 : k == 1 ? text.size() - l.size() : rng() % (text.size() - l.size() + 1);
            memcpy(&text[at], l.data(), l.size());
          }
          const Chunk c(text);
          check_chunk(prog, lits, c, icase, true, "random");
          check_chunk(prog, lits, c, icase, false, "random, words off");
          ++cases;
        }
  }
  std::printf("random cases: %d\n", cases);
}

int main() {
  neighbours();
  edges();
  walk_rule();
  random_cases();
  if (failures) return 1;
  std::printf("words_selftest ok\n");
  return 0;
}
