// set_selftest.cpp -- the host side of a literal list (x-search_amd/csrc/xsg_set.h/.cpp) on its own, built with
// -fsanitize=address,undefined by tests/test_set_host.py and run as a process: no GPU, no library, nothing loaded.
//   1. no false negative: at every position where a literal truly occurs, the host copy of the filter test passes;
//   2. the host copy of the verify step (set_verify_at, the function k_set_verify runs) equals a brute-force model --
//      the first-listed literal that occurs at the position, bounded by the chunk length -- at EVERY position with room
//      for a gram, and the blob the device receives holds the same table;
//   3. fixed cases (tests/set_edge_cases.py searches the same strings on the device): grams that share a filter bit with a
//      literal's gram without being it, 4096 literals under one gram with a chunk end that only a late-listed short one
//      fits into, 4096 literals under 4096 grams.  There the verify step runs where the kernel runs it: at candidates.
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

// ---- fixed cases: the verify step at the CANDIDATES of `text`, as k_set_verify runs it, against the model -----------------------
static xsg::SetProgram compile_fixed(const std::vector<std::string>& lits, bool icase) {
  std::string list;
  for (size_t i = 0; i < lits.size(); ++i) list += (i ? "\n" : "") + lits[i];
  xsg::SetProgram prog;
  std::string err;
  CHECK(xsg::compile_literal_set((const uint8_t*)list.data(), list.size(), icase, &prog, &err), "compile failed: %s", err.c_str());
  CHECK(prog.count == lits.size(), "wrong count");
  return prog;
}

// -> the number of candidates; every candidate's verify result equals the model's
static size_t verify_candidates(const xsg::SetProgram& prog, const std::vector<std::string>& lits, const std::vector<uint8_t>& text,
                                bool icase, const char* what) {
  const xsg::SetTable T = prog.table();
  size_t cands = 0;
  for (size_t p = 0; p + prog.g <= text.size(); ++p) {
    const uint32_t want = model_at(lits, text, p, icase);
    const bool candidate = xsg::set_filter_has(prog.filter.data(), xsg::set_gram_at(text.data() + p, prog.g, icase), prog.g);
    CHECK(!want || candidate, "%s: false negative of the filter at %zu", what, p);
    if (!candidate) continue;
    ++cands;
    const uint32_t got = xsg::set_verify_at(T, text.data(), p, text.size(), icase);
    CHECK(got == want, "%s: verify at candidate %zu: %u, model %u", what, p, got, want);
  }
  return cands;
}

static std::vector<uint8_t> bytes_of(const std::string& s) { return std::vector<uint8_t>(s.begin(), s.end()); }

// the first eight printable grams that collide with each literal's gram (tests/set_edge_cases.py: COLLIDING_PINNED)
static void collision_cases() {
  const struct {
    uint32_t g;
    const char* lit;
    const char* grams[8];
  } rows[] = {
      {3, "kqz", {"\":P", "&h%", "-@T", "N$M", "Uer", "Ye4", "`kv", "dk8"}},
      {3, "needle", {"%\\N", "0bR", ";:C", ";hV", "F@G", "QFK", "c$~", "g$@"}},
      {4, "kqzw", {"/_h!", ":el!", ">e.!", "Ekp!", "Ik2!", "PCa!", "TC#!", "[Ie!"}},
      {4, "needle", {"!vp!", "%v2!", ",|t!", "0|6!", "7Te!", ";T'!", "BZi!", "FZ+!"}},
  };
  for (uint32_t g : {3u, 4u}) {
    const std::vector<std::string> lits = {g == 3 ? "kqz" : "kqzw", "needle"};
    const xsg::SetProgram prog = compile_fixed(lits, false);
    CHECK(prog.g == g && prog.filter_bits_set == 2, "collisions: wrong gram length or filter");
    std::string text = "some text in front\n";
    std::vector<size_t> fakes;
    for (const auto& r : rows) {
      if (r.g != g) continue;
      const std::string lit = r.lit;
      const uint32_t h = xsg::set_gram_hash(xsg::set_gram_at((const uint8_t*)lit.data(), g, false), g);
      for (const char* c : r.grams) {
        const std::string gram = c;
        CHECK(gram.size() == g && gram != lit.substr(0, g), "collisions: bad row");
        CHECK(xsg::set_gram_hash(xsg::set_gram_at((const uint8_t*)gram.data(), g, false), g) == h, "%s does not collide with %s", c, r.lit);
        for (const std::string& l : lits) {  // gram + the rest of EVERY literal: whichever key a lookup without the equality test lands on
          fakes.push_back(text.size());
          text += gram + l.substr(g) + " more of it ";
        }
      }
      text += lit + "\n";  // a real occurrence
    }
    fakes.push_back(text.size());
    text += std::string(rows[g == 3 ? 0 : 2].grams[0]);  // a colliding gram as the last bytes
    const std::vector<uint8_t> t = bytes_of(text);
    for (size_t p : fakes) {
      CHECK(xsg::set_filter_has(prog.filter.data(), xsg::set_gram_at(t.data() + p, g, false), g), "collisions: %zu is no candidate", p);
      CHECK(model_at(lits, t, p, false) == 0, "collisions: the model matches at %zu", p);
    }
    CHECK(verify_candidates(prog, lits, t, false, "collisions") >= fakes.size() + 2, "collisions: too few candidates");
  }
}

static void limit_cases() {
  const std::string a16 = "abcdefghijklmnop", a8 = "abcdefgh";
  // 4096 literals under ONE gram, `abcdb` listed at place 3000 behind the 256 literals `abcdb??`
  std::vector<std::string> shared;
  for (int i = 0; i < 4096; ++i) shared.push_back(std::string("abcd") + a16[i >> 8] + a16[(i >> 4) & 15] + a16[i & 15]);
  shared[3000] = "abcdb";
  const xsg::SetProgram ps = compile_fixed(shared, false);
  CHECK(ps.keys.size() == 1 && ps.first.size() == 2 && ps.first[1] == 4096 && ps.filter_bits_set == 1, "shared gram: wrong table");
  // exactly sized: the sanitizer sees a compare that goes on behind `abcdb` (what lies behind the end on the device is `aa`)
  const std::vector<uint8_t> t1 = bytes_of("abcdbaa abcdbaq abcdqaa abcdaaa\nabcdppp abcdlli abcdb");
  CHECK(verify_candidates(ps, shared, t1, false, "shared gram") == 7, "shared gram: candidates");
  const xsg::SetTable T = ps.table();
  CHECK(xsg::set_verify_at(T, t1.data(), t1.size() - 5, t1.size(), false) == 5, "the short literal listed late does not get the room");
  CHECK(xsg::set_verify_at(T, t1.data(), 0, t1.size(), false) == 7 && xsg::set_verify_at(T, t1.data(), 8, t1.size(), false) == 5 &&
            xsg::set_verify_at(T, t1.data(), 16, t1.size(), false) == 0 && xsg::set_verify_at(T, t1.data(), 40, t1.size(), false) == 0,
        "shared gram: first-listed wins, the short one serves what no long one fits, nothing else matches");
  // 4096 distinct grams: the binary search at full depth, every key found and every neighbour value refused
  std::vector<std::string> distinct;
  for (int i = 0; i < 4096; ++i)
    distinct.push_back(std::string() + a8[(i >> 9) & 7] + a8[(i >> 6) & 7] + a8[(i >> 3) & 7] + a8[i & 7] + a8[(i * 5 + 3) & 7] + "ha");
  const xsg::SetProgram pd = compile_fixed(distinct, false);
  CHECK(pd.keys.size() == 4096 && pd.filter_bits_set > 3900, "distinct grams: wrong table");
  std::string text;
  for (int i = 0; i < 4096; i += 7) text += distinct[i] + (i % 3 ? "i" : "") + distinct[4095 - i].substr(0, 6);
  CHECK(verify_candidates(pd, distinct, bytes_of(text), false, "distinct grams") > 4096 / 7, "distinct grams: candidates");
}

int main() {
  collision_cases();
  limit_cases();
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
