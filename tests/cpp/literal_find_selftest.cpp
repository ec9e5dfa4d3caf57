// literal_find_selftest.cpp -- the host side of k_set_find_literals (x-search_amd/csrc/xsg_set_kernels.hip): the index
// arithmetic of csrc/xsg_litfind.h and set_count_at of csrc/xsg_set.h, replayed on the CPU as count pass -> prefix sum ->
// chunk_ptr gather -> fill pass, with four "waves" per tile, four wave-loads per wave, a queue per wave-load and rounds of
// 64 "lanes".  Built with -fsanitize=address,undefined by tests/test_literal_find_host.py and run as a process -- no GPU,
// no library, nothing loaded.  Every result is compared with a brute-force list of (chunk, position, literal) triples,
// under full capacity, total - 1 and 0, with guard words behind every array.  Texts are exactly sized, so the sanitizer
// sees a compare that reads behind a chunk's end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../x-search_amd/csrc/xsg_litfind.h"
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

constexpr uint64_t kTile = 16384, kSpan = 4096, kLoad = 1024;  // the kernel's kSetTile, kSetWaveSpan, kWaveLoad
constexpr uint64_t kGuard = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint32_t kGuard32 = 0xA5A5A5A5u;
constexpr size_t kSpare = 3;

struct Binding {
  std::vector<std::vector<uint8_t>> chunks;  // each exactly sized
  std::vector<uint64_t> goff, tile0;         // tile0: n + 1 entries
  std::vector<uint32_t> tile_chunk;
};

static Binding bind(std::vector<std::vector<uint8_t>> chunks, std::mt19937& rng) {
  Binding b;
  b.chunks = std::move(chunks);
  uint64_t g = rng() % 1000, t = 0;
  for (size_t c = 0; c < b.chunks.size(); ++c) {
    b.goff.push_back(g);
    g += b.chunks[c].size() + rng() % 7;  // (global offsets are the caller's: gaps are fine)
    b.tile0.push_back(t);
    const uint64_t nt = (b.chunks[c].size() + kTile - 1) / kTile;
    for (uint64_t i = 0; i < nt; ++i) b.tile_chunk.push_back((uint32_t)c);
    t += nt;
  }
  b.tile0.push_back(t);
  return b;
}

static uint8_t lower(uint8_t x) { return x >= 'A' && x <= 'Z' ? (uint8_t)(x + 32) : x; }

struct Hit {
  uint64_t pos;
  uint32_t lit;
};

// the definition: every (c, p, j) in ascending order
static void brute(const Binding& b, const std::vector<std::string>& lits, bool icase, bool words, std::vector<uint64_t>* chunk_ptr,
                  std::vector<Hit>* hits) {
  chunk_ptr->assign(1, 0);
  hits->clear();
  for (size_t c = 0; c < b.chunks.size(); ++c) {
    const std::vector<uint8_t>& d = b.chunks[c];
    for (size_t p = 0; p < d.size(); ++p)
      for (size_t j = 0; j < lits.size(); ++j) {
        const std::string& l = lits[j];
        if (p + l.size() > d.size()) continue;
        size_t k = 0;
        while (k < l.size() && (icase ? lower(d[p + k]) == lower((uint8_t)l[k]) : d[p + k] == (uint8_t)l[k])) ++k;
        if (k != l.size()) continue;
        if (words && ((p > 0 && xsg::set_word_byte(d[p - 1])) || (p + l.size() < d.size() && xsg::set_word_byte(d[p + l.size()])))) continue;
        hits->push_back(Hit{b.goff[c] + p, (uint32_t)j});
      }
    chunk_ptr->push_back(hits->size());
  }
}

struct Replay {
  const Binding& b;
  xsg::SetProgram prog;
  xsg::SetTable T;
  bool icase;
  std::vector<uint32_t> keys_copy;  // (the kernel searches a copy of the keys in LDS)

  Replay(const Binding& bb, const std::vector<std::string>& lits, bool ic, bool words) : b(bb), icase(ic) {
    std::string list, err;
    for (size_t i = 0; i < lits.size(); ++i) list += (i ? "\n" : "") + lits[i];
    const bool ok = xsg::compile_literal_set((const uint8_t*)list.data(), list.size(), icase, &prog, &err);
    CHECK(ok, "compile failed: %s", err.c_str());
    if (!ok) std::exit(1);
    T = prog.table();
    T.words = words ? 1u : 0u;
    keys_copy = prog.keys;
  }

  // the queue of one wave-load: the candidates of [load_off, load_off + 1 KiB) in ascending order, as offsets inside the load
  std::vector<uint16_t> queue(uint32_t c, uint64_t load_off) const {
    const std::vector<uint8_t>& d = b.chunks[c];
    const uint64_t L = d.size(), limit = L >= prog.g ? L - prog.g + 1u : 0u;
    std::vector<uint16_t> q;
    for (uint64_t o = 0; o < kLoad && load_off + o < limit; ++o)
      if (xsg::set_filter_has(prog.filter.data(), xsg::set_gram_at(d.data() + load_off + o, prog.g, icase), prog.g)) q.push_back((uint16_t)o);
    return q;
  }

  template <typename Visit>
  void at(uint32_t c, uint64_t p, Visit&& v) const {
    xsg::set_count_at(T, b.chunks[c].data(), p, b.chunks[c].size(), icase, v, keys_copy.data());
  }

  // count pass: one word per (tile, wave); `order`: the tiles in the order some grid would take them
  void count(const std::vector<uint64_t>& order, uint32_t* wave_occ) const {
    for (uint64_t tile : order)
      for (uint32_t wave = 0; wave < xsg::kLitFindSpans; ++wave) {
        const uint32_t c = b.tile_chunk[tile];
        const uint64_t wbase = (tile - b.tile0[c]) * kTile + wave * kSpan;
        uint32_t n = 0;
        for (uint64_t j = 0; j < kSpan / kLoad; ++j) {
          const uint64_t load_off = wbase + j * kLoad;
          for (uint16_t o : queue(c, load_off)) at(c, load_off + o, [&](uint32_t) { ++n; });
        }
        wave_occ[xsg::litfind_span_word(tile, wave)] = n;
      }
  }

  void fill(const std::vector<uint64_t>& order, const uint32_t* wave_occ, const uint64_t* wave_off, uint64_t* pos, uint32_t* lit,
            uint64_t cap) const {
    for (uint64_t tile : order)
      for (uint32_t wave = 0; wave < xsg::kLitFindSpans; ++wave) {
        const uint64_t word = xsg::litfind_span_word(tile, wave);
        if (wave_occ[word] == 0) continue;
        uint64_t at_e = wave_off[word];
        const uint32_t c = b.tile_chunk[tile];
        const uint64_t wbase = (tile - b.tile0[c]) * kTile + wave * kSpan;
        for (uint64_t j = 0; j < kSpan / kLoad; ++j) {
          const uint64_t load_off = wbase + j * kLoad;
          const std::vector<uint16_t> q = queue(c, load_off);
          const uint32_t total = (uint32_t)q.size(), rounds = xsg::litfind_rounds(total);
          CHECK(total <= 1024 && (uint64_t)rounds * xsg::kLitFindRound >= total && (rounds == 0 || (uint64_t)(rounds - 1) * xsg::kLitFindRound < total),
                "rounds of %u candidates: %u", total, rounds);
          for (uint32_t r = 0; r < rounds; ++r) {
            uint32_t hits[64], incl[64], run = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {  // every lane counts its candidate's hits, then the inclusive scan
              const uint32_t i = r * xsg::kLitFindRound + lane;
              hits[lane] = 0;
              if (i < total) at(c, load_off + q[i], [&](uint32_t) { ++hits[lane]; });
              run += hits[lane];
              incl[lane] = run;
            }
            for (uint32_t lane = 64; lane-- > 0;) {  // (the lanes store in no particular order: here, backwards)
              if (!hits[lane]) continue;
              const uint64_t p = load_off + q[r * xsg::kLitFindRound + lane];
              uint64_t e = xsg::litfind_slot(at_e, incl[lane], hits[lane]);
              at(c, p, [&](uint32_t idx) {
                if (xsg::litfind_stored(e, cap)) {
                  pos[e] = b.goff[c] + p;
                  lit[e] = idx;
                }
                ++e;
              });
            }
            at_e += incl[63];
          }
        }
        CHECK(at_e == wave_off[word + 1], "span %llu: the fill pass found %llu entries, the count pass %u", (unsigned long long)word,
              (unsigned long long)(at_e - wave_off[word]), wave_occ[word]);
      }
  }
};

static void run_case(const Binding& b, const std::vector<std::string>& lits, bool icase, bool words, std::mt19937& rng, const char* what,
                     uint64_t want_at_least = 0) {
  std::vector<uint64_t> want_ptr;
  std::vector<Hit> want;
  brute(b, lits, icase, words, &want_ptr, &want);
  CHECK(want.size() >= want_at_least, "%s: the case holds %zu occurrences, built for %llu", what, want.size(), (unsigned long long)want_at_least);
  const Replay R(b, lits, icase, words);
  const uint64_t ntiles = b.tile0.back(), nwords = xsg::litfind_words(ntiles), n = b.chunks.size();
  // the tiles in the order of a grid-stride loop over `grid` workgroups taken one after the other, and shuffled
  std::vector<std::vector<uint64_t>> orders;
  for (uint64_t grid : {(uint64_t)1, (uint64_t)3, ntiles ? ntiles : 1}) {
    std::vector<uint64_t> o;
    for (uint64_t w = 0; w < grid; ++w)
      for (uint64_t t = w; t < ntiles; t += grid) o.push_back(t);
    orders.push_back(o);
  }
  std::vector<uint64_t> shuffled = orders[0];
  std::shuffle(shuffled.begin(), shuffled.end(), rng);
  orders.push_back(shuffled);

  for (const std::vector<uint64_t>& order : orders) {
    std::vector<uint32_t> occ(nwords + kSpare, kGuard32);
    R.count(order, occ.data());
    for (size_t i = 0; i < kSpare; ++i) CHECK(occ[nwords + i] == kGuard32, "%s: a word behind wave_occ was written", what);
    for (uint64_t w = 0; w < nwords; ++w) CHECK(occ[w] <= 4096u * 4096u, "%s: wave_occ[%llu] = %u", what, (unsigned long long)w, occ[w]);
    std::vector<uint64_t> off(nwords + 1 + kSpare, kGuard);
    off[0] = 0;
    for (uint64_t w = 0; w < nwords; ++w) off[w + 1] = off[w] + occ[w];
    const uint64_t total = off[nwords];
    CHECK(total == want.size(), "%s: total %llu, brute force %zu", what, (unsigned long long)total, want.size());
    std::vector<uint64_t> chunk_ptr(n + 1 + kSpare, kGuard);
    for (uint64_t c = 0; c <= n; ++c) chunk_ptr[c] = off[xsg::litfind_chunk_word(b.tile0[c])];
    for (uint64_t c = 0; c <= n; ++c)
      CHECK(chunk_ptr[c] == want_ptr[c], "%s: chunk_ptr[%llu] = %llu, brute force %llu", what, (unsigned long long)c,
            (unsigned long long)chunk_ptr[c], (unsigned long long)want_ptr[c]);
    for (uint64_t cap : {total, total ? total - 1 : 0, (uint64_t)0}) {
      std::vector<uint64_t> pos(cap + kSpare, kGuard);
      std::vector<uint32_t> lit(cap + kSpare, kGuard32);
      R.fill(order, occ.data(), off.data(), pos.data(), lit.data(), cap);
      CHECK(xsg::litfind_overflow(total, cap) == (total > cap), "%s: status under capacity %llu", what, (unsigned long long)cap);
      for (size_t i = 0; i < kSpare; ++i)
        CHECK(pos[cap + i] == kGuard && lit[cap + i] == kGuard32, "%s: an entry at or behind the capacity %llu was written", what, (unsigned long long)cap);
      for (uint64_t e = 0; e < cap && e < want.size(); ++e)
        CHECK(pos[e] == want[e].pos && lit[e] == want[e].lit, "%s (cap %llu): entry %llu is (%llu, %u), brute force (%llu, %u)", what,
              (unsigned long long)cap, (unsigned long long)e, (unsigned long long)pos[e], lit[e], (unsigned long long)want[e].pos, want[e].lit);
    }
  }
}

static std::vector<uint8_t> bytes_of(const std::string& s) { return std::vector<uint8_t>(s.begin(), s.end()); }

static void fixed_cases(std::mt19937& rng) {
  for (bool icase : {false, true}) {
    run_case(bind({bytes_of("aaaa")}, rng), {"aa"}, icase, false, rng, "aa in aaaa", 3);
    run_case(bind({bytes_of("abc")}, rng), {"ab", "abc"}, icase, false, rng, "ab, abc on abc", 2);
    run_case(bind({bytes_of("xabab"), {}, bytes_of("ab"), bytes_of("b")}, rng), {"ab", "b", "ab", "zz"}, icase, false, rng, "duplicates", 7);
    run_case(bind({bytes_of("xa"), bytes_of("b")}, rng), {"ab"}, icase, false, rng, "no occurrence straddles two chunks");
    run_case(bind({}, rng), {"a", "b"}, icase, false, rng, "no chunks");
    run_case(bind({bytes_of("art party art"), bytes_of("art"), bytes_of("xart art_ -ART-")}, rng), {"art"}, icase, true, rng, "whole words",
             icase ? 4 : 3);
    // every position a candidate with three hits: 16 rounds per wave-load, across a tile edge
    run_case(bind({std::vector<uint8_t>(kTile + 5, 'a')}, rng), {"a", "aa", "a"}, icase, false, rng, "rounds and ranks", 3 * (kTile + 5) - 1);
  }
}

static void random_cases(std::mt19937& rng) {
  const std::string alphabets[] = {"ab", "abcAB _", "etaoinshrETAOIN ,"};
  for (const std::string& alpha : alphabets)
    for (size_t min_len : {1, 2, 3, 4, 6})
      for (size_t nlits : {1, 3, 40})
        for (int flags = 0; flags < 4; ++flags) {
          const bool icase = flags & 1, words = flags & 2;
          std::vector<std::string> lits;
          for (size_t i = 0; i < nlits; ++i) {
            std::string l(min_len + rng() % 5, ' ');
            for (char& c : l) c = alpha[rng() % alpha.size()];
            lits.push_back(l);
          }
          if (nlits > 2) lits[1] = lits[nlits - 1];  // a duplicate
          lits[rng() % nlits].resize(min_len);       // the shortest literal is min_len bytes: g = min(min_len, 4)
          std::vector<std::vector<uint8_t>> chunks;
          const size_t nchunks = 1 + rng() % 6;
          for (size_t c = 0; c < nchunks; ++c) {
            // 0 bytes, a few, just below / at / just above a load, span and tile edge, up to two tiles and a bit
            const uint64_t shapes[] = {0, 1 + rng() % 40, kLoad - 1 + rng() % 3, kSpan - 1 + rng() % 3, kTile - 2 + rng() % 5, kTile + rng() % kTile,
                                       2 * kTile + rng() % 100};
            std::vector<uint8_t> text(shapes[rng() % 7]);
            // sparse: mostly a byte no literal holds, with planted literals -- a dense random text over two letters would make
            // the brute force the bottleneck
            const bool dense = text.size() < 3000;
            for (uint8_t& x : text) x = dense ? (uint8_t)alpha[rng() % alpha.size()] : (uint8_t)'.';
            for (int k = 0; k < 60 && !text.empty(); ++k) {
              const std::string& l = lits[rng() % nlits];
              if (l.size() > text.size()) continue;
              const uint64_t edges[] = {kLoad, kSpan, kTile, text.size()};
              uint64_t at = rng() % (text.size() - l.size() + 1);
              if (k < 8) {  // around the edges of the partition, one ending exactly at the chunk's end
                const uint64_t e = edges[k % 4];
                if (e <= text.size() && e >= l.size()) at = std::min<uint64_t>(e - rng() % (l.size() + 1), text.size() - l.size());
              }
              memcpy(text.data() + at, l.data(), l.size());
            }
            chunks.push_back(std::move(text));
          }
          run_case(bind(std::move(chunks), rng), lits, icase, words, rng, "random");
        }
}

int main() {
  std::mt19937 rng(1620);
  fixed_cases(rng);
  random_cases(rng);
  if (failures) return 1;
  std::printf("literal_find_selftest ok\n");
  return 0;
}
