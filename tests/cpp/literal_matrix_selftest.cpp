// literal_matrix_selftest.cpp -- the host side of k_set_count_literals_chunks (x-search_amd/csrc/xsg_litmatrix.h): built with
// -fsanitize=address,undefined by tests/test_literal_matrix_host.py and run as a process -- no GPU, no library.
//   1. the tile partition: for the grids the launcher can pick, every tile belongs to exactly one workgroup, no workgroup
//      is empty and none owns 2^18 tiles or more;
//   2. the flush rule, replayed: workgroups walk their tile ranges, hits go into a histogram with the touched list beside
//      it (a literal is noted when its word leaves 0; more than kLitTouched noted literals make the flush sweep), a flush
//      at every change of chunk and behind the last tile adds the non-zero words to the chunk's row and 1 to the literal's
//      frequency where the row's word was 0 (summed per workgroup first for a list of at most kLitWithLds).  Against a
//      direct count over the same (tile -> chunk, hits) sequence.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../x-search_amd/csrc/xsg_litmatrix.h"

using namespace xsg;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
      if (++failures > 10) std::exit(1); \
    }                                    \
  } while (0)

static void partition(uint64_t ntiles, uint64_t asked) {
  const uint64_t want = 2048;  // (the bounded grid of a 256-CU device; only used when nothing is asked for)
  const uint64_t grid = litmatrix_grid(ntiles, want, asked);
  if (ntiles == 0) {
    CHECK(grid == 0, "0 tiles: grid %llu", (unsigned long long)grid);
    return;
  }
  CHECK(grid >= 1 && grid <= ntiles, "ntiles %llu asked %llu: grid %llu", (unsigned long long)ntiles, (unsigned long long)asked,
        (unsigned long long)grid);
  if (asked && asked <= ntiles && ntiles / asked < kLitMatrixPerLimit - 1) CHECK(grid <= asked, "more workgroups than asked for");
  const uint64_t per = litmatrix_per(ntiles, grid);
  CHECK(per >= 1 && per < kLitMatrixPerLimit, "ntiles %llu grid %llu: per %llu", (unsigned long long)ntiles,
        (unsigned long long)grid, (unsigned long long)per);
  uint64_t next = 0;
  std::vector<uint8_t> owners(ntiles <= 10000 ? ntiles : 0, 0);
  for (uint64_t b = 0; b < grid; ++b) {
    const uint64_t lo = litmatrix_first(b, per, ntiles), hi = litmatrix_last(b, per, ntiles);
    CHECK(lo == next && hi > lo && hi <= ntiles && hi - lo < kLitMatrixPerLimit, "ntiles %llu grid %llu: workgroup %llu owns [%llu, %llu)",
          (unsigned long long)ntiles, (unsigned long long)grid, (unsigned long long)b, (unsigned long long)lo, (unsigned long long)hi);
    for (uint64_t t = lo; t < hi && t < owners.size(); ++t) ++owners[t];
    next = hi;
  }
  CHECK(next == ntiles, "ntiles %llu grid %llu: the ranges end at %llu", (unsigned long long)ntiles, (unsigned long long)grid,
        (unsigned long long)next);
  for (size_t t = 0; t < owners.size(); ++t) CHECK(owners[t] == 1, "tile %zu has %u owners", t, owners[t]);
  // a workgroup beyond the grid (none is launched) would own nothing
  CHECK(litmatrix_first(grid, per, ntiles) == ntiles && litmatrix_last(grid, per, ntiles) == ntiles, "the range behind the grid is not empty");
}

// one simulated workgroup: its histogram, the touched list and the running counter with its base, as the kernel keeps them
struct Workgroup {
  std::vector<uint32_t> hist, with_local;  // with_local: chunks_with summed per workgroup (lists up to kLitWithLds)
  std::vector<uint16_t> touched = std::vector<uint16_t>(kLitTouched);
  uint32_t ntouched = 0, base = 0;
  uint64_t tile = 0, end = 0;
  unsigned sweeps = 0, walks = 0;
  void hit(uint32_t j) {
    if (hist[j]++ == 0) {
      const uint32_t slot = ntouched++ - base;
      if (slot < kLitTouched) touched[slot] = (uint16_t)j;
    }
  }
  void flush(uint64_t* row, uint64_t* with, bool listed) {
    auto add = [&](uint32_t j, uint32_t v) {
      hist[j] = 0;
      const uint64_t old = row[j];
      row[j] += v;
      if (old == 0 && with) {
        if (hist.size() <= kLitWithLds)
          ++with_local[j];
        else
          ++with[j];
      }
    };
    const uint32_t nt = ntouched - base;
    base = ntouched;
    if (listed && nt <= kLitTouched) {
      ++walks;
      for (uint32_t k = 0; k < nt; ++k) {
        CHECK(hist[touched[k]] > 0, "a noted literal has an empty word");
        add(touched[k], hist[touched[k]]);
      }
    } else {
      ++sweeps;
      for (uint32_t j = 0; j < hist.size(); ++j)
        if (hist[j]) add(j, hist[j]);
    }
    for (uint32_t v : hist) CHECK(v == 0, "the flush left a word behind");
  }
};

static void replay(std::mt19937& rng, uint32_t nlits, uint64_t nchunks, uint64_t asked_grid, bool listed, bool want_with,
                   unsigned* sweeps, unsigned* walks) {
  // chunks of 0..5 tiles; per tile a handful of hits, now and then a tile that hits more literals than the list holds
  std::vector<uint32_t> tile_chunk;
  for (uint64_t c = 0; c < nchunks; ++c)
    for (uint32_t t = rng() % 6; t > 0; --t) tile_chunk.push_back((uint32_t)c);
  const uint64_t ntiles = tile_chunk.size();
  std::vector<std::vector<uint32_t>> hits(ntiles);
  std::vector<uint64_t> want((size_t)nchunks * nlits, 0), want_freq(nlits, 0);
  for (uint64_t t = 0; t < ntiles; ++t) {
    const uint32_t n = rng() % 16 == 0 ? nlits + rng() % (2 * nlits) : rng() % 12;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t j = rng() % 4 == 0 ? rng() % std::min<uint32_t>(nlits, 3) : rng() % nlits;
      hits[t].push_back(j);
      ++want[(size_t)tile_chunk[t] * nlits + j];
    }
  }
  for (uint64_t c = 0; c < nchunks; ++c)
    for (uint32_t j = 0; j < nlits; ++j) want_freq[j] += want[(size_t)c * nlits + j] > 0;

  const uint64_t grid = litmatrix_grid(ntiles, 8, asked_grid);
  const uint64_t per = litmatrix_per(ntiles, grid);
  std::vector<Workgroup> wgs(grid);
  for (uint64_t b = 0; b < grid; ++b) {
    wgs[b].hist.assign(nlits, 0);
    wgs[b].with_local.assign(nlits, 0);
    wgs[b].tile = litmatrix_first(b, per, ntiles);
    wgs[b].end = litmatrix_last(b, per, ntiles);
  }
  std::vector<uint64_t> M((size_t)nchunks * nlits + 4, 0), freq(nlits + 4, 0);
  M[M.size() - 1] = freq[freq.size() - 1] = ~0ull;
  // the workgroups advance a tile at a time in random order: their adds to a shared chunk's row interleave
  uint64_t left = ntiles;
  while (left) {
    Workgroup& w = wgs[rng() % grid];
    if (w.tile == w.end) continue;
    const uint32_t c = tile_chunk[w.tile];
    for (uint32_t j : hits[w.tile]) w.hit(j);
    const bool boundary = w.tile + 1 == w.end || tile_chunk[w.tile + 1] != c;
    if (boundary) w.flush(M.data() + (size_t)c * nlits, want_with ? freq.data() : nullptr, listed);
    ++w.tile;
    --left;
    if (w.tile == w.end && want_with)  // behind its last tile the workgroup adds what it summed
      for (uint32_t j = 0; j < nlits; ++j) freq[j] += w.with_local[j];
  }
  for (size_t i = 0; i < want.size(); ++i) CHECK(M[i] == want[i], "matrix word %zu: %llu, want %llu", i, (unsigned long long)M[i], (unsigned long long)want[i]);
  for (uint32_t j = 0; j < nlits; ++j)
    CHECK(freq[j] == (want_with ? want_freq[j] : 0), "frequency %u: %llu, want %llu", j, (unsigned long long)freq[j], (unsigned long long)want_freq[j]);
  CHECK(M[M.size() - 1] == ~0ull && freq[freq.size() - 1] == ~0ull, "a word behind the results was written");
  for (const Workgroup& w : wgs) *sweeps += w.sweeps, *walks += w.walks;
}

int main() {
  const uint64_t sizes[] = {0, 1, 2, 7, 8, 9, 4095, 4096, 4097, (1ull << 18) * 3 + 1};
  for (uint64_t n : sizes)
    for (uint64_t g : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)7, (uint64_t)8, n, n + 5}) partition(n, g);
  // (2^18 - 1) * grid tiles: the most a grid may be asked to take
  partition((kLitMatrixPerLimit - 1) * 3, 3);
  partition((kLitMatrixPerLimit - 1) * 3 + 1, 3);

  std::mt19937 rng(20261020);
  unsigned sweeps = 0, walks = 0, plain_sweeps = 0, plain_walks = 0;
  for (uint32_t nlits : {1u, 5u, kLitTouched - 1, kLitTouched, kLitTouched + 1, 4096u})
    for (uint64_t grid : {1, 2, 3, 7})
      for (int round = 0; round < (nlits > 1000 ? 2 : 6); ++round) {
        replay(rng, nlits, 3 + rng() % 40, grid, true, round % 2 == 0, &sweeps, &walks);
        replay(rng, nlits, 3 + rng() % 40, grid, false, true, &plain_sweeps, &plain_walks);
      }
  CHECK(sweeps > 0 && walks > sweeps, "the replay took the sweep %u times and the list %u times", sweeps, walks);
  CHECK(plain_walks == 0 && plain_sweeps > 0, "without the list every flush sweeps");
  if (failures) return 1;
  std::printf("literal_matrix_selftest ok: %u walks, %u sweeps\n", walks, sweeps);
  return 0;
}
