// literal_csr_selftest.cpp -- the host side of k_set_count_literals_csr and k_set_csr_seam
// (x-search_amd/csrc/xsg_litmatrix.h): built with -fsanitize=address,undefined by tests/test_literal_csr_host.py and run as a
// process -- no GPU, no library.  On random tile -> chunk sequences, split over 1, 2, 3, 7 and ntiles workgroups:
//   1. the whole / seam predicate: every chunk with tiles is whole for exactly one workgroup or a seam, the seam chunks'
//      slots are unique, there are at most grid - 1 of them, and litcsr_slot_seam finds each from its slot;
//   2. the five stages of a call, replayed as the kernels run them: count pass (row lengths of whole chunks, seam rows
//      summed), seam count, prefix sum, fill pass (the tiles of seam chunks skipped; noted literals ranked by counting or
//      the histogram compacted by four waves), seam fill and the status word -- against the non-zeros of a direct count,
//      under full capacity, nnz - 1 and 0.
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

constexpr uint32_t kWaves = 4;
constexpr uint64_t kGuard = 0xffffffffffffffffull;

struct Binding {
  uint32_t nlits = 0;
  uint64_t nchunks = 0, ntiles = 0;
  std::vector<uint32_t> tile_chunk;
  std::vector<uint64_t> chunk_tile0;        // nchunks + 1
  std::vector<std::vector<uint32_t>> hits;  // per tile
  std::vector<uint64_t> dense;              // nchunks x nlits, the direct count
};

static Binding make_binding(std::mt19937& rng, uint32_t nlits, uint64_t nchunks) {
  Binding b;
  b.nlits = nlits;
  b.nchunks = nchunks;
  b.chunk_tile0.assign(nchunks + 1, 0);
  for (uint64_t c = 0; c < nchunks; ++c) {
    b.chunk_tile0[c] = b.tile_chunk.size();
    // chunks of 0 .. 5 tiles, now and then one of 9 .. 20: it spans several ranges of the larger grids
    const uint32_t t = rng() % 9 == 0 ? 9 + rng() % 12 : rng() % 6;
    for (uint32_t i = 0; i < t; ++i) b.tile_chunk.push_back((uint32_t)c);
  }
  b.ntiles = b.chunk_tile0[nchunks] = b.tile_chunk.size();
  b.hits.resize(b.ntiles);
  b.dense.assign((size_t)nchunks * nlits, 0);
  for (uint64_t t = 0; t < b.ntiles; ++t) {
    // a handful of hits, now and then none, now and then more literals than the touched list holds
    const uint32_t roll = rng() % 16;
    const uint32_t n = roll == 0 ? nlits + rng() % (2 * nlits) : roll == 1 ? 0 : roll == 2 ? 60 + rng() % 10 : rng() % 12;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t j = rng() % 4 == 0 ? rng() % std::min<uint32_t>(nlits, 3) : rng() % nlits;
      b.hits[t].push_back(j);
      ++b.dense[(size_t)b.tile_chunk[t] * nlits + j];
    }
  }
  return b;
}

// ---- 1. the predicates
static uint64_t check_predicates(const Binding& b, uint64_t grid) {
  const uint64_t per = litmatrix_per(b.ntiles, grid);
  std::vector<int> slot_used(grid, 0);
  uint64_t seams = 0;
  for (uint64_t c = 0; c < b.nchunks; ++c) {
    const uint64_t t0 = b.chunk_tile0[c], t1 = b.chunk_tile0[c + 1];
    if (t0 == t1) continue;
    unsigned owners = 0;
    for (uint64_t w = 0; w < grid; ++w)
      owners += litcsr_whole(t0, t1, litmatrix_first(w, per, b.ntiles), litmatrix_last(w, per, b.ntiles)) ? 1u : 0u;
    CHECK(owners <= 1, "chunk %llu is whole for %u workgroups", (unsigned long long)c, owners);
    if (owners) continue;
    ++seams;
    const uint64_t slot = litcsr_slot(t0, per);
    CHECK(slot < grid && !slot_used[slot], "chunk %llu: slot %llu beyond the grid or taken", (unsigned long long)c, (unsigned long long)slot);
    if (slot < grid) {
      slot_used[slot] = 1;
      // the seam kernel finds it from the slot: the chunk of the range's last tile
      const uint64_t first = litmatrix_first(slot, per, b.ntiles), last = litmatrix_last(slot, per, b.ntiles);
      CHECK(b.tile_chunk[last - 1] == c && litcsr_slot_seam(t0, t1, first, last), "slot %llu does not lead to chunk %llu",
            (unsigned long long)slot, (unsigned long long)c);
    }
  }
  CHECK(seams + 1 <= grid || (grid == 0 && seams == 0), "%llu seam chunks under %llu workgroups", (unsigned long long)seams, (unsigned long long)grid);
  // a slot without a seam chunk says so
  for (uint64_t w = 0; w < grid; ++w) {
    const uint64_t first = litmatrix_first(w, per, b.ntiles), last = litmatrix_last(w, per, b.ntiles);
    const uint32_t c = b.tile_chunk[last - 1];
    CHECK(litcsr_slot_seam(b.chunk_tile0[c], b.chunk_tile0[c + 1], first, last) == (slot_used[w] != 0), "slot %llu: seam or not?", (unsigned long long)w);
  }
  return seams;
}

// ---- 2. the stages
struct Workgroup {
  std::vector<uint32_t> hist;
  std::vector<uint16_t> touched = std::vector<uint16_t>(kLitTouched);
  uint32_t ntouched = 0, base = 0;
  void hit(uint32_t j, bool listed) {
    if (hist[j]++ == 0 && listed) {
      const uint32_t slot = ntouched++ - base;
      if (slot < kLitTouched) touched[slot] = (uint16_t)j;
    }
  }
};

struct Result {
  std::vector<uint64_t> row_ptr, vals;
  std::vector<uint32_t> cols;
  uint64_t status = kGuard;
};

struct Tally {
  unsigned ranked = 0, compacted = 0, walked = 0, swept = 0, seam_rows = 0;
  uint64_t fill_tiles = 0, whole_tiles = 0;
};

// csr_compact: four waves, each counts its span, then ranks its non-zero words behind the waves in front of it
template <typename Get, typename Put>
static void compact(uint32_t k, Get get, Put put) {
  const uint32_t q = litcsr_wave_span(k, kWaves);
  uint32_t wcnt[kWaves];
  for (uint32_t w = 0; w < kWaves; ++w) {
    const uint32_t lo = w * q, hi = std::min(lo + q, k);
    wcnt[w] = 0;
    for (uint32_t j = lo; j < hi; ++j) wcnt[w] += get(j) != 0;
  }
  for (uint32_t w = 0; w < kWaves; ++w) {
    uint32_t rank = 0;
    for (uint32_t v = 0; v < w; ++v) rank += wcnt[v];
    const uint32_t lo = w * q, hi = std::min(lo + q, k);
    for (uint32_t j = lo; j < hi; ++j)
      if (get(j) != 0) put(j, get(j), rank++);
  }
}

// one pass of k_set_count_literals_csr over the whole grid, the workgroups one after another in random order
static void pass(std::mt19937& rng, const Binding& b, uint64_t grid, bool listed, bool fill, std::vector<uint32_t>& row_nnz,
                 std::vector<uint64_t>& seam, Result* out, uint64_t cap, Tally* tally) {
  const uint32_t k = b.nlits;
  const uint64_t per = litmatrix_per(b.ntiles, grid);
  std::vector<uint64_t> order(grid);
  for (uint64_t w = 0; w < grid; ++w) order[w] = w;
  std::shuffle(order.begin(), order.end(), rng);
  for (uint64_t w : order) {
    Workgroup wg;
    wg.hist.assign(k, 0);
    const uint64_t first = litmatrix_first(w, per, b.ntiles), end = litmatrix_last(w, per, b.ntiles);
    uint64_t tile = first;
    while (tile < end) {
      const uint32_t c = b.tile_chunk[tile];
      const uint64_t t0 = b.chunk_tile0[c], t1 = b.chunk_tile0[c + 1];
      const bool whole = litcsr_whole(t0, t1, first, end);
      const uint64_t c_end = std::min(t1, end);
      if (fill && !whole) {
        tile = c_end;
        continue;
      }
      for (; tile < c_end; ++tile) {
        for (uint32_t j : b.hits[tile]) wg.hit(j, listed);
        if (fill) ++tally->fill_tiles;
      }
      const uint32_t nt = wg.ntouched - wg.base;
      wg.base = wg.ntouched;
      const bool walk = listed && nt <= kLitTouched;
      if (!fill) {
        ++(walk ? tally->walked : tally->swept);
        if (whole) {
          tally->whole_tiles += t1 - t0;
          if (walk) {
            for (uint32_t i = 0; i < nt; ++i) wg.hist[wg.touched[i]] = 0;
            row_nnz[c] = nt;
          } else {
            uint32_t n = 0;
            for (uint32_t j = 0; j < k; ++j) n += wg.hist[j] != 0, wg.hist[j] = 0;
            row_nnz[c] = n;
          }
        } else {
          uint64_t* row = seam.data() + litcsr_slot(t0, per) * k;
          if (walk) {
            for (uint32_t i = 0; i < nt; ++i) row[wg.touched[i]] += wg.hist[wg.touched[i]], wg.hist[wg.touched[i]] = 0;
          } else {
            for (uint32_t j = 0; j < k; ++j) row[j] += wg.hist[j], wg.hist[j] = 0;
          }
        }
      } else {
        const uint64_t at = out->row_ptr[c];
        auto put = [&](uint32_t j, uint64_t v, uint32_t rank) {
          wg.hist[j] = 0;
          if (at + rank < cap) out->cols[at + rank] = j, out->vals[at + rank] = v;
        };
        if (walk && nt <= kLitCsrRank) {
          ++tally->ranked;
          for (uint32_t i = 0; i < nt; ++i) {
            const uint32_t j = wg.touched[i];
            uint32_t rank = 0;
            for (uint32_t m = 0; m < nt; ++m) rank += wg.touched[m] < j;
            put(j, wg.hist[j], rank);
          }
        } else {
          ++tally->compacted;
          compact(k, [&](uint32_t j) { return (uint64_t)wg.hist[j]; }, put);
        }
      }
      for (uint32_t v : wg.hist) CHECK(v == 0, "a flush left a word behind");
    }
  }
}

// k_set_csr_seam over the slots
static void seam_pass(const Binding& b, uint64_t grid, bool fill, std::vector<uint32_t>& row_nnz, const std::vector<uint64_t>& seam,
                      Result* out, uint64_t cap, Tally* tally) {
  const uint32_t k = b.nlits;
  if (fill) out->status = out->row_ptr[b.nchunks] > cap ? 1u : 0u;
  const uint64_t per = litmatrix_per(b.ntiles, grid);
  for (uint64_t w = 0; w < grid; ++w) {
    const uint64_t first = litmatrix_first(w, per, b.ntiles), last = litmatrix_last(w, per, b.ntiles);
    const uint32_t c = b.tile_chunk[last - 1];
    if (!litcsr_slot_seam(b.chunk_tile0[c], b.chunk_tile0[c + 1], first, last)) continue;
    const uint64_t* row = seam.data() + w * k;
    if (!fill) {
      ++tally->seam_rows;
      uint32_t n = 0;
      for (uint32_t j = 0; j < k; ++j) n += row[j] != 0;
      row_nnz[c] = n;
    } else {
      const uint64_t at = out->row_ptr[c];
      compact(k, [&](uint32_t j) { return row[j]; },
              [&](uint32_t j, uint64_t v, uint32_t rank) {
                if (at + rank < cap) out->cols[at + rank] = j, out->vals[at + rank] = v;
              });
    }
  }
}

static void replay(std::mt19937& rng, const Binding& b, uint64_t asked_grid, bool listed, Tally* tally) {
  const uint32_t k = b.nlits;
  const uint64_t grid = litmatrix_grid(b.ntiles, litcsr_grid_cap(8, k), asked_grid ? litcsr_grid_cap(asked_grid, k) : 0);
  CHECK(grid * k <= kLitCsrSeamWords, "the seam buffer of %llu workgroups", (unsigned long long)grid);
  if (grid) check_predicates(b, grid);
  // the expected result: the non-zeros of the direct count
  Result want;
  want.row_ptr.push_back(0);
  for (uint64_t c = 0; c < b.nchunks; ++c) {
    for (uint32_t j = 0; j < k; ++j)
      if (b.dense[(size_t)c * k + j]) want.cols.push_back(j), want.vals.push_back(b.dense[(size_t)c * k + j]);
    want.row_ptr.push_back(want.cols.size());
  }
  const uint64_t nnz = want.cols.size();

  std::vector<uint32_t> row_nnz(b.nchunks, 0);
  std::vector<uint64_t> seam((size_t)grid * k, 0);
  Result got;
  pass(rng, b, grid, listed, false, row_nnz, seam, nullptr, 0, tally);
  seam_pass(b, grid, false, row_nnz, seam, nullptr, 0, tally);
  got.row_ptr.assign(b.nchunks + 1, 0);
  for (uint64_t c = 0; c < b.nchunks; ++c) got.row_ptr[c + 1] = got.row_ptr[c] + row_nnz[c];
  CHECK(got.row_ptr == want.row_ptr, "row_ptr differs (grid %llu, %u literals)", (unsigned long long)grid, k);
  if (got.row_ptr != want.row_ptr) return;

  std::vector<uint64_t> caps = {nnz, 0};
  if (nnz) caps.push_back(nnz - 1);
  for (uint64_t cap : caps) {
    const size_t room = (size_t)nnz + 4;  // (ASan guards what lies behind; the words up to there must keep the guard value)
    got.cols.assign(room, 0xffffffffu);
    got.vals.assign(room, kGuard);
    got.status = kGuard;
    Tally t2;
    pass(rng, b, grid, listed, true, row_nnz, seam, &got, cap, &t2);
    seam_pass(b, grid, true, row_nnz, seam, &got, cap, &t2);
    tally->ranked += t2.ranked, tally->compacted += t2.compacted;
    CHECK(t2.fill_tiles == tally->whole_tiles, "the fill pass scanned %llu tiles, whole chunks hold %llu", (unsigned long long)t2.fill_tiles,
          (unsigned long long)tally->whole_tiles);
    CHECK(got.status == (nnz > cap ? 1u : 0u), "status %llu under capacity %llu of %llu", (unsigned long long)got.status,
          (unsigned long long)cap, (unsigned long long)nnz);
    for (size_t e = 0; e < room; ++e) {
      if (e < cap)
        CHECK(got.cols[e] == want.cols[e] && got.vals[e] == want.vals[e], "entry %zu: (%u, %llu), want (%u, %llu)", e, got.cols[e],
              (unsigned long long)got.vals[e], want.cols[e], (unsigned long long)want.vals[e]);
      else
        CHECK(got.cols[e] == 0xffffffffu && got.vals[e] == kGuard, "entry %zu at or behind capacity %llu was written", e, (unsigned long long)cap);
    }
  }
  tally->whole_tiles = 0;
}

int main() {
  std::mt19937 rng(20261020);
  Tally listed, plain;
  unsigned long long seams = 0;
  for (uint32_t nlits : {1u, 5u, 63u, 65u, 300u, kLitTouched - 1, kLitTouched, kLitTouched + 1, 4096u})
    for (int round = 0; round < (nlits > 1000 ? 2 : 5); ++round) {
      const Binding b = make_binding(rng, nlits, round == 0 ? 0 : 3 + rng() % 40);
      for (uint64_t grid : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)7, b.ntiles}) {
        if (b.ntiles) {
          const uint64_t g = litmatrix_grid(b.ntiles, 8, grid);
          seams += check_predicates(b, g);
        }
        replay(rng, b, grid, true, &listed);
        replay(rng, b, grid, false, &plain);
      }
    }
  CHECK(seams > 50, "the bindings held %llu seam chunks", seams);
  CHECK(listed.ranked > 0 && listed.compacted > 0 && listed.walked > listed.swept && listed.swept > 0 && listed.seam_rows > 0,
        "with the list: %u ranked, %u compacted, %u walked, %u swept, %u seam rows", listed.ranked, listed.compacted, listed.walked,
        listed.swept, listed.seam_rows);
  CHECK(plain.ranked == 0 && plain.walked == 0 && plain.compacted > 0, "without the list every flush sweeps and compacts");
  // the grid cap: 4096 literals run on 2048 workgroups, 512 and fewer keep a grid of 64 per compute unit of 256
  CHECK(litcsr_grid_cap(256 * kLitMatrixGridPerCu, 4096) == 2048 && litcsr_grid_cap(256 * kLitMatrixGridPerCu, 512) == 256 * kLitMatrixGridPerCu &&
            litcsr_grid_cap(256 * kLitMatrixGridPerCu, 513) < 256 * kLitMatrixGridPerCu,
        "the grid cap");
  if (failures) return 1;
  std::printf("literal_csr_selftest ok: %llu seam chunks, %u ranked and %u compacted flushes\n", seams, listed.ranked, listed.compacted);
  return 0;
}
