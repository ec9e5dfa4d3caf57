// fileset_selftest.cpp -- the HIP-free planner of the file-set pipeline (x-search_amd/csrc/xsg_fileset.h) against a
// brute-force plan and its invariants, on random size lists.  A stand-alone program: tests/test_fileset_host.py compiles it
// with g++ -fsanitize=address,undefined and runs it; nothing is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../x-search_amd/csrc/xsg_fileset.h"

namespace fsp = xsg_fileset_plan;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// The definition, file by file, without the planner's bookkeeping: which batch a small file lands in and where.
struct Placed {
  uint64_t batch, offset;
};
static std::vector<Placed> brute(const std::vector<uint64_t>& sizes, const std::vector<uint8_t>& kinds, uint64_t batch_bytes,
                                 uint64_t max_files) {
  std::vector<Placed> out(sizes.size(), Placed{UINT64_MAX, UINT64_MAX});
  uint64_t batch = 0, used = 0, files = 0;
  for (size_t f = 0; f < sizes.size(); ++f) {
    if (kinds[f] != fsp::kSmall) continue;
    uint64_t at = (used + 15) / 16 * 16;
    if (files && (at + sizes[f] > batch_bytes || files == max_files)) {
      ++batch;
      at = used = files = 0;
    }
    out[f] = Placed{batch, at};
    used = at + sizes[f];
    ++files;
  }
  return out;
}

static void check_plan(const std::vector<uint64_t>& sizes, uint64_t chunk_bytes, uint64_t batch_bytes, uint64_t max_files,
                       const std::vector<uint8_t>& unreadable) {
  const uint64_t n = sizes.size();
  std::vector<uint8_t> kinds(n);
  for (uint64_t f = 0; f < n; ++f) kinds[f] = unreadable[f] ? fsp::kUnreadable : sizes[f] > chunk_bytes ? fsp::kLarge : fsp::kSmall;
  const fsp::Plan p = fsp::make_plan(sizes, kinds, batch_bytes, max_files);
  const std::vector<Placed> want = brute(sizes, kinds, batch_bytes, max_files);
  if (n == 0) {
    CHECK(p.batches.empty() && p.items.empty());
    return;
  }
  CHECK(!p.batches.empty());
  // the batches' file ranges partition the path list; their item ranges partition the items
  CHECK(p.batches.front().first_file == 0 && p.batches.back().end_file == n);
  CHECK(p.batches.front().first_item == 0 && p.batches.back().end_item == p.items.size());
  std::vector<uint64_t> seen(n, 0);
  for (size_t b = 0; b < p.batches.size(); ++b) {
    const fsp::Batch& B = p.batches[b];
    if (b) CHECK(B.first_file == p.batches[b - 1].end_file && B.first_item == p.batches[b - 1].end_item);
    CHECK(B.first_file <= B.end_file && B.first_item <= B.end_item);
    CHECK(B.end_item - B.first_item <= max_files);        // the cap on files
    if (p.batches.size() > 1) CHECK(B.end_item > B.first_item);  // only a plan without any small file has an empty batch
    uint64_t prev_end = 0, prev_file = B.first_file;
    for (uint64_t i = B.first_item; i < B.end_item; ++i) {
      const fsp::Item& it = p.items[i];
      CHECK(it.file >= B.first_file && it.file < B.end_file);  // no file is split across batches: it lies in its batch's range
      CHECK(i == B.first_item || it.file > prev_file);          // path order
      CHECK(kinds[it.file] == fsp::kSmall && it.length == sizes[it.file]);
      CHECK(it.offset % 16 == 0 && it.offset >= prev_end);      // 16-byte packing, no overlap
      CHECK(it.offset == (i == B.first_item ? 0 : fsp::round_up(prev_end)));  // ... and no hole either
      CHECK(it.offset + it.length <= batch_bytes);              // the cap on bytes
      CHECK(want[it.file].batch == b && want[it.file].offset == it.offset);
      prev_end = it.offset + it.length;
      prev_file = it.file;
      ++seen[it.file];
    }
    CHECK(B.bytes == fsp::round_up(prev_end));
    // a batch closes only when it must: the next small file would not have fitted, or the batch is full
    if (b + 1 < p.batches.size()) {
      const fsp::Item& nxt = p.items[B.end_item];
      CHECK(fsp::round_up(prev_end) + nxt.length > batch_bytes || B.end_item - B.first_item == max_files);
      CHECK(nxt.file == p.batches[b + 1].first_file);
    }
    // attribution: rows of the batch -> entries per file of its range; large and unreadable files get none
    std::vector<uint64_t> rows(B.end_item - B.first_item + 1, 0), file_rows;
    for (uint64_t i = 0; i + 1 < rows.size(); ++i) rows[i + 1] = rows[i] + (p.items[B.first_item + i].file % 5);
    fsp::attribute_rows(p, B, rows.data(), file_rows);
    CHECK(file_rows.size() == B.end_file - B.first_file);
    uint64_t sum = 0;
    for (uint64_t f = B.first_file; f < B.end_file; ++f) {
      CHECK(file_rows[f - B.first_file] == (kinds[f] == fsp::kSmall ? f % 5 : 0));
      sum += file_rows[f - B.first_file];
    }
    CHECK(sum == rows.back());
  }
  for (uint64_t f = 0; f < n; ++f) CHECK(seen[f] == (kinds[f] == fsp::kSmall ? 1u : 0u));  // files over chunk_bytes are set aside
}

int main() {
  std::mt19937_64 rng(20240607);
  uint64_t plans = 0;
  for (int round = 0; round < 4000; ++round) {
    const uint64_t chunk_bytes = 1 + rng() % 200;
    const uint64_t batch_bytes = chunk_bytes + rng() % 600;
    const uint64_t max_files = round % 3 == 0 ? 1 + rng() % 6 : fsp::kMaxBatchFiles;
    const uint64_t n = rng() % 60;
    std::vector<uint64_t> sizes(n);
    std::vector<uint8_t> unreadable(n);
    for (uint64_t f = 0; f < n; ++f) {
      const uint64_t kind = rng() % 10;
      sizes[f] = kind == 0 ? 0 : kind == 1 ? chunk_bytes : kind == 2 ? chunk_bytes + 1 + rng() % 1000 : rng() % (chunk_bytes + 1);
      if (kind == 3) sizes[f] = 15 + rng() % 3;  // 15, 16, 17
      unreadable[f] = rng() % 11 == 0;
    }
    check_plan(sizes, chunk_bytes, batch_bytes, max_files, unreadable);
    ++plans;
  }
  // the cap of 2^20 files: 2^20 + 5 empty files are two batches
  {
    std::vector<uint64_t> sizes(fsp::kMaxBatchFiles + 5, 0);
    std::vector<uint8_t> kinds(sizes.size(), fsp::kSmall);
    const fsp::Plan p = fsp::make_plan(sizes, kinds, 1 << 20);
    CHECK(p.batches.size() == 2 && p.batches[0].end_item == fsp::kMaxBatchFiles && p.batches[1].end_item == sizes.size());
    CHECK(p.batches[0].bytes == 0 && p.batches[1].first_file == fsp::kMaxBatchFiles);
  }
  // only large and unreadable files: one batch without items that still answers for every file
  {
    const std::vector<uint64_t> sizes = {100, 0, 300};
    const std::vector<uint8_t> kinds = {fsp::kLarge, fsp::kUnreadable, fsp::kLarge};
    const fsp::Plan p = fsp::make_plan(sizes, kinds, 64);
    CHECK(p.batches.size() == 1 && p.items.empty() && p.batches[0].first_file == 0 && p.batches[0].end_file == 3);
  }
  printf("fileset_selftest ok: %llu plans\n", (unsigned long long)plans);
  return 0;
}
