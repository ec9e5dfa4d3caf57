// xsg_fileset.h -- the HIP-free part of the file-set pipeline (xsg_fileset.cpp): which files go into which batch and where,
// and which rows of a batch's result are whose file's.  Host only, standard library only: tests/cpp/fileset_selftest.cpp
// drives it under the sanitizers with plain g++.
//
// A file set searches a LIST of files in path order.  A file of at most chunk_bytes is ONE chunk of a batch: the batch is
// one pinned buffer, the files lie in it at multiples of 16 bytes in path order, and the whole batch is bound and searched
// as one shard.  A batch closes when the next small file would not fit batch_bytes or it holds kMaxBatchFiles files.  A
// file larger than chunk_bytes is set aside (the job pipeline of xsg_job.cpp searches it); a file that cannot be read
// has no place at all.  Neither closes a batch: results are published per file in path order, whatever the cut.
#pragma once
#include <cstdint>
#include <vector>

namespace xsg_fileset_plan {

constexpr uint64_t kMaxBatchFiles = 1ull << 20;
constexpr uint64_t kAlign = 16;

enum Kind : uint8_t { kSmall = 0, kLarge = 1, kUnreadable = 2 };

inline uint64_t round_up(uint64_t n) { return (n + (kAlign - 1)) & ~(kAlign - 1); }

struct Item {
  uint64_t file;    // index into the path list
  uint64_t offset;  // in the batch buffer, a multiple of 16
  uint64_t length;
};

// Batch b holds items [first_item, end_item) and answers for the files [first_file, end_file): the batches' file ranges
// partition the path list, large and unreadable files included, so that every file is published by exactly one batch.
struct Batch {
  uint64_t first_item = 0, end_item = 0;
  uint64_t first_file = 0, end_file = 0;
  uint64_t bytes = 0;  // the end of the last item, rounded up to 16: what is uploaded
};

struct Plan {
  std::vector<Item> items;
  std::vector<Batch> batches;  // at least one if there is a file, possibly without items
};

// sizes[f], kinds[f] per file (kinds[f] is derived by the caller: kLarge iff size > chunk_bytes, kUnreadable as stat said).
// batch_bytes >= chunk_bytes is the caller's check, so every small file fits an empty batch.
inline Plan make_plan(const std::vector<uint64_t>& sizes, const std::vector<uint8_t>& kinds, uint64_t batch_bytes,
                      uint64_t max_files = kMaxBatchFiles) {
  Plan p;
  const uint64_t n = sizes.size();
  if (n == 0) return p;
  Batch cur;
  uint64_t at = 0;  // where the next item would begin
  for (uint64_t f = 0; f < n; ++f) {
    if (kinds[f] != kSmall) continue;
    const uint64_t files_in = p.items.size() - cur.first_item;
    if (files_in != 0 && (at + sizes[f] > batch_bytes || files_in >= max_files)) {
      cur.end_item = p.items.size();
      cur.end_file = f;
      cur.bytes = at;
      p.batches.push_back(cur);
      cur = Batch{};
      cur.first_item = p.items.size();
      cur.first_file = f;
      at = 0;
    }
    p.items.push_back(Item{f, at, sizes[f]});
    at = round_up(at + sizes[f]);
  }
  cur.end_item = p.items.size();
  cur.end_file = n;
  cur.bytes = at;
  p.batches.push_back(cur);
  return p;
}

// The rows of a batch's list result (xsg_result_chunk_ptr: rows[i] .. rows[i + 1] are item i's entries, i counted from the
// batch's first item) -> entries per file of the batch's file range: file_rows[f - first_file]; files without an item get 0.
inline void attribute_rows(const Plan& p, const Batch& b, const uint64_t* rows, std::vector<uint64_t>& file_rows) {
  file_rows.assign(b.end_file - b.first_file, 0);
  for (uint64_t i = b.first_item; i < b.end_item; ++i)
    file_rows[p.items[i].file - b.first_file] = rows[i - b.first_item + 1] - rows[i - b.first_item];
}

}  // namespace xsg_fileset_plan
