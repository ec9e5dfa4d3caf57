// xsg_context.h -- XSG_FLAG_CONTEXT across the chunks of one text: what the file pipeline (xsg_job.cpp) needs to make a
// job's result the context of the whole searched range, however the chunker cut it.  Host only, no HIP, no library:
// tests/cpp/context_stitch.cpp drives it alone.
//
// A chunk is searched on its own (include/xsg.h), so its context stops at its edges; xsg_result_context_edges says by
// how much (open_before / open_after) and where its own list begins and ends (first / last).  Besides its own list a
// chunk offers the lines a NEIGHBOUR may still want, taken from its text on the host:
//   head extras: its first min(A, first) lines  -- wanted by matches near the end of the chunk before it,
//   tail extras: its last min(B, lines - 1 - last) lines -- wanted by matches near the start of the chunk behind it
// (`first`, `lines - 1 - last`: the chunk's line count where it reported nothing).  At the seam between chunk k-1 and
// chunk k the stitcher appends, in this order,
//   the last  min(open_before[k],   lines behind last[k-1]) tail extras of k-1,
//   the first min(open_after[k-1],  first[k])               head extras of k,
//   chunk k's own list,
// every element only if it lies behind the last one already appended (a chunk that reported nothing offers lines from
// both ends, which may be the same lines).  ONE-NEIGHBOUR RULE: context never reaches across a whole chunk.  If
// open_before[k] exceeds the lines of chunk k-1 and k-1 is not the first chunk of the range, or open_after[k-1] exceeds
// the lines of chunk k and k is not the last, the stitcher refuses (the caller fails the job: smaller chunks than the
// context are not approximated).  At the range's own ends context is clipped.
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/xsg.h"

namespace xsg_context {

// One line of a chunk: index among the chunk's lines, bytes [start, end) without the '\n', and whether one follows.
struct Line {
  uint64_t index, start, end;
  bool terminated;
};

// the lines of a chunk, as include/xsg.h counts them: one at 0 if len > 0, one behind every '\n' that is not the last byte
inline uint64_t count_lines(const uint8_t* d, uint64_t len) {
  if (len == 0) return 0;
  uint64_t n = 1;
  for (const uint8_t* p = d; (p = static_cast<const uint8_t*>(memchr(p, '\n', (size_t)(d + len - 1 - p)))) != nullptr; ++p) ++n;
  return n;
}

// the first min(k, lines) lines of the chunk
inline std::vector<Line> first_lines(const uint8_t* d, uint64_t len, uint64_t k) {
  std::vector<Line> out;
  uint64_t at = 0;
  while (at < len && out.size() < k) {
    const uint8_t* nl = static_cast<const uint8_t*>(memchr(d + at, '\n', (size_t)(len - at)));
    const uint64_t end = nl ? (uint64_t)(nl - d) : len;
    out.push_back(Line{(uint64_t)out.size(), at, end, nl != nullptr});
    at = end + 1;
  }
  return out;
}

// the last min(k, lines) lines of a chunk of `lines` lines, ascending
inline std::vector<Line> last_lines(const uint8_t* d, uint64_t len, uint64_t lines, uint64_t k) {
  std::vector<Line> out;
  if (len == 0 || k == 0) return out;
  const bool closed = d[len - 1] == '\n';
  uint64_t end = closed ? len - 1 : len;  // end of the last line
  bool terminated = closed;
  uint64_t index = lines;
  while (out.size() < k && index > 0) {
    uint64_t start = end;
    while (start > 0 && d[start - 1] != '\n') --start;
    out.push_back(Line{--index, start, end, terminated});
    if (start == 0) break;
    end = start - 1;
    terminated = true;
  }
  for (size_t a = 0, b = out.size(); a + 1 < b; ++a, --b) std::swap(out[a], out[b - 1]);
  return out;
}

// how many lines of the chunk lie ahead of its first / behind its last reported line (all of them: nothing reported)
inline uint64_t lines_ahead(const xsg_context_edge& e) { return e.first == UINT64_MAX ? e.lines : e.first; }
inline uint64_t lines_behind(const xsg_context_edge& e) { return e.last == UINT64_MAX ? e.lines : e.lines - 1 - e.last; }

enum SeamVerdict { kSeamOk = 0, kSeamBeforeTooFar = 1, kSeamAfterTooFar = 2 };

// The seam between `prev` (chunk k-1) and `cur` (chunk k): how many of prev's tail extras (its LAST ones) and of cur's
// head extras (its FIRST ones) join the result, or which side of the one-neighbour rule refuses.
inline SeamVerdict seam_take(const xsg_context_edge& prev, const xsg_context_edge& cur, bool prev_is_first, bool cur_is_last,
                             uint64_t* take_tail, uint64_t* take_head) {
  if (cur.open_before > prev.lines && !prev_is_first) return kSeamBeforeTooFar;
  if (prev.open_after > cur.lines && !cur_is_last) return kSeamAfterTooFar;
  const uint64_t behind = lines_behind(prev), ahead = lines_ahead(cur);
  *take_tail = cur.open_before < behind ? cur.open_before : behind;
  *take_head = prev.open_after < ahead ? prev.open_after : ahead;
  return kSeamOk;
}

// An element a chunk offers beside its own list: a line by its chunk-local index, in the result's form (a string, an
// offset, an index); `reported` false: the form has no element for it (XSG_LINES: a line without its '\n').
template <typename T>
struct Extra {
  uint64_t local;
  T value;
  bool reported;
};

template <typename T>
struct Part {
  xsg_context_edge edge{};
  std::vector<T> own;             // the chunk's own result
  std::vector<Extra<T>> head;     // its first min(A, lines ahead of first) lines
  std::vector<Extra<T>> tail;     // its last min(B, lines behind last) lines
};

// Chunks go in in order; what belongs to the whole range's result comes out.
template <typename T>
class Stitcher {
 public:
  // appends to *out; kSeamOk, or the refusal (nothing of this chunk was appended, the stitcher is spent)
  template <typename Out>
  SeamVerdict add(Part<T>&& part, bool is_first, bool is_last, Out* out) {
    if (have_prev_) {
      uint64_t take_tail = 0, take_head = 0;
      const SeamVerdict v = seam_take(prev_edge_, part.edge, prev_is_first_, is_last, &take_tail, &take_head);
      if (v != kSeamOk) return v;
      const uint64_t prev_base = base_ - prev_edge_.lines;
      const size_t skip = prev_tail_.size() > take_tail ? prev_tail_.size() - (size_t)take_tail : 0;
      for (size_t i = skip; i < prev_tail_.size(); ++i) offer(prev_base, prev_tail_[i], out);
      for (size_t i = 0; i < part.head.size() && i < take_head; ++i) offer(base_, part.head[i], out);
    }
    for (T& v : part.own) out->push_back(std::move(v));
    if (part.edge.last != UINT64_MAX) next_ = base_ + part.edge.last + 1;
    base_ += part.edge.lines;
    prev_edge_ = part.edge;
    prev_tail_ = std::move(part.tail);
    prev_is_first_ = is_first;
    have_prev_ = true;
    return kSeamOk;
  }

 private:
  template <typename Out>
  void offer(uint64_t base, Extra<T>& e, Out* out) {
    const uint64_t key = base + e.local;
    if (key < next_) return;  // at or ahead of the last element already appended
    next_ = key + 1;
    if (e.reported) out->push_back(std::move(e.value));
  }
  bool have_prev_ = false, prev_is_first_ = false;
  xsg_context_edge prev_edge_{};
  std::vector<Extra<T>> prev_tail_;
  uint64_t base_ = 0;  // lines of the range ahead of the next chunk
  uint64_t next_ = 0;  // range-wide index the next element must at least have
};

}  // namespace xsg_context
