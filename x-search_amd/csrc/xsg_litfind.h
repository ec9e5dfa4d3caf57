// xsg_litfind.h -- the index arithmetic k_set_find_literals (xsg_set_kernels.hip) and its launchers share with the host:
// which word of the scratch a wave's 4 KiB span owns, where a hit of a queue round is stored and which stores the
// capacity clips.  Plain C++ when compiled without hipcc: tests/cpp/literal_find_selftest.cpp replays count pass, prefix
// sum and fill pass with it on the host, under the sanitizers.
//
// A tile of 16 KiB is four spans of 4 KiB, one per wave of the workgroup; tiles ascend by chunk and spans by position, so
// the span words in index order are the text in (chunk, position) order.  The count pass writes ONE word per span, its
// number of occurrences; an exclusive prefix sum over the 4 * ntiles words gives every span the index of its first entry,
// and the words of a chunk's first span the chunk's row of chunk_ptr.  Inside a span the order is structural as well:
// wave-loads ascend, the candidates of a load are queued in ascending position and taken 64 a round, and a candidate's
// literals are visited in listing order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XSG_LITFIND_HD __host__ __device__ inline
#else
#define XSG_LITFIND_HD inline
#endif

namespace xsg {

constexpr uint32_t kLitFindSpans = 4;    // spans (waves) per tile
constexpr uint32_t kLitFindRound = 64;   // candidates a queue round decides: one per lane

// the scratch word of a span: wave_occ[word] its occurrences, wave_off[word] the index of its first entry
XSG_LITFIND_HD uint64_t litfind_span_word(uint64_t tile, uint32_t wave) { return tile * kLitFindSpans + wave; }
// words the count pass writes and the prefix sum reads (its output holds one more: the total)
XSG_LITFIND_HD uint64_t litfind_words(uint64_t ntiles) { return ntiles * kLitFindSpans; }
// chunk_ptr[c], c in [0, nchunks]: the first entry of the chunk's first span; chunk_tile0[nchunks] = ntiles gives the total.
// A chunk without a tile shares its successor's word: an empty range.
XSG_LITFIND_HD uint64_t litfind_chunk_word(uint64_t chunk_tile0) { return chunk_tile0 * kLitFindSpans; }
// rounds a wave-load of `total` queued candidates takes
XSG_LITFIND_HD uint32_t litfind_rounds(uint32_t total) { return (total + kLitFindRound - 1u) / kLitFindRound; }
// The index of a lane's first hit in a round: `at` is the index of the round's first entry (the span's offset plus every
// earlier round's hits), `incl` the inclusive prefix sum of the lanes' hit counts up to and including this lane, `hits`
// this lane's own.  Its k-th hit, in listing order, lies k entries behind.
XSG_LITFIND_HD uint64_t litfind_slot(uint64_t at, uint32_t incl, uint32_t hits) { return at + (incl - hits); }
// the capacity clip: entry e is stored iff it lies below cap_entries; nothing at or behind the capacity is written
XSG_LITFIND_HD bool litfind_stored(uint64_t e, uint64_t cap_entries) { return e < cap_entries; }
// the status of a call: the result did not fit
XSG_LITFIND_HD bool litfind_overflow(uint64_t total, uint64_t cap_entries) { return total > cap_entries; }

}  // namespace xsg
