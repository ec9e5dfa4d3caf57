// xsg_litmatrix.h -- the arithmetic k_set_count_literals_chunks (xsg_set_kernels.hip) and its launcher share with the
// host: how the tiles of a binding are cut into one contiguous range per workgroup, and the capacity of the touched
// list.  Plain C++ when compiled without hipcc: tests/cpp/literal_matrix_selftest.cpp checks the partition and replays
// the flush rule on the host.  Behind it the arithmetic of the sparse form, k_set_count_literals_csr: which chunks a
// workgroup owns alone, where the others' rows are summed, and the cap of its grid.
//
// Workgroup b of `grid` owns the tiles [b * per, min((b + 1) * per, ntiles)), per = ceil(ntiles / grid): contiguous, so
// that a workgroup meets every chunk boundary inside its range exactly once and flushes its histogram there.  A
// histogram word counts at most one occurrence per position the workgroup looks at, 16 Ki positions per tile: per stays
// below 2^18, so a word stays below 2^32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XSG_LITMATRIX_HD __host__ __device__ inline
#else
#define XSG_LITMATRIX_HD inline
#endif

namespace xsg {

// literals a workgroup can note as "hit since the last flush" before the flush falls back to a sweep of the histogram
constexpr uint32_t kLitTouched = 1024;
// lists of at most this many literals: a workgroup sums chunks_with in LDS and adds its words once, behind its last tile --
// a short list's few words, each added to by every chunk of the binding, would otherwise serialise in the L2 (measured:
// DESIGN.md 3.5f); a longer list spreads its adds over as many words and keeps the LDS for its histogram and keys
constexpr uint32_t kLitWithLds = 1024;
// workgroups per compute unit of the default grid: contiguous ranges balance only when there are many more ranges than
// resident workgroups (measured: DESIGN.md 3.5f)
constexpr uint32_t kLitMatrixGridPerCu = 64;
// tiles per workgroup: below this, so that a histogram word cannot wrap
constexpr uint64_t kLitMatrixPerLimit = 1ull << 18;

XSG_LITMATRIX_HD uint64_t litmatrix_per(uint64_t ntiles, uint64_t grid) { return grid ? (ntiles + grid - 1u) / grid : 0u; }
XSG_LITMATRIX_HD uint64_t litmatrix_first(uint64_t b, uint64_t per, uint64_t ntiles) {
  return b * per < ntiles ? b * per : ntiles;
}
XSG_LITMATRIX_HD uint64_t litmatrix_last(uint64_t b, uint64_t per, uint64_t ntiles) {
  return (b + 1u) * per < ntiles ? (b + 1u) * per : ntiles;
}

// The grid the launcher picks.  `want`: the bounded grid of the set kernels (workgroups per compute unit x compute units);
// `forced`: XSG_LITMATRIX_GRID, 0 when unset.  Never more workgroups than tiles, never so few that a workgroup would own
// 2^18 tiles or more, and no workgroup without a tile: the count is rounded down to ceil(ntiles / per).  0 tiles: 0.
XSG_LITMATRIX_HD uint64_t litmatrix_grid(uint64_t ntiles, uint64_t want, uint64_t forced) {
  if (ntiles == 0) return 0;
  uint64_t g = forced ? forced : want;
  if (g == 0) g = 1;
  if (g > ntiles) g = ntiles;
  const uint64_t least = (ntiles + (kLitMatrixPerLimit - 1u) - 1u) / (kLitMatrixPerLimit - 1u);
  if (g < least) g = least;
  const uint64_t per = litmatrix_per(ntiles, g);
  return (ntiles + per - 1u) / per;
}

// ---- the sparse form (k_set_count_literals_csr, k_set_csr_seam; tests/cpp/literal_csr_selftest.cpp replays them) ----------
// Workgroup b owns the tiles [first, last) as above.  A chunk with the tiles [t0, t1), t0 < t1, is WHOLE for b when all of
// them lie in b's range: b alone sees its histogram and writes its row.  Every other chunk with tiles crosses a range
// boundary, a SEAM chunk: its row is summed in the seam buffer, in the slot of the range its first tile lies in.  A seam
// chunk that starts in a range goes on behind the range's end, so it is the LAST chunk that starts there: at most one per
// range, none in the last range, the slot is unique and there are at most grid - 1 seam chunks.
XSG_LITMATRIX_HD bool litcsr_whole(uint64_t t0, uint64_t t1, uint64_t first, uint64_t last) { return t0 >= first && t1 <= last; }
XSG_LITMATRIX_HD uint64_t litcsr_slot(uint64_t t0, uint64_t per) { return t0 / per; }
// [t0, t1): the tiles of the chunk that owns the range's last tile, last - 1.  Is it the seam chunk of this range's slot?
XSG_LITMATRIX_HD bool litcsr_slot_seam(uint64_t t0, uint64_t t1, uint64_t first, uint64_t last) { return t0 >= first && t1 > last; }

// words of the seam buffer, grid x literals of uint64: 64 MiB at most, whatever the binding
constexpr uint64_t kLitCsrSeamWords = 1ull << 23;
// the grid the sparse launcher asks litmatrix_grid for: `want` lowered until grid x literals fits the seam buffer (4096
// literals: 2048 workgroups; 512 literals and fewer: the dense kernel's 64 per compute unit of a 256-CU device).  A forced
// grid is lowered the same way.
XSG_LITMATRIX_HD uint64_t litcsr_grid_cap(uint64_t g, uint32_t nlits) {
  const uint64_t most = kLitCsrSeamWords / (nlits ? nlits : 1u);
  return g < most ? g : most;
}
// the ordered compaction of a row of k words by `waves` waves: wave w takes the words [w * q, (w + 1) * q), q a multiple of
// the 64 lanes, counts its non-zero words, and ranks them behind the counts of the waves in front of it
XSG_LITMATRIX_HD uint32_t litcsr_wave_span(uint32_t k, uint32_t waves) { return ((k + waves - 1u) / waves + 63u) & ~63u; }
// a fill flush of at most this many noted literals ranks each by counting the smaller ones among them (one wave, no
// barrier); more, or a list that overflowed, and the flush compacts the whole histogram in order
constexpr uint32_t kLitCsrRank = 64;

}  // namespace xsg
