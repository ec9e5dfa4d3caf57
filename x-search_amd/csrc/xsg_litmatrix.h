// xsg_litmatrix.h -- the arithmetic k_set_count_literals_chunks (xsg_set_kernels.hip) and its launcher share with the
// host: how the tiles of a binding are cut into one contiguous range per workgroup, and the capacity of the touched
// list.  Plain C++ when compiled without hipcc: tests/cpp/literal_matrix_selftest.cpp checks the partition and replays
// the flush rule on the host.
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

}  // namespace xsg
