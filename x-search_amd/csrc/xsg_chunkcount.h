// xsg_chunkcount.h -- the run arithmetic of k_count_chunks (xsg_kernels.hip), shared by the kernel and by a host-side
// unit test (plain C++ when compiled without hipcc; tests/cpu_model/chunk_runs_model.cpp).
//
// A wave takes 64 consecutive tiles, one per lane, and reads each tile's chunk id.  Tiles are numbered chunk by chunk,
// so equal ids sit side by side: the 64 lanes fall into RUNS of one chunk each.  The kernel wants one sum per run and
// one atomic per run that is not zero, issued by the run's first lane (its HEAD).  Everything the lanes need to know
// about the runs follows from two 64-bit masks:
//   active  bit i: lane i holds a tile (the last wave of a binding may hold fewer than 64; the active lanes are the
//           lanes 0 .. n - 1, never a set with gaps)
//   change  bit i: lane i holds a tile whose chunk id differs from lane i - 1's (what a ballot of `id != id of the
//           previous lane` gives; bit 0 and bits of inactive lanes may hold anything)
// A head is an active lane that is lane 0 or has its change bit set.  The head at lane h owns the lanes [h, e), e = the
// next head above h or, for the last run, the number of active lanes.  With an inclusive prefix sum P over the lanes'
// values the run's sum is P[e - 1] - (h ? P[h - 1] : 0): one cross-lane read per head, whatever the cut.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XSG_CC_HD __host__ __device__ inline
#else
#define XSG_CC_HD inline
#endif

namespace xsg {

// the active-lane mask of a wave that holds n tiles (n >= 64: all lanes)
XSG_CC_HD uint64_t run_active_mask(uint64_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

// the heads of the runs: lane 0 (if active) and every active lane whose id differs from its left neighbour's
XSG_CC_HD uint64_t run_heads(uint64_t change, uint64_t active) { return (change | 1ull) & active; }

// the lane behind the run that starts at head lane h (exclusive end): the next head above h, else the lane count
XSG_CC_HD uint32_t run_end(uint64_t heads, uint64_t active, uint32_t h) {
  const uint64_t above = h >= 63u ? 0ull : heads & (~0ull << (h + 1u));
  if (above) return (uint32_t)__builtin_ctzll(above);
  return active == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~active);  // (active is 0 .. n - 1: its first clear bit is n)
}

}  // namespace xsg
