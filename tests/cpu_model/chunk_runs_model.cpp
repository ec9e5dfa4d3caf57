// CPU model of the run arithmetic of k_count_chunks, built from the product's own header
// (x-search_amd/csrc/xsg_chunkcount.h) by tests/test_chunkcount_runs.py.
//
// cr_check(change, n, ...) takes a change mask and the number of lanes that hold a tile and compares, lane by lane, what
// the header derives from the two masks with a naive loop over the lanes; cr_check_many runs it over a list of masks.
// With -DCHUNK_RUNS_MAIN the file is a stand-alone program (its own main) for a sanitizer build.
#include <stdint.h>
#include <stdio.h>

#include "../../x-search_amd/csrc/xsg_chunkcount.h"

// 0: all agree; otherwise a code that says what differed (1 heads, 2 an end, 4 the partition)
static int check_one(uint64_t change, uint32_t n) {
  const uint64_t active = xsg::run_active_mask(n);
  // naive: walk the lanes, a run starts at lane 0 and wherever an active lane's change bit is set
  int end_of[64];
  uint64_t heads_naive = 0;
  int cur = -1;
  for (uint32_t i = 0; i < n && i < 64; ++i) {
    if (i == 0 || ((change >> i) & 1u)) {
      if (cur >= 0)
        for (uint32_t k = (uint32_t)cur; k < i; ++k) end_of[k] = (int)i;
      cur = (int)i;
      heads_naive |= 1ull << i;
    }
  }
  const uint32_t lanes = n < 64 ? n : 64;
  if (cur >= 0)
    for (uint32_t k = (uint32_t)cur; k < lanes; ++k) end_of[k] = (int)lanes;
  const uint64_t heads = xsg::run_heads(change, active);
  if (heads != heads_naive) return 1;
  uint32_t owned[64] = {0};
  for (uint32_t i = 0; i < lanes; ++i) {
    if (!((heads >> i) & 1u)) continue;
    const uint32_t e = xsg::run_end(heads, active, i);
    if ((int)e != end_of[i] || e <= i || e > lanes) return 2;
    for (uint32_t k = i; k < e; ++k) ++owned[k];
  }
  for (uint32_t i = 0; i < 64; ++i)
    if (owned[i] != (i < lanes ? 1u : 0u)) return 4;  // every active lane in exactly one run, no other lane in any
  return 0;
}

extern "C" int cr_check(uint64_t change, uint32_t n) { return check_one(change, n); }

// every mask against every lane count in `ns`; returns the number of failures, the first one in *bad_mask / *bad_n / *bad_code
extern "C" uint64_t cr_check_many(const uint64_t* masks, uint64_t nmasks, const uint32_t* ns, uint32_t nns, uint64_t* bad_mask,
                                  uint32_t* bad_n, int* bad_code) {
  uint64_t bad = 0;
  for (uint64_t k = 0; k < nmasks; ++k)
    for (uint32_t j = 0; j < nns; ++j) {
      const int r = check_one(masks[k], ns[j]);
      if (r && !bad++) *bad_mask = masks[k], *bad_n = ns[j], *bad_code = r;
    }
  return bad;
}

// the run sums as the kernel forms them -- an inclusive prefix over the lanes, one difference per head -- against a
// plain sum per chunk id; ids[i] ascending over the first n lanes.  Returns 0 if every chunk's sum agrees.
extern "C" int cr_check_sums(const uint32_t* ids, const uint32_t* vals, uint32_t n, uint32_t nids) {
  if (n == 0 || n > 64 || nids > 4096) return -1;
  uint64_t change = 0, want[4096] = {0}, got[4096] = {0};
  uint32_t incl[64], acc = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (ids[i] >= nids) return -1;
    if (i && ids[i] != ids[i - 1]) change |= 1ull << i;
    acc += vals[i];
    incl[i] = acc;
    want[ids[i]] += vals[i];
  }
  const uint64_t active = xsg::run_active_mask(n), heads = xsg::run_heads(change, active);
  for (uint32_t i = 0; i < n; ++i) {
    if (!((heads >> i) & 1u)) continue;
    const uint32_t e = xsg::run_end(heads, active, i);
    got[ids[i]] += incl[e - 1] - (i ? incl[i - 1] : 0u);
  }
  for (uint32_t c = 0; c < nids; ++c)
    if (want[c] != got[c]) return 1;
  return 0;
}

#ifdef CHUNK_RUNS_MAIN
int main() {
  uint64_t bad = 0, x = 0x9e3779b97f4a7c15ull;
  for (uint32_t n = 1; n <= 64; ++n) {
    bad += check_one(0, n) != 0;
    bad += check_one(~0ull, n) != 0;
    for (uint32_t a = 0; a < 64; ++a)
      for (uint32_t b = a; b < 64; ++b) bad += check_one((1ull << a) | (1ull << b), n) != 0;
    for (int k = 0; k < 2000; ++k) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      bad += check_one(x, n) != 0;
    }
  }
  printf("chunk_runs_model: %llu failures\n", (unsigned long long)bad);
  return bad != 0;
}
#endif
