// xsg_set_kernels.hip -- the kernels of a literal LIST (kSet; xsg_set.h has the filter, the hash and the verify table).
//   k_set_scan<EMIT, ICASE>  every position of the text against the filter of 65 536 bits (8 KiB of LDS per workgroup):
//                            a position whose g-gram has its bit is a CANDIDATE.  Same ScanArgs and per-tile outputs as
//                            k_scan -- tile_cnt, then m_pos / m_chunk ascending -- as a count pass and an emit pass.
//   k_set_verify             one lane per candidate: the literals that start with its gram, in listing order, against the
//                            chunk bytes -> c_len, in k_rx_verify's place; k_rx_heads / k_rx_chains / k_rx_compact and
//                            the shared list pipeline take over from there (xsg_list.cpp: prefilter_candidates).
//   k_set_count_literals     xsg_count_literals: the scan with the verify step inside its own pass, one count per literal
//   k_set_count_literals_chunks   xsg_count_literals_chunks: the same pass with the chunk boundaries kept, a count per
//                            chunk and literal and the number of chunks that hold each literal
//   k_set_count_literals_csr, k_set_csr_seam   xsg_count_literals_csr: that matrix in CSR form, a count pass and a fill pass
//                            of the same partition around a prefix sum of the rows' lengths
// The scanning kernels share one copy of each stage: set_stage_filter, set_tile_masks (from the chunk lookup to the
// clipped candidate masks), set_verify_load (the compacted verify of one wave-load) and lit_stage (histogram and keys);
// LitLds is the one layout of the counting kernels' dynamic LDS, for the kernels' pointers and the launchers' byte count.
// XSG_LIST_WHOLE_WORDS (PatternDev::set_words) is tested in set_entry_at alone, behind a compare that succeeded; the candidate
// scan and the filter do not know it.  k_set_verify reads it at run time through set_table().  The counting kernels take it as
// the template argument WORDS, chosen by their launchers: as a run-time flag it cost them 2 to 3 VGPRs, and three of them a
// wave per SIMD, whether the option was on or not (profiles/literal_words_registers.txt) -- with WORDS = false they are the
// kernels they were.
#include "xsg_devutil.h"
#include "xsg_litmatrix.h"
#include "xsg_set.h"

namespace xsg {

constexpr int kSetLoads = 4;                                // 16-byte units per lane: a wave covers 4 KiB, the tile 16 KiB
constexpr uint32_t kSetWaveSpan = kWaveLoad * kSetLoads;
constexpr uint32_t kSetTile = kSetWaveSpan * kWaves;
constexpr uint32_t kSetGridPerCu = 8;                       // workgroups per compute unit of the bounded grid

// candidate bits of one unit: bit b set <=> the g-gram that starts at byte b of the unit has its filter bit.  w[0..3]:
// the unit, w[4]: the dword behind it (the neighbour lane's first).
template <int G>
__device__ __forceinline__ uint32_t set_cand16(const uint32_t (&w)[5], const uint32_t* filter) {
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const int q = b >> 2, r = b & 3;
    uint32_t v = r == 0 ? w[q] : __builtin_amdgcn_alignbyte(w[q + 1], w[q], (uint32_t)r);
    if (G < 4) v &= (1u << (8 * G)) - 1u;
    const uint32_t h = set_gram_hash(v, (uint32_t)G);
    m |= ((filter[h >> 5] >> (h & 31u)) & 1u) << b;
  }
  return m;
}

// the filter into LDS: once per workgroup, 16-byte loads (8 KiB = 512 units, two per thread).  The barrier is the caller's.
__device__ __forceinline__ void set_stage_filter(const PatternDev& P, uint32_t* s_filter, uint32_t tid) {
  const uint4* src = reinterpret_cast<const uint4*>(P.d_pat);
  uint4* dst = reinterpret_cast<uint4*>(s_filter);
  for (uint32_t k = tid; k < kSetFilterBytes / 16u; k += kBlock) dst[k] = src[k];
}

// the verify table inside the pattern's blob; the counting kernels pass the offset of SetTable::idx, the search leaves it null
__device__ __forceinline__ SetTable set_table(const PatternDev& P) {
  SetTable T;
  T.keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
  T.first = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_first);
  T.ent = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_ent);
  T.bytes = P.d_pat + P.set_bytes;
  T.ngrams = P.set_ngrams;
  T.g = P.set_g;
  T.words = P.set_words;  // (wave-uniform; read only behind a compare that succeeded: set_entry_at)
  return T;
}
template <bool WORDS>
__device__ __forceinline__ SetTable set_table(const PatternDev& P, uint32_t idx_off) {
  SetTable T = set_table(P);
  T.idx = reinterpret_cast<const uint16_t*>(P.d_pat + idx_off);
  T.words = WORDS ? 1u : 0u;  // (a constant of the instantiation; the launcher picked it from P.set_words)
  return T;
}

// ---- the tile stage ------------------------------------------------------------------------------------------------------------
// What a kernel still needs of a tile behind its candidate masks: the chunk, its bytes and length, and where this wave's
// 4 KiB begin inside the chunk.
struct SetTile {
  uint32_t c;
  const uint8_t* cbase;
  uint64_t L;
  uint64_t wbase;
};
// masks[j]: the candidate bits of this lane's unit of load j.  u[j]: the unit as loaded (k_set_scan counts newlines on it;
// the counting kernels do not read it).
template <bool ICASE>
__device__ __forceinline__ SetTile set_tile_masks(const ScanArgs& A, uint64_t tile, uint32_t g, const uint32_t* s_filter,
                                                  uint32_t lane, uint32_t wave, uint4 (&u)[kSetLoads],
                                                  uint32_t (&masks)[kSetLoads]) {
  SetTile t;
  t.c = A.tile_chunk ? A.tile_chunk[tile] : 0u;
  const ChunkDev ch = A.chunks[t.c];
  t.cbase = A.base + ch.offset;
  t.L = ch.length;
  const uint64_t Lr = (t.L + 15u) & ~(uint64_t)15u;
  // a position p is a candidate only if its whole gram lies inside the chunk: p + g <= L.  Every bit at or beyond
  // `limit` is cleared below, so no decision rests on a byte at or beyond the chunk's end.
  const uint64_t limit = t.L >= g ? t.L - g + 1u : 0u;
  const uint64_t toff = (tile - A.chunk_tile0[t.c]) * (uint64_t)kSetTile;
  t.wbase = toff + (uint64_t)wave * kSetWaveSpan;

  // ---- the wave's 4 KiB: four 16-byte loads per lane, all issued before any is used; units at or beyond the chunk's
  // padded end are not read.  The dword behind the span (the next wave's or the next tile's first, same chunk) serves
  // the last grams of lane 63's last unit.
#pragma unroll
  for (int j = 0; j < kSetLoads; ++j) {
    const uint64_t off = t.wbase + ((uint32_t)j * kWaveLoad + lane * kUnit);  // (inside the span: 32 bits)
    u[j] = off < Lr ? *reinterpret_cast<const uint4*>(t.cbase + off) : uint4{0u, 0u, 0u, 0u};
  }
  const uint64_t behind = t.wbase + kSetWaveSpan;
  const uint32_t edge_last = behind < Lr ? *reinterpret_cast<const uint32_t*>(t.cbase + behind) : 0u;

#pragma unroll
  for (int j = 0; j < kSetLoads; ++j) {
    uint32_t w[5] = {u[j].x, u[j].y, u[j].z, u[j].w, 0u};
    // lane 63's neighbour: lane 0 of the next wave-load, or the dword behind the span
    const uint32_t edge = j + 1 < kSetLoads ? (uint32_t)__builtin_amdgcn_readfirstlane((int)u[j + 1 < kSetLoads ? j + 1 : j].x) : edge_last;
    w[4] = from_next_lane(w[0], edge, lane);
    if (ICASE) {
#pragma unroll
      for (int q = 0; q < 5; ++q) w[q] = fold4(w[q]);
    }
    uint32_t m;
    switch (g) {  // (wave-uniform)
      case 1: m = set_cand16<1>(w, s_filter); break;
      case 2: m = set_cand16<2>(w, s_filter); break;
      case 3: m = set_cand16<3>(w, s_filter); break;
      default: m = set_cand16<4>(w, s_filter); break;
    }
    // (the offset the load above used, added in 64 bits: spelled as one expression for both, the compiler keeps all four
    // alive from the loads to here -- 6 to 8 VGPRs and a wave per SIMD in the emit pass, profiles/set_refactor_registers.txt)
    const uint64_t unit_off = t.wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
    if (unit_off >= limit)
      m = 0u;
    else if (unit_off + kUnit > limit)
      m &= (1u << (uint32_t)(limit - unit_off)) - 1u;
    masks[j] = m;
  }
  return t;
}

template <bool EMIT, bool ICASE>
__global__ __launch_bounds__(kBlock) void k_set_scan(const ScanArgs A, const uint32_t want_nl) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  __shared__ uint32_t s_cnt[kWaves];
  __shared__ uint32_t s_nl[kWaves];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  set_stage_filter(P, s_filter, tid);
  __syncthreads();
  const uint32_t g = P.set_g;

  for (uint64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    if (EMIT && A.tile_cnt[tile] == 0) continue;  // (workgroup-uniform)
    uint4 u[kSetLoads];
    uint32_t masks[kSetLoads];
    const SetTile t = set_tile_masks<ICASE>(A, tile, g, s_filter, lane, wave, u, masks);
    const uint64_t L = t.L, wbase = t.wbase;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) cnt += (uint32_t)__popc(masks[j]);

    if (!EMIT) {
      const uint32_t wc = wave_sum_u32(cnt);
      if (lane == 0) s_cnt[wave] = wc;
      if (want_nl) {
        // newlines of the tile: counted on bytes below L only
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < kSetLoads; ++j) {
          const uint64_t unit_off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
          if (unit_off < L) {
            const uint32_t d8[8] = {u[j].x, u[j].y, u[j].z, u[j].w, 0u, 0u, 0u, 0u};
            uint32_t nm = nl_mask16(d8) & 0xffffu;
            if (unit_off + kUnit > L) nm &= (1u << (uint32_t)(L - unit_off)) - 1u;
            n += (uint32_t)__popc(nm);
          }
        }
        const uint32_t wn = wave_sum_u32(n);
        if (lane == 0) s_nl[wave] = wn;
      }
      __syncthreads();
      if (tid == 0) {
        A.tile_cnt[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (want_nl) A.tile_nl[tile] = s_nl[0] + s_nl[1] + s_nl[2] + s_nl[3];
      }
      __syncthreads();  // s_cnt / s_nl are free for the next tile
    } else {
      // ---- ordered emission: wave spans are consecutive, loads within a span are consecutive, lanes within a load are
      // consecutive, bits ascend (as k_scan's emit pass)
      const uint32_t wc = wave_sum_u32(cnt);
      if (lane == 0) s_cnt[wave] = wc;
      __syncthreads();
      uint64_t rank = A.tile_off[tile];
      for (uint32_t w2 = 0; w2 < wave; ++w2) rank += s_cnt[w2];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kSetLoads; ++j) {
        const uint32_t m = masks[j];
        const uint32_t pc = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan_u32(pc, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (m) {
          uint64_t r = rank + (incl - pc);
          const uint64_t load_off = wbase + (uint64_t)j * kWaveLoad;
          uint32_t mm = m;
          while (mm) {
            const uint32_t b = (uint32_t)__ffs((int)mm) - 1u;
            mm &= mm - 1u;
            if (A.m_cap == 0 || r < A.m_cap) {
              A.m_pos[r] = load_off + (lane * kUnit + b);  // (= this unit's offset in set_tile_masks, + b: keep them equal)
              A.m_chunk[r] = t.c;
            }
            ++r;
          }
        }
        rank += total;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_set_verify(const RxPreArgs A) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  const PatternDev P = A.pat;
  const ChunkDev ch = A.chunks[A.c_chunk[i]];
  const SetTable T = set_table(P);
  const uint64_t p = A.c_pos[i];
  // (the scan reports p only with p + g <= length; a position without that room holds nothing)
  A.c_len[i] = p + T.g <= ch.length ? set_verify_at(T, A.base + ch.offset, p, ch.length, P.icase != 0) : 0u;
}

// ---- xsg_count_literals: one count per literal, the verify step inside the candidate scan's own pass ---------------------------
// k_set_scan's tile stage as it is (set_tile_masks).  Instead of summing popc, every candidate bit is decided here:
// set_count_at looks the gram up and compares EVERY literal under it; each one that fits the room and compares equal
// adds 1 to its word of a workgroup histogram in LDS.  No candidate list, no size leaves the device; behind its
// grid-stride loop the workgroup adds its non-zero words to LitCountArgs::counts with 64-bit atomics.
//   KEYS     the sorted keys (at most 16 KiB: the launcher refuses more than XSG_MAX_LITERALS grams) are copied into LDS
//            once per workgroup: the binary search, up to 12 dependent loads per candidate, stays out of global memory
//   COMPACT  a wave's candidates of one wave-load are first packed into a queue in LDS, so that all 64 lanes verify
// (Keys read from global memory and a lane verifying the bits of its own unit were built, measured and removed:
// DESIGN.md 3.5e.)
// A histogram word cannot wrap: it counts positions at which ITS literal occurs, at most one per position the workgroup
// looks at, and a workgroup looks at no more than ceil(ntiles / grid) tiles of 16 Ki positions -- the launcher keeps that
// quotient below 2^18, so a word stays below 2^32.
constexpr uint32_t kLitQueue = kWaveLoad;  // candidates of one wave-load: 64 lanes x 16 positions

__host__ __device__ constexpr uint32_t lit_round4(uint32_t n) { return (n + 3u) & ~3u; }

// The dynamic LDS of the two counting kernels, as byte offsets: the histogram (nlits words), the keys (ngrams words), a
// queue per wave, and for the matrix kernel the touched list and chunks_with's sums.  The sums exist only where they are
// wanted and the list is short (kLitWithLds).  bytes_count: what k_set_count_literals needs, histogram, keys and queues;
// bytes: what the matrix kernel needs, all of it.
struct LitLds {
  uint32_t hist, keys, queues, bytes_count, touched, with, bytes;
  bool with_lds;
};
__host__ __device__ constexpr LitLds lit_lds(uint32_t nlits, uint32_t ngrams, bool want_with) {
  LitLds l{};
  l.hist = 0u;
  l.keys = l.hist + 4u * lit_round4(nlits);
  l.queues = l.keys + 4u * lit_round4(ngrams);
  l.bytes_count = l.queues + 2u * kLitQueue * kWaves;
  l.touched = l.bytes_count;
  l.with = l.touched + 2u * kLitTouched;
  l.with_lds = want_with && nlits <= kLitWithLds;
  l.bytes = l.with + (l.with_lds ? 4u * lit_round4(nlits) : 0u);
  return l;
}
// the largest list under as many grams: 42 KiB, and no room for chunks_with's sums above kLitWithLds
static_assert(lit_lds(XSG_MAX_LITERALS, XSG_MAX_LITERALS, false).bytes == 42u * 1024u, "dynamic LDS of the largest list");
static_assert(!lit_lds(XSG_MAX_LITERALS, XSG_MAX_LITERALS, true).with_lds &&
                  lit_lds(XSG_MAX_LITERALS, XSG_MAX_LITERALS, true).bytes == 42u * 1024u,
              "a long list keeps chunks_with out of the LDS");
static_assert(lit_lds(kLitWithLds, XSG_MAX_LITERALS, true).bytes == lit_lds(kLitWithLds, XSG_MAX_LITERALS, false).bytes + 4u * kLitWithLds,
              "a short list sums chunks_with in LDS");

// the histogram zeroed and the sorted keys copied into LDS, once per workgroup.  The barrier is the caller's.
__device__ __forceinline__ void lit_stage(const PatternDev& P, uint32_t nlits, uint32_t* s_hist, uint32_t* s_keys, uint32_t tid) {
  for (uint32_t k = tid; k < nlits; k += kBlock) s_hist[k] = 0u;
  const uint32_t* keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
  for (uint32_t k = tid; k < P.set_ngrams; k += kBlock) s_keys[k] = keys[k];
}

// The compacted verify of one wave-load: `m` holds this lane's candidate bits of the load that begins at `load_off`.  The
// wave packs its candidates into its queue, then every lane decides one: set_count_at with the keys in LDS calls hit(listing
// index) for every literal there (the bytes were just loaded: these reads hit the caches).
template <bool ICASE, typename Hit>
__device__ __forceinline__ void set_verify_load(const SetTable& T, const uint32_t* s_keys, uint16_t* s_queue, const SetTile& t,
                                                uint64_t load_off, uint32_t m, uint32_t lane, Hit& hit) {
  const uint32_t pc = (uint32_t)__popc(m);
  const uint32_t incl = wave_incl_scan_u32(pc, lane);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  if (total == 0u) return;  // (wave-uniform)
  uint32_t r = incl - pc;
  while (m) {
    const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
    m &= m - 1u;
    s_queue[r++] = (uint16_t)(lane * kUnit + b);
  }
  // the queue belongs to this wave alone: a wavefront-scope release/acquire orders its lanes' LDS accesses
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (uint32_t i = lane; i < total; i += 64u) set_count_at(T, t.cbase, load_off + s_queue[i], t.L, ICASE, hit, s_keys);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();  // the next wave-load refills the queue
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool ICASE, bool WORDS>
__global__ __launch_bounds__(kBlock) void k_set_count_literals(const ScanArgs A, const LitCountArgs C) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lit[];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LitLds lay = lit_lds(C.nlits, P.set_ngrams, false);
  uint32_t* const s_hist = reinterpret_cast<uint32_t*>(s_lit + lay.hist);
  uint32_t* const s_keys = reinterpret_cast<uint32_t*>(s_lit + lay.keys);
  uint16_t* const s_queue = reinterpret_cast<uint16_t*>(s_lit + lay.queues) + (size_t)wave * kLitQueue;
  set_stage_filter(P, s_filter, tid);
  lit_stage(P, C.nlits, s_hist, s_keys, tid);
  __syncthreads();
  const uint32_t g = P.set_g;
  const SetTable T = set_table<WORDS>(P, C.idx_off);
  auto hit = [&](uint32_t i) { atomicAdd(&s_hist[i], 1u); };

  for (uint64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    uint4 u[kSetLoads];
    uint32_t masks[kSetLoads];
    const SetTile t = set_tile_masks<ICASE>(A, tile, g, s_filter, lane, wave, u, masks);
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j)
      set_verify_load<ICASE>(T, s_keys, s_queue, t, t.wbase + (uint64_t)j * kWaveLoad, masks[j], lane, hit);
  }
  __syncthreads();
  for (uint32_t k = tid; k < C.nlits; k += kBlock) {
    const uint32_t v = s_hist[k];
    if (v) atomicAdd(&C.counts[k], (unsigned long long)v);
  }
}

// ---- xsg_count_literals_chunks: a count per chunk AND literal -------------------------------------------------------------------
// k_set_count_literals' stages with the chunk boundaries kept.  What differs:
//   PARTITION  a workgroup owns a CONTIGUOUS range of tiles (xsg_litmatrix.h), not a grid stride: tiles ascend by chunk, so
//              the histogram in LDS always belongs to ONE chunk, and the workgroup meets each boundary in its range once.
//   FLUSH      when the next tile belongs to another chunk, and behind the last tile: barrier, the non-zero words are added
//              to row c of the matrix (64-bit atomics: neighbouring workgroups may share a chunk) and zeroed, barrier.  All
//              four waves work on the same tile, so the decision is workgroup-uniform.
//   TOUCHED    with documents of a few KiB every tile is a boundary, and a sweep of the histogram would cost O(literals)
//              per tile.  hit() therefore notes a literal whose word it moved from 0 in a list of kLitTouched uint16
//              through a counter in LDS; the flush walks the list, or sweeps all words when more literals were hit than
//              the list holds.  The counter is never reset: it runs on, and `t_base`, its value at the last flush, is
//              subtracted -- every lane reads the same word between the flush's two barriers, where nobody adds to it.
//              (It grows by at most nlits per flush and a workgroup flushes fewer than 2^18 times: no wrap.)
//   FREQUENCY  an add that finds the matrix word 0 is the first that chunk gets for that literal -- every addend is
//              positive, so a word leaves 0 exactly once -- and adds 1 to chunks_with[j]: exact, no second pass.  For a
//              list of at most kLitWithLds literals the workgroup sums these ones in LDS and adds them behind its last
//              tile: the few words of a short list, added to by every chunk, serialise in the L2 otherwise.
template <bool ICASE, bool WORDS>
__global__ __launch_bounds__(kBlock) void k_set_count_literals_chunks(const ScanArgs A, const LitMatrixArgs C) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  __shared__ uint32_t s_ntouched;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lit[];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LitLds lay = lit_lds(C.nlits, P.set_ngrams, C.chunks_with != nullptr);
  uint32_t* const s_hist = reinterpret_cast<uint32_t*>(s_lit + lay.hist);
  uint32_t* const s_keys = reinterpret_cast<uint32_t*>(s_lit + lay.keys);
  uint16_t* const s_queue = reinterpret_cast<uint16_t*>(s_lit + lay.queues) + (size_t)wave * kLitQueue;
  uint16_t* const s_touched = reinterpret_cast<uint16_t*>(s_lit + lay.touched);
  uint32_t* const s_with = reinterpret_cast<uint32_t*>(s_lit + lay.with);
  const bool with_lds = lay.with_lds;
  set_stage_filter(P, s_filter, tid);
  lit_stage(P, C.nlits, s_hist, s_keys, tid);
  if (with_lds)
    for (uint32_t k = tid; k < C.nlits; k += kBlock) s_with[k] = 0u;
  if (tid == 0) s_ntouched = 0u;
  __syncthreads();
  const uint32_t g = P.set_g;
  const SetTable T = set_table<WORDS>(P, C.idx_off);
  const bool listed = C.touched != 0u;  // (XSG_LITMATRIX_TOUCHED=0, the A/B switch: every flush sweeps)
  uint32_t t_base = 0u;
  auto hit = [&](uint32_t i) {
    if (!listed) {
      atomicAdd(&s_hist[i], 1u);
    } else if (atomicAdd(&s_hist[i], 1u) == 0u) {
      const uint32_t slot = atomicAdd(&s_ntouched, 1u) - t_base;
      if (slot < kLitTouched) s_touched[slot] = (uint16_t)i;
    }
  };

  const uint64_t per = litmatrix_per(A.ntiles, gridDim.x);
  const uint64_t tile_end = litmatrix_last(blockIdx.x, per, A.ntiles);
  for (uint64_t tile = litmatrix_first(blockIdx.x, per, A.ntiles); tile < tile_end; ++tile) {
    uint4 u[kSetLoads];
    uint32_t masks[kSetLoads];
    // the next tile's chunk is read in front of this tile's loads, not behind them where it is used: behind them the pass
    // measured 0.7 % slower on 2^16 chunks of 32 KiB
    const bool last = tile + 1u == tile_end;
    const uint32_t c_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)(!last && A.tile_chunk ? A.tile_chunk[tile + 1u] : 0u));  // (workgroup-uniform)
    const SetTile t = set_tile_masks<ICASE>(A, tile, g, s_filter, lane, wave, u, masks);
    const uint32_t c = t.c;
    // (workgroup-uniform) the histogram is flushed behind this tile
    const bool boundary = last || (A.tile_chunk && c_next != c);
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j)
      set_verify_load<ICASE>(T, s_keys, s_queue, t, t.wbase + (uint64_t)j * kWaveLoad, masks[j], lane, hit);

    if (!boundary) continue;
    // ---- flush into row c
    __syncthreads();
    unsigned long long* const row = C.counts + (uint64_t)c * C.nlits;
    auto add = [&](uint32_t j, uint32_t v) {
      s_hist[j] = 0u;
      if (atomicAdd(&row[j], (unsigned long long)v) == 0ull && C.chunks_with) {
        if (with_lds)
          atomicAdd(&s_with[j], 1u);  // (at most one per chunk of the range: fewer than 2^18)
        else
          atomicAdd(&C.chunks_with[j], 1ull);
      }
    };
    const uint32_t t_now = s_ntouched;
    const uint32_t nt = t_now - t_base;
    t_base = t_now;
    if (listed && nt <= kLitTouched) {
      for (uint32_t k = tid; k < nt; k += kBlock) {
        const uint32_t j = s_touched[k];
        add(j, s_hist[j]);
      }
    } else {
      for (uint32_t k = tid; k < C.nlits; k += kBlock) {
        const uint32_t v = s_hist[k];
        if (v) add(k, v);
      }
    }
    __syncthreads();
  }
  // (behind the last flush's barrier) the chunks of this range that hold each literal
  if (with_lds)
    for (uint32_t k = tid; k < C.nlits; k += kBlock) {
      const uint32_t v = s_with[k];
      if (v) atomicAdd(&C.chunks_with[k], (unsigned long long)v);
    }
}

// ---- xsg_count_literals_csr: the same matrix in CSR form ------------------------------------------------------------------------
// Two passes of k_set_count_literals_chunks' partition around a prefix sum, so that every row has its place before an entry
// is written and no entry's place depends on scheduling.  What differs from the dense kernel:
//   WHOLE / SEAM  a chunk whose tiles all lie in the workgroup's range (xsg_litmatrix.h: litcsr_whole) has one owner: the
//              count pass stores the number of its non-zero words in row_nnz[c], a plain store.  A chunk that crosses a
//              range boundary is summed in the seam buffer, row litcsr_slot of grid x nlits uint64, with 64-bit atomics;
//              k_set_csr_seam counts that row's non-zeros behind the pass.
//   LOOP       the chunk's tile range [t0, t1) decides whole or seam, so it also gives the flush: the workgroup walks
//              min(t1, its range's end) and flushes there -- no look at the next tile's chunk.
//   FILL       the second pass skips the tiles of seam chunks (their rows are complete in the seam buffer; workgroup-
//              uniform) and flushes a whole chunk's non-zero words as (j, word) in ASCENDING j at row_ptr[c] + rank: at
//              most kLitCsrRank noted literals are ranked by counting the smaller ones among them, anything else is an
//              ordered compaction of the histogram (csr_compact).  Every store is guarded by cap_entries.
// Both passes read the same bytes, so the fill pass finds exactly the rows the count pass sized.

// csr_compact's split of a row of k words: wave w takes the words [w * q, (w + 1) * q) (xsg_litmatrix.h)
__device__ __forceinline__ uint32_t csr_wave_span(uint32_t k) { return litcsr_wave_span(k, kWaves); }

// the non-zero words of this wave's span (wave-uniform); get(j) -> unsigned long long
template <typename Get>
__device__ __forceinline__ uint32_t csr_wave_count(uint32_t k, uint32_t lane, uint32_t wave, Get& get) {
  const uint32_t q = csr_wave_span(k), lo = wave * q, hi = lo + q < k ? lo + q : k;
  uint32_t n = 0;
  for (uint32_t j0 = lo; j0 < hi; j0 += 64u) {
    const uint32_t j = j0 + lane;
    n += (uint32_t)__popcll(__ballot(j < hi && get(j) != 0ull));
  }
  return n;
}

// The ordered compaction of a row: put(j, word, rank) for every non-zero word, rank = the non-zero words in front of it.
// A wave counts its span, the counts meet in s_wcnt behind one barrier, then the wave walks its span again with a running
// base and a ballot / mbcnt rank.  Called by all four waves; the caller's barrier behind it frees s_wcnt.
template <typename Get, typename Put>
__device__ __forceinline__ void csr_compact(uint32_t k, uint32_t* s_wcnt, uint32_t lane, uint32_t wave, Get& get, Put& put) {
  const uint32_t n = csr_wave_count(k, lane, wave, get);
  if (lane == 0) s_wcnt[wave] = n;
  __syncthreads();
  uint32_t rank = 0;
  for (uint32_t w = 0; w < wave; ++w) rank += s_wcnt[w];
  const uint32_t q = csr_wave_span(k), lo = wave * q, hi = lo + q < k ? lo + q : k;
  for (uint32_t j0 = lo; j0 < hi; j0 += 64u) {
    const uint32_t j = j0 + lane;
    const unsigned long long v = j < hi ? get(j) : 0ull;
    const unsigned long long m = __ballot(v != 0ull);
    if (v != 0ull) put(j, v, rank + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)));
    rank += (uint32_t)__popcll(m);
  }
}

template <bool ICASE, bool FILL, bool WORDS>
__global__ __launch_bounds__(kBlock) void k_set_count_literals_csr(const ScanArgs A, const LitCsrArgs C) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  __shared__ uint32_t s_ntouched;
  __shared__ uint32_t s_wcnt[kWaves];
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lit[];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LitLds lay = lit_lds(C.nlits, P.set_ngrams, false);
  uint32_t* const s_hist = reinterpret_cast<uint32_t*>(s_lit + lay.hist);
  uint32_t* const s_keys = reinterpret_cast<uint32_t*>(s_lit + lay.keys);
  uint16_t* const s_queue = reinterpret_cast<uint16_t*>(s_lit + lay.queues) + (size_t)wave * kLitQueue;
  uint16_t* const s_touched = reinterpret_cast<uint16_t*>(s_lit + lay.touched);
  set_stage_filter(P, s_filter, tid);
  lit_stage(P, C.nlits, s_hist, s_keys, tid);
  if (tid == 0) s_ntouched = 0u;
  __syncthreads();
  const uint32_t g = P.set_g;
  const SetTable T = set_table<WORDS>(P, C.idx_off);
  const bool listed = C.touched != 0u;
  uint32_t t_base = 0u;  // (the counter runs on, as in k_set_count_literals_chunks)
  auto hit = [&](uint32_t i) {
    if (!listed) {
      atomicAdd(&s_hist[i], 1u);
    } else if (atomicAdd(&s_hist[i], 1u) == 0u) {
      const uint32_t slot = atomicAdd(&s_ntouched, 1u) - t_base;
      if (slot < kLitTouched) s_touched[slot] = (uint16_t)i;
    }
  };
  auto word = [&](uint32_t j) { return (unsigned long long)s_hist[j]; };

  const uint64_t per = litmatrix_per(A.ntiles, gridDim.x);
  const uint64_t tile_first = litmatrix_first(blockIdx.x, per, A.ntiles);
  const uint64_t tile_end = litmatrix_last(blockIdx.x, per, A.ntiles);
  uint64_t tile = tile_first;
  while (tile < tile_end) {
    // (workgroup-uniform) a chunk begins here, or the range does inside one
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)(A.tile_chunk ? A.tile_chunk[tile] : 0u));
    const uint64_t t0 = A.chunk_tile0[c], t1 = A.chunk_tile0[c + 1u];
    const bool whole = litcsr_whole(t0, t1, tile_first, tile_end);
    const uint64_t c_end = t1 < tile_end ? t1 : tile_end;
    if (FILL && !whole) {  // a seam chunk's row is complete in the seam buffer
      tile = c_end;
      continue;
    }
    for (; tile < c_end; ++tile) {
      uint4 u[kSetLoads];
      uint32_t masks[kSetLoads];
      const SetTile t = set_tile_masks<ICASE>(A, tile, g, s_filter, lane, wave, u, masks);
#pragma unroll
      for (int j = 0; j < kSetLoads; ++j)
        set_verify_load<ICASE>(T, s_keys, s_queue, t, t.wbase + (uint64_t)j * kWaveLoad, masks[j], lane, hit);
    }

    // ---- flush chunk c
    __syncthreads();
    const uint32_t t_now = s_ntouched;
    const uint32_t nt = t_now - t_base;
    t_base = t_now;
    const bool walk = listed && nt <= kLitTouched;
    if (!FILL) {
      if (whole) {
        // the row's length: with the list, the literals noted since the last flush
        if (walk) {
          for (uint32_t k = tid; k < nt; k += kBlock) s_hist[s_touched[k]] = 0u;
          if (tid == 0) C.row_nnz[c] = nt;
        } else {
          const uint32_t n = csr_wave_count(C.nlits, lane, wave, word);
          if (lane == 0) s_wcnt[wave] = n;
          __syncthreads();  // (every wave has counted its span: the words may go)
          for (uint32_t k = tid; k < C.nlits; k += kBlock) s_hist[k] = 0u;
          if (tid == 0) C.row_nnz[c] = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        }
      } else {
        unsigned long long* const row = C.seam + litcsr_slot(t0, per) * C.nlits;
        if (walk) {
          for (uint32_t k = tid; k < nt; k += kBlock) {
            const uint32_t j = s_touched[k];
            atomicAdd(&row[j], (unsigned long long)s_hist[j]);
            s_hist[j] = 0u;
          }
        } else {
          for (uint32_t k = tid; k < C.nlits; k += kBlock) {
            const uint32_t v = s_hist[k];
            if (v) {
              atomicAdd(&row[k], (unsigned long long)v);
              s_hist[k] = 0u;
            }
          }
        }
      }
    } else {
      const uint64_t at = C.row_ptr[c];
      auto put = [&](uint32_t j, unsigned long long v, uint32_t rank) {
        s_hist[j] = 0u;
        const uint64_t e = at + rank;
        if (e < C.cap_entries) {
          C.cols[e] = j;
          C.vals[e] = v;
        }
      };
      if (walk && nt <= kLitCsrRank) {
        // the noted literals are distinct: a literal's rank is the number of smaller ones among them
        if (tid < nt) {
          const uint32_t j = s_touched[tid];
          uint32_t rank = 0;
          for (uint32_t i = 0; i < nt; ++i) rank += s_touched[i] < j ? 1u : 0u;
          put(j, s_hist[j], rank);
        }
      } else {
        csr_compact(C.nlits, s_wcnt, lane, wave, word, put);
      }
    }
    __syncthreads();
  }
}

// One workgroup per range of the pass above: the seam chunk that starts in range `blockIdx.x`, if there is one, has its
// whole row in seam[blockIdx.x * nlits ..).  FILL = false: its non-zero words are counted into row_nnz[c]; FILL = true: they
// are compacted in order to row_ptr[c], and one lane of the launch writes *status.  nslots: the grid of the pass (the fill
// launch has one workgroup even for a binding without tiles, for the status word).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_set_csr_seam(const uint32_t* tile_chunk, const uint64_t* chunk_tile0, uint64_t ntiles,
                                                          uint32_t nslots, const LitCsrArgs C) {
  __shared__ uint32_t s_wcnt[kWaves];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (FILL && blockIdx.x == 0 && tid == 0)
    *C.status = C.row_ptr[C.nchunks] > C.cap_entries ? (uint64_t)XSG_STATUS_OVERFLOW : 0ull;
  if (blockIdx.x >= nslots) return;
  const uint64_t per = litmatrix_per(ntiles, nslots);
  const uint64_t first = litmatrix_first(blockIdx.x, per, ntiles), last = litmatrix_last(blockIdx.x, per, ntiles);
  if (first == last) return;
  const uint32_t c = tile_chunk ? tile_chunk[last - 1u] : 0u;
  if (!litcsr_slot_seam(chunk_tile0[c], chunk_tile0[c + 1u], first, last)) return;  // (workgroup-uniform)
  const unsigned long long* const row = C.seam + (uint64_t)blockIdx.x * C.nlits;
  auto word = [&](uint32_t j) { return row[j]; };
  if (!FILL) {
    const uint32_t n = csr_wave_count(C.nlits, lane, wave, word);
    if (lane == 0) s_wcnt[wave] = n;
    __syncthreads();
    if (tid == 0) C.row_nnz[c] = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
  } else {
    const uint64_t at = C.row_ptr[c];
    auto put = [&](uint32_t j, unsigned long long v, uint32_t rank) {
      const uint64_t e = at + rank;
      if (e < C.cap_entries) {
        C.cols[e] = j;
        C.vals[e] = v;
      }
    };
    csr_compact(C.nlits, s_wcnt, lane, wave, word, put);
  }
}

static unsigned set_grid(const ScanArgs& a) {
  static const unsigned cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return (unsigned)n;
  }();
  return (unsigned)std::min<uint64_t>(a.ntiles, (uint64_t)cus * kSetGridPerCu);
}

// what every launcher of a scanning kernel asks of its arguments; the counting launchers add their result and the bounds
// that size the LDS (lit_lds: at most XSG_MAX_LITERALS literals and grams)
static bool set_args_ok(const ScanArgs& a) { return a.tile_bytes == kSetTile && a.pat.set_g >= 1 && a.pat.set_g <= 4; }
static bool set_args_ok(const ScanArgs& a, const unsigned long long* counts, uint32_t nlits) {
  return set_args_ok(a) && counts && nlits != 0 && nlits <= XSG_MAX_LITERALS && a.pat.set_ngrams <= XSG_MAX_LITERALS;
}
// a counting kernel's instantiation for this pattern: [ignore-case][whole words]
template <typename K>
static K lit_kernel(const K (&k)[2][2], const PatternDev& p) {
  return k[p.icase ? 1 : 0][p.set_words ? 1 : 0];
}

hipError_t launch_set_count(const ScanArgs& a, bool want_nl, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (!set_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((a.pat.icase ? k_set_scan<false, true> : k_set_scan<false, false>), dim3(set_grid(a)), dim3(kBlock), 0, s, a,
                     want_nl ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_set_emit(const ScanArgs& a, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (!set_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((a.pat.icase ? k_set_scan<true, true> : k_set_scan<true, false>), dim3(set_grid(a)), dim3(kBlock), 0, s, a, 0u);
  return hipGetLastError();
}

hipError_t launch_set_verify(const RxPreArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_set_verify, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_set_count_literals(const ScanArgs& a, const LitCountArgs& c, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (!set_args_ok(a, c.counts, c.nlits)) return hipErrorInvalidValue;
  // (a histogram word stays below 2^32: fewer than 2^18 tiles per workgroup, see the kernel)
  const uint64_t per = (1u << 18) - 1u;
  const dim3 grid((unsigned)std::max<uint64_t>(set_grid(a), (a.ntiles + per - 1u) / per));
  const size_t lds = lit_lds(c.nlits, a.pat.set_ngrams, false).bytes_count;
  using K = void (*)(const ScanArgs, const LitCountArgs);
  static const K k[2][2] = {{k_set_count_literals<false, false>, k_set_count_literals<false, true>},
                            {k_set_count_literals<true, false>, k_set_count_literals<true, true>}};
  hipLaunchKernelGGL(lit_kernel(k, a.pat), grid, dim3(kBlock), lds, s, a, c);
  return hipGetLastError();
}

unsigned set_litmatrix_grid(const ScanArgs& a, uint32_t forced) {
  ScanArgs all{};  // (set_grid of a binding with tiles to spare: workgroups per compute unit x compute units)
  all.ntiles = ~0ull;
  return (unsigned)litmatrix_grid(a.ntiles, (uint64_t)set_grid(all) / kSetGridPerCu * kLitMatrixGridPerCu, forced);
}

hipError_t launch_set_count_literals_chunks(const ScanArgs& a, const LitMatrixArgs& c, uint32_t forced_grid, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (!set_args_ok(a, c.counts, c.nlits)) return hipErrorInvalidValue;
  const dim3 grid(set_litmatrix_grid(a, forced_grid));
  // (a histogram word stays below 2^32: fewer than 2^18 tiles per workgroup, xsg_litmatrix.h)
  if (litmatrix_per(a.ntiles, grid.x) >= kLitMatrixPerLimit) return hipErrorInvalidValue;
  const size_t lds = lit_lds(c.nlits, a.pat.set_ngrams, c.chunks_with != nullptr).bytes;
  using K = void (*)(const ScanArgs, const LitMatrixArgs);
  static const K k[2][2] = {{k_set_count_literals_chunks<false, false>, k_set_count_literals_chunks<false, true>},
                            {k_set_count_literals_chunks<true, false>, k_set_count_literals_chunks<true, true>}};
  hipLaunchKernelGGL(lit_kernel(k, a.pat), grid, dim3(kBlock), lds, s, a, c);
  return hipGetLastError();
}

unsigned set_litcsr_grid(const ScanArgs& a, uint32_t nlits, uint32_t forced) {
  ScanArgs all{};
  all.ntiles = ~0ull;
  const uint64_t want = (uint64_t)set_grid(all) / kSetGridPerCu * kLitMatrixGridPerCu;
  return (unsigned)litmatrix_grid(a.ntiles, litcsr_grid_cap(want, nlits), forced ? litcsr_grid_cap(forced, nlits) : 0u);
}

hipError_t launch_set_count_literals_csr(const ScanArgs& a, const LitCsrArgs& c, uint32_t grid, bool fill, hipStream_t s) {
  if (!c.row_nnz || (fill && (!c.row_ptr || !c.cols || !c.vals || !c.status))) return hipErrorInvalidValue;
  if (a.ntiles && grid) {
    if (!set_args_ok(a, c.seam, c.nlits)) return hipErrorInvalidValue;
    // (the seam buffer's rows, the workgroups without a tile and the histogram's words: xsg_litmatrix.h)
    if ((uint64_t)grid * c.nlits > kLitCsrSeamWords || grid != litmatrix_grid(a.ntiles, grid, grid) ||
        litmatrix_per(a.ntiles, grid) >= kLitMatrixPerLimit)
      return hipErrorInvalidValue;
    const size_t lds = lit_lds(c.nlits, a.pat.set_ngrams, false).bytes;
    using K = void (*)(const ScanArgs, const LitCsrArgs);
    static const K k_count[2][2] = {{k_set_count_literals_csr<false, false, false>, k_set_count_literals_csr<false, false, true>},
                                    {k_set_count_literals_csr<true, false, false>, k_set_count_literals_csr<true, false, true>}};
    static const K k_fill[2][2] = {{k_set_count_literals_csr<false, true, false>, k_set_count_literals_csr<false, true, true>},
                                   {k_set_count_literals_csr<true, true, false>, k_set_count_literals_csr<true, true, true>}};
    if (fill) {
      hipLaunchKernelGGL(lit_kernel(k_fill, a.pat), dim3(grid), dim3(kBlock), lds, s, a, c);
      hipLaunchKernelGGL(k_set_csr_seam<true>, dim3(grid), dim3(kBlock), 0, s, a.tile_chunk, a.chunk_tile0, a.ntiles, grid, c);
    } else {
      hipLaunchKernelGGL(lit_kernel(k_count, a.pat), dim3(grid), dim3(kBlock), lds, s, a, c);
      hipLaunchKernelGGL(k_set_csr_seam<false>, dim3(grid), dim3(kBlock), 0, s, a.tile_chunk, a.chunk_tile0, a.ntiles, grid, c);
    }
  } else if (fill) {  // no tile: every row is empty, the status word is still due
    hipLaunchKernelGGL(k_set_csr_seam<true>, dim3(1), dim3(kBlock), 0, s, a.tile_chunk, a.chunk_tile0, (uint64_t)0, 0u, c);
  }
  return hipGetLastError();
}

void describe_set_scan(const ScanArgs& a, bool emit, char* out, size_t cap) {
  snprintf(out, cap, "xsg::k_set_scan<%s, %s> g=%u + xsg::k_set_verify%s", emit ? "true" : "false", a.pat.icase ? "true" : "false",
           a.pat.set_g, a.pat.set_words ? " whole words" : "");
}

__global__ void k_warm_set() {}
hipError_t warm_set_kernels(hipStream_t s) {
  hipLaunchKernelGGL(k_warm_set, dim3(1), dim3(1), 0, s);
  return hipGetLastError();
}

}  // namespace xsg
