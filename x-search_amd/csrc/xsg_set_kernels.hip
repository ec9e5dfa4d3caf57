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
#include "xsg_devutil.h"
#include "xsg_litmatrix.h"
#include "xsg_set.h"

namespace xsg {

constexpr int kSetLoads = 4;                                // 16-byte units per lane: a wave covers 4 KiB, the tile 16 KiB
constexpr uint32_t kSetWaveSpan = kWaveLoad * kSetLoads;
constexpr uint32_t kSetTile = kSetWaveSpan * kWaves;
constexpr uint32_t kSetGridPerCu = 8;                       // workgroups per compute unit of the bounded grid

// ASCII-lower the four bytes of a dword: 0x20 is added to every byte in 'A'..'Z'
__device__ __forceinline__ uint32_t set_fold4(uint32_t d) {
  const uint32_t low7 = d & 0x7f7f7f7fu;
  const uint32_t ge_A = low7 + 0x3f3f3f3fu;  // bit 7 of a byte set <=> its low 7 bits >= 'A'
  const uint32_t gt_Z = low7 + 0x25252525u;  // ... <=> its low 7 bits > 'Z'
  const uint32_t is_upper = ge_A & ~gt_Z & ~d & 0x80808080u;  // (bytes >= 0x80 are not letters)
  return d | (is_upper >> 2);
}

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

template <bool EMIT, bool ICASE>
__global__ __launch_bounds__(kBlock) void k_set_scan(const ScanArgs A, const uint32_t want_nl) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  __shared__ uint32_t s_cnt[kWaves];
  __shared__ uint32_t s_nl[kWaves];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the filter: once per workgroup, 16-byte loads (8 KiB = 512 units, two per thread)
  {
    const uint4* src = reinterpret_cast<const uint4*>(P.d_pat);
    uint4* dst = reinterpret_cast<uint4*>(s_filter);
    for (uint32_t k = tid; k < kSetFilterBytes / 16u; k += kBlock) dst[k] = src[k];
  }
  __syncthreads();
  const uint32_t g = P.set_g;

  for (uint64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    if (EMIT && A.tile_cnt[tile] == 0) continue;  // (workgroup-uniform)
    const uint32_t c = A.tile_chunk ? A.tile_chunk[tile] : 0u;
    const ChunkDev ch = A.chunks[c];
    const uint8_t* cbase = A.base + ch.offset;
    const uint64_t L = ch.length;
    const uint64_t Lr = (L + 15u) & ~(uint64_t)15u;
    // a position p is a candidate only if its whole gram lies inside the chunk: p + g <= L.  Every bit at or beyond
    // `limit` is cleared below, so no decision rests on a byte at or beyond the chunk's end.
    const uint64_t limit = L >= g ? L - g + 1u : 0u;
    const uint64_t toff = (tile - A.chunk_tile0[c]) * (uint64_t)kSetTile;
    const uint64_t wbase = toff + (uint64_t)wave * kSetWaveSpan;

    // ---- the wave's 4 KiB: four 16-byte loads per lane, all issued before any is used; units at or beyond the chunk's
    // padded end are not read.  The dword behind the span (the next wave's or the next tile's first, same chunk) serves
    // the last grams of lane 63's last unit.
    uint4 u[kSetLoads];
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      const uint64_t off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
      u[j] = off < Lr ? *reinterpret_cast<const uint4*>(cbase + off) : uint4{0u, 0u, 0u, 0u};
    }
    const uint64_t behind = wbase + kSetWaveSpan;
    const uint32_t edge_last = behind < Lr ? *reinterpret_cast<const uint32_t*>(cbase + behind) : 0u;

    uint32_t masks[kSetLoads];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      uint32_t w[5] = {u[j].x, u[j].y, u[j].z, u[j].w, 0u};
      // lane 63's neighbour: lane 0 of the next wave-load, or the dword behind the span
      const uint32_t edge = j + 1 < kSetLoads ? (uint32_t)__builtin_amdgcn_readfirstlane((int)u[j + 1 < kSetLoads ? j + 1 : j].x) : edge_last;
      w[4] = from_next_lane(w[0], edge, lane);
      if (ICASE) {
#pragma unroll
        for (int q = 0; q < 5; ++q) w[q] = set_fold4(w[q]);
      }
      uint32_t m;
      switch (g) {  // (wave-uniform)
        case 1: m = set_cand16<1>(w, s_filter); break;
        case 2: m = set_cand16<2>(w, s_filter); break;
        case 3: m = set_cand16<3>(w, s_filter); break;
        default: m = set_cand16<4>(w, s_filter); break;
      }
      const uint64_t unit_off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
      if (unit_off >= limit)
        m = 0u;
      else if (unit_off + kUnit > limit)
        m &= (1u << (uint32_t)(limit - unit_off)) - 1u;
      masks[j] = m;
      cnt += (uint32_t)__popc(m);
    }

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
          const uint64_t unit_off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
          uint32_t mm = m;
          while (mm) {
            const uint32_t b = (uint32_t)__ffs((int)mm) - 1u;
            mm &= mm - 1u;
            if (A.m_cap == 0 || r < A.m_cap) {
              A.m_pos[r] = unit_off + b;
              A.m_chunk[r] = c;
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
  SetTable T;
  T.keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
  T.first = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_first);
  T.ent = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_ent);
  T.bytes = P.d_pat + P.set_bytes;
  T.ngrams = P.set_ngrams;
  T.g = P.set_g;
  const uint64_t p = A.c_pos[i];
  // (the scan reports p only with p + g <= length; a position without that room holds nothing)
  A.c_len[i] = p + T.g <= ch.length ? set_verify_at(T, A.base + ch.offset, p, ch.length, P.icase != 0) : 0u;
}

// ---- xsg_count_literals: one count per literal, the verify step inside the candidate scan's own pass ---------------------------
// k_set_scan<false, ICASE>'s tile loop, loads, fold and candidate masks as they are (copied, not factored out: the
// existing instantiations keep their code byte for byte).  Instead of summing popc, every candidate bit is decided
// here: set_count_at looks the gram up and compares EVERY literal under it; each one that fits the room and compares
// equal adds 1 to its word of a workgroup histogram in LDS.  No candidate list, no size leaves the device; behind its
// grid-stride loop the workgroup adds its non-zero words to LitCountArgs::counts with 64-bit atomics.
//   KEYS_LDS  the sorted keys (at most 16 KiB) are copied into LDS once per workgroup: the binary search, up to 12
//             dependent loads per candidate, stays out of global memory
//   COMPACT   a wave's candidates of one wave-load are first packed into a queue in LDS, so that all 64 lanes verify;
//             otherwise a lane verifies the bits of its own unit as it finds them
// Dynamic LDS: the histogram (nlits words, at most 16 KiB), then the keys, then the queues.
// A histogram word cannot wrap: it counts positions at which ITS literal occurs, at most one per position the workgroup
// looks at, and a workgroup looks at no more than ceil(ntiles / grid) tiles of 16 Ki positions -- the launcher keeps that
// quotient below 2^18, so a word stays below 2^32.
constexpr uint32_t kLitQueue = kWaveLoad;  // candidates of one wave-load: 64 lanes x 16 positions

__host__ __device__ constexpr uint32_t lit_round4(uint32_t n) { return (n + 3u) & ~3u; }

template <bool ICASE, bool KEYS_LDS, bool COMPACT>
__global__ __launch_bounds__(kBlock) void k_set_count_literals(const ScanArgs A, const LitCountArgs C) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lit[];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t* const s_hist = s_lit;
  uint32_t* const s_keys = s_lit + lit_round4(C.nlits);
  uint16_t* const s_queue =
      reinterpret_cast<uint16_t*>(s_keys + (KEYS_LDS ? lit_round4(P.set_ngrams) : 0u)) + (size_t)wave * kLitQueue;
  {
    const uint4* src = reinterpret_cast<const uint4*>(P.d_pat);
    uint4* dst = reinterpret_cast<uint4*>(s_filter);
    for (uint32_t k = tid; k < kSetFilterBytes / 16u; k += kBlock) dst[k] = src[k];
    for (uint32_t k = tid; k < C.nlits; k += kBlock) s_hist[k] = 0u;
    if (KEYS_LDS) {
      const uint32_t* keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
      for (uint32_t k = tid; k < P.set_ngrams; k += kBlock) s_keys[k] = keys[k];
    }
  }
  __syncthreads();
  const uint32_t g = P.set_g;
  SetTable T;
  T.keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
  T.first = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_first);
  T.ent = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_ent);
  T.bytes = P.d_pat + P.set_bytes;
  T.ngrams = P.set_ngrams;
  T.g = g;
  T.idx = reinterpret_cast<const uint16_t*>(P.d_pat + C.idx_off);
  auto hit = [&](uint32_t i) { atomicAdd(&s_hist[i], 1u); };

  for (uint64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const uint32_t c = A.tile_chunk ? A.tile_chunk[tile] : 0u;
    const ChunkDev ch = A.chunks[c];
    const uint8_t* cbase = A.base + ch.offset;
    const uint64_t L = ch.length;
    const uint64_t Lr = (L + 15u) & ~(uint64_t)15u;
    // as in k_set_scan: a candidate's whole gram lies inside the chunk, p + g <= L; no bit at or beyond `limit` survives
    const uint64_t limit = L >= g ? L - g + 1u : 0u;
    const uint64_t toff = (tile - A.chunk_tile0[c]) * (uint64_t)kSetTile;
    const uint64_t wbase = toff + (uint64_t)wave * kSetWaveSpan;

    uint4 u[kSetLoads];
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      const uint64_t off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
      u[j] = off < Lr ? *reinterpret_cast<const uint4*>(cbase + off) : uint4{0u, 0u, 0u, 0u};
    }
    const uint64_t behind = wbase + kSetWaveSpan;
    const uint32_t edge_last = behind < Lr ? *reinterpret_cast<const uint32_t*>(cbase + behind) : 0u;

    uint32_t masks[kSetLoads];
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      uint32_t w[5] = {u[j].x, u[j].y, u[j].z, u[j].w, 0u};
      const uint32_t edge = j + 1 < kSetLoads ? (uint32_t)__builtin_amdgcn_readfirstlane((int)u[j + 1 < kSetLoads ? j + 1 : j].x) : edge_last;
      w[4] = from_next_lane(w[0], edge, lane);
      if (ICASE) {
#pragma unroll
        for (int q = 0; q < 5; ++q) w[q] = set_fold4(w[q]);
      }
      uint32_t m;
      switch (g) {  // (wave-uniform)
        case 1: m = set_cand16<1>(w, s_filter); break;
        case 2: m = set_cand16<2>(w, s_filter); break;
        case 3: m = set_cand16<3>(w, s_filter); break;
        default: m = set_cand16<4>(w, s_filter); break;
      }
      const uint64_t unit_off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
      if (unit_off >= limit)
        m = 0u;
      else if (unit_off + kUnit > limit)
        m &= (1u << (uint32_t)(limit - unit_off)) - 1u;
      masks[j] = m;
    }

    // ---- verify: every candidate, every literal under its gram (the bytes were just loaded: these reads hit the caches)
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      uint32_t m = masks[j];
      const uint64_t load_off = wbase + (uint64_t)j * kWaveLoad;
      if (!COMPACT) {
        while (m) {
          const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
          m &= m - 1u;
          set_count_at(T, cbase, load_off + (uint64_t)lane * kUnit + b, L, ICASE, hit, KEYS_LDS ? s_keys : T.keys);
        }
      } else {
        const uint32_t pc = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan_u32(pc, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (total == 0u) continue;  // (wave-uniform)
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
        for (uint32_t i = lane; i < total; i += 64u)
          set_count_at(T, cbase, load_off + s_queue[i], L, ICASE, hit, KEYS_LDS ? s_keys : T.keys);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the next wave-load refills the queue
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
  }
  __syncthreads();
  for (uint32_t k = tid; k < C.nlits; k += kBlock) {
    const uint32_t v = s_hist[k];
    if (v) atomicAdd(&C.counts[k], (unsigned long long)v);
  }
}

// ---- xsg_count_literals_chunks: a count per chunk AND literal -------------------------------------------------------------------
// k_set_count_literals' tile loop in its default form -- candidates compacted through the per-wave queue -- with the chunk
// boundaries kept (copied again, not factored out: the instantiations above keep their code).  What differs:
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
// Dynamic LDS: the histogram, the keys (KEYS_LDS), the queues, the touched list, chunks_with's sums (short lists).
template <bool ICASE, bool KEYS_LDS>
__global__ __launch_bounds__(kBlock) void k_set_count_literals_chunks(const ScanArgs A, const LitMatrixArgs C) {
  __shared__ __attribute__((aligned(16))) uint32_t s_filter[kSetFilterWords];
  __shared__ uint32_t s_ntouched;
  extern __shared__ __attribute__((aligned(16))) uint32_t s_lit[];
  const PatternDev P = A.pat;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t* const s_hist = s_lit;
  uint32_t* const s_keys = s_lit + lit_round4(C.nlits);
  uint16_t* const s_queues = reinterpret_cast<uint16_t*>(s_keys + (KEYS_LDS ? lit_round4(P.set_ngrams) : 0u));
  uint16_t* const s_queue = s_queues + (size_t)wave * kLitQueue;
  uint16_t* const s_touched = s_queues + (size_t)kWaves * kLitQueue;
  uint32_t* const s_with = reinterpret_cast<uint32_t*>(s_touched + kLitTouched);
  const bool with_lds = C.chunks_with && C.nlits <= kLitWithLds;  // (the launcher sized the LDS by the same rule)
  {
    const uint4* src = reinterpret_cast<const uint4*>(P.d_pat);
    uint4* dst = reinterpret_cast<uint4*>(s_filter);
    for (uint32_t k = tid; k < kSetFilterBytes / 16u; k += kBlock) dst[k] = src[k];
    for (uint32_t k = tid; k < C.nlits; k += kBlock) s_hist[k] = 0u;
    if (KEYS_LDS) {
      const uint32_t* keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
      for (uint32_t k = tid; k < P.set_ngrams; k += kBlock) s_keys[k] = keys[k];
    }
    if (with_lds)
      for (uint32_t k = tid; k < C.nlits; k += kBlock) s_with[k] = 0u;
    if (tid == 0) s_ntouched = 0u;
  }
  __syncthreads();
  const uint32_t g = P.set_g;
  SetTable T;
  T.keys = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_keys);
  T.first = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_first);
  T.ent = reinterpret_cast<const uint32_t*>(P.d_pat + P.set_ent);
  T.bytes = P.d_pat + P.set_bytes;
  T.ngrams = P.set_ngrams;
  T.g = g;
  T.idx = reinterpret_cast<const uint16_t*>(P.d_pat + C.idx_off);
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
    const uint32_t c = A.tile_chunk ? A.tile_chunk[tile] : 0u;
    // (workgroup-uniform) the histogram is flushed behind this tile
    const bool boundary = tile + 1u == tile_end || (A.tile_chunk && A.tile_chunk[tile + 1u] != c);
    const ChunkDev ch = A.chunks[c];
    const uint8_t* cbase = A.base + ch.offset;
    const uint64_t L = ch.length;
    const uint64_t Lr = (L + 15u) & ~(uint64_t)15u;
    // as in k_set_scan: a candidate's whole gram lies inside the chunk, p + g <= L; no bit at or beyond `limit` survives
    const uint64_t limit = L >= g ? L - g + 1u : 0u;
    const uint64_t toff = (tile - A.chunk_tile0[c]) * (uint64_t)kSetTile;
    const uint64_t wbase = toff + (uint64_t)wave * kSetWaveSpan;

    uint4 u[kSetLoads];
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      const uint64_t off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
      u[j] = off < Lr ? *reinterpret_cast<const uint4*>(cbase + off) : uint4{0u, 0u, 0u, 0u};
    }
    const uint64_t behind = wbase + kSetWaveSpan;
    const uint32_t edge_last = behind < Lr ? *reinterpret_cast<const uint32_t*>(cbase + behind) : 0u;

    uint32_t masks[kSetLoads];
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      uint32_t w[5] = {u[j].x, u[j].y, u[j].z, u[j].w, 0u};
      const uint32_t edge = j + 1 < kSetLoads ? (uint32_t)__builtin_amdgcn_readfirstlane((int)u[j + 1 < kSetLoads ? j + 1 : j].x) : edge_last;
      w[4] = from_next_lane(w[0], edge, lane);
      if (ICASE) {
#pragma unroll
        for (int q = 0; q < 5; ++q) w[q] = set_fold4(w[q]);
      }
      uint32_t m;
      switch (g) {  // (wave-uniform)
        case 1: m = set_cand16<1>(w, s_filter); break;
        case 2: m = set_cand16<2>(w, s_filter); break;
        case 3: m = set_cand16<3>(w, s_filter); break;
        default: m = set_cand16<4>(w, s_filter); break;
      }
      const uint64_t unit_off = wbase + (uint64_t)j * kWaveLoad + (uint64_t)lane * kUnit;
      if (unit_off >= limit)
        m = 0u;
      else if (unit_off + kUnit > limit)
        m &= (1u << (uint32_t)(limit - unit_off)) - 1u;
      masks[j] = m;
    }

    // ---- verify: a wave-load's candidates packed into the wave's queue, then every lane decides one
#pragma unroll
    for (int j = 0; j < kSetLoads; ++j) {
      uint32_t m = masks[j];
      const uint64_t load_off = wbase + (uint64_t)j * kWaveLoad;
      const uint32_t pc = (uint32_t)__popc(m);
      const uint32_t incl = wave_incl_scan_u32(pc, lane);
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      if (total == 0u) continue;  // (wave-uniform)
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
      for (uint32_t i = lane; i < total; i += 64u)
        set_count_at(T, cbase, load_off + s_queue[i], L, ICASE, hit, KEYS_LDS ? s_keys : T.keys);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the next wave-load refills the queue
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

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

static unsigned set_grid(const ScanArgs& a) {
  static const unsigned cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return (unsigned)n;
  }();
  return (unsigned)std::min<uint64_t>(a.ntiles, (uint64_t)cus * kSetGridPerCu);
}

hipError_t launch_set_count(const ScanArgs& a, bool want_nl, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (a.tile_bytes != kSetTile || a.pat.set_g < 1 || a.pat.set_g > 4) return hipErrorInvalidValue;
  const dim3 grid(set_grid(a));
  if (a.pat.icase)
    hipLaunchKernelGGL((k_set_scan<false, true>), grid, dim3(kBlock), 0, s, a, want_nl ? 1u : 0u);
  else
    hipLaunchKernelGGL((k_set_scan<false, false>), grid, dim3(kBlock), 0, s, a, want_nl ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_set_emit(const ScanArgs& a, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (a.tile_bytes != kSetTile || a.pat.set_g < 1 || a.pat.set_g > 4) return hipErrorInvalidValue;
  const dim3 grid(set_grid(a));
  if (a.pat.icase)
    hipLaunchKernelGGL((k_set_scan<true, true>), grid, dim3(kBlock), 0, s, a, 0u);
  else
    hipLaunchKernelGGL((k_set_scan<true, false>), grid, dim3(kBlock), 0, s, a, 0u);
  return hipGetLastError();
}

hipError_t launch_set_verify(const RxPreArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_set_verify, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <bool ICASE, bool KEYS_LDS>
static void launch_lit(const ScanArgs& a, const LitCountArgs& c, dim3 grid, size_t lds, hipStream_t s) {
  if (c.compact)
    hipLaunchKernelGGL((k_set_count_literals<ICASE, KEYS_LDS, true>), grid, dim3(kBlock), lds, s, a, c);
  else
    hipLaunchKernelGGL((k_set_count_literals<ICASE, KEYS_LDS, false>), grid, dim3(kBlock), lds, s, a, c);
}

hipError_t launch_set_count_literals(const ScanArgs& a, const LitCountArgs& c, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (a.tile_bytes != kSetTile || a.pat.set_g < 1 || a.pat.set_g > 4 || !c.counts || c.nlits == 0 || c.nlits > XSG_MAX_LITERALS ||
      a.pat.set_ngrams > XSG_MAX_LITERALS)
    return hipErrorInvalidValue;
  // (a histogram word stays below 2^32: fewer than 2^18 tiles per workgroup, see the kernel)
  const uint64_t per = (1u << 18) - 1u;
  const dim3 grid((unsigned)std::max<uint64_t>(set_grid(a), (a.ntiles + per - 1u) / per));
  const size_t lds = 4u * (size_t)lit_round4(c.nlits) + (c.keys_lds ? 4u * (size_t)lit_round4(a.pat.set_ngrams) : 0u) +
                     (c.compact ? 2u * (size_t)kLitQueue * kWaves : 0u);
  if (a.pat.icase)
    c.keys_lds ? launch_lit<true, true>(a, c, grid, lds, s) : launch_lit<true, false>(a, c, grid, lds, s);
  else
    c.keys_lds ? launch_lit<false, true>(a, c, grid, lds, s) : launch_lit<false, false>(a, c, grid, lds, s);
  return hipGetLastError();
}

unsigned set_litmatrix_grid(const ScanArgs& a, uint32_t forced) {
  ScanArgs all{};  // (set_grid of a binding with tiles to spare: workgroups per compute unit x compute units)
  all.ntiles = ~0ull;
  return (unsigned)litmatrix_grid(a.ntiles, (uint64_t)set_grid(all) / kSetGridPerCu * kLitMatrixGridPerCu, forced);
}

hipError_t launch_set_count_literals_chunks(const ScanArgs& a, const LitMatrixArgs& c, uint32_t forced_grid, hipStream_t s) {
  if (a.ntiles == 0) return hipSuccess;
  if (a.tile_bytes != kSetTile || a.pat.set_g < 1 || a.pat.set_g > 4 || !c.counts || c.nlits == 0 || c.nlits > XSG_MAX_LITERALS ||
      a.pat.set_ngrams > XSG_MAX_LITERALS)
    return hipErrorInvalidValue;
  const dim3 grid(set_litmatrix_grid(a, forced_grid));
  // (a histogram word stays below 2^32: fewer than 2^18 tiles per workgroup, xsg_litmatrix.h)
  if (litmatrix_per(a.ntiles, grid.x) >= kLitMatrixPerLimit) return hipErrorInvalidValue;
  const size_t lds = 4u * (size_t)lit_round4(c.nlits) + (c.keys_lds ? 4u * (size_t)lit_round4(a.pat.set_ngrams) : 0u) +
                     2u * (size_t)kLitQueue * kWaves + 2u * (size_t)kLitTouched +
                     (c.chunks_with && c.nlits <= kLitWithLds ? 4u * (size_t)lit_round4(c.nlits) : 0u);
  if (a.pat.icase) {
    if (c.keys_lds)
      hipLaunchKernelGGL((k_set_count_literals_chunks<true, true>), grid, dim3(kBlock), lds, s, a, c);
    else
      hipLaunchKernelGGL((k_set_count_literals_chunks<true, false>), grid, dim3(kBlock), lds, s, a, c);
  } else {
    if (c.keys_lds)
      hipLaunchKernelGGL((k_set_count_literals_chunks<false, true>), grid, dim3(kBlock), lds, s, a, c);
    else
      hipLaunchKernelGGL((k_set_count_literals_chunks<false, false>), grid, dim3(kBlock), lds, s, a, c);
  }
  return hipGetLastError();
}

void describe_set_scan(const ScanArgs& a, bool emit, char* out, size_t cap) {
  snprintf(out, cap, "xsg::k_set_scan<%s, %s> g=%u + xsg::k_set_verify", emit ? "true" : "false", a.pat.icase ? "true" : "false",
           a.pat.set_g);
}

__global__ void k_warm_set() {}
hipError_t warm_set_kernels(hipStream_t s) {
  hipLaunchKernelGGL(k_warm_set, dim3(1), dim3(1), 0, s);
  return hipGetLastError();
}

}  // namespace xsg
