// xsg_shard.cpp -- the C ABI of include/xsg.h, part 3: shards, the bindings of device-resident chunks.
#include <cstring>
#include <new>
#include <vector>

#include "xsg_host.h"

using namespace xsg;

// whatever was derived from the bytes of a binding is void once they change (re-bind, xsg_shard_invalidate)
static void forget_derived(xsg_shard* s) {
  s->nl_cached = s->nl_off_cached = false;  // newline counts per tile and their prefix
  s->hot_serial = 0;                         // measured hot filter / filter window of a pattern
  s->koff_chosen = false;
  s->pre_dense_serial = 0;                   // regex prefilter: candidates found dense
  s->mask_serial = s->mask_dense_serial = 0; // regex factor prefilter: tile marks
  s->fast_dense_serial = 0;                  // a pattern whose lists did not fit the one-sync route
  s->fast_result = false;
  s->line_len_on_device = false;
  s->density_serial = 0;                     // a pattern found dense in this data (scan_args: stagger)
  s->overlap_serial = 0;                     // a bordered pattern whose occurrences do not overlap in this data
  s->sketch_tiles = s->span_tiles = s->plane_tiles = 0;  // the 4-gram sketch of the tiles, its span locator, its bit planes and the gate's verdict on a pattern
  s->sketch_passes = 0;
  s->sketch_refused = false;
  s->gate_serial = 0;
  s->kept_csr.valid = false;                 // the kept result of xsg_count_literals_csr
  s->kept_find.valid = false;                // the kept result of xsg_find_literals
}

static int bind_shard(xsg_shard* s, const void* d_base, uint64_t capacity, const xsg_chunk* chunks, uint64_t nchunks) {
  xsg_ctx* c = s->ctx;
  if (nchunks && !chunks) return fail(XSG_EINVAL, "chunks is null");
  if (nchunks && !d_base) return fail(XSG_EINVAL, "d_base is null");
  if (((uintptr_t)d_base & 15u) != 0) return fail(XSG_EINVAL, "d_base is not 16-byte aligned");
  if (nchunks >= (1ull << 32)) return fail(XSG_EINVAL, "too many chunks");
  uint64_t prev_end = 0, ntiles = 0, total = 0;
  const uint32_t tile_bytes = c->tile_bytes;
  std::vector<uint64_t> tile0(nchunks + 1, 0);
  for (uint64_t i = 0; i < nchunks; ++i) {
    const xsg_chunk& k = chunks[i];
    if (k.offset & 15u) return fail(XSG_EINVAL, "chunk %llu: offset %llu is not a multiple of 16", (unsigned long long)i,
                                    (unsigned long long)k.offset);
    if (k.length >= (1ull << 40)) return fail(XSG_EINVAL, "chunk %llu: length too large", (unsigned long long)i);
    const uint64_t rl = (k.length + 15u) & ~(uint64_t)15u;
    if (k.offset < prev_end) return fail(XSG_EINVAL, "chunk %llu overlaps its predecessor or is out of order",
                                         (unsigned long long)i);
    if (k.offset + rl > capacity || k.offset + rl < k.offset)
      return fail(XSG_EINVAL, "chunk %llu: offset+round_up(length,16) exceeds the shard capacity",
                  (unsigned long long)i);
    prev_end = k.offset + k.length;
    tile0[i] = ntiles;
    ntiles += (k.length + tile_bytes - 1) / tile_bytes;
    total += k.length;
  }
  tile0[nchunks] = ntiles;
  HIP_TRY(hipSetDevice(c->device));

  s->base = static_cast<const uint8_t*>(d_base);
  s->capacity = capacity;
  s->chunks.assign(chunks, chunks + nchunks);
  s->chunk_tile0 = std::move(tile0);
  s->ntiles = ntiles;
  s->tile_bytes = tile_bytes;
  s->total_bytes = total;
  s->last_mode = -1;
  s->total = 0;

  forget_derived(s);
  bool grew = false;
  XSG_TRY(s->d_chunks.ensure(sizeof(ChunkDev) * std::max<uint64_t>(nchunks, 1)));
  XSG_TRY(s->d_chunk_tile0.ensure(8 * (nchunks + 1)));
  XSG_TRY(s->d_tile_last.ensure(4 * std::max<uint64_t>(ntiles, 1), &grew));
  if (grew) s->last_valid = false;
  grew = false;
  XSG_TRY(s->d_tile_cnt.ensure(4 * std::max<uint64_t>(ntiles, 1), &grew));
  if (grew) s->cnt_clean = false;
  XSG_TRY(s->d_counters.ensure(8 * XSG_NUM_COUNTERS));
  grew = false;
  // k_count_finish scratch: the partial sums, then 128 bytes of u32 words: [0] ticket, [1] scan flags; behind them the
  // arrival words of the finishing form of the gated count (GateFinArgs::word)
  constexpr size_t kFinishBytes = 8 * 3 * (size_t)kFinishBlocks + 128 + 8 * (1 + (size_t)kFinGroups);
  XSG_TRY(s->d_finish.ensure(kFinishBytes, &grew));
  if (grew) HIP_TRY(hipMemsetAsync(s->d_finish.p, 0, kFinishBytes, c->stream));  // tickets and arrival words = 0
  if (!s->h_counters) HIP_TRY(hipHostMalloc((void**)&s->h_counters, 8 * XSG_NUM_COUNTERS, hipHostMallocDefault));
  if (!s->table_ev) HIP_TRY(hipEventCreateWithFlags(&s->table_ev, hipEventDisableTiming));
  static_assert(sizeof(ChunkDev) == sizeof(xsg_chunk), "layout");
  if (nchunks <= 1) {
    // The file pipeline re-binds its one-chunk shard for every chunk it feeds: the 48 bytes of table go through
    // a pinned staging block and no host sync.  The block is reused only after the previous upload has run.
    if (!s->h_stage) HIP_TRY(hipHostMalloc(&s->h_stage, 64, hipHostMallocDefault));
    if (s->table_pending) HIP_TRY(hipEventSynchronize(s->table_ev));
    uint8_t* st = static_cast<uint8_t*>(s->h_stage);
    if (nchunks) memcpy(st, s->chunks.data(), sizeof(xsg_chunk));
    memcpy(st + 32, s->chunk_tile0.data(), 8 * (nchunks + 1));
    if (nchunks) HIP_TRY(hipMemcpyAsync(s->d_chunks.p, st, sizeof(xsg_chunk), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->d_chunk_tile0.p, st + 32, 8 * (nchunks + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(s->table_ev, c->stream));
    s->table_pending = true;
    return XSG_OK;
  }
  HIP_TRY(hipMemcpyAsync(s->d_chunks.p, s->chunks.data(), sizeof(xsg_chunk) * nchunks, hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipMemcpyAsync(s->d_chunk_tile0.p, s->chunk_tile0.data(), 8 * (nchunks + 1), hipMemcpyHostToDevice,
                         c->stream));
  std::vector<uint32_t> map(ntiles);
  for (uint64_t i = 0; i < nchunks; ++i)
    for (uint64_t t = s->chunk_tile0[i]; t < s->chunk_tile0[i + 1]; ++t) map[t] = (uint32_t)i;
  XSG_TRY(s->d_tile_chunk.ensure(4 * std::max<uint64_t>(ntiles, 1)));
  if (ntiles) HIP_TRY(hipMemcpyAsync(s->d_tile_chunk.p, map.data(), 4 * ntiles, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // `map` is a local
  s->table_pending = false;
  return XSG_OK;
}

extern "C" int xsg_shard_invalidate(xsg_shard* s) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  if (s->ctx->memo.base == s->base) s->ctx->memo = xsg_ctx::ProbeMemo{};
  forget_derived(s);
  s->last_mode = -1;
  s->total = 0;
  return XSG_OK;
}

extern "C" int xsg_shard_create(xsg_ctx* c, const void* d_base, uint64_t capacity, const xsg_chunk* chunks,
                                uint64_t nchunks, xsg_shard** out) {
  if (!c) return fail(XSG_EINVAL, "ctx is null");
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  xsg_shard* s = new (std::nothrow) xsg_shard();
  if (!s) return fail(XSG_ENOMEM, "host allocation failed");
  s->ctx = c;
  int r = bind_shard(s, d_base, capacity, chunks, nchunks);
  if (r != XSG_OK) {
    s->release_all();
    delete s;
    return r;
  }
  *out = s;
  return XSG_OK;
}

extern "C" int xsg_shard_rebind(xsg_shard* s, const void* d_base, uint64_t capacity, const xsg_chunk* chunks,
                                uint64_t nchunks) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  if (s->ctx->memo.base == s->base || s->ctx->memo.base == d_base) s->ctx->memo = xsg_ctx::ProbeMemo{};  // (the bytes changed)
  return bind_shard(s, d_base, capacity, chunks, nchunks);
}

extern "C" void xsg_shard_destroy(xsg_shard* s) {
  if (!s) return;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  s->release_all();
  delete s;
}

extern "C" int xsg_shard_set_line_base(xsg_shard* s, uint64_t line_base) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  s->shard_line_base = line_base;
  return XSG_OK;
}

// XSG_TEST_HOOKS=1 only (not part of include/xsg.h): the host-side bookkeeping of a binding, for tests that must show
// which state a call order met (tests/test_gpu_call_sequences.py).  Waits for the context's stream unless n <= 18.
extern "C" int xsg_test_shard_state(xsg_shard* s, uint64_t* out, size_t n) {
  if (!s || !out) return fail(XSG_EINVAL, "null argument");
  if (!test_hooks()) return fail(XSG_ENOTSUP, "xsg_test_shard_state needs XSG_TEST_HOOKS=1");
  const xsg_ctx* c = s->ctx;
  const uint64_t serial = c->pattern_serial;
  uint32_t word = 0;
  if (n > 18) {  // the first tile's tile_last word
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (s->d_tile_last.p) HIP_TRY(hipMemcpy(&word, s->d_tile_last.p, 4, hipMemcpyDeviceToHost));
  }
  const uint64_t v[] = {s->epoch,
                        s->cnt_clean,
                        s->sum_clean,
                        s->last_valid,
                        s->nl_cached,
                        s->table_pending,
                        s->fast_result,
                        (uint64_t)(s->fast_dense_serial == serial || c->fast_dense_serial == serial),
                        (uint64_t)(s->overlap_serial == serial),
                        (uint64_t)(s->overlap_serial == serial && s->overlap_free),
                        s->last_raw_matches,
                        (uint64_t)(s->mask_serial != 0 && s->mask_serial == serial),
                        s->density_serial == serial ? s->dense : 0u,
                        s->tune,
                        (uint64_t)(s->tune_serial == serial),
                        s->d_tile_cnt.cap,
                        s->d_tile_sum.cap,
                        (uint64_t)(uintptr_t)c->stream,
                        word};
  for (size_t i = 0; i < n && i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
  return XSG_OK;
}
