// xsg_count.cpp -- the C ABI of include/xsg.h, part 4: the count passes (synchronous, split-phase, stream-ordered),
// the probe that measures the hot filter / filter window / stagger of a pattern on a binding, and the tuner.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xsg_host.h"
#include "xsg_sketch.h"

using namespace xsg;

uint32_t xsg::scan_variant(bool want_nl, bool want_lines) { return (want_nl ? 1u : 0u) | (want_lines ? 2u : 0u); }

ScanArgs xsg::scan_args(xsg_shard* s, uint32_t variant) {
  ScanArgs a{};
  a.base = s->base;
  a.chunks = s->d_chunks.as<ChunkDev>();
  a.tile_chunk = s->chunks.size() > 1 ? s->d_tile_chunk.as<uint32_t>() : nullptr;
  a.chunk_tile0 = s->d_chunk_tile0.as<uint64_t>();
  a.ntiles = s->ntiles;
  a.nchunks = s->chunks.size();
  a.tile_bytes = s->tile_bytes;
  // XSG_TUNE, else xsg_shard_tune's choice -- for the pattern it was measured with: a stagger tuned for a literal would
  // cost an instruction-bound class-sequence scan 10 % -- else per variant
  a.tune = s->ctx->tune != kTuneAuto ? s->ctx->tune
                                     : (s->tune_serial == s->ctx->pattern_serial || s->tune_serial == 0) ? s->tune : kTuneAuto;
  a.epoch = s->epoch;
  a.dense_hint = s->density_serial == s->ctx->pattern_serial ? s->dense : 0u;
  a.pat = s->ctx->pat;
  a.pat.hot = s->ctx->hot_env >= 0 ? (uint32_t)s->ctx->hot_env
              : (s->hot_serial == s->ctx->pattern_serial && ((s->hot_known >> variant) & 1u)) ? s->hot_v[variant] : 0u;
  if (a.pat.kind == kLong && s->hot_serial == s->ctx->pattern_serial && s->koff_chosen)
    window_fields(s->ctx->pattern.data(), s->ctx->pattern.size(), s->koff, &a.pat);  // the window measured best on this shard
  a.tile_cnt = s->d_tile_cnt.as<uint32_t>();
  a.tile_nl = s->d_tile_nl.as<uint32_t>();
  a.tile_sum = s->d_tile_sum.as<uint32_t>();
  a.tile_last = s->d_tile_last.as<uint32_t>();
  a.flags = reinterpret_cast<uint32_t*>(s->d_finish.as<uint64_t>() + 3 * (size_t)kFinishBlocks) + 1;  // behind the ticket
  a.tile_mask = (a.pat.kind == kDfa && s->mask_serial != 0 && s->mask_serial == s->ctx->pattern_serial)
                    ? s->d_tile_mask.as<uint32_t>() : nullptr;
  // the gate: the sketch of these bytes, unless a verdict for this pattern and window says it does not pay (a pass
  // without a verdict -- xsg_count_async ahead of any synchronous call -- gates: a wrong guess costs the sketch's 3 %)
  const bool verdict = s->gate_serial == s->ctx->pattern_serial && s->gate_koff == a.pat.koff;
  if (sketch_ready(s) && (!verdict || s->gate_on)) sketch_fields(s, &a);
  return a;
}

// ---- the per-tile 4-gram sketch of a binding and the gate of the plain count pass (xsg_sketch.h) ------------------------
static bool sketch_enabled() {
  const char* e = XSG_TOGGLE("XSG_SKETCH");
  return !(e && *e == '0');
}
// the context's pattern is one the gate serves: a case-sensitive literal of 4 bytes and more
// (not kSet: a tile would have to lack the grams of EVERY literal, and the list route runs no k_scan to gate)
static bool sketch_pattern(const xsg_ctx* c) {
  const uint32_t k = c->pat.kind;
  return (k == kOne || k == kMask2 || k == kTwo || k == kLong) && !c->pat.icase && c->sketch_hashes.size() + 3 == c->pat.plen;
}
bool xsg::sketch_ready(const xsg_shard* s) {
  return s->sketch_tiles != 0 && s->sketch_tiles == s->ntiles && s->d_sketch.p && sketch_enabled() && sketch_pattern(s->ctx);
}
// The pattern's bits as (word, mask) pairs, one per distinct word of a tile's sketch: the grams at the pattern offsets
// koff .. min(plen - 4, koff + 28), koff = the filter window of `a->pat` -- k_scan counts an occurrence in the tile its
// WINDOW starts in.
void xsg::sketch_fields(const xsg_shard* s, ScanArgs* a) {
  const xsg_ctx* c = s->ctx;
  const uint32_t first = a->pat.koff, n = sketch_pattern_grams(a->pat.plen, first);
  if (n == 0 || first + n > c->sketch_hashes.size()) return;
  uint32_t used = 0;
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t h = c->sketch_hashes[first + g], w = h >> 5, bit = 1u << (h & 31u);
    uint32_t k = 0;
    while (k < used && a->sk_word[k] != w) ++k;
    if (k == used) a->sk_word[used] = w, a->sk_mask[used] = 0u, ++used;
    a->sk_mask[k] |= bit;
  }
  a->sk_n = used;
  a->sketch = s->d_sketch.as<uint32_t>();
  a->gate_grid = XSG_TOGGLE_GRID("XSG_GATE_GRID");
  a->sk_pat = a->pat.d_pat;
  a->sk_koff = first;
}

static int build_sketch(xsg_shard* s) {
  xsg_ctx* c = s->ctx;
  if (s->sketch_refused || s->ntiles == 0 || s->tile_bytes != kSketchTileBytes) return XSG_OK;
  if (s->d_sketch.ensure((size_t)sketch_alloc_words(s->ntiles) * 4) != XSG_OK) {
    s->sketch_refused = true;  // no memory for it: this binding simply has no sketch
    return XSG_OK;
  }
  SketchArgs b{};
  b.base = s->base;
  b.chunks = s->d_chunks.as<ChunkDev>();
  b.tile_chunk = s->chunks.size() > 1 ? s->d_tile_chunk.as<uint32_t>() : nullptr;
  b.chunk_tile0 = s->d_chunk_tile0.as<uint64_t>();
  b.ntiles = s->ntiles;
  b.sketch = s->d_sketch.as<uint32_t>();
  // the span locator rides along; without memory for it the binding keeps the tile sketch and whole-tile reads
  const bool spans = s->d_spans.ensure((size_t)span_alloc_words(s->ntiles) * 4) == XSG_OK;
  b.spans = spans ? s->d_spans.as<uint32_t>() : nullptr;
  HIP_TRY(launch_sketch_build(b, c->stream));
  // the bit planes, transposed from the finished sketch right behind it -- with the locator only: the wave form of the
  // finishing pass is their one reader; without memory for them the binding keeps the select from sketch words
  const bool planes = spans && s->d_planes.ensure((size_t)plane_alloc_words(s->ntiles) * 8) == XSG_OK;
  if (planes) HIP_TRY(launch_sketch_planes(b.sketch, s->ntiles, s->d_planes.as<uint64_t>(), c->stream));
  // a pass on a caller's stream must find it complete: the event that orders the chunk table orders the sketch as well
  HIP_TRY(hipEventRecord(s->table_ev, c->stream));
  s->table_pending = true;
  s->sketch_tiles = s->ntiles;
  s->span_tiles = spans ? s->ntiles : 0;
  s->plane_tiles = planes ? s->ntiles : 0;
  s->gate_serial = 0;
  return XSG_OK;
}

int xsg::sketch_before_pass(xsg_shard* s, hipStream_t st, bool plain, bool may_sync, bool counts) {
  xsg_ctx* c = s->ctx;
  if (!plain || !may_sync || st != c->stream || !sketch_enabled() || !sketch_pattern(c)) return XSG_OK;
  if (s->sketch_tiles != s->ntiles && s->total_bytes >= c->sketch_min_bytes) {
    // a synchronous entry point builds before its SECOND eligible pass over a binding (the file pipeline re-binds per
    // chunk and must not pay); XSG_SKETCH=1: before the first; xsg_shard_tune: at once (counts == false, forced there)
    const char* e = XSG_TOGGLE("XSG_SKETCH");
    if (counts && (++s->sketch_passes >= 2u || (e && *e == '1'))) XSG_TRY(build_sketch(s));
  }
  if (!sketch_ready(s)) return XSG_OK;
  if (s->gate_serial == c->pattern_serial && s->gate_koff == scan_args(s).pat.koff) return XSG_OK;
  // The verdict for (binding, pattern, window): the pattern's bits against a strided sample of about 4096 tiles' sketches.
  // A needle whose grams are words of the text passes nearly everywhere and the gate would only add its reads: it is
  // used where fewer than a quarter of the sampled tiles pass.
  ScanArgs a = scan_args(s);
  s->gate_serial = c->pattern_serial;
  s->gate_koff = a.pat.koff;
  s->gate_on = false;
  if (!a.sketch) sketch_fields(s, &a);
  if (!a.sketch) return XSG_OK;
  const uint64_t stride = std::max<uint64_t>(1, s->ntiles / 4096);
  const uint32_t nsamp = (uint32_t)((s->ntiles + stride - 1) / stride);
  uint32_t* word = reinterpret_cast<uint32_t*>(s->d_finish.as<uint64_t>() + 3 * (size_t)kFinishBlocks) + 2;  // behind ticket and flags
  uint32_t passed = 0;
  HIP_TRY(hipMemsetAsync(word, 0, 4, st));
  HIP_TRY(launch_sketch_sample(a, stride, nsamp, word, st));
  HIP_TRY(hipMemcpyAsync(&passed, word, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->gate_on = (uint64_t)passed * 4u < nsamp;
  static const bool probe_log = getenv("XSG_PROBE_LOG") != nullptr;
  if (probe_log) fprintf(stderr, "[xsg] sketch gate: %u of %u sampled tiles pass -> %s\n", passed, nsamp, s->gate_on ? "on" : "off");
  return XSG_OK;
}

int xsg::check_ready(xsg_shard* s) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  if (s->ctx->pattern.empty()) return fail(XSG_ESTATE, "xsg_set_pattern has not been called");
  return XSG_OK;
}

// k_scan only writes where a wave found something: "nothing found" must be in place before it runs.  After a
// count pass it already is (k_count_finish cleaned up behind itself): the steady state enqueues no memset at all.
// Also opens a new epoch for tile_last, and orders a pending chunk-table upload before work on a foreign stream.
int xsg::prepare_tiles(xsg_shard* s, bool want_lines, hipStream_t st) {
  xsg_ctx* c = s->ctx;
  const uint64_t nt = std::max<uint64_t>(s->ntiles, 1);
  if (s->table_pending && st != c->stream) HIP_TRY(hipStreamWaitEvent(st, s->table_ev, 0));
  // A clean-up always covers the WHOLE allocation (the buffers grow geometrically): a later binding with more
  // tiles that still fits must find the words beyond today's ntiles clean as well.
  if (!s->cnt_clean) {
    HIP_TRY(hipMemsetAsync(s->d_tile_cnt.p, 0, s->d_tile_cnt.cap, st));
    s->cnt_clean = true;
  }
  if (!s->last_valid || s->epoch >= 0xffffu) {
    HIP_TRY(hipMemsetAsync(s->d_tile_last.p, 0, s->d_tile_last.cap, st));
    s->last_valid = true;
    s->epoch = 0;
  }
  ++s->epoch;
  if (want_lines) {
    bool grew = false;
    XSG_TRY(s->d_tile_sum.ensure(4 * kWaves * nt, &grew));
    if (grew) s->sum_clean = false;
    if (!s->sum_clean) {
      HIP_TRY(hipMemsetAsync(s->d_tile_sum.p, 0, s->d_tile_sum.cap, st));
      s->sum_clean = true;
    }
  }
  return XSG_OK;
}

int xsg::ensure_tile_nl(xsg_shard* s) {
  bool grew = false;
  XSG_TRY(s->d_tile_nl.ensure(4 * std::max<uint64_t>(s->ntiles, 1), &grew));
  if (grew) s->nl_cached = s->nl_off_cached = false;
  return XSG_OK;
}

// Two events to time launches on a stream between; destroyed with their scope, whichever way it is left.
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t init() {
    const hipError_t e = hipEventCreate(&a);
    return e == hipSuccess ? hipEventCreate(&b) : e;
  }
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// `warm`: one untimed launch first (it pulls the code in); then *ms = the time of `n` launches of this variant
// fin: the launches are the finishing form of the gated count (a plain match count's one kernel), into these counters
static hipError_t time_scan(const ScanArgs& a, bool want_nl, bool want_lines, bool warm, int n, hipStream_t st,
                            const EventPair& ev, float* ms, const GateFinArgs* fin = nullptr) {
  auto launch = [&] { return fin ? launch_scan_count_finishing(a, *fin, st) : launch_scan_count(a, want_nl, want_lines, st); };
  hipError_t e = warm ? launch() : hipSuccess;
  if (e == hipSuccess) e = hipEventRecord(ev.a, st);
  for (int i = 0; i < n && e == hipSuccess; ++i) e = launch();
  if (e == hipSuccess) e = hipEventRecord(ev.b, st);
  if (e == hipSuccess) e = hipEventSynchronize(ev.b);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, ev.a, ev.b);
  return e;
}

static bool is_window_kind(uint32_t k) { return k == kTwo || k == kLong || k == kClass; }

// The window kinds have two hot filters (k_scan<..., ALIGNED>): the aligned-dword trigger does half the VALU work
// but looks at 4 bytes of the window where the window filter looks at 8, so text in which the window's 4-byte
// pieces are common (a window made of words of the text) sends it into the slow path all the time.  Which one is
// faster is a property of (pattern, data, kernel variant): measured once per binding, pattern and VARIANT on a prefix
// of the shard (up to 2 GiB, a few launches of a fraction of a millisecond and one sync), remembered until the shard
// is re-bound or the pattern changes.  The probe times the variant the caller's pass is about to launch (round 3
// timed the newline-counting variant for every mode: the VALU-heaviest shows the largest difference -- but the answer
// differs: on the bench corpus the aligned trigger wins the count + newlines pass by 12 % and loses the plain count,
// which waits for memory with either filter, by 1.7 %).  Shards under 64 MiB keep the window filter (their scans
// take microseconds either way); XSG_HOT pins the choice.
int xsg::choose_hot_filter(xsg_shard* s, hipStream_t st, bool want_nl, bool want_lines) {
  xsg_ctx* c = s->ctx;
  // (kSet is no window kind: k_set_scan has one filter, the list's, and nothing to choose between)
  if (!is_window_kind(c->pat.kind) || c->hot_env >= 0) return XSG_OK;
  const uint32_t v = scan_variant(want_nl, want_lines);
  const bool first = s->hot_serial != c->pattern_serial;  // nothing measured for this pattern on this binding yet
  if (first) {
    s->hot_known = 0;
    memset(s->hot_v, 0, sizeof s->hot_v);
    s->koff_chosen = false;
    s->hot_serial = c->pattern_serial;
  }
  if ((s->hot_known >> v) & 1u) return XSG_OK;
  if (s->total_bytes < c->probe_min_bytes || s->ntiles == 0) {
    s->hot_known = 0xfu;  // too small to measure: the window filter for every variant
    return XSG_OK;
  }
  // Another binding of this buffer may have measured this pattern already (a caller that creates a shard per search).
  // The memo is keyed by address, size, chunk count and a content tag -- the first and last 16 bytes of the text: an
  // allocator that hands a freed address out again for OTHER data of the same size does not inherit the choice.
  bool memo_hit = c->memo.serial == c->pattern_serial && c->memo.base == s->base && c->memo.total_bytes == s->total_bytes &&
                  c->memo.nchunks == s->chunks.size();
  uint64_t tag[4] = {0, 0, 0, 0};
  {
    const xsg_chunk& c0 = s->chunks.front();
    const xsg_chunk& c1 = s->chunks.back();
    HIP_TRY(hipMemcpyAsync(tag, s->base + c0.offset, std::min<uint64_t>(16, c0.length), hipMemcpyDeviceToHost, st));
    if (c1.length >= 16) HIP_TRY(hipMemcpyAsync(tag + 2, s->base + c1.offset + c1.length - 16, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memo_hit = memo_hit && memcmp(tag, c->memo.tag, sizeof tag) == 0;
  }
  if (memo_hit && first) {  // measured on this buffer for this pattern by another binding
    s->koff = c->memo.koff;
    s->koff_chosen = c->memo.koff_chosen;
    if (c->memo.tune_probe && (s->tune_serial != c->pattern_serial || s->tune_probe)) {
      s->tune = c->memo.tune;
      s->tune_serial = s->tune == kTuneAuto ? 0 : c->pattern_serial;
      s->tune_probe = true;
    }
  }
  if (memo_hit && ((c->memo.hot_known >> v) & 1u)) {
    s->hot_v[v] = c->memo.hot_v[v];
    s->hot_known |= (uint8_t)(1u << v);
    return XSG_OK;
  }
  const bool settle_window = first && !memo_hit;  // the filter window and the stagger of a long pattern: once per pattern
  if (want_nl) XSG_TRY(ensure_tile_nl(s));
  XSG_TRY(prepare_tiles(s, want_lines, st));
  s->cnt_clean = false;  // no finish kernel behind these launches
  if (want_lines) s->sum_clean = false;
  EventPair ev;
  HIP_TRY(ev.init());
  float ms[2] = {1e30f, 1e30f};
  int rc = XSG_OK;
  // Long patterns first settle WHICH 8 bytes the hot loop looks for: how often a window occurs in this text decides
  // how often the slow path runs (`detective street` on the bench corpus: "ective s" every 4 KiB, "ve stree" every
  // 11 KiB), and no static letter table knows the text.  Each candidate: the window filter on a 1 GiB prefix.
  if (settle_window && c->pat.kind == kLong && c->koff_cands.size() > 1) {
    // (the candidates are timed on the newline-counting instantiation -- the VALU-heaviest, which shows a window's slow-path
    // rate best -- whatever variant the caller is about to launch: its per-tile newline array must exist.  Since the probe
    // became per-variant in round 4 a plain count no longer allocated it, and a long pattern's first count on a fresh binding
    // stored through a null pointer: tests/test_gpu_parity.py::test_first_search_of_a_fresh_binding_with_a_long_pattern)
    XSG_TRY(ensure_tile_nl(s));
    float best = 1e30f;
    uint32_t best_koff = c->koff_cands[0];
    for (uint32_t koff : c->koff_cands) {
      ScanArgs a = scan_args(s);
      window_fields(c->pattern.data(), c->pattern.size(), koff, &a.pat);
      a.pat.hot = 0;
      a.tune = 0;
      a.sketch = nullptr;  // (the probes measure the filters on the text itself, not the gate in front of them)
      a.ntiles = std::min<uint64_t>(a.ntiles, 65536);
      float t = 0;
      const hipError_t e = time_scan(a, true, false, true, 1, st, ev, &t);  // warm-up, then one timed launch
      if (e != hipSuccess) {
        rc = fail(XSG_EHIP, "window probe failed: %s", hipGetErrorString(e));
        break;
      }
      if (t < 0.97f * best) {  // the first candidate is the heuristic's pick; a later one must beat the best clearly
        best = t;
        best_koff = koff;
      }
    }
    if (rc == XSG_OK) {
      s->koff = best_koff;
      s->koff_chosen = true;
    }
  }
  // A B A B A B, the best of three rounds each: the first launches after a quiet spell run on ramping clocks (measured
  // on fresh bindings of one 50 GiB shard, scripts/probe_check.py: `Sherlock` 0.658 against 0.600 ms in seven probes
  // of eight, 0.664 against 0.633 in the first -- two rounds and a 3 % bar picked the slower filter now and then)
  for (int round = 0; round < 3 && rc == XSG_OK; ++round) {
    for (uint32_t hot = 0; hot < 2 && rc == XSG_OK; ++hot) {
      ScanArgs a = scan_args(s);
      a.pat.hot = hot;
      a.sketch = nullptr;
      // (with the wave stagger the variant's real launches use: round 3 timed with the stagger off, which is how the
      // newline-counting variant runs anyway -- but count_lines runs with 16, and there the aligned trigger wins by 3.7 %
      // where it ties with the stagger off: profiles/r04_dense_variants.txt)
      a.ntiles = std::min<uint64_t>(a.ntiles, 131072);
      // one timed launch per round (0.3 ms on the 2 GiB prefix); the first round warms up first (that pulls the code in)
      float t = 0;
      const hipError_t e = time_scan(a, want_nl, want_lines, round == 0, 1, st, ev, &t);
      if (e != hipSuccess) rc = fail(XSG_EHIP, "hot-filter probe failed: %s", hipGetErrorString(e));
      ms[hot] = std::min(ms[hot], t);
    }
  }
  // The plain count waits for memory and the window filter is its better half at every size measured with warm clocks
  // (10 / 20 / 50 GiB: 0.925 / 0.933 / 0.938 of peak against 0.89-0.90): the aligned trigger has to win visibly.  The
  // variants that also count newlines or keep line summaries are VALU-bound, the trigger is half the filter work and wins
  // by 3-6 % at full size (count_lines 0.92-0.94 against 0.89; with newline counts 0.89 against 0.84) -- but on the 2 GiB
  // prefix the launch ramp dilutes that to ~1 %, inside the probe's noise (a 10 GiB shard: 0.2962 against 0.2993 ms, and a
  // 1.5 % bar kept the window filter): there the WINDOW filter has to win by 1.5 %, as it does when the trigger's pieces
  // are common in the text (profiles/r04_dense_variants.txt).
  s->hot_v[v] = (v == 0 ? ms[1] < 0.995f * ms[0] : ms[1] < 1.015f * ms[0]) ? 1u : 0u;
  s->hot_known |= (uint8_t)(1u << v);
  static const bool probe_log = getenv("XSG_PROBE_LOG") != nullptr;
  if (probe_log)
    fprintf(stderr, "[xsg] hot-filter probe (variant nl=%d lines=%d): window %.4f ms, aligned %.4f ms -> %u (koff %u)\n", (int)want_nl,
            (int)want_lines, ms[0], ms[1], (unsigned)s->hot_v[v], s->koff_chosen ? s->koff : 0u);
  // Long patterns also settle their wave stagger here: the default (16) is right for a scan that waits for memory and
  // costs one that waits for its slow path -- which of the two a long pattern is depends on how often its window occurs
  // in THIS text (`detective street` on the bench corpus: 5.4 TB/s with the default, 6.1 without; `Sherlock Holmes` the
  // other way round).  The plain count with the window and filter just chosen, stagger 0 against the default, on the
  // same prefix; a tie keeps the default.  xsg_shard_tune (all staggers, full size) overrides it.
  if (rc == XSG_OK && settle_window && c->pat.kind == kLong && c->tune == kTuneAuto && (s->tune_serial != c->pattern_serial || s->tune_probe)) {
    float tms[2] = {1e30f, 1e30f};
    static const uint32_t cand[2] = {kDefaultStagger, 0u};
    for (int round = 0; round < 3 && rc == XSG_OK; ++round) {
      for (int k = 0; k < 2 && rc == XSG_OK; ++k) {
        ScanArgs a = scan_args(s);
        a.pat.hot = s->hot_v[v];
        a.tune = cand[k];
        a.sketch = nullptr;
        a.ntiles = std::min<uint64_t>(a.ntiles, 131072);
        float t = 0;
        const hipError_t e = time_scan(a, false, false, round == 0, 1, st, ev, &t);
        if (e != hipSuccess) rc = fail(XSG_EHIP, "stagger probe failed: %s", hipGetErrorString(e));
        tms[k] = std::min(tms[k], t);
      }
    }
    if (rc == XSG_OK) {
      s->tune = tms[1] < 0.97f * tms[0] ? 0u : kTuneAuto;
      s->tune_serial = s->tune == kTuneAuto ? 0 : c->pattern_serial;
      s->tune_probe = true;
    }
  }
  if (rc != XSG_OK) return rc;
  HIP_TRY(hipMemsetAsync(scan_args(s).flags, 0, 4, st));
  if (!memo_hit) {
    c->memo = xsg_ctx::ProbeMemo{};
    c->memo.serial = c->pattern_serial;
    c->memo.base = s->base;
    c->memo.total_bytes = s->total_bytes;
    c->memo.nchunks = s->chunks.size();
    memcpy(c->memo.tag, tag, sizeof tag);
  }
  c->memo.hot_v[v] = s->hot_v[v];
  c->memo.hot_known |= (uint8_t)(1u << v);
  c->memo.koff = s->koff, c->memo.koff_chosen = s->koff_chosen;
  c->memo.tune = s->tune, c->memo.tune_probe = s->tune_probe;
  return XSG_OK;
}

// the finishing form's own arguments: where the result goes, and its scratch words (1 + kFinGroups) behind
// k_count_finish's partials and the 128 bytes of u32 words there (ticket, scan flags, the list route's two)
// The span locator serves these arguments' pass: the binding holds one for its tiles, the arguments gate on the binding's
// sketch with the context's pattern, and XSG_GATE_SPANS is not 0 (the A/B switch: whole-tile reads in the same build).
static bool spans_apply(const xsg_shard* s, const ScanArgs& a) {
  const char* e = XSG_TOGGLE("XSG_GATE_SPANS");
  if (e && *e == '0') return false;
  const xsg_ctx* c = s->ctx;
  return a.sketch != nullptr && a.sk_n != 0 && a.sk_pat == a.pat.d_pat && s->span_tiles != 0 && s->span_tiles == s->ntiles &&
         s->d_spans.p && c->span_hashes.size() == c->sketch_hashes.size() && a.sk_koff + 4u <= a.pat.plen;
}
static GateFinArgs fin_args(xsg_shard* s, const ScanArgs& a, uint64_t* d_counters, uint64_t* host_counters, uint64_t* d_status) {
  GateFinArgs f{};
  f.counters = d_counters;
  f.host_counters = host_counters;
  f.status = d_status;
  f.word = reinterpret_cast<unsigned long long*>(s->d_finish.as<uint64_t>() + 3 * (size_t)kFinishBlocks + 16);
  f.total_bytes = s->total_bytes;
  if (spans_apply(s, a)) {
    // the grams the tile sketch tests (sketch_fields), as (word, mask) pairs of a span's bits (span_entries)
    const xsg_ctx* c = s->ctx;
    const uint32_t first = a.sk_koff, n = sketch_pattern_grams(a.pat.plen, first);
    if (n != 0 && first + n <= c->span_hashes.size()) f.sp_n = span_entries(c->span_hashes.data() + first, n, f.sp_word, f.sp_mask);
    if (f.sp_n) f.spans = s->d_spans.as<uint32_t>();
  }
  // with a locator the pass runs as a wave per sketch group (gated_pass_waves); XSG_GATE_WAVES=0 is the A/B switch that
  // keeps the workgroup form in the same build
  const char* e = XSG_TOGGLE("XSG_GATE_WAVES");
  // (chunk offsets below 2^48: the wave form keeps a passing lane's geometry in four registers)
  f.waves = f.spans != nullptr && !(e && *e == '0') && s->capacity < (1ull << 48);
  // the wave form selects, locates and scans kGateBatch of a wave's groups at a time; XSG_GATE_BATCH=1 is the A/B switch
  // that keeps one group at a time in the same build
  const char* b = XSG_TOGGLE("XSG_GATE_BATCH");
  f.batch = b && *b == '1' && b[1] == 0 ? 1u : kGateBatch;
  // the wave form selects from the sketch's bit planes where the binding holds them for its tiles: one word per gram
  // sketch_fields folded into sk_word / sk_mask, all of them; XSG_GATE_PLANES=0 is the A/B switch that keeps the select
  // from sketch words in the same build
  const char* p = XSG_TOGGLE("XSG_GATE_PLANES");
  if (f.waves && !(p && *p == '0') && s->plane_tiles != 0 && s->plane_tiles == s->ntiles && s->d_planes.p) {
    const xsg_ctx* c = s->ctx;
    const uint32_t first = a.sk_koff, n = sketch_pattern_grams(a.pat.plen, first);
    if (n != 0 && n <= kSketchMaxGrams && first + n <= c->sketch_hashes.size()) {
      for (uint32_t g = 0; g < n; ++g) f.pl_bit[g] = c->sketch_hashes[first + g];
      f.pl_n = n;
      f.pl_stride = plane_stride(s->ntiles);
      f.planes = s->d_planes.as<uint64_t>();
    }
  }
  return f;
}

// does a count of this mode over these arguments go through enqueue_count's finishing form?  (a needle that can overlap
// itself in this data counts through its list: the storing form)
static bool count_finishes(const xsg_shard* s, const ScanArgs& a, uint32_t m, bool want_nl) {
  const xsg_ctx* c = s->ctx;
  return m == XSG_COUNT_MATCHES && !want_nl && !(c->bordered && !overlap_free_known(s)) && scan_finishing(a, s->total_bytes);
}

static int enqueue_count(xsg_shard* s, bool want_matches, bool want_lines, bool want_nl, hipStream_t st,
                         uint64_t* d_counters, uint64_t* host_counters, const PatternDev* other_pattern = nullptr,
                         uint64_t* d_status = nullptr, bool may_sync = true, const ChunkCountArgs* per_chunk = nullptr) {
  if (want_nl) XSG_TRY(ensure_tile_nl(s));
  const uint64_t nchunks = s->chunks.size();
  // kDfa: k_rx_scan counts matching lines directly into tile_cnt (a line is one lane's work): no line summaries
  const bool rx_lines = want_lines && s->ctx->pat.kind == kDfa;
  if (rx_lines) want_lines = false;
  const bool scan_nl = want_nl && !s->nl_cached;  // the per-tile newline counts of this binding may already exist
  if (!other_pattern) XSG_TRY(choose_hot_filter(s, st, scan_nl, want_lines));  // measured for the variant this pass launches
  if (!other_pattern) XSG_TRY(sketch_before_pass(s, st, !scan_nl && !want_lines, may_sync, true));
  XSG_TRY(prepare_tiles(s, want_lines, st));
  ScanArgs a = scan_args(s, scan_variant(scan_nl, want_lines));
  if (other_pattern) {  // (ensure_overlap_check: a word derived from the ctx's pattern, nothing measured or remembered for it)
    a.pat = *other_pattern;
    a.sketch = nullptr;
    a.dense_hint = 0;
    if (s->tune_serial != 0) a.tune = kTuneAuto;
  }
  // A plain match count behind the gate finishes inside its own pass (k_scan_fin): one launch, the per-tile arrays are
  // neither written nor read and stay as prepare_tiles left them.  Everything else -- newline totals, line counts,
  // needles of 34 bytes and more with the lossy tail, the ungated kinds, another pattern -- keeps the two launches below.
  // So does a count per chunk (per_chunk): the finishing form writes no per-tile words for k_count_chunks to sort by chunk;
  // the gate stays, in its storing form.
  if (want_matches && !want_lines && !rx_lines && !want_nl && !other_pattern && !per_chunk && scan_finishing(a, s->total_bytes)) {
    HIP_TRY(launch_scan_count_finishing(a, fin_args(s, a, d_counters, host_counters, d_status), st));
    return XSG_OK;
  }
  // dirty until the finish kernel is in the queue behind the scan
  s->cnt_clean = false;
  if (want_lines) s->sum_clean = false;
  a.lines_only = want_lines && !want_matches;
  HIP_TRY(launch_scan_count(a, scan_nl, want_lines || rx_lines, st));
  FinishArgs f{};
  f.base = s->base;
  f.chunks = a.chunks;
  f.chunk_tile0 = a.chunk_tile0;
  f.nchunks = nchunks;
  f.ntiles = s->ntiles;
  f.pat = a.pat;
  f.tile_cnt = a.tile_cnt;
  f.tile_nl = a.tile_nl;
  f.tile_sum = a.tile_sum;
  f.tile_last = a.tile_last;
  f.epoch = a.epoch;
  f.tile_bytes = s->tile_bytes;
  f.counters = d_counters;
  f.host_counters = host_counters;
  f.status = d_status;
  f.partials = s->d_finish.as<uint64_t>();
  f.ticket = reinterpret_cast<uint32_t*>(s->d_finish.as<uint64_t>() + 3 * (size_t)kFinishBlocks);
  f.flags = a.flags;
  f.total_bytes = s->total_bytes;
  f.want_nl = want_nl;
  f.want_lines = want_lines;
  f.want_matches = want_matches || rx_lines;
  f.cnt_is_lines = rx_lines ? 1u : 0u;
  if (per_chunk) {
    ChunkCountArgs cc = *per_chunk;
    cc.tile_chunk = a.tile_chunk;
    HIP_TRY(launch_count_chunks(f, cc, st));
  } else {
    HIP_TRY(launch_count_finish(f, st));
  }
  s->cnt_clean = true;
  if (want_lines) s->sum_clean = true;
  if (scan_nl) s->nl_cached = true;
  return XSG_OK;
}

// A literal pattern with a border CAN overlap itself; whether it DOES in the bound data is a property of that data, and in
// text it nearly never does (`that`: "thathat" would have to occur).  Two occurrences plen - b apart spell the word
// P[0 .. plen - b) + P, one word per border b: a count pass for each (exact to the end of the chunk, so pairs reaching into
// the end-of-chunk zone are seen too) settles it once per (binding, pattern).  No such word -> every occurrence is kept by
// the reference's walk, and the pattern is counted and listed like one without a border: one pass and no list where
// xs::count took the whole list route (`that` on 10 GiB: 5.3 ms -> one pass).
bool xsg::overlap_free_known(const xsg_shard* s) {
  return s->overlap_serial == s->ctx->pattern_serial && s->overlap_free;
}
int xsg::ensure_overlap_check(xsg_shard* s) {
  xsg_ctx* c = s->ctx;
  if (s->overlap_serial == c->pattern_serial) return XSG_OK;
  s->overlap_serial = c->pattern_serial;
  s->overlap_free = false;
  if (!c->bordered || c->overlap_words.empty() || s->ntiles == 0) return XSG_OK;
  hipStream_t st = c->stream;
  // the words go to the device once per PATTERN (every binding of the file pipeline asks again), side by side
  size_t stride = 0;
  for (const std::vector<uint8_t>& w : c->overlap_words) stride = std::max(stride, (std::max<size_t>(w.size(), 1024) + 16 + 255) & ~(size_t)255);
  if (c->aux_serial != c->pattern_serial) {
    std::vector<uint8_t> all(stride * c->overlap_words.size(), 0);
    for (size_t k = 0; k < c->overlap_words.size(); ++k) memcpy(all.data() + k * stride, c->overlap_words[k].data(), c->overlap_words[k].size());
    XSG_TRY(c->d_aux_pat.ensure(all.size()));
    HIP_TRY(hipMemcpyAsync(c->d_aux_pat.p, all.data(), all.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (`all` leaves scope)
    c->aux_serial = c->pattern_serial;
  }
  for (size_t k = 0; k < c->overlap_words.size(); ++k) {
    const std::vector<uint8_t>& w = c->overlap_words[k];
    PatternDev P{};
    P.plen = (uint32_t)w.size();
    window_fields(w.data(), w.size(), pick_filter_window(w.data(), w.size()), &P);
    P.kind = w.size() < 4 ? kMask1 : w.size() == 4 ? kOne : w.size() < 8 ? kMask2 : w.size() == 8 ? kTwo : kLong;
    P.d_pat = c->d_aux_pat.as<uint8_t>() + k * stride;
    P.exact_tail = 1u;
    P.has_newline = c->pat.has_newline;
    P.icase = c->pat.icase;
    XSG_TRY(enqueue_count(s, true, false, false, st, s->d_counters.as<uint64_t>(), s->h_counters, &P));
    HIP_TRY(hipStreamSynchronize(st));
    s->table_pending = false;
    if (s->h_counters[XSG_CTR_MATCHES] != 0) return XSG_OK;  // they do overlap here: the list route decides which are kept
  }
  s->overlap_free = true;
  return XSG_OK;
}

// XSG_COUNT_MATCHES for a pattern that can overlap itself, without a trip to the host: the list route of xsg_count
// (count pass, ranks, ordered emission, greedy keep, end-of-chunk walk) with the one number it used to fetch --
// how many raw occurrences there are -- left on the device: the arrays get a CAPACITY (twice what the last such
// pass on this shard found, at least a million), emission is bounded by it, the list kernels read the count
// from tile_off[ntiles], and a final kernel adds up keep[] and the tail counts.  More occurrences than capacity
// -> all four counters UINT64_MAX (like the ascii_only refusal): the caller takes xsg_count, which also teaches
// the shard the size for next time.
static int enqueue_count_bordered(xsg_shard* s, hipStream_t st, uint64_t* d_counters, uint64_t* d_status) {
  const uint64_t nchunks = s->chunks.size();
  const uint64_t ntiles = s->ntiles;
  XSG_TRY(choose_hot_filter(s, st));  // (stream-ordered entry point: the sketch and the gate's verdict are used as they are)
  XSG_TRY(prepare_tiles(s, false, st));
  ScanArgs a = scan_args(s);
  s->cnt_clean = false;  // the tile counts stay for the emit pass
  HIP_TRY(launch_scan_count(a, false, false, st));
  XSG_TRY(s->d_tile_off.ensure(8 * (ntiles + 1)));
  const uint64_t cap = std::max<uint64_t>(1u << 20, 2 * s->last_raw_matches);
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(std::max<uint64_t>(ntiles, nchunks) + 1)));
  HIP_TRY(launch_exclusive_scan_u32(a.tile_cnt, s->d_tile_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
  XSG_TRY(s->d_m_pos.ensure(8 * cap));
  XSG_TRY(s->d_m_chunk.ensure(4 * cap));
  XSG_TRY(s->d_keep.ensure(4 * cap));
  uint32_t tail_cap = 0;
  XSG_TRY(ensure_tail_buffers(s, &tail_cap));
  a.tile_off = s->d_tile_off.as<uint64_t>();
  a.m_pos = s->d_m_pos.as<uint64_t>();
  a.m_chunk = s->d_m_chunk.as<uint32_t>();
  a.m_cap = cap;
  HIP_TRY(launch_scan_emit(a, st));
  ListArgs l = list_args(s, a);
  l.pat = a.pat;
  l.M = cap;
  l.M_dev = a.tile_off + ntiles;
  l.keep = s->d_keep.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(l.keep, 0, 4 * cap, st));  // entries that are not chain heads or members are written; be safe
  HIP_TRY(launch_greedy_keep(l, st));
  HIP_TRY(launch_chunk_shift0(l, st));
  HIP_TRY(launch_tail_list(l, st));
  HIP_TRY(hipMemsetAsync(d_counters, 0, 8 * XSG_NUM_COUNTERS, st));
  HIP_TRY(launch_bordered_total(l, d_counters, s->total_bytes, a.flags, d_status, st));
  s->last_mode = -1;
  return XSG_OK;
}

// XSG_FLAG_INVERT, XSG_COUNT_LINES: the lines WITHOUT a match = all lines of the chunks - the matching ones.  The count
// pass ahead ran with newline counts; one small kernel behind it on the same stream turns XSG_CTR_LINES round.
static bool inverted(const xsg_ctx* c) { return (c->flags & XSG_FLAG_INVERT) != 0; }
static int enqueue_invert_lines(xsg_shard* s, hipStream_t st, uint64_t* d_counters, uint64_t* host_counters, uint64_t* d_status,
                                bool keep_nl) {
  HIP_TRY(launch_invert_count_lines(s->base, s->d_chunks.as<ChunkDev>(), s->chunks.size(), d_counters, host_counters, d_status,
                                    keep_nl ? 1u : 0u, st));
  return XSG_OK;
}
// ... for counters a list route left on the host (xsg_count on the prefilter route)
static int invert_lines_sync(xsg_shard* s, uint64_t counters[XSG_NUM_COUNTERS], bool keep_nl) {
  hipStream_t st = s->ctx->stream;
  uint64_t* d = s->d_counters.as<uint64_t>();
  HIP_TRY(hipMemcpyAsync(d, counters, 8 * XSG_NUM_COUNTERS, hipMemcpyHostToDevice, st));
  XSG_TRY(enqueue_invert_lines(s, st, d, nullptr, nullptr, keep_nl));
  HIP_TRY(hipMemcpyAsync(counters, d, 8 * XSG_NUM_COUNTERS, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return XSG_OK;
}

static int refuse_if_poisoned(const uint64_t counters[XSG_NUM_COUNTERS]) {
  if (counters[XSG_CTR_BYTES] == UINT64_MAX) return fail(XSG_ENOTSUP, "%s", kNonAsciiMsg);
  return XSG_OK;
}

static bool is_count_mode(uint32_t mode) { return (mode & 0xffu) == XSG_COUNT_MATCHES || (mode & 0xffu) == XSG_COUNT_LINES; }

// a count entry point's mode word: the mode proper in the low byte, XSG_WITH_NEWLINES beside it, nothing else
static int parse_count_mode(uint32_t mode, uint32_t* m, bool* want_nl) {
  *m = mode & 0xffu;
  *want_nl = (mode & XSG_WITH_NEWLINES) != 0;
  if (mode & ~(0xffu | XSG_WITH_NEWLINES)) return fail(XSG_EINVAL, "unknown mode bits 0x%x", mode);
  return XSG_OK;
}

// xsg_set_max_count: a limit clamps every chunk's count, and the clamped sum needs the per-chunk words and a kernel behind
// them that the stream-ordered entry points do not have: refused behind every refusal they already make
static int refuse_limited(const xsg_ctx* c, const char* who) {
  if (!c->max_count) return XSG_OK;
  return fail(XSG_ENOTSUP, "%s does not serve a limit (xsg_set_max_count): xsg_count(), xsg_count_begin() and xsg_count_chunks() do", who);
}

static int count_async_impl(xsg_shard* s, uint32_t mode, void* stream, uint64_t* d_counters, uint64_t* d_status) {
  XSG_TRY(check_ready(s));
  if (!d_counters) return fail(XSG_EINVAL, "d_counters is null");
  uint32_t m = 0;
  bool want_nl = false;
  XSG_TRY(parse_count_mode(mode, &m, &want_nl));
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
  if (c->pat.kind == kSet)  // (no sketch, no hot-filter probe, no one-pass count either: candidates are verified from a fetched size)
    return fail(XSG_ENOTSUP, "a literal list fetches sizes from the device: the stream-ordered counts do not serve it, xsg_count() does");
  if (m == XSG_COUNT_MATCHES && inverted(c)) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  if (m == XSG_COUNT_MATCHES && all_of_list(c)) return fail(XSG_ENOTSUP, "%s", kAllOfMatchMsg);
  if (m == XSG_COUNT_MATCHES) {
    if (c->bordered && !overlap_free_known(s)) {  // (known from an earlier synchronous call: this entry point may not wait)
      if (want_nl)
        return fail(XSG_ENOTSUP, "pattern can overlap itself: XSG_WITH_NEWLINES next to its match count needs xsg_count()");
      XSG_TRY(refuse_limited(c, "xsg_count_async"));
      return enqueue_count_bordered(s, st, d_counters, d_status);
    }
    XSG_TRY(refuse_limited(c, "xsg_count_async"));
    return enqueue_count(s, true, false, want_nl, st, d_counters, nullptr, nullptr, d_status, false);
  }
  if (m == XSG_COUNT_LINES) {
    if (c->pat.has_newline)
      return fail(XSG_ENOTSUP, "count_lines of a pattern that contains '\\n' walks a chain of occurrences: the stream-ordered entry "
                               "point does not serve it, xsg_count() does");
    XSG_TRY(refuse_limited(c, "xsg_count_async"));
    if (!inverted(c)) return enqueue_count(s, false, true, want_nl, st, d_counters, nullptr, nullptr, d_status, false);
    XSG_TRY(enqueue_count(s, false, true, true, st, d_counters, nullptr, nullptr, d_status, false));
    return enqueue_invert_lines(s, st, d_counters, nullptr, d_status, want_nl);
  }
  return fail(XSG_EINVAL, "xsg_count_async: mode %u is not a count mode", m);
}

extern "C" int xsg_count_async(xsg_shard* s, uint32_t mode, void* stream, uint64_t* d_counters) {
  return count_async_impl(s, mode, stream, d_counters, nullptr);
}

extern "C" int xsg_count_async_status(xsg_shard* s, uint32_t mode, void* stream, uint64_t* d_counters, uint64_t* d_status) {
  if (!d_status) return fail(XSG_EINVAL, "d_status is null");
  return count_async_impl(s, mode, stream, d_counters, d_status);
}

// What the next pass of this pattern over this data can know: a needle found at least once per 2 KiB keeps the slow
// path of the 4..8-byte kinds busy in two wave-loads of five, and the kernel waits for its ALUs, not for memory -- the
// wave stagger that pays for a sparse needle (16) costs such a scan 7 % (`that`: 8.25 ms against 7.66 at 4, 50 GiB).
static void note_density(xsg_shard* s, uint64_t results) {
  if (results == UINT64_MAX) return;
  s->density_serial = s->ctx->pattern_serial;
  // 2: the wave stagger that pays for a sparse needle costs such a scan (pick_stagger); 1: already at one result per 8 KiB a
  // 4..8-byte needle sends a quarter of its wave-loads into the slow path and is cheaper decided byte-parallel
  // (dense_bytes_route; natural text, 10 GiB: `return`, one per 4 KiB, 0.72 of peak on the hot filter -- profiles/r04_natural_variants.txt)
  uint64_t per = 8192u;
  if (const char* e = XSG_TOGGLE("XSG_DENSE_PER")) per = std::max<uint64_t>(strtoull(e, nullptr, 10), 1u);  // A/B: scripts/natural_density.py
  s->dense = results > s->total_bytes / 2048u ? 2u : results > s->total_bytes / per ? 1u : 0u;
}

static int count_chunks_impl(xsg_shard* s, uint32_t mode, uint32_t m, bool want_nl, uint64_t* counts, uint64_t* newlines,
                             uint64_t totals[XSG_NUM_COUNTERS]);

extern "C" int xsg_count(xsg_shard* s, uint32_t mode, uint64_t counters[XSG_NUM_COUNTERS]) {
  XSG_TRY(check_ready(s));
  if (!counters) return fail(XSG_EINVAL, "counters is null");
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  if (!is_count_mode(mode)) return fail(XSG_EINVAL, "mode %u is not a count mode", mode & 0xffu);
  uint32_t m = 0;
  bool want_nl = false;
  XSG_TRY(parse_count_mode(mode, &m, &want_nl));
  if (m == XSG_COUNT_MATCHES && inverted(c)) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  if (m == XSG_COUNT_MATCHES && all_of_list(c)) return fail(XSG_ENOTSUP, "%s", kAllOfMatchMsg);
  // xsg_set_max_count: the sum of the chunks' clamped counts -- the per-chunk machinery into the shard's scratch, one
  // kernel that clamps and sums (a binding without chunks counts nothing either way)
  if (c->max_count && !s->chunks.empty()) return count_chunks_impl(s, mode, m, want_nl, nullptr, nullptr, counters);
  const bool inv = inverted(c);  // (XSG_COUNT_LINES from here on: the pass below also counts newlines)
  XSG_TRY(ensure_factor_mask(s));
  if (use_prefilter(s, false) && s->pre_dense_serial != c->pattern_serial) {  // (not again where the candidates were found dense)
    // the prefilter route of the automaton family: candidates, verification and the walk produce the list; its
    // length is the count (the newline total, if asked for, comes from the cached per-tile counts)
    if (m == XSG_COUNT_LINES && c->pat.has_newline) return fail(XSG_ENOTSUP, "%s", kNewlineExprMsg);
    const int r = run_list(s, m == XSG_COUNT_MATCHES ? XSG_MATCH_BYTE_OFFSETS : XSG_LINE_BYTE_OFFSETS, false, want_nl || inv);
    if (r != kDenseCandidates) {
      XSG_TRY(r);
      memset(counters, 0, 8 * XSG_NUM_COUNTERS);
      counters[m == XSG_COUNT_MATCHES ? XSG_CTR_MATCHES : XSG_CTR_LINES] = s->total;
      counters[XSG_CTR_BYTES] = s->total_bytes;
      if (want_nl || inv) counters[XSG_CTR_NEWLINES] = s->last_newlines;
      s->last_mode = -1;
      if (inv) XSG_TRY(invert_lines_sync(s, counters, want_nl));
      return XSG_OK;
    }
    // too many candidates for the list route to pay: the count passes below walk every line (k_rx_scan)
  }
  if (m == XSG_COUNT_MATCHES && c->bordered) XSG_TRY(ensure_overlap_check(s));
  const bool chain_lines = m == XSG_COUNT_LINES && newline_literal(c);  // the line walk of a literal with '\n' in it
  if ((m == XSG_COUNT_MATCHES && c->bordered && !overlap_free_known(s)) || chain_lines) {
    // greedy non-overlap (and the line walk of a pattern that holds a newline) needs the ordered occurrence list
    XSG_TRY(run_list(s, chain_lines ? XSG_LINE_BYTE_OFFSETS : XSG_MATCH_BYTE_OFFSETS, false));
    note_density(s, s->total);
    memset(counters, 0, 8 * XSG_NUM_COUNTERS);
    counters[chain_lines ? XSG_CTR_LINES : XSG_CTR_MATCHES] = s->total;
    counters[XSG_CTR_BYTES] = s->total_bytes;
    if (want_nl) {
      XSG_TRY(enqueue_count(s, false, false, true, c->stream, s->d_counters.as<uint64_t>(), s->h_counters));
      HIP_TRY(hipStreamSynchronize(c->stream));
      s->table_pending = false;
      counters[XSG_CTR_NEWLINES] = s->h_counters[XSG_CTR_NEWLINES];
    }
    s->last_mode = -1;
    return XSG_OK;
  }
  if (m == XSG_COUNT_LINES && c->pat.has_newline) return fail(XSG_ENOTSUP, "%s", kNewlineExprMsg);
  // the finish kernel writes the four values straight into pinned host memory: no copy, one sync
  XSG_TRY(enqueue_count(s, m == XSG_COUNT_MATCHES, m == XSG_COUNT_LINES, want_nl || inv, c->stream,
                        s->d_counters.as<uint64_t>(), s->h_counters));
  if (inv) XSG_TRY(enqueue_invert_lines(s, c->stream, s->d_counters.as<uint64_t>(), s->h_counters, nullptr, want_nl));
  HIP_TRY(hipStreamSynchronize(c->stream));
  s->table_pending = false;
  memcpy(counters, s->h_counters, 8 * XSG_NUM_COUNTERS);
  if (!inv) note_density(s, counters[m == XSG_COUNT_MATCHES ? XSG_CTR_MATCHES : XSG_CTR_LINES]);  // (of the needle, not of its complement)
  return refuse_if_poisoned(counters);
}

// ---- counts per chunk (xsg_count_chunks, xsg_count_chunks_async) -----------------------------------------------------------
// The scan in its storing form, k_count_chunks behind it, and -- for an inverted line count, or a pattern whose pass can
// be refused -- the small kernel that turns the chunks' words round or zeroes them.  d_counts / d_nl: nchunks words each;
// d_nl is the caller's array (want_nl) or scratch (an inverted count needs every chunk's newlines either way), else null.
static int enqueue_count_chunks(xsg_shard* s, uint32_t m, bool want_nl, hipStream_t st, uint64_t* d_counts, uint64_t* d_nl,
                                uint64_t* d_counters, uint64_t* host_counters, uint64_t* d_status, bool may_sync) {
  xsg_ctx* c = s->ctx;
  const uint64_t nchunks = s->chunks.size();
  const bool inv = inverted(c);  // (XSG_COUNT_LINES: the callers refused the other)
  if (nchunks) HIP_TRY(hipMemsetAsync(d_counts, 0, 8 * nchunks, st));
  if (nchunks && d_nl) HIP_TRY(hipMemsetAsync(d_nl, 0, 8 * nchunks, st));
  ChunkCountArgs cc{};
  cc.counts = d_counts;
  cc.newlines = d_nl;
  XSG_TRY(enqueue_count(s, m == XSG_COUNT_MATCHES, m == XSG_COUNT_LINES, want_nl || inv, st, d_counters, host_counters, nullptr,
                        d_status, may_sync, &cc));
  if (inv) XSG_TRY(enqueue_invert_lines(s, st, d_counters, host_counters, d_status, want_nl));
  const bool refusable = (c->pat.kind == kClass || c->pat.kind == kDfa) && c->pat.ascii_only;
  if (inv || refusable)
    HIP_TRY(launch_chunk_counts_post(s->base, s->d_chunks.as<ChunkDev>(), nchunks, d_counts, d_nl, d_counters, d_status,
                                     inv ? 1u : 0u, st));
  return XSG_OK;
}

// the per-chunk figures behind run_list(outputs = false): from the chunk column of the raw entries, what the walk kept of
// them and the chunks' tail entries (k_list_chunk_counts); newlines from the prefix of the per-tile counts
static int enqueue_list_chunk_counts(xsg_shard* s, uint64_t* d_counts, uint64_t* d_nl, bool with_nl, bool inv) {
  ListChunkArgs a{};
  a.base = s->base;
  a.chunks = s->d_chunks.as<ChunkDev>();
  a.chunk_tile0 = s->d_chunk_tile0.as<uint64_t>();
  a.nchunks = s->chunks.size();
  a.M = s->list_entries;
  a.m_chunk = s->d_m_chunk.as<uint32_t>();
  a.keep_pre = s->d_keep_pre.as<uint64_t>();
  a.tail_cnt = s->d_tail_cnt.as<uint32_t>();
  a.tile_nl_off = with_nl || inv ? s->d_tile_nl_off.as<uint64_t>() : nullptr;
  a.counts = d_counts;
  a.newlines = with_nl ? d_nl : nullptr;
  a.invert = inv ? 1u : 0u;
  HIP_TRY(launch_list_chunk_counts(a, s->ctx->stream));
  return XSG_OK;
}

static int count_chunks_args(xsg_shard* s, uint32_t mode, const uint64_t* counts, const uint64_t* newlines, uint64_t cap_chunks,
                             uint32_t* m, bool* want_nl) {
  XSG_TRY(check_ready(s));
  if (!counts) return fail(XSG_EINVAL, "counts is null");
  if (!is_count_mode(mode)) return fail(XSG_EINVAL, "mode %u is not a count mode", mode & 0xffu);
  XSG_TRY(parse_count_mode(mode, m, want_nl));
  if (newlines && !*want_nl) return fail(XSG_EINVAL, "newlines per chunk need mode | XSG_WITH_NEWLINES");
  if (cap_chunks < s->chunks.size())
    return fail(XSG_EINVAL, "room for %llu chunks, the binding holds %llu", (unsigned long long)cap_chunks,
                (unsigned long long)s->chunks.size());
  if (*m == XSG_COUNT_MATCHES && inverted(s->ctx)) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  if (*m == XSG_COUNT_MATCHES && all_of_list(s->ctx)) return fail(XSG_ENOTSUP, "%s", kAllOfMatchMsg);
  return XSG_OK;
}

extern "C" int xsg_count_chunks(xsg_shard* s, uint32_t mode, uint64_t* counts, uint64_t* newlines, uint64_t cap_chunks,
                                uint64_t totals[XSG_NUM_COUNTERS]) {
  uint32_t m = 0;
  bool want_nl = false;
  XSG_TRY(count_chunks_args(s, mode, counts, newlines, cap_chunks, &m, &want_nl));
  return count_chunks_impl(s, mode, m, want_nl, counts, newlines, totals);
}

// ... behind its argument checks.  counts == null: xsg_count under a limit (xsg_set_max_count), which wants the totals alone
// -- the chunks' words stay in the shard's scratch.  Under a limit one more kernel clamps every chunk's word and sums them:
// the sum replaces the pass's own total, and sum(counts) == totals[...] keeps holding.
static int count_chunks_impl(xsg_shard* s, uint32_t mode, uint32_t m, bool want_nl, uint64_t* counts, uint64_t* newlines,
                             uint64_t totals[XSG_NUM_COUNTERS]) {
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const uint64_t nchunks = s->chunks.size();
  uint64_t tot[XSG_NUM_COUNTERS] = {0, 0, 0, 0};
  if (nchunks == 0) {  // nothing to write per chunk; the totals are xsg_count's
    if (totals) XSG_TRY(xsg_count(s, mode, totals));
    return XSG_OK;
  }
  const bool inv = inverted(c);
  const bool per_nl = newlines != nullptr;
  XSG_TRY(s->d_chunk_counts.ensure(16 * nchunks));
  XSG_TRY(s->h_chunk_counts.ensure(16 * nchunks));
  uint64_t* d_counts = s->d_chunk_counts.as<uint64_t>();
  uint64_t* d_nl = d_counts + nchunks;
  // the same routes as xsg_count, in the same order
  bool listed = false;
  XSG_TRY(ensure_factor_mask(s));
  if (use_prefilter(s, false) && s->pre_dense_serial != c->pattern_serial) {
    if (m == XSG_COUNT_LINES && c->pat.has_newline) return fail(XSG_ENOTSUP, "%s", kNewlineExprMsg);
    const int r = run_list(s, m == XSG_COUNT_MATCHES ? XSG_MATCH_BYTE_OFFSETS : XSG_LINE_BYTE_OFFSETS, false, want_nl || inv);
    if (r != kDenseCandidates) {
      XSG_TRY(r);
      XSG_TRY(enqueue_list_chunk_counts(s, d_counts, d_nl, per_nl, inv));
      tot[m == XSG_COUNT_MATCHES ? XSG_CTR_MATCHES : XSG_CTR_LINES] = s->total;
      tot[XSG_CTR_BYTES] = s->total_bytes;
      if (want_nl || inv) tot[XSG_CTR_NEWLINES] = s->last_newlines;
      s->last_mode = -1;
      if (inv) XSG_TRY(invert_lines_sync(s, tot, want_nl));
      listed = true;
    }
  }
  if (!listed) {
    if (m == XSG_COUNT_MATCHES && c->bordered) XSG_TRY(ensure_overlap_check(s));
    const bool chain_lines = m == XSG_COUNT_LINES && newline_literal(c);
    if ((m == XSG_COUNT_MATCHES && c->bordered && !overlap_free_known(s)) || chain_lines) {
      XSG_TRY(run_list(s, chain_lines ? XSG_LINE_BYTE_OFFSETS : XSG_MATCH_BYTE_OFFSETS, false, want_nl));
      note_density(s, s->total);
      XSG_TRY(enqueue_list_chunk_counts(s, d_counts, d_nl, per_nl, false));
      tot[chain_lines ? XSG_CTR_LINES : XSG_CTR_MATCHES] = s->total;
      tot[XSG_CTR_BYTES] = s->total_bytes;
      if (want_nl) tot[XSG_CTR_NEWLINES] = s->last_newlines;
      s->last_mode = -1;
      listed = true;
    }
  }
  if (!listed) {
    if (m == XSG_COUNT_LINES && c->pat.has_newline) return fail(XSG_ENOTSUP, "%s", kNewlineExprMsg);
    XSG_TRY(enqueue_count_chunks(s, m, want_nl, st, d_counts, per_nl || inv ? d_nl : nullptr, s->d_counters.as<uint64_t>(),
                                 s->h_counters, nullptr, true));
  }
  uint64_t limited_sum = 0;
  if (c->max_count) {
    XSG_TRY(s->d_lim_sum.ensure(8));
    HIP_TRY(hipMemsetAsync(s->d_lim_sum.p, 0, 8, st));
    HIP_TRY(launch_limit_counts(d_counts, nchunks, c->max_count, s->d_lim_sum.as<unsigned long long>(), st));
    HIP_TRY(hipMemcpyAsync(&limited_sum, s->d_lim_sum.p, 8, hipMemcpyDeviceToHost, st));
  }
  uint64_t* h = s->h_chunk_counts.as<uint64_t>();
  if (counts) HIP_TRY(hipMemcpyAsync(h, d_counts, 8 * nchunks * (per_nl ? 2 : 1), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->table_pending = false;
  if (!listed) {
    memcpy(tot, s->h_counters, sizeof tot);
    XSG_TRY(refuse_if_poisoned(tot));
    if (!inv) note_density(s, tot[m == XSG_COUNT_MATCHES ? XSG_CTR_MATCHES : XSG_CTR_LINES]);
  }
  if (c->max_count) tot[m == XSG_COUNT_MATCHES ? XSG_CTR_MATCHES : XSG_CTR_LINES] = limited_sum;
  if (counts) memcpy(counts, h, 8 * nchunks);
  if (per_nl) memcpy(newlines, h + nchunks, 8 * nchunks);
  if (totals) memcpy(totals, tot, sizeof tot);
  return XSG_OK;
}

extern "C" int xsg_count_chunks_async(xsg_shard* s, uint32_t mode, void* stream, uint64_t* d_counts, uint64_t* d_newlines,
                                      uint64_t cap_chunks, uint64_t* d_counters, uint64_t* d_status) {
  uint32_t m = 0;
  bool want_nl = false;
  XSG_TRY(count_chunks_args(s, mode, d_counts, d_newlines, cap_chunks, &m, &want_nl));
  if (!d_counters) return fail(XSG_EINVAL, "d_counters is null");
  if (!d_status) return fail(XSG_EINVAL, "d_status is null");
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
  // what the stream-ordered counts serve through scan + finish, and nothing else: the counts that are lists need sizes
  if (c->pat.kind == kSet)
    return fail(XSG_ENOTSUP, "a literal list fetches sizes from the device: xsg_count_chunks_async does not serve it, xsg_count_chunks() does");
  if (m == XSG_COUNT_MATCHES && c->bordered && !overlap_free_known(s))
    return fail(XSG_ENOTSUP, "pattern can overlap itself and is not known overlap-free on this binding: its matches per chunk "
                             "come from the ordered list, xsg_count_chunks() serves them");
  if (m == XSG_COUNT_LINES && c->pat.has_newline)
    return fail(XSG_ENOTSUP, "count_lines of a pattern that contains '\\n' walks a chain of occurrences: xsg_count_chunks_async "
                             "does not serve it, xsg_count_chunks() does");
  XSG_TRY(refuse_limited(c, "xsg_count_chunks_async"));
  uint64_t* d_nl = d_newlines;
  if (!d_nl && inverted(c) && !s->chunks.empty()) {  // an inverted count needs every chunk's newlines: the shard's scratch
    XSG_TRY(s->d_chunk_counts.ensure(16 * s->chunks.size()));
    d_nl = s->d_chunk_counts.as<uint64_t>() + s->chunks.size();
  }
  return enqueue_count_chunks(s, m, want_nl, st, d_counts, d_nl, d_counters, nullptr, d_status, false);
}

// Split-phase xsg_count for host pipelines: begin enqueues the pass on the ctx stream (results go to the shard's
// pinned mirror), end waits for it.  Between the two the caller may enqueue work for other shards/contexts.
extern "C" int xsg_count_begin(xsg_shard* s, uint32_t mode) {
  XSG_TRY(check_ready(s));
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  if (!is_count_mode(mode)) return fail(XSG_EINVAL, "mode %u is not a count mode", mode & 0xffu);
  uint32_t m = 0;
  bool want_nl = false;
  XSG_TRY(parse_count_mode(mode, &m, &want_nl));
  if (m == XSG_COUNT_MATCHES && inverted(c)) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  if (m == XSG_COUNT_MATCHES && all_of_list(c)) return fail(XSG_ENOTSUP, "%s", kAllOfMatchMsg);
  const bool inv = inverted(c);
  s->begin_sync_result = false;
  XSG_TRY(ensure_factor_mask(s));
  if (m == XSG_COUNT_MATCHES && c->bordered) XSG_TRY(ensure_overlap_check(s));
  if ((m == XSG_COUNT_MATCHES && c->bordered && !overlap_free_known(s)) || (m == XSG_COUNT_LINES && newline_literal(c)) ||
      (use_prefilter(s, false) && s->pre_dense_serial != c->pattern_serial) ||
      c->max_count) {  // needs the ordered list, or the chunks' clamped words (xsg_set_max_count): done synchronously, handed out by _end
    XSG_TRY(xsg_count(s, mode, s->begin_counters));
    s->begin_sync_result = true;
    return XSG_OK;
  }
  if (m == XSG_COUNT_LINES && c->pat.has_newline) return fail(XSG_ENOTSUP, "%s", kNewlineExprMsg);
  XSG_TRY(enqueue_count(s, m == XSG_COUNT_MATCHES, m == XSG_COUNT_LINES, want_nl || inv, c->stream,
                        s->d_counters.as<uint64_t>(), s->h_counters));
  if (inv) XSG_TRY(enqueue_invert_lines(s, c->stream, s->d_counters.as<uint64_t>(), s->h_counters, nullptr, want_nl));
  HIP_TRY(hipEventRecord(s->table_ev, c->stream));  // doubles as "pass done": it covers the table upload too
  s->table_pending = true;
  return XSG_OK;
}

extern "C" int xsg_count_end(xsg_shard* s, uint64_t counters[XSG_NUM_COUNTERS]) {
  if (!s || !counters) return fail(XSG_EINVAL, "null argument");
  if (s->begin_sync_result) {
    memcpy(counters, s->begin_counters, 8 * XSG_NUM_COUNTERS);
    s->begin_sync_result = false;
    return XSG_OK;
  }
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipEventSynchronize(s->table_ev));
  s->table_pending = false;
  memcpy(counters, s->h_counters, 8 * XSG_NUM_COUNTERS);
  return refuse_if_poisoned(counters);
}

extern "C" int xsg_time_scan_kernel(xsg_shard* s, uint32_t mode, int iters, float* avg_ms) {
  XSG_TRY(check_ready(s));
  if (!avg_ms || iters <= 0) return fail(XSG_EINVAL, "bad iters/avg_ms");
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t m = mode & 0xffu;
  const bool want_nl = (mode & XSG_WITH_NEWLINES) != 0;
  // (a literal list: the candidate count pass, which builds no line summaries)
  const bool want_lines = m == XSG_COUNT_LINES && c->pat.kind != kSet;
  if (want_nl) XSG_TRY(ensure_tile_nl(s));
  XSG_TRY(choose_hot_filter(s, c->stream, want_nl, want_lines));  // time what a real pass of this mode would launch
  XSG_TRY(sketch_before_pass(s, c->stream, !want_nl && !want_lines, true, false));  // (its verdict; a timing loop builds none)
  XSG_TRY(prepare_tiles(s, want_lines, c->stream));
  ScanArgs a = scan_args(s, scan_variant(want_nl, want_lines));
  a.lines_only = want_lines;  // XSG_COUNT_LINES: what xsg_count launches for it (enqueue_count)
  // a plain match count that enqueue_count would finish inside its pass is timed in that form (not in the storing form
  // of the list routes), into the binding's scratch counters: the per-tile arrays stay clean
  const bool fin = count_finishes(s, a, m, want_nl);
  const GateFinArgs f = fin_args(s, a, s->d_counters.as<uint64_t>(), nullptr, nullptr);
  if (!fin) s->cnt_clean = s->sum_clean = false;  // no finish kernel runs behind these launches
  EventPair ev;
  HIP_TRY(ev.init());
  float ms = 0;
  HIP_TRY(time_scan(a, want_nl, want_lines, true, iters, c->stream, ev, &ms, fin ? &f : nullptr));  // a warm-up, then the timed launches
  *avg_ms = ms / (float)iters;
  HIP_TRY(hipMemsetAsync(a.flags, 0, 4, c->stream));  // no finish kernel consumed what the scans may have raised
  return XSG_OK;
}

extern "C" int xsg_scan_kernel_name(xsg_shard* s, uint32_t mode, char* out, size_t cap) {
  XSG_TRY(check_ready(s));
  if (!out || !cap) return fail(XSG_EINVAL, "null output");
  const uint32_t m = mode & 0xffu;
  const bool list = m >= XSG_MATCH_BYTE_OFFSETS;
  // what the FIRST pass of this mode launches on this shard right now (newline counts already cached -> plain kernel)
  const bool context = (m == XSG_LINE_BYTE_OFFSETS || m == XSG_LINE_INDICES || m == XSG_LINES) &&
                       (XSG_CONTEXT_BEFORE(s->ctx->flags) != 0 || XSG_CONTEXT_AFTER(s->ctx->flags) != 0);
  const bool want_nl = ((mode & XSG_WITH_NEWLINES) != 0 || m == XSG_LINE_INDICES || context) && !s->nl_cached;
  ScanArgs a = scan_args(s, scan_variant(want_nl, !list && m == XSG_COUNT_LINES));
  if (s->ctx->pat.kind == kSet) {  // a literal list: the candidate scan and its verifier, for every mode
    describe_scan(a, want_nl, false, false, out, cap);
  } else if (use_prefilter(s, false)) {  // what xsg_count / xsg_search launch: the candidate scan, then the automaton at candidates
    a.pat = s->ctx->pre_pat;
    a.pat.hot = 0;
    char inner[160];
    describe_scan(a, want_nl, false, false, inner, sizeof inner);
    snprintf(out, cap, "%s + xsg::k_rx_verify (prefilter route; xsg_count_async: k_rx_scan)", inner);
  } else {
    // (a plain match count says which form of the gated pass it launches: the finishing one, or the storing one)
    const GateFinArgs f = fin_args(s, a, nullptr, nullptr, nullptr);
    describe_scan(a, want_nl, !list && m == XSG_COUNT_LINES, false, out, cap,
                  !list && count_finishes(s, a, m, (mode & XSG_WITH_NEWLINES) != 0), s->total_bytes, spans_apply(s, a),
                  f.waves != 0, f.batch, f.planes != nullptr);
  }
  if (inverted(s->ctx)) {  // the inverted form: the same scan, then the complement (of the list, or of the line count)
    const size_t n = strlen(out);
    snprintf(out + n, cap - n, "%s", list ? " + xsg::k_invert_tile (inverted)" : " + xsg::k_invert_count_lines (inverted)");
  }
  if (s->ctx->max_count) {  // the limit stage: behind the complement, in front of the widening (of the list, or of the chunks' counts)
    const size_t n = strlen(out);
    snprintf(out + n, cap - n, "%s", list ? " + xsg::k_limit_copy (max count)" : " + xsg::k_limit_counts (max count)");
  }
  if (context) {  // the widening stage behind the assembled (or inverted) list
    const size_t n = strlen(out);
    snprintf(out + n, cap - n, " + xsg::k_context_tile (context)");
  }
  return XSG_OK;
}

// Picks the wave stagger of the bulk kernel for THIS shard, pattern and mode by measurement instead of the
// per-variant default (the optimum is sharp and depends on how memory-bound the variant is on the actual data:
// a needle that is dense in this text wants none).  A few launches per candidate; shards under 1 GiB keep the default.
extern "C" int xsg_shard_tune(xsg_shard* s, uint32_t mode, uint32_t* chosen) {
  XSG_TRY(check_ready(s));
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  s->tune = kTuneAuto;
  s->tune_serial = 0;  // (0: the candidate values set inside the loop below apply whatever the serial)
  s->tune_probe = false;
  if (chosen) *chosen = kTuneAuto;
  // The caller is investing in this binding: its sketch is built now (bindings under the sketch's own size limit keep
  // none), ahead of the sweep, which then times the kernel the real passes launch -- gated where the gate pays.
  if (sketch_enabled() && sketch_pattern(c) && (mode & XSG_WITH_NEWLINES) == 0 && (mode & 0xffu) != XSG_COUNT_LINES &&
      s->sketch_tiles != s->ntiles && s->total_bytes >= c->sketch_min_bytes) {
    XSG_TRY(build_sketch(s));
    XSG_TRY(sketch_before_pass(s, c->stream, true, true, false));
  }
  if (c->tune != kTuneAuto || s->total_bytes < (1ull << 30)) return XSG_OK;  // XSG_TUNE wins; too small to measure
  if (c->pat.kind == kDfa || c->pat.kind == kSet) return XSG_OK;  // k_rx_scan and k_set_scan have no stagger
  static const uint32_t cand[] = {0, 4, 8, 10, 12, 14, 16, 20};
  float best_ms = 0;
  uint32_t best = kTuneAuto, best_hot = 0;
  const uint32_t nhot = (is_window_kind(c->pat.kind) && c->hot_env < 0) ? 2u : 1u;
  // the probe first (it also settles a long pattern's filter window, which the loop below keeps), then both hot
  // filters against every stagger at full size
  const bool tune_nl = (mode & XSG_WITH_NEWLINES) != 0, tune_lines = (mode & 0xffu) == XSG_COUNT_LINES;
  const uint32_t v = scan_variant(tune_nl, tune_lines);
  s->hot_serial = 0;
  XSG_TRY(choose_hot_filter(s, c->stream, tune_nl, tune_lines));
  if (nhot == 2) best_hot = s->hot_v[v];
  auto give_up = [&](int r) {
    s->tune = kTuneAuto;
    s->hot_serial = 0;
    s->koff_chosen = false;
    return r;
  };
  // The clocks first: an idle card ramps for several ms and the candidates measured first (the window filter, the small
  // staggers) would be read 3-7 % low -- one bench run in three came back with the slower filter.  ~150 ms of untimed
  // launches, then TWO sweeps and every candidate's better time (profiles/r04_dense_variants.txt).
  {
    float ms = 0;
    s->tune = kDefaultStagger;
    int r = xsg_time_scan_kernel(s, mode, 3, &ms);
    if (r != XSG_OK) return give_up(r);
    const int more = (int)std::min(40.0f, std::max(0.0f, 150.0f / std::max(ms, 0.05f) - 3.0f));
    if (more > 0 && (r = xsg_time_scan_kernel(s, mode, more, &ms)) != XSG_OK) return give_up(r);
  }
  // The wave form of the finishing pass (gated_pass_waves) has no stagger: no four waves share a tile there.  Both hot
  // filters are still timed at full size, once each per round and with as many launches as a sweep would spend; the
  // stagger stays kTuneAuto -- a pick among eight identical timings would be noise, and the value applies to the
  // binding's other passes, where 16 against 0 is worth 5 %.
  bool waves = false;
  {
    const ScanArgs a = scan_args(s, v);
    waves = count_finishes(s, a, mode & 0xffu, tune_nl) && fin_args(s, a, nullptr, nullptr, nullptr).waves != 0;
  }
  constexpr int kCand = (int)(sizeof cand / sizeof cand[0]);
  const int ncand = waves ? 1 : kCand;
  float t_ms[2][kCand];
  for (auto& row : t_ms)
    for (float& x : row) x = 1e30f;
  for (int round = 0; round < 2; ++round) {
    for (uint32_t hot = 0; hot < nhot; ++hot) {
      if (nhot == 2) {
        s->hot_v[v] = (uint8_t)hot;
        s->hot_known |= (uint8_t)(1u << v);
      }
      for (int k = 0; k < ncand; ++k) {
        s->tune = waves ? kTuneAuto : cand[k];
        float ms = 0;
        const int r = xsg_time_scan_kernel(s, mode, waves ? 3 * kCand : 3, &ms);
        if (r != XSG_OK) return give_up(r);
        t_ms[hot][k] = std::min(t_ms[hot][k], ms);
      }
    }
  }
  bool have = false;
  for (uint32_t hot = 0; hot < nhot; ++hot)
    for (int k = 0; k < ncand; ++k)
      if (!have || t_ms[hot][k] < best_ms) have = true, best_ms = t_ms[hot][k], best = waves ? kTuneAuto : cand[k], best_hot = hot;
  s->tune = best;
  s->tune_serial = best == kTuneAuto ? 0 : c->pattern_serial;
  s->tune_probe = false;
  if (nhot == 2) s->hot_v[v] = (uint8_t)best_hot;
  if (chosen) *chosen = best;
  return XSG_OK;
}
