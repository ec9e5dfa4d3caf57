// xsg_list.cpp -- the list searches of the C ABI of include/xsg.h: the one-sync route, the exact route with its
// prefilter and factor-mask variants for the automaton family, xsg_search and the result accessors.  Host glue only;
// the kernels are in xsg_kernels.hip, xsg_list_kernels.hip and xsg_rx_kernels.hip.  No CPU fallback.
#include <algorithm>
#include <cstring>
#include <vector>

#include "xsg_host.h"
#include "xsg_tail.h"

using namespace xsg;

static int d2h_u64(xsg_ctx* c, const uint64_t* d, uint64_t* h) {
  HIP_TRY(hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XSG_OK;
}

// XSG_FLAG_CONTEXT with a non-zero count (the line-list tags widen their list; every other tag ignores the bits)
static bool context_on(const xsg_ctx* c) { return XSG_CONTEXT_BEFORE(c->flags) != 0 || XSG_CONTEXT_AFTER(c->flags) != 0; }

// XSG_LIST_ALL_OF: the context's pattern is a literal list whose lines must hold every literal
bool xsg::all_of_list(const xsg_ctx* c) { return c->pat.kind == kSet && c->pat.set_all_of != 0; }

bool xsg::newline_literal(const xsg_ctx* c) { return c->pat.has_newline && c->pat.kind != kClass && c->pat.kind != kDfa && c->pat.kind != kSet; }

// ---------------------------------------------------------------------------
// argument blocks
// ---------------------------------------------------------------------------
static uint32_t tail_capacity(const xsg_ctx* c) { return std::max<uint32_t>(tail_max_matches(c->pat.plen), 1u); }

int xsg::ensure_tail_buffers(xsg_shard* s, uint32_t* tail_cap) {
  const uint64_t nchunks = s->chunks.size();
  *tail_cap = tail_capacity(s->ctx);
  XSG_TRY(s->d_chunk_shift0.ensure(8 * std::max<uint64_t>(nchunks, 1)));
  XSG_TRY(s->d_tail_cnt.ensure(4 * std::max<uint64_t>(nchunks, 1)));
  XSG_TRY(s->d_tail_pos.ensure(8 * std::max<uint64_t>(nchunks, 1) * *tail_cap));
  XSG_TRY(s->d_tail_pre.ensure(8 * (nchunks + 1)));
  return XSG_OK;
}

ListArgs xsg::list_args(const xsg_shard* s, const ScanArgs& a) {
  ListArgs l{};
  l.base = s->base;
  l.chunks = a.chunks;
  l.chunk_tile0 = a.chunk_tile0;
  l.nchunks = s->chunks.size();
  l.m_pos = a.m_pos;
  l.m_chunk = a.m_chunk;
  l.m_len = a.m_len;
  l.tile_off = a.tile_off;
  l.chunk_shift0 = s->d_chunk_shift0.as<uint64_t>();
  l.tail_cnt = s->d_tail_cnt.as<uint32_t>();
  l.tail_pos = s->d_tail_pos.as<uint64_t>();
  l.tail_cap = tail_capacity(s->ctx);
  l.tail_pre = s->d_tail_pre.as<uint64_t>();
  return l;
}

// What the kernels behind the final list share (`total`: its length, or its capacity on the one-sync route); the
// pinned mirrors and the per-tag arrays are the caller's.
static LineOutArgs line_out_args(const xsg_shard* s, const ScanArgs& a, const ListArgs& l, uint64_t total) {
  LineOutArgs o{};
  o.base = s->base;
  o.chunks = a.chunks;
  o.chunk_tile0 = a.chunk_tile0;
  o.nchunks = l.nchunks;
  o.pat = s->ctx->pat;
  o.total = total;
  o.f_pos = l.f_pos;
  o.f_match = l.f_match;
  o.f_chunk = l.f_chunk;
  o.f_len = l.f_len;
  o.out_u64 = s->d_out_u64.as<uint64_t>();
  o.shard_line_base = s->shard_line_base;
  o.tile_bytes = s->tile_bytes;
  return o;
}

// ---------------------------------------------------------------------------
// the automaton family's two prefilters
// ---------------------------------------------------------------------------
// The factor prefilter of the automaton route: for an expression without a selective start but with a class sequence
// every match contains, the occurrences of that factor are found by the scan kernel's class-sequence matcher (count +
// emit), the first occurrence of every line gives the line's start (k_line_starts_keep, as for any line tag), and the
// tiles in which such lines start are marked.  k_rx_scan then leaves every other tile at once.  Built once per
// (binding, pattern) by the first synchronous call and used by every later pass, the stream-ordered ones included;
// not built where the factor turns out dense (most tiles would be marked) or the shard is small.
int xsg::ensure_factor_mask(xsg_shard* s) {
  xsg_ctx* c = s->ctx;
  if (c->pat.kind != kDfa || !c->rx_fac || s->ntiles == 0) return XSG_OK;  // (kSet: no factor, no tile marks)
  if (s->mask_serial == c->pattern_serial || s->mask_dense_serial == c->pattern_serial) return XSG_OK;
  if (!c->rx_fac_forced && s->total_bytes < (512ull << 20)) return XSG_OK;
  hipStream_t st = c->stream;
  const uint64_t nchunks = s->chunks.size(), ntiles = s->ntiles;
  XSG_TRY(prepare_tiles(s, false, st));
  ScanArgs a = scan_args(s);
  a.pat = c->fac_pat;
  a.pat.hot = 0;
  a.tile_mask = nullptr;
  s->cnt_clean = false;
  HIP_TRY(launch_scan_count(a, false, false, st));
  XSG_TRY(s->d_tile_off.ensure(8 * (ntiles + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(std::max<uint64_t>(ntiles, nchunks) + 1)));
  HIP_TRY(launch_exclusive_scan_u32(a.tile_cnt, s->d_tile_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
  uint64_t M = 0;
  uint32_t flags = 0;
  HIP_TRY(hipMemcpyAsync(&flags, a.flags, 4, hipMemcpyDeviceToHost, st));
  XSG_TRY(d2h_u64(c, s->d_tile_off.as<uint64_t>() + ntiles, &M));
  if (flags & 1u) {  // non-ASCII data under an ascii_only expression: the search itself will refuse
    HIP_TRY(hipMemsetAsync(a.flags, 0, 4, st));
    return fail(XSG_ENOTSUP, "%s", kNonAsciiMsg);
  }
  if (!c->rx_fac_forced && M * 256 > s->total_bytes) {  // most tiles would be marked
    s->mask_dense_serial = c->pattern_serial;
    return XSG_OK;
  }
  XSG_TRY(s->d_c_pos.ensure(8 * std::max<uint64_t>(M, 1)));
  XSG_TRY(s->d_c_chunk.ensure(4 * std::max<uint64_t>(M, 1)));
  XSG_TRY(s->d_c_keep.ensure(4 * std::max<uint64_t>(M, 1)));
  XSG_TRY(s->d_m_ls.ensure(8 * std::max<uint64_t>(M, 1)));
  XSG_TRY(s->d_tile_mask.ensure(4 * ntiles));
  a.tile_off = s->d_tile_off.as<uint64_t>();
  a.m_pos = s->d_c_pos.as<uint64_t>();  // (the factor's occurrences live in the candidate buffers, not in the result's)
  a.m_chunk = s->d_c_chunk.as<uint32_t>();
  if (M) HIP_TRY(launch_scan_emit(a, st));
  ListArgs l = list_args(s, a);
  l.pat = a.pat;
  l.M = M;
  l.m_ls = s->d_m_ls.as<uint64_t>();
  l.keep = s->d_c_keep.as<uint32_t>();
  l.line_mode = 1;
  HIP_TRY(launch_line_starts_keep(l, st));
  HIP_TRY(hipMemsetAsync(s->d_tile_mask.p, 0, 4 * ntiles, st));
  HIP_TRY(launch_rx_mark_tiles(l, s->d_tile_mask.as<uint32_t>(), st));
  s->mask_serial = c->pattern_serial;
  return XSG_OK;
}

// A literal list is served by the candidate route alone, whose walk keys a candidate by chunk number above 40 bits of offset.
int xsg::set_route_serves(const xsg_shard* s) {
  if (s->ctx->pat.kind == kSet && s->chunks.size() >= (1u << 24))
    return fail(XSG_ENOTSUP, "a literal list is not served on a binding of 2^24 chunks or more");
  return XSG_OK;
}

// The prefilter route is half a dozen kernels and three trips to the host where k_rx_scan is one pass: it pays on
// shards where a pass takes longer than that (the file pipeline's 16 MiB chunks are walked by k_rx_scan in tens of
// microseconds).
bool xsg::use_prefilter(const xsg_shard* s, bool pre_off) {
  const xsg_ctx* c = s->ctx;
  // a literal list has no other route: its candidates (k_set_scan) are always verified and walked here, on shards of
  // any size and whatever their density (the entry points refuse a binding of 2^24 chunks and more: set_route_serves)
  if (c->pat.kind == kSet) return true;
  return c->pat.kind == kDfa && c->rx_pre && !pre_off && (c->rx_pre_forced || s->total_bytes >= (512ull << 20)) &&
         s->chunks.size() < (1u << 24);  // k_rx_heads' keys: chunk number above 40 bits of offset
}

// ---------------------------------------------------------------------------
// The one-sync list route.  A list search on the exact route below fetches three to four sizes from the device (raw
// occurrences, kept + tail matches, line bytes), each a stream sync, and launches 17-25 small kernels -- ~0.45 ms on
// top of a 1.5 ms scan of 10 GiB for a few thousand matches (profiles/r03_list_before_kernel_trace.txt).  Here the
// sizes stay on the device: arrays get capacities (a sparse result fits them by a wide margin), every kernel reads
// the counts it needs from a block of device words (FastTot) and bounds itself, the tile ranks and the keep prefix
// take two launches each (ticketed last workgroup), the emit pass visits only the tiles that hold a match, the
// end-of-chunk walk is one wave per chunk on bit masks, and totals and results are ALSO stored into pinned host
// memory by the kernels that produce them.  The host syncs once and reads them there.  A result that does not fit
// (kTotOverflow) is redone on the exact route, which reuses the tile counts of this pass; the binding remembers it.
// ---------------------------------------------------------------------------
constexpr int kFastOverflow = 2;  // run_list_fast: capacity exceeded, tile counts in place -> the exact route from step 2

static uint64_t fast_capacity(const xsg_shard* s) {
  if (const char* e = XSG_TOGGLE("XSG_LIST_CAP")) {  // tests: tiny capacities force the fallback
    const long long v = atoll(e);
    if (v > 0) return (uint64_t)v;
  }
  // one entry per 256 bytes of text, 16 Ki .. 1 Mi entries (a 16 MiB chunk of the file pipeline: 64 Ki)
  return std::min<uint64_t>(std::max<uint64_t>(s->total_bytes / 256, 1u << 14), 1u << 20);
}

static bool fast_route_serves(const xsg_shard* s, uint32_t mode, bool outputs, bool want_nl_total) {
  const xsg_ctx* c = s->ctx;
  const char* e = XSG_TOGGLE("XSG_LIST_FAST");  // 0: every list search takes the exact route (tests, A/B)
  if ((e && *e == '0') || !outputs || s->ntiles == 0 || want_nl_total) return false;
  if (mode == XSG_MATCHES) return false;                                // the span and gather stages sit on the exact route
  if (c->flags & XSG_FLAG_INVERT) return false;                         // the complement stage sits on the exact route
  if (c->max_count) return false;                                       // the limit stage sits on the exact route
  if (context_on(c) && mode != XSG_MATCH_BYTE_OFFSETS) return false;    // the widening stage sits on the exact route
  if (c->pat.kind == kDfa) return false;                                // k_rx_scan / the prefilter route: exact route
  if (c->pat.kind == kSet) return false;                                // a literal list: the candidate route sits on the exact route
  if (mode != XSG_MATCH_BYTE_OFFSETS && c->pat.has_newline) return false;  // the line walk of a literal with '\n': a chain, exact route
  if (mode == XSG_MATCH_BYTE_OFFSETS && c->bordered && !overlap_free_known(s)) return false;  // greedy keep: exact route
  if (s->chunks.size() > (1u << 20)) return false;                      // the tail prefix is one workgroup's work
  if (s->ntiles >= (1ull << 32)) return false;                          // hit list: uint32 tile numbers
  return s->fast_dense_serial != c->pattern_serial && c->fast_dense_serial != c->pattern_serial;
}

// The pinned mirrors of list results only grow while results grow: one needle in most lines of a large shard leaves
// gigabytes page-locked (offsets, line lengths, line bytes).  A search that needs less than a sixteenth of what is
// retained gives the large buffers back before it runs (PinBuf::trim; they come again on demand; a caller that repeats
// the dense search keeps them: its results keep needing them).  Sizes in bytes.
static void trim_pinned(xsg_shard* s, size_t need_u64, size_t need_len, size_t need_bytes) {
  s->h_result.trim(need_u64);
  s->hp_line_len.trim(need_len);
  s->hp_line_bytes.trim(need_bytes);
}

// The buffers of the one-sync route for `cap` raw occurrences (grow-only; the file pipeline re-binds the same shard for
// every chunk).  *fcap: final entries they hold, *bytes_cap: packed line bytes.
static int ensure_fast_buffers(xsg_shard* s, uint32_t mode, uint64_t cap, uint64_t* fcap_out, uint64_t* bytes_cap_out) {
  hipStream_t st = s->ctx->stream;
  const bool line_mode = mode != XSG_MATCH_BYTE_OFFSETS;
  const uint64_t nchunks = s->chunks.size(), ntiles = s->ntiles;
  uint32_t tail_cap = 0;
  XSG_TRY(ensure_tail_buffers(s, &tail_cap));
  const uint64_t fcap = *fcap_out = cap + nchunks * tail_cap;  // a list whose raw part fits always fits
  const uint64_t bytes_cap = *bytes_cap_out = std::min<uint64_t>(fcap * 128, 32ull << 20);
  bool grew = false;
  XSG_TRY(s->d_tot.ensure(8 * kTotWords + 64, &grew));
  if (grew) HIP_TRY(hipMemsetAsync(s->d_tot.p, 0, 8 * kTotWords + 64, st));  // tickets = 0
  if (!s->h_tot) HIP_TRY(hipHostMalloc((void**)&s->h_tot, 8 * (kTotWords + 1), hipHostMallocDefault));
  XSG_TRY(s->d_tile_off.ensure(8 * (ntiles + 1)));
  XSG_TRY(s->d_scan2.ensure(8 * scan2_tmp_elems(std::max<uint64_t>(ntiles, fcap) + 1)));
  XSG_TRY(s->d_hit.ensure(4 * cap));
  grew = false;
  XSG_TRY(s->d_wmask.ensure(4 * (ntiles / 4 + 1), &grew));
  if (grew) HIP_TRY(hipMemsetAsync(s->d_wmask.p, 0, s->d_wmask.cap, st));
  XSG_TRY(s->d_m_pos.ensure(8 * cap));
  XSG_TRY(s->d_m_chunk.ensure(4 * cap));
  if (line_mode) {
    XSG_TRY(s->d_m_ls.ensure(8 * cap));
    XSG_TRY(s->d_keep.ensure(4 * cap));
    XSG_TRY(s->d_keep_pre.ensure(8 * (cap + 1)));
  }
  XSG_TRY(s->d_out_u64.ensure(8 * fcap));
  if (mode == XSG_LINE_INDICES || mode == XSG_LINES) {
    XSG_TRY(s->d_f_pos.ensure(8 * fcap));
    XSG_TRY(s->d_f_match.ensure(8 * fcap));
    XSG_TRY(s->d_f_chunk.ensure(4 * fcap));
  }
  trim_pinned(s, 8 * (size_t)fcap, 8 * (size_t)fcap, (size_t)bytes_cap);  // what an earlier dense result left page-locked
  XSG_TRY(s->h_result.ensure(8 * (size_t)fcap));
  if (mode == XSG_LINES) {
    XSG_TRY(s->d_line_len.ensure(8 * fcap));
    XSG_TRY(s->d_line_off.ensure(8 * (fcap + 1)));
    XSG_TRY(s->d_line_bytes.ensure(bytes_cap));
    XSG_TRY(s->hp_line_len.ensure(8 * (size_t)fcap));
    XSG_TRY(s->hp_line_bytes.ensure((size_t)bytes_cap));
  }
  if (mode == XSG_LINE_INDICES) {
    XSG_TRY(ensure_tile_nl(s));
    grew = false;
    XSG_TRY(s->d_tile_nl_off.ensure(8 * (ntiles + 1), &grew));
    if (grew) s->nl_off_cached = false;
  }
  return XSG_OK;
}

static int run_list_fast(xsg_shard* s, uint32_t mode) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const bool line_mode = mode != XSG_MATCH_BYTE_OFFSETS;
  const bool want_f = mode == XSG_LINE_INDICES || mode == XSG_LINES;
  const bool want_nl = mode == XSG_LINE_INDICES;
  const uint64_t ntiles = s->ntiles;
  const uint64_t cap = fast_capacity(s);
  uint64_t fcap = 0, bytes_cap = 0;
  XSG_TRY(ensure_fast_buffers(s, mode, cap, &fcap, &bytes_cap));
  uint64_t* tot = s->d_tot.as<uint64_t>();
  uint32_t* tickets = reinterpret_cast<uint32_t*>(tot + kTotWords);
  memset(s->h_tot, 0, 8 * (kTotWords + 1));  // nothing of this shard is in flight: every search ends in a sync

  // ---- 1. bulk count per tile (+ newlines per tile, once per binding)
  const bool scan_nl = want_nl && !s->nl_cached;
  XSG_TRY(choose_hot_filter(s, st, scan_nl, false));
  XSG_TRY(sketch_before_pass(s, st, !scan_nl, true, true));
  XSG_TRY(prepare_tiles(s, false, st));
  ScanArgs a = scan_args(s, scan_variant(scan_nl, false));
  a.tile_wmask = s->d_wmask.as<uint32_t>();  // the count pass marks the waves that found something, the emit pass reads only those
  s->cnt_clean = false;  // the tile counts stay in place for the emit pass: the next pass re-zeroes them
  HIP_TRY(launch_scan_count(a, scan_nl, false, st));
  if (scan_nl) s->nl_cached = true;

  // ---- 2. ranks of the tiles + the ordered list of the tiles that hold a match (two launches)
  Scan2Args r{};
  r.in = a.tile_cnt;
  r.out = s->d_tile_off.as<uint64_t>();
  r.n_cap = ntiles;
  r.blk = s->d_scan2.as<uint64_t>();
  r.ticket = tickets;
  r.tot_dev = tot + kTotRaw;
  r.tot_host = s->h_tot + kTotRaw;
  r.hit_idx = s->d_hit.as<uint32_t>();
  r.hit_cap = cap;
  r.hits_dev = tot + kTotHits;
  r.hits_host = s->h_tot + kTotHits;
  r.ovf_dev = tot + kTotOverflow;
  r.ovf_host = s->h_tot + kTotOverflow;
  r.total_cap = cap;
  r.ovf_bit = 1;
  r.ovf_init = 1;
  HIP_TRY(launch_scan2_u32(r, true, st));
  if (want_nl && !s->nl_off_cached) {
    Scan2Args n{};
    n.in = a.tile_nl;
    n.out = s->d_tile_nl_off.as<uint64_t>();
    n.n_cap = ntiles;
    n.blk = r.blk;
    n.ticket = tickets;
    n.tot_dev = tot + kTotNewlines;
    n.tot_host = s->h_tot + kTotNewlines;
    HIP_TRY(launch_scan2_u32(n, false, st));
  }

  // ---- 3. ordered emission, only from the tiles on the list
  a.tile_off = r.out;
  a.m_pos = s->d_m_pos.as<uint64_t>();
  a.m_chunk = s->d_m_chunk.as<uint32_t>();
  a.m_cap = cap;
  a.hit_tiles = r.hit_idx;
  a.n_hits_dev = tot + kTotHits;
  a.hit_cap = cap;
  HIP_TRY(launch_scan_emit(a, st));

  // ---- 4. which occurrences the walk reports; 5. the end of every chunk; 6. the list
  ListArgs l = list_args(s, a);
  l.pat = a.pat;
  l.M = cap;
  l.M_dev = tot + kTotRaw;
  l.m_ls = s->d_m_ls.as<uint64_t>();
  l.keep = s->d_keep.as<uint32_t>();
  l.keep_pre = s->d_keep_pre.as<uint64_t>();
  l.line_mode = line_mode ? 1u : 0u;
  l.keep_all = line_mode ? 0u : 1u;
  l.tot_dev = tot;
  l.tot_host = s->h_tot;
  l.ticket = tickets;
  l.f_cap = fcap;
  l.f_pos = s->d_f_pos.as<uint64_t>();
  l.f_match = s->d_f_match.as<uint64_t>();
  l.f_chunk = s->d_f_chunk.as<uint32_t>();
  l.want_f = want_f ? 1u : 0u;
  // the global offsets of the final entries leave with k_list_out for every tag but xs::line_indices (whose values
  // are indices); xs::lines also gets its line lengths there
  l.out_u64 = mode == XSG_LINE_INDICES ? nullptr : s->d_out_u64.as<uint64_t>();
  l.out_host = mode == XSG_LINE_INDICES ? nullptr : s->h_result.as<uint64_t>();
  if (mode == XSG_LINES) {
    l.line_len = s->d_line_len.as<uint64_t>();
    l.line_len_host = s->hp_line_len.as<uint64_t>();
  }
  if (line_mode) {
    HIP_TRY(launch_line_starts_keep(l, st));
    Scan2Args k{};
    k.in = l.keep;
    k.out = s->d_keep_pre.as<uint64_t>();
    k.n_cap = cap;
    k.n_dev = tot + kTotRaw;
    k.blk = r.blk;
    k.ticket = tickets;
    HIP_TRY(launch_scan2_u32(k, false, st));
  }
  HIP_TRY(launch_chunk_tail(l, st));
  HIP_TRY(launch_list_out(l, st));

  if (want_f) {
    LineOutArgs o = line_out_args(s, a, l, fcap);
    o.tot_dev = tot;
    o.out_host = s->h_result.as<uint64_t>();
    if (mode == XSG_LINE_INDICES) {
      o.tile_nl_off = s->d_tile_nl_off.as<uint64_t>();
      HIP_TRY(launch_line_index_waves(o, st));
    } else {
      o.line_len = s->d_line_len.as<uint64_t>();
      o.line_len_host = s->hp_line_len.as<uint64_t>();
      o.line_out_off = s->d_line_off.as<uint64_t>();
      o.line_bytes = s->d_line_bytes.as<uint8_t>();
      o.line_bytes_host = s->hp_line_bytes.as<uint8_t>();
      o.line_bytes_cap = bytes_cap;
      Scan2Args b{};  // (the lengths came with k_list_out)
      b.in = o.line_len;
      b.out = s->d_line_off.as<uint64_t>();
      b.n_cap = fcap;
      b.n_dev = tot + kTotFinal;
      b.blk = r.blk;
      b.ticket = tickets;
      b.tot_dev = tot + kTotLineBytes;
      b.tot_host = s->h_tot + kTotLineBytes;
      b.ovf_dev = tot + kTotOverflow;
      b.ovf_host = s->h_tot + kTotOverflow;
      b.total_cap = bytes_cap;
      b.ovf_bit = 4;
      HIP_TRY(launch_scan2_u64(b, st));
      HIP_TRY(launch_line_gather(o, st));
    }
  }
  const bool ascii_only = c->pat.kind == kClass && c->pat.ascii_only;
  if (ascii_only) HIP_TRY(hipMemcpyAsync(s->h_tot + kTotWords, a.flags, 4, hipMemcpyDeviceToHost, st));

  // ---- the one sync
  HIP_TRY(hipStreamSynchronize(st));
  s->table_pending = false;
  if (ascii_only && (s->h_tot[kTotWords] & 1u)) {  // non-ASCII data under an ascii_only expression
    HIP_TRY(hipMemsetAsync(a.flags, 0, 4, st));
    return fail(XSG_ENOTSUP, "%s", kNonAsciiMsg);
  }
  s->last_raw_matches = s->h_tot[kTotRaw];
  if (want_nl && !s->nl_off_cached) {
    s->nl_total = s->h_tot[kTotNewlines];
    s->nl_off_cached = true;
  }
  if (s->h_tot[kTotOverflow]) {
    s->fast_dense_serial = c->pattern_serial;  // later searches of this pattern on this binding: the exact route at once
    c->fast_dense_serial = c->pattern_serial;  // ... and on later bindings of this context (the next chunks of a file)
    return kFastOverflow;
  }
  const uint64_t total = s->h_tot[kTotFinal];
  s->total = total;
  s->fast_result = true;
  // xsg_result_chunk_ptr: k_list_out wrote the chunk column for two of the tags; the other two keep what it placed them by
  s->rows_chunk = want_f ? l.f_chunk : nullptr;
  s->rows_entries = want_f ? total : s->h_tot[kTotRaw];
  s->rows_keep_all = !line_mode;
  if (want_nl) s->last_newlines = s->nl_total;
  if (mode == XSG_LINES) {
    // lines without a terminating '\n' are not reported (search_wrappers.h:199-202)
    const uint64_t* len = s->hp_line_len.as<uint64_t>();
    uint64_t n = 0;
    for (uint64_t i = 0; i < total; ++i) n += len[i] != UINT64_MAX;
    s->fast_raw_lines = total;
    s->total = n;
    s->line_bytes = s->h_tot[kTotLineBytes];
  }
  s->last_mode = (int)mode;
  return XSG_OK;
}

// ---------------------------------------------------------------------------
// The exact list route: every array is sized from a count fetched from the device.  Its stages, in run_list's order.
// ---------------------------------------------------------------------------
constexpr int kRedoUnfiltered = 3;  // prefilter_candidates: the prefilter does not pay here, walk the text (use_prefilter: pre_off)

// 3 on the prefilter route.  *M candidates of the class-sequence scan in, *M matches out, listed in a.m_pos / a.m_chunk
// as the emit pass of k_rx_scan would have written them.
static int prefilter_candidates(xsg_shard* s, bool outputs, bool want_len, ScanArgs& a, uint64_t* M) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t nchunks = s->chunks.size(), ntiles = s->ntiles;
  const uint64_t Mc = *M;
  // Candidates every few hundred bytes (a start that is a word of the text): a count is cheaper by walking all
  // lines once (k_rx_scan + finish, no list at all) than by listing, verifying and packing tens of millions of
  // entries -- measured on the bench corpus, where `Sher` is a lexicon word: count_lines of `lock(ed|s)?` 18 ms
  // by candidates against 10 ms by k_rx_scan (8 GiB).  The caller takes the other route.
  // (a literal list has no other route and no bail-out: dense candidates are slow but exact)
  if (c->pat.kind != kSet && !c->pat.rx_multiline && Mc * 128 > s->total_bytes) {
    s->cnt_clean = false;
    s->pre_dense_serial = c->pattern_serial;  // later counts of this pattern on this binding go straight to k_rx_scan
    // a list: the same verdict (tens of millions of anchored scans, each up to 4 KiB, and chains between them, against
    // one walk of the text) -- redone on the line-walking route
    return outputs ? kRedoUnfiltered : kDenseCandidates;
  }
  // Mc candidates so far: emit them, run the anchored automaton at each, walk every chunk's occurrences as the
  // reference does, pack what it reports -- then *M is the number of matches
  XSG_TRY(s->d_c_pos.ensure(8 * std::max<uint64_t>(Mc, 1)));
  XSG_TRY(s->d_c_chunk.ensure(4 * std::max<uint64_t>(Mc, 1)));
  XSG_TRY(s->d_c_len.ensure(4 * std::max<uint64_t>(Mc, 1)));
  XSG_TRY(s->d_c_keep.ensure(4 * std::max<uint64_t>(Mc, 1)));
  XSG_TRY(s->d_c_pre.ensure(8 * (Mc + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(std::max<uint64_t>(Mc, std::max<uint64_t>(ntiles, nchunks)) + 1)));
  a.m_pos = s->d_c_pos.as<uint64_t>();
  a.m_chunk = s->d_c_chunk.as<uint32_t>();
  if (Mc) HIP_TRY(launch_scan_emit(a, st));
  if (all_of_list(c)) {
    // XSG_LIST_ALL_OF: every literal at every candidate (k_set_verify_all: a mask per candidate), and EVERY position with
    // an occurrence becomes an entry -- no leftmost-first walk, a covered occurrence still serves its literal -- packed
    // with its mask.  One size from the device, as on the plain list's pass.
    XSG_TRY(s->d_c_mask.ensure(8 * std::max<uint64_t>(Mc, 1)));
    SetAllArgs v{};
    v.base = s->base;
    v.chunks = a.chunks;
    v.pat = c->pat;
    v.idx_off = c->set_idx_off;
    v.n = Mc;
    v.c_pos = a.m_pos;
    v.c_chunk = a.m_chunk;
    v.c_mask = s->d_c_mask.as<uint64_t>();
    v.c_keep = s->d_c_keep.as<uint32_t>();
    v.c_pre = s->d_c_pre.as<uint64_t>();
    HIP_TRY(launch_set_verify_all(v, st));
    HIP_TRY(launch_exclusive_scan_u32(v.c_keep, s->d_c_pre.as<uint64_t>(), Mc, s->d_scan_tmp.as<uint64_t>(), st));
    XSG_TRY(d2h_u64(c, s->d_c_pre.as<uint64_t>() + Mc, M));
    XSG_TRY(s->d_m_pos.ensure(8 * std::max<uint64_t>(*M, 1)));
    XSG_TRY(s->d_m_chunk.ensure(4 * std::max<uint64_t>(*M, 1)));
    XSG_TRY(s->d_m_mask.ensure(8 * std::max<uint64_t>(*M, 1)));
    v.m_pos = s->d_m_pos.as<uint64_t>();
    v.m_chunk = s->d_m_chunk.as<uint32_t>();
    v.m_mask = s->d_m_mask.as<uint64_t>();
    HIP_TRY(launch_set_compact_all(v, st));
    a.m_pos = v.m_pos;
    a.m_chunk = v.m_chunk;
    a.m_len = nullptr;
    return XSG_OK;
  }
  RxPreArgs r{};
  r.base = s->base;
  r.chunks = a.chunks;
  r.chunk_tile0 = a.chunk_tile0;
  r.nchunks = nchunks;
  r.pat = c->pat;
  r.n = Mc;
  r.tile_off = a.tile_off;
  r.c_pos = a.m_pos;
  r.c_chunk = a.m_chunk;
  r.c_len = s->d_c_len.as<uint32_t>();
  r.c_keep = s->d_c_keep.as<uint32_t>();
  r.c_pre = s->d_c_pre.as<uint64_t>();
  r.scan_tmp = s->d_scan_tmp.as<uint64_t>();
  r.flags = a.flags;
  HIP_TRY(launch_rx_verify_keep(r, st));
  HIP_TRY(launch_exclusive_scan_u32(r.c_keep, s->d_c_pre.as<uint64_t>(), Mc, s->d_scan_tmp.as<uint64_t>(), st));
  uint32_t vflags = 0;
  // (k_set_verify has no budget to outrun and raises nothing: a list's pass does not read the word at all)
  if (c->pat.kind != kSet) HIP_TRY(hipMemcpyAsync(&vflags, a.flags, 4, hipMemcpyDeviceToHost, st));
  XSG_TRY(d2h_u64(c, s->d_c_pre.as<uint64_t>() + Mc, M));
  if (vflags & 2u) {  // a candidate outran the verification budget: walk the text once instead (the other route)
    HIP_TRY(hipMemsetAsync(a.flags, 0, 4, st));
    s->cnt_clean = false;
    return kRedoUnfiltered;
  }
  XSG_TRY(s->d_m_pos.ensure(8 * std::max<uint64_t>(*M, 1)));
  XSG_TRY(s->d_m_chunk.ensure(4 * std::max<uint64_t>(*M, 1)));
  r.m_pos = s->d_m_pos.as<uint64_t>();
  r.m_chunk = s->d_m_chunk.as<uint32_t>();
  if (want_len) {  // XSG_MATCHES: the lengths k_rx_verify measured travel with the reported candidates
    XSG_TRY(s->d_m_len.ensure(4 * std::max<uint64_t>(*M, 1)));
    r.m_len = s->d_m_len.as<uint32_t>();
  }
  HIP_TRY(launch_rx_compact(r, st));
  a.m_pos = r.m_pos;
  a.m_chunk = r.m_chunk;
  a.m_len = r.m_len;
  return XSG_OK;
}

// closure of the marked entries under the links J (J2: scratch): pointer jumping, log2(longest chain) rounds of
// "mark J(marked), square J" until a round marks nothing new (xsg_list_kernels.hip: k_greedy_jump)
static int close_chains(const ListArgs& l, uint32_t* J, uint32_t* J2, uint32_t* changed_dev, hipStream_t st) {
  for (int round = 0; round < 40; ++round) {  // 2^40 entries would not fit the index type anyway
    uint32_t changed = 0;
    HIP_TRY(hipMemsetAsync(changed_dev, 0, 4, st));
    HIP_TRY(launch_greedy_jump(l, J, J2, changed_dev, st));
    HIP_TRY(hipMemcpyAsync(&changed, changed_dev, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!changed) break;
    std::swap(J, J2);
  }
  return XSG_OK;
}

// 4. which of the l.M occurrences the reference walk reports: l.keep and its prefix l.keep_pre
static int decide_keep(xsg_shard* s, ListArgs& l, bool chain_lines) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t M = l.M;
  // words behind the finish kernel's ticket and the scan flags: [0] "a chain outran its walker", [1] "a round marked something"
  uint32_t* words = reinterpret_cast<uint32_t*>(s->d_finish.as<uint64_t>() + 3 * (size_t)kFinishBlocks) + 2;
  if (chain_lines) {
    // a literal that contains '\n': line starts, chunk heads and the walk's links, then the closure (see k_nlpat_links)
    if (M >= 0xffffffffull) return fail(XSG_ENOTSUP, "more than 2^32 occurrences of a pattern that contains '\\n': its line walk is not served");
    if (M) {
      XSG_TRY(s->d_c_pos.ensure(4 * M));  // the link arrays borrow the prefilter route's candidate buffers (unused by literals)
      XSG_TRY(s->d_c_pre.ensure(4 * M));
      HIP_TRY(launch_nlpat_links(l, s->d_c_pos.as<uint32_t>(), st));
      XSG_TRY(close_chains(l, s->d_c_pos.as<uint32_t>(), s->d_c_pre.as<uint32_t>(), words + 1, st));
    }
  } else if (l.line_mode) {
    HIP_TRY(launch_line_starts_keep(l, st));
    if (all_of_list(c) && M) {
      // XSG_LIST_ALL_OF: keep marks the first entry of every line; its prefix numbers the lines, one OR per line of the
      // entries' masks (k_all_of_or), and keep stays only where the line's mask is full.  The prefix below is taken again.
      HIP_TRY(launch_exclusive_scan_u32(l.keep, s->d_keep_pre.as<uint64_t>(), M, s->d_scan_tmp.as<uint64_t>(), st));
      XSG_TRY(s->d_line_mask.ensure(8 * M));
      HIP_TRY(hipMemsetAsync(s->d_line_mask.p, 0, 8 * M, st));
      AllOfArgs o{};
      o.M = M;
      o.keep = l.keep;
      o.keep_pre = s->d_keep_pre.as<uint64_t>();
      o.m_mask = s->d_m_mask.as<uint64_t>();
      o.line_mask = s->d_line_mask.as<unsigned long long>();
      o.full = c->set_count >= 64u ? ~0ull : (1ull << c->set_count) - 1ull;  // (never 1 << 64)
      HIP_TRY(launch_all_of_or(o, st));
      HIP_TRY(launch_all_of_keep(o, st));
    }
  } else if (c->bordered && !overlap_free_known(s)) {
    // chain heads walk their chains (a few entries at text densities); a chain over the budget -- a long run of one
    // byte searched for `aa` is ONE chain per chunk -- raises a flag and is finished by pointer jumping, log2(length)
    // parallel rounds (xsg_list_kernels.hip: k_greedy_links / k_greedy_jump)
    const bool can_jump = M < 0xffffffffull;
    if (M) HIP_TRY(hipMemsetAsync(l.keep, 0, 4 * M, st));
    HIP_TRY(hipMemsetAsync(words, 0, 8, st));
    l.long_flag = can_jump ? words : nullptr;
    HIP_TRY(launch_greedy_keep(l, st));
    uint32_t is_long = 0;
    if (can_jump) {
      HIP_TRY(hipMemcpyAsync(&is_long, words, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    if (is_long) {
      XSG_TRY(s->d_c_pos.ensure(4 * M));  // the link arrays borrow the prefilter route's candidate buffers (unused by literals)
      XSG_TRY(s->d_c_pre.ensure(4 * M));
      HIP_TRY(launch_greedy_links(l, s->d_c_pos.as<uint32_t>(), st));
      XSG_TRY(close_chains(l, s->d_c_pos.as<uint32_t>(), s->d_c_pre.as<uint32_t>(), words + 1, st));
    }
  } else {
    HIP_TRY(launch_keep_all(l, st));
  }
  HIP_TRY(launch_exclusive_scan_u32(l.keep, s->d_keep_pre.as<uint64_t>(), M, s->d_scan_tmp.as<uint64_t>(), st));
  return XSG_OK;
}

// 5. the tail zone of every chunk, replayed as the reference walks it; *total = kept + tail matches
static int tails_and_total(xsg_shard* s, const ScanArgs& a, const ListArgs& l, bool want_nl_total, uint64_t* total) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t ntiles = s->ntiles;
  // (k_chunk_shift0 looks backwards from a chunk's last entry for a kept one, one lane per chunk: under XSG_LIST_ALL_OF
  // kept entries can be arbitrarily rare and the loop would run over the chunk's whole column.  A list has no tail zone
  // -- exact_tail: k_tail_list reads no chunk_shift0 and writes 0 -- so the kernel is not launched for such a list.)
  if (!all_of_list(c)) HIP_TRY(launch_chunk_shift0(l, st));
  HIP_TRY(launch_tail_list(l, st));
  HIP_TRY(launch_exclusive_scan_u32(l.tail_cnt, s->d_tail_pre.as<uint64_t>(), l.nchunks, s->d_scan_tmp.as<uint64_t>(), st));
  uint64_t kept = 0, tails = 0;
  HIP_TRY(hipMemcpyAsync(&kept, s->d_keep_pre.as<uint64_t>() + l.M, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tails, s->d_tail_pre.as<uint64_t>() + l.nchunks, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *total = kept + tails;
  s->total = *total;
  if (want_nl_total) {  // xsg_count(... | XSG_WITH_NEWLINES) on the prefilter route: the sum of the per-tile counts
    bool grew = false;
    XSG_TRY(s->d_tile_nl_off.ensure(8 * (ntiles + 1), &grew));
    if (grew) s->nl_off_cached = false;
    XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(ntiles + 1)));
    if (!s->nl_off_cached) {
      HIP_TRY(launch_exclusive_scan_u32(a.tile_nl, s->d_tile_nl_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
      s->nl_off_cached = true;
    }
    XSG_TRY(d2h_u64(c, s->d_tile_nl_off.as<uint64_t>() + ntiles, &s->last_newlines));
    s->nl_total = s->last_newlines;
  }
  return XSG_OK;
}

// 6, XSG_LINE_INDICES: per-entry newline differences -> prefix sums -> indices (k_line_nl_delta / k_line_indices)
static int out_line_indices(xsg_shard* s, const ScanArgs& a, LineOutArgs& o) {
  hipStream_t st = s->ctx->stream;
  const uint64_t ntiles = s->ntiles, total = o.total;
  bool grew = false;
  XSG_TRY(s->d_tile_nl_off.ensure(8 * (ntiles + 1), &grew));
  if (grew) s->nl_off_cached = false;
  XSG_TRY(s->d_line_len.ensure(8 * std::max<uint64_t>(total, 1)));
  XSG_TRY(s->d_line_off.ensure(8 * (total + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(std::max<uint64_t>(total + 1, ntiles + 1))));
  if (!s->nl_off_cached) {
    HIP_TRY(launch_exclusive_scan_u32(a.tile_nl, s->d_tile_nl_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
    s->nl_off_cached = true;
  }
  o.tile_nl_off = s->d_tile_nl_off.as<uint64_t>();
  o.line_len = s->d_line_len.as<uint64_t>();
  o.line_out_off = s->d_line_off.as<uint64_t>();
  HIP_TRY(launch_line_nl_delta(o, st));
  HIP_TRY(launch_exclusive_scan_u64(o.line_len, s->d_line_off.as<uint64_t>(), total, s->d_scan_tmp.as<uint64_t>(), st));
  HIP_TRY(launch_line_indices(o, st));
  HIP_TRY(hipMemcpyAsync(&s->last_newlines, s->d_tile_nl_off.as<uint64_t>() + ntiles, 8, hipMemcpyDeviceToHost, st));
  return XSG_OK;
}

// 6, XSG_LINES: lengths, global offsets and the packed bytes of every entry's line.
// XSG_MATCHES (`matches`): the same of every entry's match -- k_match_spans instead of k_line_lengths (no newline query,
// nothing to drop) and the short-string gather; the buffers, the pinned mirrors and the one fetched size are shared.
static int out_lines(xsg_shard* s, LineOutArgs& o, bool matches) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t total = o.total;
  XSG_TRY(s->d_line_len.ensure(8 * std::max<uint64_t>(total, 1)));
  XSG_TRY(s->d_line_off.ensure(8 * (total + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(total + 1)));
  o.line_len = s->d_line_len.as<uint64_t>();
  if (!matches) {
    XSG_TRY(s->d_dropped.ensure(16));
    o.dropped = s->d_dropped.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(o.dropped, 0, 4, st));
  }
  // The result leaves for the shard's pinned mirrors AS IT IS PRODUCED (what xsg_result_lines_view hands out;
  // xsg_result_lines copies from there): k_line_lengths stores lengths and global offsets there as well as on the device,
  // and the gather writes the packed bytes straight into pinned memory -- the kernels are the copies.  A needle in most
  // lines of 10 GiB returns 3 GB over a link that moves 57 GB/s: round 3 moved them in three copies one after the other
  // behind the whole gather (94 ms a search); copies on side streams behind each slice of the gather came to 85 ms, because
  // a kernel that runs beside a device-to-host copy crawls (the copy is a blit kernel whose waves wait for the link and
  // hold the compute units: each 250 MB slice of the gather took 7 ms beside one, the first one 19 ms:
  // profiles/r04_dense_timeline.txt).  Now the link is busy from the moment the list is assembled until the last byte.
  bool eager = 16 * total < (16ull << 30);  // (beyond 16 GiB of pinned memory: the accessors copy on demand)
  if (const char* e = XSG_TOGGLE("XSG_LINES_EAGER")) eager = *e != '0';  // tests: the on-demand path on small results
  if (eager) {
    trim_pinned(s, 8 * (size_t)total, 8 * (size_t)total, SIZE_MAX);  // (what a far larger earlier result left page-locked)
    XSG_TRY(s->hp_line_len.ensure(8 * (size_t)total));
    XSG_TRY(s->h_result.ensure(8 * (size_t)total));
    o.line_len_host = s->hp_line_len.as<uint64_t>();
    o.out_host = s->h_result.as<uint64_t>();
  }
  HIP_TRY(matches ? launch_match_spans(o, st) : launch_line_lengths(o, st));
  HIP_TRY(launch_exclusive_scan_u64(o.line_len, s->d_line_off.as<uint64_t>(), total, s->d_scan_tmp.as<uint64_t>(), st));
  uint64_t nbytes = 0;
  if (matches)
    s->h_dropped = 0;
  else
    HIP_TRY(hipMemcpyAsync(&s->h_dropped, o.dropped, 4, hipMemcpyDeviceToHost, st));  // (rides on the sync below)
  XSG_TRY(d2h_u64(c, s->d_line_off.as<uint64_t>() + total, &nbytes));
  o.line_out_off = s->d_line_off.as<uint64_t>();
  if (!eager) {
    XSG_TRY(s->d_line_bytes.ensure(std::max<uint64_t>(nbytes, 1)));
    o.line_bytes = s->d_line_bytes.as<uint8_t>();
    HIP_TRY(launch_line_gather(o, st, matches));
    // the lengths stay on the device until a result accessor asks (fetch_line_lengths): how many lines lack their
    // newline -- all the search itself needs to know -- was counted by the kernel
    s->line_len_on_device = true;
  } else {
    trim_pinned(s, SIZE_MAX, SIZE_MAX, (size_t)nbytes + 16);
    XSG_TRY(s->hp_line_bytes.ensure((size_t)nbytes + 16));  // (+16: k_line_gather_edges writes whole units)
    const uint64_t nbnd = total / kBlock + 2;
    XSG_TRY(s->d_scan_tmp.ensure(16 * nbnd));  // (the scan is done with it)
    HIP_TRY(hipMemsetAsync(s->d_scan_tmp.p, 0, 16 * nbnd, st));
    o.edge_units = s->d_scan_tmp.as<uint32_t>();
    o.line_bytes = nullptr;  // no device copy of the packed bytes: nothing reads one when the mirrors hold the result
    o.line_bytes_host = s->hp_line_bytes.as<uint8_t>();
    HIP_TRY(launch_line_gather(o, st, matches));
    s->fast_result = true;  // the result lives in the pinned mirrors: the accessors read it there
  }
  s->line_bytes = nbytes;
  s->fast_raw_lines = total;
  return XSG_OK;
}

// XSG_FLAG_INVERT: the assembled list (the starts of the lines the walk reports) is replaced by its complement among
// the line starts of the chunks, l.f_* and *total with it; every output kernel then runs on the new list unchanged.
// Count per tile, ranks, one more size from the device, emit (xsg_list_kernels.hip: k_invert_tile).
static int invert_list(xsg_shard* s, const ScanArgs& a, ListArgs& l, uint64_t* total) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t ntiles = s->ntiles;
  XSG_TRY(s->d_inv_lo.ensure(8 * (ntiles + 1)));
  XSG_TRY(s->d_inv_cnt.ensure(4 * std::max<uint64_t>(ntiles, 1)));
  XSG_TRY(s->d_inv_off.ensure(8 * (ntiles + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(ntiles + 1)));
  InvertArgs v{};
  v.base = s->base;
  v.chunks = a.chunks;
  v.tile_chunk = a.tile_chunk;
  v.chunk_tile0 = a.chunk_tile0;
  v.ntiles = ntiles;
  v.tile_bytes = s->tile_bytes;
  v.total = *total;
  v.r_pos = l.f_pos;
  v.r_chunk = l.f_chunk;
  v.tile_lo = s->d_inv_lo.as<uint64_t>();
  v.tile_cnt = s->d_inv_cnt.as<uint32_t>();
  HIP_TRY(launch_invert_count(v, st));
  HIP_TRY(launch_exclusive_scan_u32(v.tile_cnt, s->d_inv_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
  uint64_t n = 0;
  XSG_TRY(d2h_u64(c, s->d_inv_off.as<uint64_t>() + ntiles, &n));
  XSG_TRY(s->d_inv_pos.ensure(8 * std::max<uint64_t>(n, 1)));
  XSG_TRY(s->d_inv_chunk.ensure(4 * std::max<uint64_t>(n, 1)));
  XSG_TRY(s->d_out_u64.ensure(8 * std::max<uint64_t>(n, 1)));
  v.tile_off = s->d_inv_off.as<uint64_t>();
  v.inv_total = n;
  v.i_pos = s->d_inv_pos.as<uint64_t>();
  v.i_chunk = s->d_inv_chunk.as<uint32_t>();
  HIP_TRY(launch_invert_emit(v, st));
  l.f_pos = v.i_pos;
  l.f_match = v.i_pos;  // (no match in such a line: LineOutArgs::invert keeps the output kernels away from it)
  l.f_chunk = v.i_chunk;
  l.total = n;
  *total = s->total = n;
  return XSG_OK;
}

// xsg_set_max_count: the assembled (or inverted) list is replaced by the first N entries of every chunk, l.f_* and *total
// with it; the widening stage and every output kernel run on the new list unchanged.  Rows per chunk, one prefix sum, one
// more size from the device, the copy (xsg_list_kernels.hip: k_limit_rows, k_limit_copy).  A list of N entries and fewer
// cannot lose one: the stage is not run at all.
static int limit_list(xsg_shard* s, ListArgs& l, uint64_t* total) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t n_in = *total, nchunks = s->chunks.size();
  if (n_in <= c->max_count) return XSG_OK;
  XSG_TRY(s->d_lim_cnt.ensure(8 * std::max<uint64_t>(nchunks, 1)));
  XSG_TRY(s->d_lim_old.ensure(8 * std::max<uint64_t>(nchunks, 1)));
  XSG_TRY(s->d_lim_ptr.ensure(8 * (nchunks + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(nchunks + 1)));
  LimitArgs a{};
  a.nchunks = nchunks;
  a.total = n_in;
  a.limit = c->max_count;
  a.f_pos = l.f_pos;
  a.f_match = l.f_match;
  a.f_chunk = l.f_chunk;
  a.f_len = l.f_len;
  a.cnt = s->d_lim_cnt.as<uint64_t>();
  a.old_ptr = s->d_lim_old.as<uint64_t>();
  HIP_TRY(launch_limit_rows(a, st));
  HIP_TRY(launch_exclusive_scan_u64(a.cnt, s->d_lim_ptr.as<uint64_t>(), nchunks, s->d_scan_tmp.as<uint64_t>(), st));
  uint64_t n = 0;
  XSG_TRY(d2h_u64(c, s->d_lim_ptr.as<uint64_t>() + nchunks, &n));
  if (n > n_in) return fail(XSG_EHIP, "the limit stage counted %llu entries of %llu", (unsigned long long)n, (unsigned long long)n_in);
  const bool own_match = l.f_match != l.f_pos;
  XSG_TRY(s->d_lim_pos.ensure(8 * std::max<uint64_t>(n, 1)));
  if (own_match) XSG_TRY(s->d_lim_match.ensure(8 * std::max<uint64_t>(n, 1)));
  XSG_TRY(s->d_lim_chunk.ensure(4 * std::max<uint64_t>(n, 1)));
  if (l.f_len) XSG_TRY(s->d_lim_len.ensure(4 * std::max<uint64_t>(n, 1)));
  a.new_ptr = s->d_lim_ptr.as<uint64_t>();
  a.o_pos = s->d_lim_pos.as<uint64_t>();
  a.o_match = own_match ? s->d_lim_match.as<uint64_t>() : a.o_pos;
  a.o_chunk = s->d_lim_chunk.as<uint32_t>();
  a.o_len = l.f_len ? s->d_lim_len.as<uint32_t>() : nullptr;
  HIP_TRY(launch_limit_copy(a, st));
  l.f_pos = a.o_pos;
  l.f_match = a.o_match;
  l.f_chunk = a.o_chunk;
  if (l.f_len) l.f_len = a.o_len;
  l.total = n;
  *total = s->total = n;
  return XSG_OK;
}

// the exclusive prefix of the per-tile newline counts (a.tile_nl: the caller's count pass ran with them), once per binding
static int ensure_tile_nl_off(xsg_shard* s, const ScanArgs& a) {
  hipStream_t st = s->ctx->stream;
  const uint64_t ntiles = s->ntiles;
  bool grew = false;
  XSG_TRY(s->d_tile_nl_off.ensure(8 * (ntiles + 1), &grew));
  if (grew) s->nl_off_cached = false;
  if (s->nl_off_cached) return XSG_OK;
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(ntiles + 1)));
  HIP_TRY(launch_exclusive_scan_u32(a.tile_nl, s->d_tile_nl_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
  s->nl_off_cached = true;
  return XSG_OK;
}

// XSG_FLAG_CONTEXT: the assembled (or inverted) list is replaced by the starts of every line within `before` lines ahead
// of or `after` lines behind one of its lines, in the same chunk, each once; l.f_* and *total with it, and the output
// kernels run on the new list unchanged.  Ranks of the entries (the passes of XSG_LINE_INDICES: near entries count their
// gap, far ones their tile), spans and edges, one prefix sum, one more size from the device, then the select pass over
// the tiles (xsg_list_kernels.hip: k_context_spans, k_context_tile).  The edges of the chunks stay on the shard for
// xsg_result_context_edges.
static int context_list(xsg_shard* s, const ScanArgs& a, ListArgs& l, uint64_t* total) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  const uint64_t n_in = *total, nchunks = s->chunks.size();
  XSG_TRY(ensure_tile_nl_off(s, a));
  XSG_TRY(s->d_line_len.ensure(8 * std::max<uint64_t>(n_in, 1)));
  XSG_TRY(s->d_line_off.ensure(8 * (n_in + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(n_in + 1)));
  XSG_TRY(s->d_cx_lo.ensure(8 * std::max<uint64_t>(n_in, 1)));
  XSG_TRY(s->d_cx_hi.ensure(8 * std::max<uint64_t>(n_in, 1)));
  XSG_TRY(s->d_cx_cnt.ensure(4 * std::max<uint64_t>(n_in, 1)));
  XSG_TRY(s->d_cx_slot.ensure(8 * (n_in + 1)));
  XSG_TRY(s->d_cx_edge.ensure(sizeof(xsg_context_edge) * std::max<uint64_t>(nchunks, 1)));
  // 1. newlines of the shard before every entry: d_line_off[i + 1] (d_out_u64 and d_line_len are scratch here)
  LineOutArgs o = line_out_args(s, a, l, n_in);
  o.tile_nl_off = s->d_tile_nl_off.as<uint64_t>();
  o.line_len = s->d_line_len.as<uint64_t>();
  o.line_out_off = s->d_line_off.as<uint64_t>();
  HIP_TRY(launch_line_nl_delta(o, st));
  HIP_TRY(launch_exclusive_scan_u64(o.line_len, s->d_line_off.as<uint64_t>(), n_in, s->d_scan_tmp.as<uint64_t>(), st));
  // 2. spans, edges, slots
  ContextArgs x{};
  x.base = s->base;
  x.chunks = a.chunks;
  x.tile_chunk = a.tile_chunk;
  x.chunk_tile0 = a.chunk_tile0;
  x.nchunks = nchunks;
  x.ntiles = s->ntiles;
  x.tile_bytes = s->tile_bytes;
  x.before = XSG_CONTEXT_BEFORE(c->flags);
  x.after = XSG_CONTEXT_AFTER(c->flags);
  x.tile_nl_off = o.tile_nl_off;
  x.total = n_in;
  x.r_pos = l.f_pos;
  x.r_chunk = l.f_chunk;
  x.nl_before = s->d_line_off.as<uint64_t>();
  x.lo = s->d_cx_lo.as<uint64_t>();
  x.hi = s->d_cx_hi.as<uint64_t>();
  x.cnt = s->d_cx_cnt.as<uint32_t>();
  x.edges = s->d_cx_edge.as<xsg_context_edge>();
  HIP_TRY(launch_context_spans(x, st));
  HIP_TRY(launch_exclusive_scan_u32(x.cnt, s->d_cx_slot.as<uint64_t>(), n_in, s->d_scan_tmp.as<uint64_t>(), st));
  s->context_edges.resize(nchunks);
  if (nchunks)
    HIP_TRY(hipMemcpyAsync(s->context_edges.data(), x.edges, sizeof(xsg_context_edge) * nchunks, hipMemcpyDeviceToHost, st));
  uint64_t n = 0;
  XSG_TRY(d2h_u64(c, s->d_cx_slot.as<uint64_t>() + n_in, &n));
  // 3. the starts whose rank lies in a span, at their slots
  XSG_TRY(s->d_cx_pos.ensure(8 * std::max<uint64_t>(n, 1)));
  XSG_TRY(s->d_cx_chunk.ensure(4 * std::max<uint64_t>(n, 1)));
  XSG_TRY(s->d_out_u64.ensure(8 * std::max<uint64_t>(n, 1)));
  x.slot = s->d_cx_slot.as<uint64_t>();
  x.out_total = n;
  x.o_pos = s->d_cx_pos.as<uint64_t>();
  x.o_chunk = s->d_cx_chunk.as<uint32_t>();
  HIP_TRY(launch_context_emit(x, st));
  l.f_pos = x.o_pos;
  l.f_match = x.o_pos;  // (most of these lines hold no match: LineOutArgs::invert keeps the output kernels away from it)
  l.f_chunk = x.o_chunk;
  l.total = n;
  *total = s->total = n;
  return XSG_OK;
}

// 6. the final list of `total` entries, in file order, in the form the tag asks for
static int list_outputs(xsg_shard* s, uint32_t mode, const ScanArgs& a, ListArgs& l, uint64_t total) {
  hipStream_t st = s->ctx->stream;
  XSG_TRY(s->d_f_pos.ensure(8 * std::max<uint64_t>(total, 1)));
  XSG_TRY(s->d_f_match.ensure(8 * std::max<uint64_t>(total, 1)));
  XSG_TRY(s->d_f_chunk.ensure(4 * std::max<uint64_t>(total, 1)));
  XSG_TRY(s->d_out_u64.ensure(8 * std::max<uint64_t>(total, 1)));
  l.f_pos = s->d_f_pos.as<uint64_t>();
  l.f_match = s->d_f_match.as<uint64_t>();
  l.f_chunk = s->d_f_chunk.as<uint32_t>();
  if (l.m_len) {  // XSG_MATCHES on the automaton routes
    XSG_TRY(s->d_f_len.ensure(4 * std::max<uint64_t>(total, 1)));
    l.f_len = s->d_f_len.as<uint32_t>();
  }
  l.total = total;
  HIP_TRY(launch_assemble(l, st));
  const bool invert = (s->ctx->flags & XSG_FLAG_INVERT) != 0;
  if (invert) XSG_TRY(invert_list(s, a, l, &total));
  if (s->ctx->max_count) XSG_TRY(limit_list(s, l, &total));
  const bool context = context_on(s->ctx) && mode != XSG_MATCH_BYTE_OFFSETS && mode != XSG_MATCHES;
  if (context) XSG_TRY(context_list(s, a, l, &total));
  LineOutArgs o = line_out_args(s, a, l, total);
  o.invert = invert || context ? 1u : 0u;
  if (mode == XSG_MATCH_BYTE_OFFSETS || mode == XSG_LINE_BYTE_OFFSETS)
    HIP_TRY(launch_globalize(o, st));
  else if (mode == XSG_LINE_INDICES)
    XSG_TRY(out_line_indices(s, a, o));
  else
    XSG_TRY(out_lines(s, o, mode == XSG_MATCHES));
  HIP_TRY(hipStreamSynchronize(st));
  if (mode == XSG_LINE_INDICES) s->nl_total = s->last_newlines;
  if (mode == XSG_LINES) s->total = total - s->h_dropped;  // lines without a terminating '\n' are not reported (search_wrappers.h:199-202)
  s->last_mode = (int)mode;
  s->context_edges_valid = context;
  s->rows_chunk = l.f_chunk;  // (xsg_result_chunk_ptr: the column behind the last of assemble, invert and context)
  s->rows_entries = total;
  return XSG_OK;
}

int xsg::run_list(xsg_shard* s, uint32_t mode, bool outputs, bool want_nl_total, bool pre_off) {
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  // XSG_MATCHES is the walk of XSG_MATCH_BYTE_OFFSETS up to the assembled list; only what leaves it differs
  const bool match_mode = mode == XSG_MATCH_BYTE_OFFSETS || mode == XSG_MATCHES;
  const bool line_mode = !match_mode;
  const bool want_len = mode == XSG_MATCHES && (c->pat.kind == kDfa || c->pat.kind == kSet);  // a length per emitted match (ScanArgs::m_len)
  // (the widening stage of XSG_FLAG_CONTEXT ranks lines by the per-tile newline counts)
  const bool want_nl = mode == XSG_LINE_INDICES || want_nl_total || (outputs && line_mode && context_on(c));
  const uint64_t nchunks = s->chunks.size();
  const uint64_t ntiles = s->ntiles;
  if (want_len)  // the lengths travel as uint32: no match may reach 4 GiB (a literal's or a class sequence's cannot)
    for (const xsg_chunk& ch : s->chunks)
      if (ch.length >= (1ull << 32)) return fail(XSG_ENOTSUP, "XSG_MATCHES with an expression of variable length needs chunks shorter than 4 GiB");
  if (line_mode && c->pat.has_newline && !newline_literal(c)) return fail(XSG_ENOTSUP, "%s", kNewlineExprMsg);
  const bool chain_lines = line_mode && newline_literal(c);
  if (match_mode && all_of_list(c)) return fail(XSG_ENOTSUP, "%s", kAllOfMatchMsg);  // (before any launch)

  s->last_mode = -1;
  s->context_edges_valid = false;
  s->total = 0;
  s->line_bytes = 0;
  s->fast_result = false;
  s->line_len_on_device = false;
  XSG_TRY(set_route_serves(s));
  XSG_TRY(ensure_factor_mask(s));

  if (match_mode && c->bordered) XSG_TRY(ensure_overlap_check(s));
  // 0. a result that fits the one-sync route's capacities is done there (one stream sync, a third of the launches)
  bool counts_ready = false;
  if (fast_route_serves(s, mode, outputs, want_nl_total)) {
    const int fr = run_list_fast(s, mode);
    if (fr != kFastOverflow) return fr;
    counts_ready = true;  // the per-tile counts (and newline counts) of that pass stand: continue at the ranks
    s->last_mode = -1;
    s->total = 0;
  }

  // 1. bulk count per tile
  if (want_nl) XSG_TRY(ensure_tile_nl(s));
  const bool scan_nl = want_nl && !s->nl_cached;  // newline counts per tile: once per binding, whatever the pattern
  if (!counts_ready) {
    XSG_TRY(choose_hot_filter(s, st, scan_nl, false));
    if (!use_prefilter(s, pre_off)) XSG_TRY(sketch_before_pass(s, st, !scan_nl, true, true));
    XSG_TRY(prepare_tiles(s, false, st));
  }
  ScanArgs a = scan_args(s, scan_variant(scan_nl, false));
  const bool pre = use_prefilter(s, pre_off);  // candidates by the class-sequence matcher, then the automaton
  if (pre && c->pat.kind != kSet) {  // (a literal list's candidate scan is its own pattern's: k_set_scan)
    a.pat = c->pre_pat;
    a.pat.hot = 0;
    a.sketch = nullptr;
  }
  s->cnt_clean = false;  // the tile counts stay in place for the emit pass: the next pass re-zeroes them
  if (!counts_ready) HIP_TRY(launch_scan_count(a, scan_nl, false, st));
  if (scan_nl) s->nl_cached = true;

  // 2. ranks
  XSG_TRY(s->d_tile_off.ensure(8 * (ntiles + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(std::max<uint64_t>(ntiles, nchunks) + 1)));
  HIP_TRY(launch_exclusive_scan_u32(a.tile_cnt, s->d_tile_off.as<uint64_t>(), ntiles, s->d_scan_tmp.as<uint64_t>(), st));
  uint64_t M = 0;
  uint32_t scan_flags = 0;
  if ((c->pat.kind == kClass || c->pat.kind == kDfa) && c->pat.ascii_only)
    HIP_TRY(hipMemcpyAsync(&scan_flags, a.flags, 4, hipMemcpyDeviceToHost, st));
  XSG_TRY(d2h_u64(c, s->d_tile_off.as<uint64_t>() + ntiles, &M));
  if (scan_flags & 1u) {  // non-ASCII data under an ascii_only expression
    HIP_TRY(hipMemsetAsync(a.flags, 0, 4, st));
    return fail(XSG_ENOTSUP, "%s", kNonAsciiMsg);
  }
  s->last_raw_matches = M;  // sizes the arrays of the next device-only pass (enqueue_count_bordered)

  // 3. ordered emission of every bulk occurrence, or of the prefilter's candidates and what is left of them
  a.tile_off = s->d_tile_off.as<uint64_t>();
  if (!pre) {
    XSG_TRY(s->d_m_pos.ensure(8 * std::max<uint64_t>(M, 1)));
    XSG_TRY(s->d_m_chunk.ensure(4 * std::max<uint64_t>(M, 1)));
    a.m_pos = s->d_m_pos.as<uint64_t>();
    a.m_chunk = s->d_m_chunk.as<uint32_t>();
    if (want_len) {
      XSG_TRY(s->d_m_len.ensure(4 * std::max<uint64_t>(M, 1)));
      a.m_len = s->d_m_len.as<uint32_t>();
    }
    if (M) HIP_TRY(launch_scan_emit(a, st));
  } else {
    const int pr = prefilter_candidates(s, outputs, want_len, a, &M);
    if (pr == kRedoUnfiltered) return run_list(s, mode, outputs, want_nl_total, true);
    if (pr != XSG_OK) return pr;  // (kDenseCandidates among them)
  }

  // 4. which occurrences the reference walk reports
  XSG_TRY(s->d_keep.ensure(4 * std::max<uint64_t>(M, 1)));
  XSG_TRY(s->d_keep_pre.ensure(8 * (M + 1)));
  XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(std::max<uint64_t>(M, std::max<uint64_t>(ntiles, nchunks)) + 1)));
  if (line_mode) XSG_TRY(s->d_m_ls.ensure(8 * std::max<uint64_t>(M, 1)));
  uint32_t tail_cap = 0;
  XSG_TRY(ensure_tail_buffers(s, &tail_cap));
  ListArgs l = list_args(s, a);
  l.pat = c->pat;  // (not a.pat: the scan may have run with the prefilter's pattern)
  l.M = M;
  l.m_ls = s->d_m_ls.as<uint64_t>();
  l.keep = s->d_keep.as<uint32_t>();
  l.keep_pre = s->d_keep_pre.as<uint64_t>();
  l.line_mode = line_mode ? 1u : 0u;
  XSG_TRY(decide_keep(s, l, chain_lines));

  // 5. the tail zone of every chunk and the totals; 6. the final list
  s->list_entries = M;  // (xsg_count_chunks reads the chunk column and keep_pre behind a pass without outputs)
  uint64_t total = 0;
  XSG_TRY(tails_and_total(s, a, l, want_nl_total, &total));
  if (!outputs) return XSG_OK;
  return list_outputs(s, mode, a, l, total);
}

extern "C" int xsg_search(xsg_shard* s, uint32_t mode, uint64_t* n_results) {
  if (s) s->rows_valid = false;  // (xsg_result_chunk_ptr: a search that is refused here leaves no rows either)
  XSG_TRY(check_ready(s));
  if (mode != XSG_MATCH_BYTE_OFFSETS && mode != XSG_LINE_BYTE_OFFSETS && mode != XSG_LINE_INDICES &&
      mode != XSG_LINES && mode != XSG_MATCHES)
    return fail(XSG_EINVAL, "xsg_search: mode %u is not a list mode", mode);
  if ((mode == XSG_MATCH_BYTE_OFFSETS || mode == XSG_MATCHES) && (s->ctx->flags & XSG_FLAG_INVERT)) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  if ((mode == XSG_MATCH_BYTE_OFFSETS || mode == XSG_MATCHES) && all_of_list(s->ctx)) return fail(XSG_ENOTSUP, "%s", kAllOfMatchMsg);
  HIP_TRY(hipSetDevice(s->ctx->device));
  XSG_TRY(run_list(s, mode, true));
  if (!s->fast_result) trim_pinned(s, 8 * (size_t)s->total, 8 * (size_t)s->total, (size_t)s->line_bytes);  // (an exact-route result is still on the device)
  if (n_results) *n_results = s->total;
  s->rows_valid = true;
  return XSG_OK;
}

// ---------------------------------------------------------------------------
// results
// ---------------------------------------------------------------------------
static int check_u64_result(const xsg_shard* s) {
  if (s->last_mode != XSG_MATCH_BYTE_OFFSETS && s->last_mode != XSG_LINE_BYTE_OFFSETS &&
      s->last_mode != XSG_LINE_INDICES)
    return fail(XSG_ESTATE, "no uint64 list result is pending on this shard");
  return XSG_OK;
}

extern "C" int xsg_result_u64(xsg_shard* s, uint64_t* out, uint64_t cap) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  XSG_TRY(check_u64_result(s));
  if (cap < s->total) return fail(XSG_EINVAL, "output capacity %llu < %llu results", (unsigned long long)cap,
                                  (unsigned long long)s->total);
  if (s->total == 0) return XSG_OK;
  if (!out) return fail(XSG_EINVAL, "out is null");
  if (s->fast_result) {  // the one-sync route: the kernels stored the result into the shard's pinned buffer as well
    memcpy(out, s->h_result.p, 8 * s->total);
    return XSG_OK;
  }
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, s->d_out_u64.p, 8 * s->total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XSG_OK;
}

// The same result without a copy into caller memory: moved once into a pinned buffer the shard owns (grow-only) and
// handed out as a pointer, valid until the next search on the shard.  A D2H copy into pageable memory runs at
// ~8 GB/s on this platform, into pinned memory at ~50: what matters when a dense needle returns hundreds of MB.
extern "C" int xsg_result_u64_view(xsg_shard* s, const uint64_t** out, uint64_t* n) {
  if (!s || !out || !n) return fail(XSG_EINVAL, "null argument");
  XSG_TRY(check_u64_result(s));
  *out = nullptr;
  *n = s->total;
  if (s->total == 0) return XSG_OK;
  if (!s->fast_result) {  // (else: already there)
    xsg_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = 8 * (size_t)s->total;
    XSG_TRY(s->h_result.ensure(need));
    HIP_TRY(hipMemcpyAsync(s->h_result.p, s->d_out_u64.p, need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  *out = s->h_result.as<uint64_t>();
  return XSG_OK;
}

extern "C" int xsg_result_newlines(xsg_shard* s, uint64_t* newlines) {
  if (!s || !newlines) return fail(XSG_EINVAL, "null argument");
  if (s->last_mode != XSG_LINE_INDICES) return fail(XSG_ESTATE, "no XSG_LINE_INDICES result is pending on this shard");
  *newlines = s->last_newlines;
  return XSG_OK;
}

extern "C" int xsg_result_context_edges(xsg_shard* s, xsg_context_edge* out, uint64_t cap_chunks) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  if (!s->context_edges_valid || (s->last_mode != XSG_LINE_BYTE_OFFSETS && s->last_mode != XSG_LINE_INDICES && s->last_mode != XSG_LINES))
    return fail(XSG_ESTATE, "no line-list result of a search with XSG_FLAG_CONTEXT is pending on this shard");
  const uint64_t n = s->context_edges.size();
  if (cap_chunks < n) return fail(XSG_EINVAL, "cap_chunks %llu < %llu chunks", (unsigned long long)cap_chunks, (unsigned long long)n);
  if (n && !out) return fail(XSG_EINVAL, "out is null");
  if (n) memcpy(out, s->context_edges.data(), sizeof(xsg_context_edge) * n);
  return XSG_OK;
}

// The rows of the pending list result: which of its entries are whose chunk's.  Computed here, when asked for, from the
// chunk bookkeeping the search left on the device (xsg_shard::rows_chunk) -- one launch (three more where XSG_LINES
// dropped a line: the prefix sum of the shortened rows), one copy of the words, one sync; the search itself does
// nothing for it.  The result and its other accessors are not touched: the words have buffers of their own.
extern "C" int xsg_result_chunk_ptr(xsg_shard* s, uint64_t* chunk_ptr, uint64_t cap_rows, uint64_t* byte_ptr) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  const int m = s->last_mode;
  const bool packed = m == XSG_LINES || m == XSG_MATCHES;
  if (!s->rows_valid || (!packed && m != XSG_MATCH_BYTE_OFFSETS && m != XSG_LINE_BYTE_OFFSETS && m != XSG_LINE_INDICES))
    return fail(XSG_ESTATE, "no list result of a successful xsg_search is pending on this shard");
  const uint64_t n = s->chunks.size();
  if (!chunk_ptr) return fail(XSG_EINVAL, "chunk_ptr is null");
  if (cap_rows < n + 1) return fail(XSG_EINVAL, "room for %llu rows' words, the binding needs %llu", (unsigned long long)cap_rows,
                                    (unsigned long long)(n + 1));
  if (byte_ptr && !packed) return fail(XSG_EINVAL, "byte_ptr belongs to an XSG_LINES or XSG_MATCHES result: the pending one holds uint64 values");
  if (n == 0) {
    chunk_ptr[0] = 0;
    if (byte_ptr) byte_ptr[0] = 0;
    return XSG_OK;
  }
  xsg_ctx* c = s->ctx;
  hipStream_t st = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t words = (n + 1) * (byte_ptr ? 2 : 1);
  XSG_TRY(s->d_rows.ensure(8 * (3 * n + 2)));
  XSG_TRY(s->h_rows.ensure(8 * (size_t)(2 * n + 2)));
  const bool dropped = m == XSG_LINES && s->total != s->rows_entries;
  ChunkRowsArgs a{};
  a.nchunks = n;
  a.total = s->rows_entries;
  a.f_chunk = s->rows_chunk;
  a.rows = s->d_rows.as<uint64_t>();
  if (a.f_chunk) {
    if (dropped) {
      a.line_len = s->d_line_len.as<uint64_t>();
      a.lens = a.rows + 2 * (n + 1);
    }
    if (byte_ptr) {
      a.line_off = s->d_line_off.as<uint64_t>();
      a.line_bytes = s->line_bytes;
      a.byte_rows = a.rows + (n + 1);
    }
  } else {
    a.m_chunk = s->d_m_chunk.as<uint32_t>();
    a.keep_pre = s->rows_keep_all ? nullptr : s->d_keep_pre.as<uint64_t>();
    a.tail_pre = s->d_tail_pre.as<uint64_t>();
  }
  HIP_TRY(launch_chunk_rows(a, st));
  if (a.lens) {
    XSG_TRY(s->d_scan_tmp.ensure(8 * scan_tmp_elems(n + 1)));
    HIP_TRY(launch_exclusive_scan_u64(a.lens, a.rows, n, s->d_scan_tmp.as<uint64_t>(), st));
  }
  uint64_t* h = s->h_rows.as<uint64_t>();
  HIP_TRY(hipMemcpyAsync(h, a.rows, 8 * words, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[n] != s->total) return fail(XSG_ESTATE, "the rows end at %llu, the result holds %llu entries: a call since the search took its bookkeeping",
                                    (unsigned long long)h[n], (unsigned long long)s->total);
  memcpy(chunk_ptr, h, 8 * (n + 1));
  if (byte_ptr) memcpy(byte_ptr, h + n + 1, 8 * (n + 1));
  return XSG_OK;
}

// xs::lines, exact route: the line lengths into the shard's pinned buffer (once per result)
static int fetch_line_lengths(xsg_shard* s) {
  if (!s->line_len_on_device) return XSG_OK;
  xsg_ctx* c = s->ctx;
  const uint64_t raw = s->fast_raw_lines;
  HIP_TRY(hipSetDevice(c->device));
  XSG_TRY(s->hp_line_len.ensure(8 * (size_t)raw));
  if (raw) HIP_TRY(hipMemcpyAsync(s->hp_line_len.p, s->d_line_len.p, 8 * raw, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  s->line_len_on_device = false;
  return XSG_OK;
}

static int check_lines_result(const xsg_shard* s) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  if (s->last_mode != XSG_LINES && s->last_mode != XSG_MATCHES)
    return fail(XSG_ESTATE, "no XSG_LINES or XSG_MATCHES result is pending on this shard");
  return XSG_OK;
}

extern "C" int xsg_result_lines_size(xsg_shard* s, uint64_t* n_lines, uint64_t* total_bytes) {
  XSG_TRY(check_lines_result(s));
  if (n_lines) *n_lines = s->total;
  if (total_bytes) *total_bytes = s->line_bytes;
  return XSG_OK;
}

// lengths (and offsets) of the `raw` entries without the dropped ones: lines without a terminating '\n' are not
// reported and own no bytes, so the packed bytes are already contiguous.  In place when out == in.  Returns how many stay.
static uint64_t squeeze_dropped(const uint64_t* len, const uint64_t* off, uint64_t raw, uint64_t* len_out, uint64_t* off_out) {
  uint64_t k = 0;
  for (uint64_t i = 0; i < raw; ++i) {
    if (len[i] == UINT64_MAX) continue;
    if (len_out) len_out[k] = len[i];
    if (off_out) off_out[k] = off[i];
    ++k;
  }
  return k;
}

// ... for the caller of xsg_result_lines.  An XSG_MATCHES result never drops an entry: two copies, no loop over matches.
static void copy_entries(const xsg_shard* s, const uint64_t* len, const uint64_t* off, uint64_t raw, uint64_t* len_out,
                         uint64_t* off_out) {
  if (s->last_mode != XSG_MATCHES) {
    squeeze_dropped(len, off, raw, len_out, off_out);
    return;
  }
  if (len_out && raw) memcpy(len_out, len, 8 * raw);
  if (off_out && raw) memcpy(off_out, off, 8 * raw);
}

extern "C" int xsg_result_lines(xsg_shard* s, uint64_t* lengths, char* bytes, uint64_t bytes_cap, uint64_t* offsets) {
  XSG_TRY(check_lines_result(s));
  if (bytes_cap < s->line_bytes) return fail(XSG_EINVAL, "bytes_cap too small");
  if (s->fast_result) {  // the one-sync route: lengths, offsets and bytes are in the pinned mirrors
    if (s->line_bytes) {
      if (!bytes) return fail(XSG_EINVAL, "bytes is null");
      memcpy(bytes, s->hp_line_bytes.p, s->line_bytes);
    }
    copy_entries(s, s->hp_line_len.as<uint64_t>(), s->h_result.as<uint64_t>(), s->fast_raw_lines, lengths, offsets);
    return XSG_OK;
  }
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  XSG_TRY(fetch_line_lengths(s));
  const uint64_t raw = s->fast_raw_lines;
  std::vector<uint64_t> goff;
  if (offsets && raw) {
    goff.resize(raw);
    HIP_TRY(hipMemcpyAsync(goff.data(), s->d_out_u64.p, 8 * raw, hipMemcpyDeviceToHost, c->stream));
  }
  if (s->line_bytes) {
    if (!bytes) return fail(XSG_EINVAL, "bytes is null");
    HIP_TRY(hipMemcpyAsync(bytes, s->d_line_bytes.p, s->line_bytes, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  copy_entries(s, s->hp_line_len.as<uint64_t>(), goff.data(), raw, lengths, goff.empty() ? nullptr : offsets);
  return XSG_OK;
}

// xs::lines without a copy into caller memory: lengths, offsets and packed bytes in the shard's pinned buffers.
extern "C" int xsg_result_lines_view(xsg_shard* s, const uint64_t** lengths, const char** bytes, const uint64_t** offsets,
                                     uint64_t* n_lines, uint64_t* total_bytes) {
  XSG_TRY(check_lines_result(s));
  xsg_ctx* c = s->ctx;
  uint64_t raw = s->fast_raw_lines;
  XSG_TRY(fetch_line_lengths(s));
  if (!s->fast_result) {  // the exact route left bytes and offsets on the device as well: two more pinned copies
    if (8 * raw * 2 + s->line_bytes > (16ull << 30)) return fail(XSG_ENOMEM, "the result needs more than 16 GiB of pinned memory");
    HIP_TRY(hipSetDevice(c->device));
    XSG_TRY(s->hp_line_bytes.ensure((size_t)s->line_bytes));
    XSG_TRY(s->h_result.ensure(8 * (size_t)raw));
    if (raw) HIP_TRY(hipMemcpyAsync(s->h_result.p, s->d_out_u64.p, 8 * raw, hipMemcpyDeviceToHost, c->stream));
    if (s->line_bytes) HIP_TRY(hipMemcpyAsync(s->hp_line_bytes.p, s->d_line_bytes.p, s->line_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    s->fast_result = true;  // from here on the result lives in the pinned buffers (xsg_result_lines reads them too)
  }
  uint64_t* len = s->hp_line_len.as<uint64_t>();
  uint64_t* off = s->h_result.as<uint64_t>();
  if (s->total != raw) s->fast_raw_lines = squeeze_dropped(len, off, raw, len, off);  // in place
  if (lengths) *lengths = len;
  if (offsets) *offsets = off;
  if (bytes) *bytes = s->hp_line_bytes.as<char>();
  if (n_lines) *n_lines = s->total;
  if (total_bytes) *total_bytes = s->line_bytes;
  return XSG_OK;
}
