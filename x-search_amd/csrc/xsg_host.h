// xsg_host.h -- what the host files of the C ABI share besides the objects of xsg_objects.h: xsg_ctx.cpp (errors,
// trace, contexts), xsg_pattern.cpp (compilation and upload), xsg_shard.cpp (bindings), xsg_count.cpp (count passes,
// probe, tuner), xsg_count_literals.cpp and xsg_litcount.cpp (counts per literal and their host-memory seam) and
// xsg_list.cpp (both list routes and the result accessors).  Everything else in those files is static.  Not installed.
#pragma once
#include "xsg_objects.h"

namespace xsg {

// ---- xsg_pattern.cpp ---------------------------------------------------------------------------------------------
uint32_t pick_filter_window(const uint8_t* p, size_t plen);
// the window-dependent fields of a literal pattern: the 8 bytes at p[koff..] as compare dwords and masks
void window_fields(const uint8_t* p, size_t plen, uint32_t koff, PatternDev* P);

// ---- xsg_count.cpp -----------------------------------------------------------------------------------------------
int check_ready(xsg_shard* s);
uint32_t scan_variant(bool want_nl, bool want_lines);
// `variant`: which k_scan instantiation the arguments are for (scan_variant): it selects the measured hot filter
ScanArgs scan_args(xsg_shard* s, uint32_t variant = 0);
int prepare_tiles(xsg_shard* s, bool want_lines, hipStream_t st);
int ensure_tile_nl(xsg_shard* s);
int choose_hot_filter(xsg_shard* s, hipStream_t st, bool want_nl = false, bool want_lines = false);
// Ahead of a pass with the context's own pattern, behind choose_hot_filter: builds the binding's sketch where it is due
// (`counts`: the pass is one of a synchronous entry point, which builds before its second) and takes the gate's verdict
// for (binding, pattern).  `may_sync` false (xsg_count_async): neither -- the pass uses what exists.
int sketch_before_pass(xsg_shard* s, hipStream_t st, bool plain, bool may_sync, bool counts);
bool sketch_ready(const xsg_shard* s);                  // the binding holds a sketch and the context's pattern has a gate
void sketch_fields(const xsg_shard* s, ScanArgs* a);    // ScanArgs::sketch, cand_*, gate_grid, sk_* for a->pat's filter window
int ensure_overlap_check(xsg_shard* s);
bool overlap_free_known(const xsg_shard* s);

// ---- xsg_count_literals.cpp --------------------------------------------------------------------------------------
// The pass of xsg_count_literals on `st` for the context's list (the callers checked that it is one): d_counts[j] += the
// occurrences of literal j in the bound chunks, behind a memset of the words when `zero` (xsg_litcount.cpp accumulates).
int enqueue_count_literals(xsg_shard* s, hipStream_t st, uint64_t* d_counts, bool zero);
// The pass of xsg_count_literals_chunks on `st`: both results zeroed on the stream, then one launch.  d_counts: chunks x
// literals words, d_chunks_with: a word per literal or null.
int enqueue_count_literals_chunks(xsg_shard* s, hipStream_t st, uint64_t* d_counts, uint64_t* d_chunks_with);
// The passes of xsg_count_literals_csr on `st`: the shard's scratch zeroed, count pass, prefix sum into d_row_ptr (chunks + 1
// words), fill pass into d_cols / d_vals below cap_entries, *d_status.  No size leaves the device.
int enqueue_count_literals_csr(xsg_shard* s, hipStream_t st, uint64_t* d_row_ptr, uint32_t* d_cols, uint64_t* d_vals,
                               uint64_t cap_entries, uint64_t* d_status);

// The passes of xsg_find_literals on `st`: count pass into the shard's scratch, prefix sum over the wave spans, d_chunk_ptr
// (chunks + 1 words) and *d_status gathered from it, fill pass into d_pos / d_lit below cap_entries (none for a capacity of
// 0).  No size leaves the device and nothing is zeroed.
int enqueue_find_literals(xsg_shard* s, hipStream_t st, uint64_t* d_chunk_ptr, uint64_t* d_pos, uint32_t* d_lit,
                          uint64_t cap_entries, uint64_t* d_status);

inline const char* const kNonAsciiMsg =
    "the expression uses '.', a negated class or \\D \\W \\S, which match whole code points in RE2; the data holds "
    "bytes >= 0x80, where one byte per position is not the same thing: refused, not approximated";
inline const char* const kInvertMatchMsg =
    "XSG_FLAG_INVERT: an inverted search reports lines without a match; the match tags have no inverted form";
inline const char* const kAllOfMatchMsg =
    "XSG_LIST_ALL_OF: a conjunction selects lines; it has no single match, and the match tags are not served for it";
inline const char* const kNewlineExprMsg = "line modes do not accept an expression that can match '\\n'";

// ---- xsg_list.cpp ------------------------------------------------------------------------------------------------
// A LITERAL that contains '\n': its line tags are a chain of occurrences (k_nlpat_links), resolved on the exact list
// route.  (An EXPRESSION that can match '\n' keeps being refused by the line tags: RE2's walk over a re-sliced input is
// not restated for it.)
bool newline_literal(const xsg_ctx* c);
bool all_of_list(const xsg_ctx* c);  // a literal list set with XSG_LIST_ALL_OF (PatternDev::set_all_of)
int ensure_factor_mask(xsg_shard* s);
// `pre_off`: the caller must not take the prefilter route (run_list: its candidates were dense or outran their budget)
bool use_prefilter(const xsg_shard* s, bool pre_off);
// XSG_ENOTSUP where the candidate route cannot serve a literal list on this binding (2^24 chunks and more)
int set_route_serves(const xsg_shard* s);
// The tail zone of every chunk: its buffers sized for this binding and pattern, *tail_cap = entries per chunk.
int ensure_tail_buffers(xsg_shard* s, uint32_t* tail_cap);
// What every list kernel's arguments share: the shard, the scan's emitted list (a.m_pos / a.m_chunk / a.tile_off) and
// the tail-zone buffers.  `pat`, M / M_dev, keep / m_ls / keep_pre and the mode are the caller's.
ListArgs list_args(const xsg_shard* s, const ScanArgs& a);
constexpr int kDenseCandidates = 1;  // run_list(outputs = false) on the prefilter route: too many candidates, count by k_rx_scan
// The exact list route behind xsg_search and the counts that need the ordered list (the one-sync route first where it
// serves).  `want_nl_total`: also leave the shard's newline total in last_newlines (xsg_count on the prefilter route);
// `pre_off`: as for use_prefilter, set by run_list itself when it starts over
int run_list(xsg_shard* s, uint32_t mode, bool outputs, bool want_nl_total = false, bool pre_off = false);

}  // namespace xsg
