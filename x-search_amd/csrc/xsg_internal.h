// xsg_internal.h -- shared between the HIP kernels (xsg_kernels.hip, xsg_list_kernels.hip, xsg_rx_kernels.hip) and the
// C-ABI host code (through xsg_objects.h: xsg_ctx / xsg_pattern / xsg_shard / xsg_count / xsg_list.cpp, xsg_job.cpp).
// Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsg.h"
#include "xsg_sketch.h"

namespace xsg {

// ---- tile geometry ---------------------------------------------------------
// A workgroup of 4 wave64s scans one tile.  Each lane reads kLoads 16-byte
// units; a wave-instruction therefore covers 1 KiB of consecutive bytes
// (fully coalesced global_load_dwordx4), a wave covers a contiguous span of
// kLoads KiB and the tile is the 4 spans back to back.
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kUnit = 16;
constexpr uint32_t kWaveLoad = 64 * kUnit;
// kLoads (units per lane) is a template parameter of k_scan: the tile is
// kLoads KiB per wave x 4 waves = 16 KiB (kLoads 4) or 32 KiB (kLoads 8).
constexpr uint32_t kDefaultTileBytes = 16384;
constexpr uint32_t kDefaultStagger = 16;  // see k_scan / pick_stagger (round 2: xsg_shard_tune picked 16 in every 50 GiB run)
constexpr uint32_t kGateGrid = 8192;      // workgroups of the gated count pass (k_scan<..., GATED>): DESIGN.md section 5, "Sketch gate"
constexpr uint32_t kTuneAuto = 0xffffffffu;  // ScanArgs::tune: let launch_scan pick the stagger per variant

// Same layout as xsg_chunk (include/xsg.h).
struct ChunkDev {
  uint64_t offset;
  uint64_t length;
  uint64_t global_offset;
  uint64_t line_base;
};

// Candidate filter shapes (how many of the first 8 pattern bytes the
// in-register window compare covers; longer patterns are verified from memory).
enum FilterKind : int {
  kMask1 = 0,  // plen 1..3 : one masked dword compare
  kOne = 1,    // plen 4    : one dword compare
  kMask2 = 2,  // plen 5..7 : one dword + one masked dword
  kTwo = 3,    // plen 8    : two dword compares (exact)
  kLong = 4,   // plen > 8  : two dword compares on the 8-byte filter window (koff), then memory for the rest
  kClass = 5,  // class sequence (xsg_classseq.h): two masked dword compares over the literal bytes of the window,
               // then every position against its 256-bit set (d_pat holds the sets, 32 bytes per position)
  kClassFast = 7,  // instantiation only (PatternDev::kind stays kClass): a class sequence whose window takes the exact
                   // 16 + 32 bit compare (PatternDev::cls_fast), window filter
  kDfa = 6,    // variable-length expression (xsg_regex.h): k_rx_scan walks every line with a byte-class DFA; d_pat holds
               // class_of[256], the forward table, the reverse table (uint16 row offsets)
  kSet = 8     // a list of literals (xsg_set.h): k_set_scan finds the positions whose g-gram is in the filter, k_set_verify
               // decides them; d_pat holds the filter (8 KiB) and the verify table.  Always on the candidate route.
};

struct PatternDev {
  uint32_t plen;
  uint32_t kind;
  uint32_t p0, m0, p1, m1;  // the 8 pattern bytes of the filter window (pattern[koff..koff+8)) as dwords + byte masks
  uint32_t q0, q1;          // ignore_case hot filter: (p0 | 0x20202020) & m0, (p1 | 0x20202020) & m1 (k_scan, LAZY)
  uint32_t koff;            // kLong, kClass: offset of the 8-byte filter window inside the pattern (0 for the other kinds)
  uint16_t set_words;       // kSet: XSG_LIST_WHOLE_WORDS (SetTable::words).  It lies HERE, in the four bytes that padded d_pat to
                            // its alignment: the structure keeps its size and every other field its offset, so no other
                            // kernel's arguments change (profiles/literal_words_registers.txt)
  uint16_t set_all_of;      // kSet: XSG_LIST_ALL_OF, in the upper half of those four bytes.  No kernel reads it: the host picks
                            // the all-of stages by it (xsg_list.cpp), and 0 / 1 in the lower half reads as it did
                            // (profiles/all_of_registers.txt)
  const uint8_t* d_pat;     // device copy of the pattern
  uint32_t exact_tail;      // XSG_FLAG_EXACT_TAIL
  uint32_t nl_first;        // literal whose FIRST byte is '\n': the reference's line start of a match then lies one byte behind the
                            // match's first byte (previous_new_line_offset_relative_to_match looks at that byte first, :111-123)
  uint32_t has_newline;     // pattern contains '\n'
  uint32_t icase;           // XSG_FLAG_IGNORE_CASE: data bytes are ASCII-lowered before every compare (pattern is lowered on the host)
  uint32_t lazy_exact;      // ignore_case: every byte of the filter window is a letter, so the hot filter on (data | 0x20) IS the
                            // exact folded compare and its results stand (no second, properly folded pass over the window)
  uint32_t hot;             // window kinds (kTwo, kLong, kClass): 1 = aligned-dword trigger, 0 = window filter (k_scan<..., ALIGNED>)
  uint32_t cls_fast;        // kClass: m1 is all ones and the low half of m0 too: the window filter compares 16 + 32 exact bits
  uint32_t cls_inreg;       // kClass, plen <= 8 (koff = 0): candidates are decided in registers (k_scan: cls_verify_at) ...
  uint32_t cls_chk;         // ... looking up only these positions (bit k) in the sets: the ones the hot filter's compare does
                            // not already decide exactly
  uint32_t cls_exact;       // kClass, one alternative, plen <= 8, and the masked window compare decides every position exactly:
                            // a candidate IS a match, nothing is looked up
  uint32_t nalt;            // kClass: alternatives (d_pat holds nalt x plen sets, alternative-major); 0/1 otherwise
  uint32_t ascii_only;      // kClass: the expression is exact on ASCII data only ('.', negated classes): k_scan raises
                            // ScanArgs::flags bit 0 when it meets a byte >= 0x80
  // kDfa (ascii_only as for kClass; plen = the shortest match; exact_tail = 1)
  uint32_t rx_ncls;                // byte classes
  uint32_t rx_fwd_n, rx_rev_n;     // table entries (states x classes) of the forward / reverse automaton
  uint32_t rx_fwd_start, rx_fwd_acc;  // ROW OFFSETS (state x ncls): start state, first accepting state
  uint32_t rx_rev_start, rx_rev_acc;
  uint32_t rx_anc_n, rx_anc_start, rx_anc_acc;  // the ANCHORED forward automaton (behind the reverse table in d_pat): k_rx_verify
  uint32_t rx_multiline;           // a set of the expression accepts '\n': the chunk, not the line, is the unit (k_rx_chunk)
  uint32_t rx_ntrig, rx_trig4;     // rx_skip and at most four trigger byte values besides '\n' (packed in rx_trig4): k_rx_scan tests
                                   // the tile for them on the 16-byte loads and leaves a tile that holds none without staging it
  uint32_t rx_skip;                // bit 7 of every class_of[] entry flags a TRIGGER byte: one that moves the forward automaton
                                   // out of its start state, or '\n' (needs ncls <= 128; XSG_RX_SKIP=0 switches it off)
  uint32_t rx_bol, rx_eol;         // the line-anchor form (?m)^BODY$ (xsg_regex.h): rx_bol -- the forward table is the
                                   // ANCHORED automaton, walked from each line start (and each match end), never skipping;
                                   // rx_eol -- it runs over BODY '\n', a '\n' is stepped at the chunk's end, at most one
                                   // match per line, ending one byte before the last accepting position
  // kSet (plen = the shortest literal; exact_tail = 1; icase: the data is folded, the literals are folded on the host)
  uint32_t set_g;                  // gram length, 1..4
  uint32_t set_ngrams;             // distinct grams = entries of the sorted key array
  uint32_t set_keys, set_first, set_ent, set_bytes;  // byte offsets of the verify table's arrays inside d_pat (xsg_set.h: SetTable)
};

// Per-tile line summaries (XSG_COUNT_LINES): see xsg_linesum.h.

struct ScanArgs {
  const uint8_t* base;          // shard buffer
  const ChunkDev* chunks;       // device chunk table
  const uint32_t* tile_chunk;   // tile -> chunk (null when the shard has one chunk)
  const uint64_t* chunk_tile0;  // first tile of every chunk (nchunks + 1 entries)
  uint64_t ntiles;
  uint64_t nchunks;             // entries of `chunks` (k_rx_chunk: one lane per chunk)
  uint32_t tile_bytes;          // 16384 (selects the k_scan instantiation)
  uint32_t tune;                // bits 0-7: wave stagger in units of s_sleep(1) = 64 clocks; kTuneAuto = per variant (XSG_TUNE overrides)
  uint32_t epoch;               // 1..0xffff: tag of this pass in the upper half of the tile_last words
  PatternDev pat;
  // outputs of the counting pass.  Only waves that found something write (no store on the common path), so
  // "nothing found" must already be in place: tile_cnt == 0 and tile_sum == 0 (k_count_finish restores both as
  // it consumes them), tile_last from an older epoch (never reset: a newer tag wins the atomicMax).
  uint32_t* tile_cnt;                  // matches starting in the tile (o < limit)
  uint32_t* tile_nl;                   // '\n' in the tile              (WANT_NL; every tile is written)
  uint32_t* tile_sum;                  // line summary PER WAVE (4 per tile), stored XOR kSumNl (WANT_LINES)
  uint32_t* tile_last;                 // (epoch << 16) | max (match offset + plen) in the tile, relative to the tile start
  uint32_t dense_hint;                 // an earlier count of this pattern over this shard found it dense: 1 = more than one result
                                       // per 8 KiB (dense_bytes_route), 2 = more than one per 2 KiB (pick_stagger too)
  uint32_t lines_only;                 // count pass with line summaries, matches not asked for (xs::count_lines): a kMask1
                                       // needle skips its match counting (and, where no end-of-chunk walk exists, tile_cnt /
                                       // tile_last altogether)
  uint32_t* flags;                     // one word per shard, zero at rest: bit 0 = "non-ASCII byte under an ascii_only expression"
  const uint32_t* tile_mask;           // k_rx_scan: if set, only tiles with a non-zero word can hold the start of a line with a
                                       // match (the factor prefilter, xsg_list.cpp: ensure_factor_mask); null: every tile
  // inputs/outputs of the emit pass
  uint64_t m_cap;            // entries m_pos / m_chunk can hold (ranks beyond are dropped; 0 = as many as there are)
  const uint64_t* tile_off;  // exclusive prefix of tile_cnt
  uint64_t* m_pos;           // chunk-local offset of every match, ascending
  uint32_t* m_chunk;         // its chunk
  uint32_t* m_len;           // kDfa, XSG_MATCHES: its length (the walk's resume point minus its start); null for every other
                             // tag -- the test is uniform per launch, and a launch without it stores what it always stored
  // emit pass over the tiles that hold a match only (the one-sync list route): the ordered list of those tiles and
  // where its length lives; null: one workgroup per tile of the shard, each leaving at once if its count is 0
  const uint32_t* hit_tiles;
  const uint64_t* n_hits_dev;
  uint64_t hit_cap;
  // one byte per tile (four tiles a word): bit w = wave w of the tile found something.  Set by a count pass that is
  // followed by an emit pass over the hit list (null otherwise), read and cleared by that emit pass; a stale bit is
  // harmless (the wave reads its 4 KiB and finds nothing), so the array is only ever zeroed when it is (re)allocated
  uint32_t* tile_wmask;
  // The gate of the plain count pass (k_scan<..., GATED>: gated_pass): the binding's per-tile 4-gram sketch
  // (xsg_sketch.h; null: none, or not to be used for this pattern here) and the pattern's bits in it, one entry per
  // distinct word of the tile's 128 (sk_n entries).  The gated k_scan is a bounded grid of persistent workgroups that
  // stride over units of 256 tiles, test each tile's words and scan the tiles that hold every bit: no list, no counter,
  // nothing to reset between passes.  sk_pat / sk_koff say which pattern and filter window the entries were computed for: launch_scan gates only a
  // pass whose `pat` is still that one (callers put other patterns and windows into a copy of these arguments).
  const uint32_t* sketch;
  const uint8_t* sk_pat;
  uint32_t sk_koff;
  uint32_t sk_n;
  uint32_t gate_grid;           // workgroups of the gated k_scan (XSG_GATE_GRID); 0: kGateGrid
  uint32_t sk_word[32];
  uint32_t sk_mask[32];
};

// k_sketch_build: one workgroup per tile, 512 B per tile (xsg_sketch.h)
struct SketchArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint32_t* tile_chunk;   // tile -> chunk (null when the shard has one chunk)
  const uint64_t* chunk_tile0;
  uint64_t ntiles;
  uint32_t* sketch;             // sketch_alloc_words(ntiles), at sketch_index(tile, word)
  uint32_t* spans;              // the span locator: span_alloc_words(ntiles), at span_index(tile, word, span); null: not built
};
hipError_t launch_sketch_build(const SketchArgs& a, hipStream_t s);
// k_sketch_planes: the finished sketch transposed into its bit planes (xsg_sketch.h), plane_alloc_words(ntiles) words of
// 64 bits; stream-ordered behind launch_sketch_build
hipError_t launch_sketch_planes(const uint32_t* sketch, uint64_t ntiles, uint64_t* planes, hipStream_t s);
// k_sketch_sample: *passed += the number of tiles among 0, stride, 2 * stride, ... (nsamp of them, all < ntiles) whose
// sketch holds every bit of a.sk_word / a.sk_mask -- what share of the tiles the gate of this pattern would let through
hipError_t launch_sketch_sample(const ScanArgs& a, uint64_t stride, uint32_t nsamp, uint32_t* passed, hipStream_t s);
// would launch_scan_count run the gated instantiation for these arguments?
bool scan_gated(const ScanArgs& a, bool want_nl, bool want_lines);

// The FINISHING form of the gated count pass (k_scan_fin: gated_pass<..., FIN>): a plain match count that sums in
// registers, walks the end-of-chunk zones that hold an occurrence itself and writes the counters -- one launch, no
// k_count_finish, no store to the per-tile arrays.  What it needs beyond ScanArgs travels as a second kernel parameter,
// so that every other k_scan instantiation keeps its argument block.
constexpr uint32_t kGateRegs = 6;  // sketch words a lane requests at once; entries beyond (long needles) follow in batches
struct GateFinArgs {
  uint64_t* counters;         // device, XSG_NUM_COUNTERS: {matches, 0, 0, total_bytes}
  uint64_t* host_counters;    // optional pinned mirror
  uint64_t* status;           // optional: receives 0
  unsigned long long* word;   // 1 + kFinGroups words, zero at rest, each (arrivals << kFinTotalBits) | their matches so
                              // far: workgroup b arrives at word 1 + b % kFinGroups, the last of a group at word 0; who
                              // is last learns it and the sum from the value its atomicAdd returns and puts the word back
  uint64_t total_bytes;
  // The span locator of the binding (xsg_sketch.h; null: whole-tile reads) and the pattern's bits in a span's kSpanBits,
  // one entry per distinct word like sk_word / sk_mask: a candidate tile's wave reads its 4 KiB only if its span holds
  // them all.  At most kSpanRegs entries: fewer grams are still a superset filter.  (Here, not in ScanArgs: every other
  // k_scan instantiation keeps its argument block.)
  const uint32_t* spans;
  uint32_t sp_n;
  uint32_t sp_word[kSpanRegs];
  uint32_t sp_mask[kSpanRegs];
  // The wave form (k_scan_fin<..., true>: gated_pass_waves): a wave owns a sketch group of 64 tiles from its sketch words
  // to its text, no workgroup barrier in the pass.  Only with `spans` (a 4 KiB span is one wave's load batch);
  // XSG_GATE_WAVES=0 keeps the workgroup form.
  uint32_t waves;
  // The wave form takes its groups in batches: a wave's next `batch` rounds (1 .. kGateBatch) are selected together,
  // their candidates located in one round trip and then scanned.  XSG_GATE_BATCH=1 keeps one group at a time.
  uint32_t batch;
  // The wave form's select from the sketch's bit planes (xsg_sketch.h; null: from the sketch words, as the other forms
  // do): a group's candidates are the AND of one 64-bit word per tested gram, pl_bit[k] = the gram's sketch_hash = its
  // plane -- every gram sketch_fields folds into sk_word / sk_mask, pl_n of them.  XSG_GATE_PLANES=0 keeps the word select.
  const uint64_t* planes;
  uint64_t pl_stride;         // plane_stride(ntiles)
  uint32_t pl_n;
  uint16_t pl_bit[kSketchMaxGrams];
};
#ifndef XSG_GATE_BATCH_N
#define XSG_GATE_BATCH_N 4
#endif
constexpr uint32_t kGateBatch = XSG_GATE_BATCH_N;  // rounds of a wave per batch (gated_pass_waves): DESIGN.md section 5
static_assert(kGateBatch >= 1 && kGateBatch <= 8, "a candidate's place in its batch: 3 + 6 bits; 7 registers a round in the select phase");
// workgroups of the wave form when XSG_GATE_GRID does not say (the storing form and the workgroup finishing form:
// kGateGrid): one resident round at six waves per SIMD on 256 compute units, every wave taking its groups in batches.
// On 50 GiB level with 3200; on 10 GiB (2560 units) ahead of one workgroup per unit, where no wave has a second group
// to batch ("Batches")
constexpr uint32_t kGateGridWaves = 1536;
constexpr uint32_t kFinGroups = 64;
constexpr uint32_t kFinTotalBits = 40;  // matches <= total_bytes < 2^40; the grid stays below 2^24 (scan_finishing)
// would a plain match count over these arguments take the finishing form?  (gated, an end-of-chunk zone the wave walk
// serves -- exact_tail or plen <= kTailMaskMaxPlen -- and both fields of GateFinArgs::word wide enough)
bool scan_finishing(const ScanArgs& a, uint64_t total_bytes);
hipError_t launch_scan_count_finishing(const ScanArgs& a, const GateFinArgs& f, hipStream_t s);

constexpr int kFinishBlocks = 2048;  // upper bound of k_count_finish's grid (size of FinishArgs::partials / 3)

struct FinishArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint64_t* chunk_tile0;
  uint64_t nchunks;
  uint64_t ntiles;
  PatternDev pat;
  uint32_t* tile_cnt;         // read, then zeroed again
  const uint32_t* tile_nl;
  uint32_t* tile_sum;         // read, then zeroed again
  const uint32_t* tile_last;  // valid where the upper half equals `epoch`
  uint32_t epoch;
  uint32_t tile_bytes;
  uint64_t* counters;       // device, XSG_NUM_COUNTERS: overwritten (no zeroing needed)
  uint64_t* host_counters;  // optional: pinned host mirror of the same four values
  uint64_t* status;         // optional (xsg_count_async_status): receives XSG_STATUS_* bits; a refusal then ZEROES the counters
                            // instead of poisoning them
  uint64_t* partials;       // scratch: 3 x kFinishBlocks
  uint32_t* ticket;         // zero at rest: the last workgroup to arrive does the final sum and resets it
  uint32_t* flags;          // ScanArgs::flags: read and cleared by that workgroup; bit 0 poisons the counters (UINT64_MAX)
  uint64_t total_bytes;     // sum of the chunk lengths (host-side knowledge)
  uint32_t want_nl;
  uint32_t want_lines;
  uint32_t want_matches;
  uint32_t cnt_is_lines;  // kDfa, XSG_COUNT_LINES: tile_cnt holds matching lines, its sum is reported as XSG_CTR_LINES
};

// k_count_chunks (xsg_count_chunks*): k_count_finish's work with the chunk boundaries kept.  What it needs beyond
// FinishArgs travels as a second kernel parameter, so that k_count_finish keeps its argument block.  Both arrays hold
// nchunks words and are ZERO before the launch (the kernel adds; a chunk in which nothing is found is never touched).
struct ChunkCountArgs {
  const uint32_t* tile_chunk;  // tile -> chunk (null when the shard has one chunk)
  uint64_t* counts;            // per chunk: what the pass puts into XSG_CTR_MATCHES (want_matches) or XSG_CTR_LINES
                               // (want_lines); null: not asked for (a pass for the newline counts alone)
  uint64_t* newlines;          // per chunk: its '\n' (needs FinishArgs::want_nl); null: not asked for
};
hipError_t launch_count_chunks(const FinishArgs& a, const ChunkCountArgs& c, hipStream_t s);
// behind it, one lane per chunk: a refusal (*status != 0, or the poisoned counters of a pass without a status word)
// zeroes counts[c] and newlines[c]; otherwise, `invert`, counts[c] = lines of chunk c (newlines[c], plus one for a last
// line without its '\n') - counts[c]: the per-chunk form of k_invert_count_lines.  `newlines` may be null unless `invert`.
hipError_t launch_chunk_counts_post(const uint8_t* base, const ChunkDev* chunks, uint64_t nchunks, uint64_t* counts,
                                    uint64_t* newlines, const uint64_t* counters, const uint64_t* status, uint32_t invert,
                                    hipStream_t s);
// The per-chunk figures of a count that IS a list (xsg_list_kernels.hip: k_list_chunk_counts): one lane per chunk, two
// binary searches in the chunk column of the M raw entries (ascending), the kept ones between them from keep_pre, plus
// the chunk's tail entries; newlines[c] (if asked for, or `invert`) from the prefix of the per-tile newline counts.
struct ListChunkArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint64_t* chunk_tile0;
  uint64_t nchunks;
  uint64_t M;
  const uint32_t* m_chunk;
  const uint64_t* keep_pre;     // M + 1 entries
  const uint32_t* tail_cnt;     // per chunk
  const uint64_t* tile_nl_off;  // exclusive prefix of tile_nl (ntiles + 1); null: no newline figures
  uint64_t* counts;
  uint64_t* newlines;           // optional
  uint32_t invert;              // counts[c] = lines of chunk c - counts[c] (needs tile_nl_off)
};
hipError_t launch_list_chunk_counts(const ListChunkArgs& a, hipStream_t s);
// xsg_result_chunk_ptr (xsg_list_kernels.hip: k_chunk_rows): the rows of a finished list result, computed when asked for
// from what the search left on the device.  One lane per word of the nchunks + 1, a binary search each:
//   f_chunk != null   the chunk column of the `total` final entries (the exact route behind launch_assemble, invert_list
//                     or context_list; the one-sync route's line-index and line tags): rows[c] = first entry of chunk c.
//                     With line_len (XSG_LINES that dropped unterminated lines, UINT64_MAX in line_len: a chunk's last
//                     entries) the lane writes the row's LENGTH without them to lens[c]; their prefix sum is the rows.
//   f_chunk == null   the one-sync route's two offset tags, which write no such column: rows[c] = what the walk kept of
//                     the raw entries in front of chunk c (keep_pre; null: all of them) + the tail entries of the chunks
//                     in front of it (tail_pre) -- where k_list_out put chunk c's first entry.
// byte_rows (optional, with f_chunk): line_off at the row's first entry, line_bytes behind the last.
struct ChunkRowsArgs {
  uint64_t nchunks;
  uint64_t total;             // entries of f_chunk, or raw entries of m_chunk
  const uint32_t* f_chunk;
  const uint32_t* m_chunk;
  const uint64_t* keep_pre;   // total + 1 entries
  const uint64_t* tail_pre;   // nchunks + 1 entries
  const uint64_t* line_len;   // `total` entries
  const uint64_t* line_off;   // exclusive prefix of line_len (dropped: 0), `total` entries
  uint64_t line_bytes;
  uint64_t* rows;             // nchunks + 1
  uint64_t* lens;             // nchunks (with line_len)
  uint64_t* byte_rows;        // nchunks + 1, or null
};
hipError_t launch_chunk_rows(const ChunkRowsArgs& a, hipStream_t s);
// xsg_set_max_count, the limit stage of the exact list route (xsg_list_kernels.hip: k_limit_rows, k_limit_copy): the final
// list (behind launch_assemble or invert_list) is replaced by the first `limit` entries of every chunk.  Rows: one lane per
// chunk, the two binary searches of k_chunk_rows in the chunk column; old_ptr[c] = the chunk's first entry, cnt[c] =
// min(its entries, limit).  The caller takes the exclusive prefix of cnt (new_ptr, nchunks + 1 words) and fetches its last
// word.  Copy: one lane per old entry i of chunk c; rank i - old_ptr[c] below limit -> slot new_ptr[c] + rank.  Ranks and
// counts are 64-bit: a limit of 2^32 + 1 or UINT64_MAX cuts nothing.
struct LimitArgs {
  uint64_t nchunks;
  uint64_t total;            // entries of the list that comes in
  uint64_t limit;            // > 0
  const uint64_t* f_pos;
  const uint64_t* f_match;   // may be f_pos (an inverted list has no matches): then o_match is o_pos and is not written twice
  const uint32_t* f_chunk;
  const uint32_t* f_len;     // null: the tag has no length column
  uint64_t* cnt;             // nchunks
  uint64_t* old_ptr;         // nchunks
  const uint64_t* new_ptr;   // nchunks + 1 (copy)
  uint64_t* o_pos;
  uint64_t* o_match;
  uint32_t* o_chunk;
  uint32_t* o_len;
};
hipError_t launch_limit_rows(const LimitArgs& a, hipStream_t s);
hipError_t launch_limit_copy(const LimitArgs& a, hipStream_t s);
// ... and its count-side twin (k_limit_counts): counts[c] = min(counts[c], limit) in place, their sum ADDED to *sum (zero
// before the launch).  A refused pass left the words zero (launch_chunk_counts_post): the sum is then 0 as well.
hipError_t launch_limit_counts(uint64_t* counts, uint64_t nchunks, uint64_t limit, unsigned long long* sum, hipStream_t s);

// ---- launchers (xsg_kernels.hip) --------------------------------------------
hipError_t launch_scan_count(const ScanArgs& a, bool want_nl, bool want_lines, hipStream_t s);
hipError_t launch_scan_emit(const ScanArgs& a, hipStream_t s);
hipError_t launch_count_finish(const FinishArgs& a, hipStream_t s);
// kDfa (xsg_rx_kernels.hip): same ScanArgs, same per-tile outputs.  count: tile_cnt = matches (or, want_lines, matching
// lines) of the lines that START in the tile, tile_nl if want_nl; emit: the matches at their ranks.
hipError_t launch_rx_count(const ScanArgs& a, bool want_nl, bool want_lines, hipStream_t s);
hipError_t launch_rx_emit(const ScanArgs& a, hipStream_t s);
// the prefilter route of kDfa (xsg_rx_kernels.hip): candidates of the scan kernel -> verified, walked, packed
struct RxPreArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint64_t* chunk_tile0;
  uint64_t nchunks;
  PatternDev pat;            // the kDfa pattern (tables in d_pat)
  uint64_t n;                // candidates, ascending per chunk
  const uint64_t* tile_off;  // their ranks by tile: a chunk's candidates are [tile_off[tile0[c]], tile_off[tile0[c+1]])
  const uint64_t* c_pos;
  const uint32_t* c_chunk;
  uint32_t* c_len;           // length of the match that starts at the candidate, 0: none
  uint32_t* c_keep;          // reported by the reference's walk
  uint64_t* scan_tmp;        // n / 2048 + 1 words
  uint32_t* flags;           // ScanArgs::flags; bit 1: a candidate outran k_rx_verify's budget (the host takes the other route)
  const uint64_t* c_pre;     // exclusive prefix of c_keep
  uint64_t* m_pos;           // the reported ones, packed
  uint32_t* m_chunk;
  uint32_t* m_len;           // XSG_MATCHES: their c_len, packed with them (null otherwise)
};
hipError_t launch_rx_verify_keep(const RxPreArgs& a, hipStream_t s);
hipError_t launch_rx_compact(const RxPreArgs& a, hipStream_t s);
// kSet (xsg_set_kernels.hip): k_set_scan with k_scan's ScanArgs and per-tile outputs (tile_cnt of every tile, tile_nl if
// want_nl; emit: m_pos / m_chunk ascending) on a bounded grid; k_set_verify in k_rx_verify's place (c_len per candidate)
hipError_t launch_set_count(const ScanArgs& a, bool want_nl, hipStream_t s);
hipError_t launch_set_emit(const ScanArgs& a, hipStream_t s);
hipError_t launch_set_verify(const RxPreArgs& a, hipStream_t s);
void describe_set_scan(const ScanArgs& a, bool emit, char* out, size_t cap);
// XSG_LIST_ALL_OF (xsg_list.cpp: prefilter_candidates, decide_keep).  k_set_verify_all in k_set_verify's place: c_mask[i] =
// the listing indices of EVERY literal that occurs at candidate i, as bits, c_keep[i] = c_mask[i] != 0; k_set_compact_all packs
// the kept candidates with their masks at the ranks c_pre.  The arguments are their own, so that RxPreArgs and every kernel
// that takes it stay what they are.
struct SetAllArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  PatternDev pat;
  uint32_t idx_off;          // byte offset of SetTable::idx inside PatternDev::d_pat (SetProgram::idx_offset)
  uint64_t n;                // candidates
  const uint64_t* c_pos;
  const uint32_t* c_chunk;
  uint64_t* c_mask;          // one word per candidate
  uint32_t* c_keep;
  const uint64_t* c_pre;     // exclusive prefix of c_keep (compact)
  uint64_t* m_pos;           // the entries, packed (compact)
  uint32_t* m_chunk;
  uint64_t* m_mask;          // one word per entry
};
hipError_t launch_set_verify_all(const SetAllArgs& a, hipStream_t s);
hipError_t launch_set_compact_all(const SetAllArgs& a, hipStream_t s);
// k_all_of_or / k_all_of_keep (xsg_list_kernels.hip), behind k_line_starts_keep and the exclusive prefix of its keep column:
// entry i lies in the line of ordinal keep_pre[i] + keep[i] - 1.  or: line_mask[ordinal] |= m_mask[i], one atomic per run
// of equal ordinals inside a wave; line_mask must be zero on entry (one word per kept entry at most: M words always do).
// keep: keep[i] &= line_mask[ordinal] == full.  The caller scans keep again behind it.
struct AllOfArgs {
  uint64_t M;                     // entries
  uint32_t* keep;                 // first entry of its line (k_line_starts_keep)
  const uint64_t* keep_pre;       // exclusive prefix of keep
  const uint64_t* m_mask;         // the literals that occur at entry i
  unsigned long long* line_mask;  // one word per line that holds an entry
  uint64_t full;                  // the mask of a line that holds every literal of the list
};
hipError_t launch_all_of_or(const AllOfArgs& a, hipStream_t s);
hipError_t launch_all_of_keep(const AllOfArgs& a, hipStream_t s);
// k_set_count_literals (xsg_count_literals*): k_set_scan's pass with the verify step inside it, one count per literal.  What
// it needs beyond ScanArgs travels as a second kernel parameter, so that every other kernel keeps its argument block.  The
// kernel ADDS to counts[0 .. nlits): the caller zeroes them on the stream in front of the launch, or accumulates.  One
// form: the sorted keys in LDS, a wave's candidates packed through LDS before they are verified.
struct LitCountArgs {
  unsigned long long* counts;  // device, one word per literal in listing order
  uint32_t nlits;              // literals of the list (SetProgram::count)
  uint32_t idx_off;            // byte offset of SetTable::idx inside PatternDev::d_pat (SetProgram::idx_offset)
};
hipError_t launch_set_count_literals(const ScanArgs& a, const LitCountArgs& c, hipStream_t s);
// k_set_count_literals_chunks (xsg_count_literals_chunks*): the same pass with the chunk boundaries kept.  The kernel ADDS
// to counts[c * nlits + j] and, where a word leaves 0, 1 to chunks_with[j]: the caller zeroes both on the stream in front
// of the launch.  forced_grid: XSG_LITMATRIX_GRID, 0 when unset (xsg_litmatrix.h: litmatrix_grid).
struct LitMatrixArgs {
  unsigned long long* counts;       // device, nchunks x nlits words, row-major by chunk
  unsigned long long* chunks_with;  // device, one word per literal, or null: not wanted
  uint32_t nlits;                   // literals of the list (SetProgram::count)
  uint32_t idx_off;                 // byte offset of SetTable::idx inside PatternDev::d_pat
  uint32_t touched;                 // the flush walks the touched list (XSG_LITMATRIX_TOUCHED=0: it always sweeps)
};
hipError_t launch_set_count_literals_chunks(const ScanArgs& a, const LitMatrixArgs& c, uint32_t forced_grid, hipStream_t s);
unsigned set_litmatrix_grid(const ScanArgs& a, uint32_t forced);  // the workgroups that launch would use
// k_set_count_literals_csr<ICASE, FILL, WORDS> and k_set_csr_seam<FILL> (xsg_count_literals_csr*): the matrix in CSR form, in two
// passes of the same partition around a prefix sum.  The count pass (FILL = false) stores row_nnz[c] for
// the chunks a workgroup owns alone and sums the others' rows in `seam`, whose non-zeros the seam kernel counts; the fill
// pass writes cols / vals at row_ptr[c] + rank, every store guarded by cap_entries, and the seam kernel does the same for
// the seam rows and writes *status.  The caller zeroes row_nnz (nchunks words) and seam (grid x nlits words) on the stream
// in front of the count pass and scans row_nnz into row_ptr between the passes; `grid` is set_litcsr_grid's for both.
struct LitCsrArgs {
  uint32_t* row_nnz;            // device, one word per chunk
  unsigned long long* seam;     // device, grid x nlits words: row `slot` is the seam chunk's that starts in that range
  const uint64_t* row_ptr;      // device, nchunks + 1 words (fill pass)
  uint32_t* cols;               // device, cap_entries words (fill pass)
  unsigned long long* vals;     // device, cap_entries words (fill pass)
  uint64_t cap_entries;
  uint64_t* status;             // device, one word (fill pass): XSG_STATUS_OVERFLOW iff row_ptr[nchunks] > cap_entries
  uint64_t nchunks;
  uint32_t nlits;               // literals of the list (SetProgram::count)
  uint32_t idx_off;             // byte offset of SetTable::idx inside PatternDev::d_pat
  uint32_t touched;             // the flushes walk the touched list (XSG_LITMATRIX_TOUCHED=0: they always sweep)
};
unsigned set_litcsr_grid(const ScanArgs& a, uint32_t nlits, uint32_t forced);  // 0: the binding has no tile
hipError_t launch_set_count_literals_csr(const ScanArgs& a, const LitCsrArgs& c, uint32_t grid, bool fill, hipStream_t s);
// k_set_find_literals<ICASE, FILL, WORDS> and k_set_find_chunk_ptr (xsg_find_literals*): every occurrence of every literal as
// (position, listing index), sorted by (chunk, position, listing index), in two passes of one grid-stride loop around a
// prefix sum (xsg_litfind.h).  The count pass (FILL = false) writes wave_occ[4 * tile + wave], every word;
// the caller scans them into wave_off (4 * ntiles + 1 words), launch_set_find_chunk_ptr gathers chunk_ptr from it and
// writes *status, and the fill pass stores pos / lit below cap_entries.  Nothing needs a memset.
struct LitFindArgs {
  uint32_t* wave_occ;        // device, 4 * ntiles words: the occurrences of every wave span
  const uint64_t* wave_off;  // device, 4 * ntiles + 1 words: their exclusive prefix (fill pass)
  uint64_t* pos;             // device, cap_entries words: global_offset(c) + p (fill pass)
  uint32_t* lit;             // device, cap_entries words: the listing index (fill pass)
  uint64_t cap_entries;
  uint32_t idx_off;          // byte offset of SetTable::idx inside PatternDev::d_pat
};
unsigned set_litfind_grid(const ScanArgs& a, uint32_t forced);  // forced: XSG_LITFIND_GRID, 0 when unset; 0 tiles: 0
hipError_t launch_set_find_literals(const ScanArgs& a, const LitFindArgs& f, uint32_t forced_grid, bool fill, hipStream_t s);
// chunk_ptr[c] = wave_off[4 * chunk_tile0[c]] for c in [0, nchunks]; *status (optional) = XSG_STATUS_OVERFLOW iff
// chunk_ptr[nchunks] > cap_entries
hipError_t launch_set_find_chunk_ptr(const ScanArgs& a, const uint64_t* wave_off, uint64_t* chunk_ptr, uint64_t cap_entries,
                                     uint64_t* status, hipStream_t s);
// "xsg::k_scan<KIND, WANT_NL, WANT_LINES, EMIT, LOADS, ICASE>" + the stagger launch_scan would use, for reports
// finishing: the caller's pass is a plain match count that takes the finishing form where scan_finishing says so;
// spans: that form would run with the binding's span locator (GateFinArgs::spans); waves: and as the wave form, taking
// `batch` groups at a time (GateFinArgs::batch); planes: selecting from the sketch's bit planes (GateFinArgs::planes)
void describe_scan(const ScanArgs& a, bool want_nl, bool want_lines, bool emit, char* out, size_t cap,
                   bool finishing = false, uint64_t total_bytes = 0, bool spans = false, bool waves = false, uint32_t batch = 1,
                   bool planes = false);

// exclusive scan: out[i] = sum_{k<i} in[k] for i in [0, n]; out has n+1 entries.
// tmp must hold scan_tmp_elems(n) uint64 values.
uint64_t scan_tmp_elems(uint64_t n);
hipError_t launch_exclusive_scan_u32(const uint32_t* in, uint64_t* out, uint64_t n, uint64_t* tmp, hipStream_t s);
hipError_t launch_exclusive_scan_u64(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tmp, hipStream_t s);

// ---- the one-sync list route (xsg_list.cpp: run_list_fast) ---------------------------------------------------
// Every size the host used to fetch between the stages of a list search (raw occurrences, kept ones, tail matches,
// line bytes) stays on the device: arrays have CAPACITIES, kernels read the counts they need from this block of
// device words and bound themselves by the capacities, and the kernels that produce a count also store it in a
// pinned host mirror.  The host syncs once, at the end, and reads the mirror; kTotOverflow != 0 means a capacity
// was too small and the search is repeated on the exact route (which sizes every array from a fetched count).
enum FastTot : int {
  kTotRaw = 0,        // raw bulk occurrences = sum of tile_cnt
  kTotHits = 1,       // tiles that hold at least one
  kTotKept = 2,       // raw occurrences the reference walk reports
  kTotFinal = 3,      // kept + end-of-chunk matches = length of the list
  kTotNewlines = 4,   // '\n' in the shard (xs::line_indices)
  kTotLineBytes = 5,  // xs::lines: packed bytes
  kTotOverflow = 6,   // != 0: some capacity was exceeded (bit 0 raw, 1 list, 2 line bytes)
  kTotWords = 8
};

// exclusive prefix sums in two launches with the count on the device: k_scan2_a (block sums; the last workgroup to
// arrive scans them and publishes the total), k_scan2_b (writes out[0..n)); out[n] = total.
struct Scan2Args {
  const void* in;          // uint32 or uint64 (UINT64_MAX scans as 0: dropped lines)
  uint64_t* out;           // n + 1 entries
  uint64_t n_cap;          // the grids cover this many entries
  const uint64_t* n_dev;   // optional: n = min(*n_dev, n_cap); null: n = n_cap
  uint64_t* blk;           // scratch: 2 x (blocks + 1) words
  uint32_t* ticket;        // zero at rest
  uint64_t* tot_dev;       // optional: the grand total (device word) ...
  uint64_t* tot_host;      // ... and its pinned mirror
  // HITS: the ordered list of indices with a non-zero entry
  uint32_t* hit_idx;
  uint64_t hit_cap;
  uint64_t* hits_dev;
  uint64_t* hits_host;
  uint64_t* ovf_dev;       // optional: |= ovf_bit when the total exceeds total_cap (or the hits exceed hit_cap)
  uint64_t* ovf_host;
  uint64_t total_cap;
  uint64_t ovf_bit;
  uint32_t ovf_init;       // the first producer of a search: the overflow word is STORED (bit or 0), not OR-ed into
};
uint64_t scan2_tmp_elems(uint64_t n_cap);
hipError_t launch_scan2_u32(const Scan2Args& a, bool hits, hipStream_t s);
hipError_t launch_scan2_u64(const Scan2Args& a, hipStream_t s);

struct ListArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint64_t* chunk_tile0;
  uint64_t nchunks;
  PatternDev pat;
  uint64_t M;                // raw matches (bulk, o < limit), ascending per chunk
  const uint64_t* M_dev;     // if set: the number lives on the device (tile_off[ntiles]); M is then the CAPACITY of the
                             // arrays and the kernels work on min(*M_dev, M) entries (xsg_count_async, bordered patterns)
  const uint64_t* m_pos;     // chunk-local offsets
  const uint32_t* m_chunk;
  const uint32_t* m_len;     // kDfa, XSG_MATCHES: length of every raw match (ScanArgs::m_len); null otherwise
  const uint64_t* tile_off;  // -> first raw index of each chunk = tile_off[chunk_tile0[c]]
  uint64_t* m_ls;            // line start per raw match (line modes)
  uint32_t* keep;            // 1 = survives the walk (greedy / first in line)
  const uint64_t* keep_pre;  // exclusive prefix of keep (M + 1 entries)
  uint64_t* chunk_shift0;    // per chunk: where the reference walk enters the tail zone
  uint32_t* tail_cnt;        // per chunk
  uint64_t* tail_pos;        // per chunk x tail_cap: chunk-local match offsets from the tail walk
  uint32_t tail_cap;
  const uint64_t* tail_pre;  // exclusive prefix of tail_cnt (nchunks + 1)
  uint32_t line_mode;        // 0: matches, 1: lines (skip_to_nl)
  // final list
  uint64_t* f_pos;    // chunk-local: match offset (match mode) or line start (line modes)
  uint64_t* f_match;  // chunk-local offset of the (first) match of that line
  uint32_t* f_chunk;
  uint32_t* f_len;    // k_assemble, XSG_MATCHES on the automaton routes: m_len of the entry (null otherwise)
  uint64_t total;
  // one-sync route
  uint32_t keep_all;         // every raw occurrence is reported (no keep[] / keep_pre[]: entry i stays entry i)
  uint64_t* tot_dev;         // FastTot words
  uint64_t* tot_host;        // pinned mirror
  uint32_t* ticket;          // zero at rest
  uint64_t f_cap;            // entries f_pos / f_match / f_chunk / out arrays can hold
  uint64_t* out_u64;         // k_list_out: global offset of every final entry (match / line-start tags) ...
  uint64_t* out_host;        // ... and its pinned mirror (may be null)
  uint32_t want_f;           // k_list_out: also write f_pos / f_match / f_chunk (line indices, lines)
  uint32_t* long_flag;       // k_greedy_keep: if set, a chain over its budget is left unfinished and this word raised
  uint64_t* line_len;        // k_list_out, xs::lines: length of every final entry's line (UINT64_MAX: unterminated -> dropped) ...
  uint64_t* line_len_host;   // ... and its pinned mirror
};

// mask[tile of the line start] = 1 for every kept entry of a candidate list (ListArgs after launch_line_starts_keep)
hipError_t launch_rx_mark_tiles(const ListArgs& a, uint32_t* mask, hipStream_t s);
hipError_t launch_greedy_keep(const ListArgs& a, hipStream_t s);
// long chains: J[i] = nxt(i) (uint32 index or 0xffffffff), then rounds of "mark J(marked), square J" until *changed stays 0
hipError_t launch_greedy_links(const ListArgs& a, uint32_t* J, hipStream_t s);
hipError_t launch_greedy_jump(const ListArgs& a, const uint32_t* J, uint32_t* J2, uint32_t* changed, hipStream_t s);
// line tags of a literal that contains '\n': line start of every raw occurrence, the chunk heads, and the links of the
// reference's walk (next = the first occurrence behind the first '\n' at or behind this one's end)
hipError_t launch_nlpat_links(const ListArgs& a, uint32_t* J, hipStream_t s);
hipError_t launch_line_starts_keep(const ListArgs& a, hipStream_t s);
hipError_t launch_keep_all(const ListArgs& a, hipStream_t s);
hipError_t launch_chunk_shift0(const ListArgs& a, hipStream_t s);
hipError_t launch_tail_list(const ListArgs& a, hipStream_t s);
hipError_t launch_assemble(const ListArgs& a, hipStream_t s);
// counters[XSG_CTR_MATCHES] = sum of keep[0..M) + sum of tail_cnt, counters[XSG_CTR_BYTES] = total_bytes, the other two 0;
// all four UINT64_MAX if *M_dev exceeds the capacity (the caller falls back to the synchronous route) or the scan
// raised flags bit 0 (ascii_only expression on non-ASCII data).  counters must be zero on entry.
// status (optional): as FinishArgs::status
hipError_t launch_bordered_total(const ListArgs& a, uint64_t* counters, uint64_t total_bytes, uint32_t* flags, uint64_t* status,
                                 hipStream_t s);
// one-sync route: chunk_shift0 + tail walk by one wave per chunk, the prefix of the tail counts and kTotFinal by the
// last workgroup to arrive; then the final list (k_assemble + k_globalize in one)
hipError_t launch_chunk_tail(const ListArgs& a, hipStream_t s);
hipError_t launch_list_out(const ListArgs& a, hipStream_t s);

struct LineOutArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint64_t* chunk_tile0;
  uint64_t nchunks;
  PatternDev pat;
  uint64_t total;
  const uint64_t* f_pos;
  const uint64_t* f_match;
  const uint32_t* f_chunk;
  const uint32_t* f_len;  // k_match_spans: length of every entry's match; null: pat.plen (a literal, a class sequence)
  uint64_t* out_u64;  // global offsets or line indices
  // line indices
  const uint64_t* tile_nl_off;  // exclusive prefix of tile_nl over all tiles of the shard
  uint32_t tile_bytes;
  uint64_t shard_line_base;
  // lines
  uint64_t* line_len;  // length without '\n'; UINT64_MAX marks "no terminating newline" (dropped)
  const uint64_t* line_out_off;
  uint8_t* line_bytes;
  // one-sync route: `total` is the capacity, the length of the list is tot_dev[kTotFinal]
  const uint64_t* tot_dev;
  uint64_t* out_host;        // pinned mirror of out_u64 (may be null)
  uint64_t* line_len_host;   // pinned mirror of line_len (xs::lines)
  uint8_t* line_bytes_host;  // pinned mirror of line_bytes
  uint64_t line_bytes_cap;   // bytes line_bytes (and its mirror) can hold
  uint32_t* dropped;         // k_line_lengths: incremented per line without a terminating newline (may be null)
  uint64_t slice_begin, slice_end;  // k_line_gather: only the entries [slice_begin, slice_end) (slice_end == 0: all of them)
  uint32_t* edge_units;      // k_line_gather_span into a pinned mirror: 4 zeroed words per workgroup boundary (total / kBlock + 2), or null
  uint32_t invert;           // XSG_FLAG_INVERT: the entries are lines WITHOUT a match (f_match is not meaningful): k_line_lengths
                             // looks for the line's end from its start, not from behind a match
};
hipError_t launch_globalize(const LineOutArgs& a, hipStream_t s);
hipError_t launch_line_nl_delta(const LineOutArgs& a, hipStream_t s);
hipError_t launch_line_indices(const LineOutArgs& a, hipStream_t s);
hipError_t launch_line_lengths(const LineOutArgs& a, hipStream_t s);
hipError_t launch_line_gather(const LineOutArgs& a, hipStream_t s, bool short_strings = false);
// XSG_MATCHES: the matched text of every entry of a list assembled in match mode (f_pos = where the match starts).
// spans: line_len (never UINT64_MAX: a match always has a length), out_u64 and their pinned mirrors; the gather is
// launch_line_gather(.., short_strings = true)
hipError_t launch_match_spans(const LineOutArgs& a, hipStream_t s);

// ---- XSG_FLAG_INVERT: the complement stage (xsg_list.cpp: invert_list) ---------------------------------------------
// The assembled list of a line tag (r_pos / r_chunk: the chunk-relative starts of the lines the walk reports, ascending
// inside a chunk, in chunk order) is replaced by the list of all OTHER line starts of the chunks.  Two passes over the
// text, one workgroup per tile, around one prefix sum over the tiles; both passes decide a line start the same way (the
// tile's slice of the reported list as a bitmap in LDS), so the emit pass stores exactly what the count pass counted.
struct InvertArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint32_t* tile_chunk;   // tile -> chunk (null when the shard has one chunk)
  const uint64_t* chunk_tile0;
  uint64_t ntiles;
  uint32_t tile_bytes;
  uint64_t total;               // entries of the reported list
  const uint64_t* r_pos;
  const uint32_t* r_chunk;
  uint64_t* tile_lo;            // ntiles + 1: the first reported entry at or behind the tile's first byte ([ntiles] = total)
  uint32_t* tile_cnt;           // line starts in the tile that are not reported
  const uint64_t* tile_off;     // exclusive prefix of tile_cnt (emit pass)
  uint64_t inv_total;           // its total = entries of i_pos / i_chunk
  uint64_t* i_pos;
  uint32_t* i_chunk;
};
hipError_t launch_invert_count(const InvertArgs& a, hipStream_t s);  // tile_lo, tile_cnt
hipError_t launch_invert_emit(const InvertArgs& a, hipStream_t s);   // i_pos, i_chunk
// XSG_COUNT_LINES: counters[XSG_CTR_LINES] = newlines + chunks whose last line lacks its '\n' - counters[XSG_CTR_LINES], behind
// a count pass that also counted newlines, on the same stream; a refusal (status word set, or poisoned counters) passes
// through.  keep_nl == 0: the caller did not ask for XSG_CTR_NEWLINES, it is zeroed again.  host_counters, status: optional
hipError_t launch_invert_count_lines(const uint8_t* base, const ChunkDev* chunks, uint64_t nchunks, uint64_t* counters,
                                     uint64_t* host_counters, const uint64_t* status, uint32_t keep_nl, hipStream_t s);
// ---- XSG_FLAG_CONTEXT: the widening stage (xsg_list.cpp: context_list) ----------------------------------------------
// The assembled (and possibly inverted) list of a line tag is replaced by the list of every line start whose index lies
// within `before` lines ahead of or `after` lines behind a reported line of the same chunk, each once, in file order.
// The line index (rank) of every entry comes from the newline prefix of the tiles plus the near/far count of the
// line-index passes (nl_before); k_context_spans turns the ranks into disjoint rank spans [lo, hi] per entry -- hi is
// monotone, so the previous entry's hi follows from its rank alone -- and one prefix sum over the span lengths gives
// every span its slots.  k_context_tile then selects: one workgroup per tile, which knows its own rank range from the
// newline prefix, finds the spans that touch it by binary search and leaves without a load if none does.
struct ContextArgs {
  const uint8_t* base;
  const ChunkDev* chunks;
  const uint32_t* tile_chunk;   // tile -> chunk (null when the shard has one chunk)
  const uint64_t* chunk_tile0;  // nchunks + 1 entries
  uint64_t nchunks;
  uint64_t ntiles;
  uint32_t tile_bytes;
  uint32_t before, after;
  const uint64_t* tile_nl_off;  // exclusive prefix of the newline counts of the tiles (ntiles + 1)
  uint64_t total;               // entries of the reported list
  const uint64_t* r_pos;
  const uint32_t* r_chunk;
  const uint64_t* nl_before;    // total + 1: [i + 1] = newlines of the shard before entry i's line start
  uint64_t* lo;                 // per entry: its span of chunk-local line indices; empty where lo > hi
  uint64_t* hi;
  uint32_t* cnt;                // its length
  const uint64_t* slot;         // exclusive prefix of cnt
  xsg_context_edge* edges;      // nchunks
  uint64_t out_total;           // slot[total] = entries of o_pos / o_chunk
  uint64_t* o_pos;
  uint32_t* o_chunk;
};
hipError_t launch_context_spans(const ContextArgs& a, hipStream_t s);  // edges, lo, hi, cnt
hipError_t launch_context_emit(const ContextArgs& a, hipStream_t s);   // o_pos, o_chunk
// one empty launch per kernel file (code object): see xsg_kernels.hip
hipError_t warm_scan_kernels(hipStream_t s);
hipError_t warm_list_kernels(hipStream_t s);
hipError_t warm_rx_kernels(hipStream_t s);
hipError_t warm_set_kernels(hipStream_t s);
// one-sync route: the line index of every entry by one wave per entry (sparse lists: no prefix pass over the entries)
hipError_t launch_line_index_waves(const LineOutArgs& a, hipStream_t s);

}  // namespace xsg
