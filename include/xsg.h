/*
 * xsg.h -- C ABI of the MI355X literal-scan engine (libxsg.so).
 *
 * This is the drop-in boundary for the hot path of lfreist/x-search: the
 * per-chunk literal search that the reference implements in
 *   src/string_search/simd_search.cpp                       (AVX2 primitives)
 *   include/xsearch/string_search/search_wrappers.h:29-207  (per-chunk walks)
 * and calls from the task functors include/xsearch/tasks/searchers.h:38-93
 * inside the worker loop include/xsearch/Searcher.h:100-120.  With
 * XSG_FLAG_REGEX the same entry points stand in for the regex walks
 * (search_wrappers.h:63-103, 209-271) on fixed-length class-sequence expressions.
 *
 * Everything here is plain C: opaque handles, pointers and sizes.  No torch
 * or C++ types cross this boundary.  The C++ surface the reference's users see
 * (xs::extern_search<Tag>(...)->join()/getResult()) is the header-only layer
 * include/xsearch/xsearch.h on top of this ABI; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Results are bit-identical to the reference's CPU path on the same chunk
 * bytes, including its end-of-chunk behaviour (see XSG_FLAG_EXACT_TAIL).
 *
 * Threading: a ctx may be used from several host threads as long as each
 * thread works on its own shard; calls on ONE shard must not overlap.
 * All functions return XSG_OK (0) or a negative XSG_E* code;
 * xsg_last_error() gives the message of the calling thread's last failure.
 * There is NO CPU fallback: without a usable HIP device every compute entry
 * point fails with XSG_ENODEV.
 */
#ifndef XSG_H
#define XSG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: xsg_shard_invalidate and xsg_result_lines_view joined (round 3); 4: xsg_count_async_status joined, XSG_MAX_PATTERN
 * grew and the line tags accept a literal that contains '\n' (round 4); still 4: XSG_FLAG_INVERT, XSG_MATCHES,
 * XSG_FLAG_CONTEXT and xsg_result_context_edges joined; xsg_set_literals, xsg_literals_info, xsg_host_searcher_create_list
 * and xsg_job_opts.pattern_is_list joined (the structure grew: see there for what that asks of a program built before);
 * xsg_count_chunks and xsg_count_chunks_async joined; xsg_count_literals, xsg_count_literals_async and xsg_literal_counter_*
 * joined; xsg_count_literals_chunks, xsg_count_literals_chunks_async and xsg_literals_chunks_touched_capacity joined;
 * xsg_count_literals_csr, xsg_result_literals_csr and xsg_count_literals_csr_async joined; XSG_LIST_WHOLE_WORDS with
 * xsg_set_literals_opts, xsg_host_searcher_create_list_opts, xsg_literal_counter_create_opts and xsg_job_start_list joined;
 * xsg_find_literals, xsg_result_literal_hits, xsg_find_literals_async and xsg_literal_finder_* joined;
 * XSG_LIST_ALL_OF joined the list_flags of xsg_set_literals_opts, xsg_host_searcher_create_list_opts and xsg_job_start_list;
 * xsg_result_chunk_ptr and xsg_fileset_* joined; xsg_set_max_count, xsg_job_start_max_count, xsg_fileset_start_max_count and
 * xsg_host_searcher_set_max_count joined;
 * no entry point was removed or changed in meaning */
#define XSG_ABI_VERSION 4

/* ---- status codes ------------------------------------------------------- */
#define XSG_OK 0
#define XSG_EINVAL (-1)   /* bad argument (empty pattern, misaligned chunk, ...) */
#define XSG_ENODEV (-2)   /* no HIP device / device index out of range */
#define XSG_EHIP (-3)     /* a HIP runtime call failed (message has the HIP error) */
#define XSG_ENOMEM (-4)   /* host or device allocation failed */
#define XSG_ENOTSUP (-5)  /* valid request this entry point cannot serve (see docs) */
#define XSG_EIO (-6)      /* file open/read/parse failure */
#define XSG_ESTATE (-7)   /* call sequence error (e.g. result fetched before search) */

/* ---- what to compute: one value per xs:: tag ----------------------------- */
/* README.md:71-81 / test/src/xsearchTest.cpp:344 name the tags; the function
 * of search_wrappers.h each one maps to is given on the right. */
enum xsg_mode {
  XSG_COUNT_MATCHES = 0,      /* xs::count, xs::count_matches -> search::count(data, p, false)   (:163-185) */
  XSG_COUNT_LINES = 1,        /* xs::count_lines              -> search::count(data, p, true)    (:163-185) */
  XSG_MATCH_BYTE_OFFSETS = 2, /* xs::match_byte_offsets       -> search::byte_offsets_match      (:136-139) */
  XSG_LINE_BYTE_OFFSETS = 3,  /* xs::line_byte_offsets        -> search::byte_offsets_line       (:149-154) */
  XSG_LINE_INDICES = 4,       /* xs::line_indices             -> (no reference impl)     */
  XSG_LINES = 5,              /* xs::lines                    -> search::line                    (:187-207) */
  XSG_MATCHES = 6             /* xs::matches                  -> the matched text (grep -o); no reference impl, see below */
};
/* XSG_MATCHES: what matched, not only where.  Let M be the list XSG_MATCH_BYTE_OFFSETS reports for the same binding,
 * pattern and flags -- the default lossy end-of-chunk behaviour included, lifted by XSG_FLAG_EXACT_TAIL.  XSG_MATCHES
 * reports, for every element of M and in the same order, the bytes [start, start + len) of the chunk, where len is
 *   the pattern length                      for a literal,
 *   the number of positions                 for a fixed-length class sequence (XSG_FLAG_REGEX),
 *   the length of the leftmost-first match  on the automaton route
 * -- the same len the walk uses as its resume point; under the (?m)...$ form the '\n' is not part of the match.  The
 * bytes are the ORIGINAL ones: under XSG_FLAG_IGNORE_CASE the text keeps its case, as for XSG_LINES.  A literal or an
 * expression that can match '\n' is served (the match tags serve it); the strings then contain newlines, which is why
 * lengths are reported.  Nothing is dropped: |M| strings come out, a match at a chunk's end that no '\n' follows
 * included (a match always has a length; UINT64_MAX never appears among the lengths).  A match is shorter than 4 GiB:
 * an expression whose matches vary in length is refused (XSG_ENOTSUP) on a binding with a chunk of 4 GiB or more.
 * XSG_FLAG_INVERT refuses this tag as it refuses the other two match tags (XSG_ENOTSUP); the non-ASCII refusal of '.'
 * and negated classes is unchanged; the count entry points do not take it (XSG_EINVAL, as for any list mode).
 * Results: xsg_search sets *n_results = |M|; xsg_result_lines_size / xsg_result_lines / xsg_result_lines_view hand
 * out the lengths, the packed bytes and, in `offsets`, global_offset + start of every match.  Every other accessor
 * behaves after an XSG_MATCHES search as after an XSG_LINES search. */

/* ---- pattern flags ------------------------------------------------------- */
/* Default (0): reproduce the reference exactly, including the lossy scalar
 * search it applies to the last <plen+32 bytes of every chunk
 * (simd_search.cpp:58-78,203).  With XSG_FLAG_EXACT_TAIL every occurrence in
 * the chunk is reported (what the reference intends). */
#define XSG_FLAG_EXACT_TAIL 0x1u
/* ASCII case-insensitive search (the `ignore_case` argument of xs::extern_search,
 * example/grep.cpp:69, test/src/xsearchTest.cpp:350).  The snapshot holds no
 * implementation of the case-insensitive wrappers; the semantics here are the
 * reference's building block applied to both sides: simd::toLower
 * (src/utils/string_utils.cpp:11-33: 'A'..'Z' += 32, other bytes unchanged) on
 * the chunk and on the pattern, then the normal search.  That is also exactly
 * what the reference's own (uncalled) case-insensitive primitive computes:
 * simd::strcasestr (src/string_search/simd_search.cpp:220-287) returns the same
 * offset as strstr on the lowered chunk and pattern, end-of-chunk behaviour
 * included (checked on the compiled reference, tests/test_oracle_golden.py).
 * Offsets are unchanged and xs::lines returns the ORIGINAL bytes (goldens keep
 * their case, test/src/xsearchTest.cpp:227-240). */
#define XSG_FLAG_IGNORE_CASE 0x2u
/* The pattern is a regular expression.  The reference hands a pattern that "does
 * not match itself as a regex" (include/xsearch/utils/utils.h:17-25) to RE2 and
 * walks the chunk with RE2::PartialMatch
 * (include/xsearch/string_search/search_wrappers.h:63-87,209-271).  Served here,
 * decided position by position in the scan kernel: alternations of fixed-length
 * sequences of byte classes -- literals, [ASCII classes] incl. [:alpha:] & co,
 * \d \w \s, escapes, x{n}, groups ( ) (?: ), `a|b` at any depth as long as all
 * alternatives of the whole expression have one length (then leftmost-first has
 * nothing to choose) -- which covers every regex the reference's tests use
 * (`She[r ]lock`, test/src/xsearchTest.cpp:9; `(a[n|m]t)`,
 * test/src/string_search/search_wrappersTest.cpp:78).  Up to 32 positions, 8
 * alternatives, 64 sets in all.
 * '.', negated classes and \D \W \S are accepted with their ASCII meaning ('.' =
 * any ASCII byte but '\n'); RE2 matches whole code points there, so a search with
 * such an expression REFUSES data that holds a byte >= 0x80 (XSG_ENOTSUP from the
 * search call; xsg_count_async hands out UINT64_MAX in all four counters) rather
 * than decide it differently.
 * Expressions of VARIABLE length -- x* x+ x? x{n,} x{n,m}, the lazy forms, alternatives
 * of different lengths, more than 32 positions or 8 alternatives -- take a second
 * route: a forward leftmost-first DFA and a reverse longest-match DFA (what RE2
 * itself runs for such a search), compiled on the host, and a kernel that walks every
 * line of the shard with them, one line per lane (csrc/xsg_regex.h,
 * csrc/xsg_rx_kernels.hip).  All six tags; same refusal of non-ASCII data for '.'
 * and negated classes.  An expression of this kind whose sets accept '\n' (\s+,
 * [^,]*) can match across lines: it is walked chunk by chunk, one lane per chunk
 * (slow), and serves XSG_COUNT_MATCHES / XSG_MATCH_BYTE_OFFSETS only.  Refused on
 * this route (XSG_ENOTSUP from xsg_set_pattern, never approximated): expressions
 * that can match the empty string, automata over 16384 table entries.  Refused on both routes: anchors ^ $ \b \A \z, (?flags), \p, \C
 * -- except LINE ANCHORS in RE2's multi-line form  (?m) [^] BODY [$] : `(?m)` as the first four bytes, `^` as the next
 * token, `$` as the last, BODY any expression served above with no top-level `|` (write (?m)^(?:a|b)$), no set that
 * accepts '\n' and no empty match.  `^` holds at a line start and at the walk's resume point (in the match tags
 * (?m)^ab on "abab" matches at 0 and 2, as the reference computes), `$` at a line end; a chunk's edges are line edges
 * and the bytes beyond them are never read.  Such an expression is searched by the automaton route's line walks, all
 * six tags; xsg_regex_check / xsg_regex_info describe BODY.  (?m) with neither anchor is BODY's search.  Anchors or
 * flags anywhere else, (?m:...), (?mi) and the plain ^ $ stay refused.
 * CAPTURE GROUPS: the reference's walk is RE2::PartialMatch(input, pattern, &match) (search_wrappers.h:71-75,
 * 254-257), where `match` receives capture group ONE; its tests hand over an expression that IS one group,
 * re2::RE2("(a[n|m]t)") (test/src/string_search/search_wrappersTest.cpp:78).  XSG_FLAG_REGEX(expr) is that call with
 * "(" + expr + ")": offset, length and resume point are those of the WHOLE match; groups inside `expr` only group
 * (`Sher(lock|wood)` reports where `Sher` starts, not where `lock` does; an expression the caller already wrapped,
 * `(a[n|m]t)`, is the same search).  A maintainer who binds this flag passes the expression without relying on an inner
 * group being reported (tests/test_oracle_regex.py::test_the_whole_match_is_group_one_of_the_wrapped_expression).
 * No tail quirk applies (RE2 is exact); XSG_FLAG_IGNORE_CASE folds ASCII letters in
 * the data and in every class, as for literals (automaton route: the classes are
 * closed under case instead, the same thing). */
#define XSG_FLAG_REGEX 0x4u
/* Inverted line search (grep -v): the line tags report the lines WITHOUT a match.  May be combined with any flag above.
 * The lines of a chunk of `len` bytes start at offset 0 (if len > 0) and at p + 1 for every '\n' at p with p + 1 < len:
 * "a\nb" has two lines, "a\n" one, "a\n\n" two (the second is empty), "" none; the last line is TERMINATED if the
 * chunk ends in '\n'.  Let R be the line starts XSG_LINE_BYTE_OFFSETS reports for the same pattern and the same other
 * flags without this one -- the default lossy end-of-chunk behaviour included: a line whose only occurrence the
 * reference loses there counts as not matching unless XSG_FLAG_EXACT_TAIL is set.  The inverted set is
 * I = lines(chunk) \ R, in file order, and with the flag set
 *   XSG_COUNT_LINES        counts |I| over the chunks into XSG_CTR_LINES (every count entry point; XSG_CTR_NEWLINES,
 *                          XSG_CTR_BYTES, the status word and the UINT64_MAX refusal are as without the flag),
 *   XSG_LINE_BYTE_OFFSETS  lists global_offset + start of every line of I,
 *   XSG_LINE_INDICES       lists their line indices (line bases and xsg_result_newlines as without the flag),
 *   XSG_LINES              hands out the lines of I that are terminated, without their '\n' (the reference never hands
 *                          out a last line that lacks its newline); a rare needle's inverted result is the whole text,
 *   XSG_COUNT_MATCHES, XSG_MATCH_BYTE_OFFSETS  are refused (XSG_ENOTSUP): a non-match has no offset.
 * A pattern that can match '\n' (a literal that contains one, an expression whose sets accept one) is refused with
 * XSG_ENOTSUP by xsg_set_pattern -- the context then holds no pattern -- never approximated.  The complement is taken on
 * the device from the assembled list of matching lines (csrc/xsg_list_kernels.hip: k_invert_tile); the scan kernels
 * are the ones of the plain search. */
#define XSG_FLAG_INVERT 0x8u
/* Context lines (grep -B before -A after): the line-LIST tags also report the lines around every reported line.  The
 * two counts ride in the pattern flags (bits 8-19: before, bits 20-31: after; bits 4-7 stay unknown flags, XSG_EINVAL),
 * so they pass through xsg_set_pattern, xsg_job_opts.pattern_flags and xsg_host_searcher_create.  The macro masks: a
 * caller that takes the numbers from a user refuses values above XSG_CONTEXT_MAX itself.  XSG_FLAG_CONTEXT(0, 0) == 0 is
 * the plain search.  May be combined with every flag above.
 * The lines of a chunk and their indices are the ones defined under XSG_FLAG_INVERT (index 0 is the line at offset 0).
 * Let R be the lines XSG_LINE_BYTE_OFFSETS reports for the same pattern and the same other flags -- XSG_FLAG_INVERT
 * included if set (context around the NON-matching lines, grep -v -C), and the default lossy end-of-chunk behaviour
 * included.  With B = XSG_CONTEXT_BEFORE(flags), A = XSG_CONTEXT_AFTER(flags) and n the chunk's line count
 *   C = { q : 0 <= q < n and some r in R of the same chunk has r - B <= q <= r + A },
 * every line of C once, in file order.  A chunk is searched on its own: context is cut at the chunk's edges.
 *   XSG_LINE_BYTE_OFFSETS  lists global_offset + start of every line of C,
 *   XSG_LINE_INDICES       lists their indices (line bases and xsg_result_newlines as without the bits),
 *   XSG_LINES              hands out the lines of C that are terminated, without their '\n'; a line's end is looked for
 *                          from its start, and an unterminated last line is dropped, as always,
 *   everything else        ignores the bits (as grep -c -C and grep -o -C do): XSG_COUNT_MATCHES, XSG_COUNT_LINES, every
 *                          count entry point, XSG_MATCH_BYTE_OFFSETS, XSG_MATCHES.
 * A pattern that can match '\n' is refused with XSG_ENOTSUP by xsg_set_pattern when A or B is non-zero -- the context
 * then holds no pattern -- exactly as under XSG_FLAG_INVERT.  The host-only inspection calls (xsg_regex_check,
 * xsg_regex_info, xsg_regex_dfa_info, xsg_regex_prefix, xsg_regex_factor) accept and ignore the bits.  The list is
 * widened on the device behind the assembled (and possibly inverted) list (csrc/xsg_list_kernels.hip: k_context_tile),
 * on the exact list route; the scan kernels are the ones of the plain search. */
#define XSG_CONTEXT_MAX 4095u
#define XSG_FLAG_CONTEXT(before, after) ((((uint32_t)(before)) & 0xfffu) << 8 | (((uint32_t)(after)) & 0xfffu) << 20)
#define XSG_CONTEXT_BEFORE(flags) (((flags) >> 8) & 0xfffu)
#define XSG_CONTEXT_AFTER(flags) (((flags) >> 20) & 0xfffu)

/* A literal may be up to 32 KiB long (the reference's walk takes any std::string; what bounds it here is one 16-bit
 * field: the end of a tile's last match, relative to the tile, must stay below 2^16).  The scan kernel keeps the first
 * KiB of a long pattern in LDS and verifies the rest of a candidate from the device copy of the pattern.  A regular
 * expression (XSG_FLAG_REGEX) is at most XSG_MAX_REGEX bytes of text. */
#define XSG_MAX_PATTERN 32768u
#define XSG_MAX_REGEX 1024u
/* A literal LIST (xsg_set_literals): at most XSG_MAX_PATTERN bytes in all, XSG_MAX_LITERALS literals, each of
 * 1..XSG_MAX_LITERAL_BYTES bytes. */
#define XSG_MAX_LITERALS 4096u
#define XSG_MAX_LITERAL_BYTES 255u

/* ---- counters written by the count entry points --------------------------- */
#define XSG_CTR_MATCHES 0  /* XSG_COUNT_MATCHES result */
#define XSG_CTR_LINES 1    /* XSG_COUNT_LINES result   */
#define XSG_CTR_NEWLINES 2 /* number of '\n' in the shard (only if requested) */
#define XSG_CTR_BYTES 3    /* bytes scanned */
#define XSG_NUM_COUNTERS 4

/* OR into `mode` of the count entry points to also count '\n' (needed to
 * derive line-index bases across GPUs). */
#define XSG_WITH_NEWLINES 0x100u

/* line_base value meaning "derive from the preceding chunks of this shard" */
#define XSG_LINE_BASE_AUTO UINT64_MAX

typedef struct xsg_ctx xsg_ctx;     /* one per (process, device): streams, pattern, scratch */
typedef struct xsg_shard xsg_shard; /* a set of chunks resident in device memory */

/* A chunk = what the reference's reader hands to a searcher functor
 * (tasks/readers.h:39-48 -> tasks/searchers.h:49): a run of bytes that is
 * searched on its own.  No match or line spans two chunks. */
typedef struct xsg_chunk {
  uint64_t offset;        /* byte offset of the chunk inside the shard buffer; multiple of 16 */
  uint64_t length;        /* chunk length in bytes (< 2^40) */
  uint64_t global_offset; /* offset of the chunk in the (uncompressed) file: added to every reported byte offset */
  uint64_t line_base;     /* number of '\n' in the file before this chunk, or XSG_LINE_BASE_AUTO */
} xsg_chunk;

/* ---- library ------------------------------------------------------------- */
int xsg_abi_version(void);
const char* xsg_strerror(int code);
const char* xsg_last_error(void);
int xsg_device_count(int* count);

/* ---- context -------------------------------------------------------------- */
int xsg_ctx_create(int device, xsg_ctx** out);
void xsg_ctx_destroy(xsg_ctx* ctx);
/* Literal pattern, 1..XSG_MAX_PATTERN bytes, any byte values (or, with
 * XSG_FLAG_REGEX, a regular expression of the families above, at most XSG_MAX_REGEX bytes).  A LITERAL that contains
 * '\n' is served by every tag: the reference's line walk (search_wrappers.h:29-50,163-207: after a match, on to the
 * first '\n' at or behind its end) is then a chain from occurrence to occurrence, resolved on the device; the line
 * it reports for a match begins behind the last '\n' before the match (at the byte after the match's first byte if
 * that byte is a '\n' itself: previous_new_line_offset_relative_to_match, :111-123) and ends at the first '\n' at or
 * behind the match's end -- so xs::lines hands out strings that contain newlines.  xsg_count_async does not serve
 * XSG_COUNT_LINES for such a pattern (XSG_ENOTSUP: use xsg_count).  A regular EXPRESSION that can match '\n' keeps
 * to XSG_COUNT_MATCHES / XSG_MATCH_BYTE_OFFSETS (the line modes return XSG_ENOTSUP for it). */
int xsg_set_pattern(xsg_ctx* ctx, const void* pattern, size_t plen, uint32_t flags);
/* A LIST of literals as the pattern (grep -F -e a -e b, grep -F -f words.txt): the counterpart of xsg_set_pattern, and
 * like it a failed call leaves the context without a pattern.  `list` holds the literals l1 .. lk separated by '\n' --
 * the format of a grep -f file; one final '\n' is allowed.  Limits (XSG_EINVAL, never approximated): 1..XSG_MAX_PATTERN
 * bytes in all, 1..XSG_MAX_LITERALS literals, each 1..XSG_MAX_LITERAL_BYTES bytes of any value but '\n'; an EMPTY literal
 * ("a\n\nb", a leading '\n') is refused: grep lets it match every line, and that is not served.  Duplicates are allowed.
 * Under flags F the search is BY DEFINITION the one XSG_FLAG_REGEX | F performs for esc(l1)|esc(l2)|...|esc(lk), esc
 * backslash-escaping ASCII punctuation -- for every tag and every other flag, without that route's size limits and
 * without RE2's code-point reading (a literal is bytes).  That is:
 *   leftmost-first  at the leftmost position where any literal occurs, the FIRST-LISTED literal that occurs there is the
 *                   match (("ab","abc") on "abcd" matches "ab"; GNU grep -o would print the longest), and the walk
 *                   resumes at its end; XSG_MATCHES reports that literal's bytes and length;
 *   exact           up to the chunk's end, as the regex routes are: XSG_FLAG_EXACT_TAIL is accepted and changes nothing;
 *   XSG_FLAG_IGNORE_CASE folds ASCII letters on both sides, reported bytes keep their case;
 *   XSG_FLAG_INVERT, XSG_FLAG_CONTEXT work as for any pattern that cannot match '\n' (a list never can);
 *   XSG_FLAG_REGEX  together with a list is XSG_EINVAL.
 * Afterwards xsg_count, xsg_count_begin / _end (done synchronously inside _begin), xsg_search with every result accessor
 * and xsg_result_context_edges serve the list on all seven tags.  xsg_count_async and xsg_count_async_status return
 * XSG_ENOTSUP (the route fetches sizes from the device); a binding of 2^24 chunks or more is XSG_ENOTSUP.
 * How: every position of the text is tested against a filter of 65 536 bits held in LDS -- one bit per hashed g-gram a
 * literal starts with, g = min(shortest literal, 4) (k_set_scan) -- the candidates are verified against the literals in
 * listing order (k_set_verify), and the walk and the list stages are the ones of every other pattern.  There is no
 * density bail-out: a list that makes most positions candidates ("e", "th") is slow but exact. */
int xsg_set_literals(xsg_ctx* ctx, const void* list, size_t n, uint32_t flags);
/* WHOLE WORDS (grep -w -F): options of a literal list, given in `list_flags` -- the pattern flags have no free bit.  The
 * _opts entry points take them; list_flags == 0 is the call without _opts, result for result, and every bit but
 * XSG_LIST_WHOLE_WORDS and XSG_LIST_ALL_OF (below) is XSG_EINVAL.  Single patterns (xsg_set_pattern, literal or expression) have no such option: a
 * single word goes in as a list of one.
 * A WORD BYTE is one of 0-9 A-Z a-z _ (63 values).  Every other byte is none, '\n' and every byte >= 0x80 included (GNU
 * grep in the C locale); XSG_FLAG_IGNORE_CASE does not change the set.  With XSG_LIST_WHOLE_WORDS an occurrence of
 * literal l at position p of a chunk of length L is ADMISSIBLE iff
 *   p == 0           or chunk[p - 1]      is no word byte, and
 *   p + len(l) == L  or chunk[p + len(l)] is no word byte.
 * A chunk's edges are word boundaries: no byte in front of the chunk's first or at or beyond L is read for this test or
 * decides anything.  The test looks at the NEIGHBOURS whatever the literal's own edge bytes are, as grep -w does: "-x-" in
 * "a-x-b" is not admissible.
 *   list tags   xsg_count, xsg_count_begin / _end, xsg_search on all seven tags, xsg_count_chunks, with XSG_FLAG_INVERT,
 *               XSG_FLAG_CONTEXT and XSG_MATCHES: the search xsg_set_literals defines, restricted to admissible
 *               occurrences.  At the leftmost position where any literal occurs ADMISSIBLY, the first-listed literal that
 *               does so is the match, and the walk resumes at its end: ("ab","abc") on "abc ab abcd" matches "abc" at 0
 *               and "ab" at 4.  This is what a backtracking leftmost-first engine computes for
 *               (?<![0-9A-Za-z_])(?:l1|l2|...)(?![0-9A-Za-z_]); the set of matching lines is grep -w -F's.
 *   counts      xsg_count_literals, xsg_count_literals_chunks, xsg_count_literals_csr (and their _async forms),
 *               xsg_literal_counter_*: counts[j] is the number of admissible occurrences of l_j -- per literal,
 *               independent of the rest of the list; duplicates get the same number each; the matrix's column sums still
 *               equal xsg_count_literals, and the CSR form the dense one.
 * The option is a property of the pattern: any later xsg_set_pattern, xsg_set_literals or failed set call clears it.
 * xsg_scan_kernel_name of such a list ends in " whole words". */
#define XSG_LIST_WHOLE_WORDS 0x1u /* list_flags */
/* ALL OF (grep -F a | grep -F b | ...): a bit of list_flags, accepted wherever XSG_LIST_WHOLE_WORDS is and combinable with
 * it.  Let l_0 .. l_{k-1} be the list as parsed.  The lines of a chunk are those defined under XSG_FLAG_INVERT.  An
 * occurrence is what xsg_count_literals counts: both sides folded under XSG_FLAG_IGNORE_CASE, and under
 * XSG_LIST_WHOLE_WORDS only admissible occurrences count.  A literal holds no '\n', so an occurrence lies in exactly one
 * line.  With the bit set, the set R of selected lines of a chunk is
 *     R = { lines in which, for EVERY j, at least one occurrence of l_j starts }
 * which equals the intersection over j of the set XSG_LINE_BYTE_OFFSETS reports for the list (l_j) alone, under the same
 * flags and the same XSG_LIST_WHOLE_WORDS bit.  Overlapping occurrences may serve different literals, and so may covered
 * ones ("ab" and "abc" on "abc"); duplicates in the list are one requirement; a list of one is the plain list search; a
 * chunk's edges are line edges, and no byte at or beyond a chunk's end decides anything.
 *   served    with R in place of the plain list's line set: XSG_COUNT_LINES through xsg_count, xsg_count_begin / _end and
 *             xsg_count_chunks; XSG_LINE_BYTE_OFFSETS, XSG_LINE_INDICES and XSG_LINES through xsg_search and every
 *             accessor; XSG_FLAG_INVERT (the lines that lack at least one literal); XSG_FLAG_CONTEXT and
 *             xsg_result_context_edges; xsg_job_start_list; xsg_host_searcher_create_list_opts with
 *             xsg_host_count(skip_to_nl = 1), xsg_host_offsets in the two line modes and xsg_host_lines.
 *   refused   never approximated: XSG_COUNT_MATCHES, XSG_MATCH_BYTE_OFFSETS and XSG_MATCHES are XSG_ENOTSUP from the count,
 *             search, job or host call, xsg_host_count(skip_to_nl = 0) and xsg_host_matches too -- a conjunction has no
 *             single match.  More than XSG_MAX_ALL_OF_LITERALS literals under the bit is XSG_EINVAL from the set call, and
 *             the context then holds no pattern.  xsg_literal_counter_create_opts and xsg_literal_finder_create_opts
 *             refuse the bit with XSG_EINVAL: it means nothing for a count per literal.
 *   unchanged xsg_count_literals, _chunks, _csr, xsg_find_literals and their stream-ordered forms answer per literal on a
 *             context whose list carries the bit, as they do without it; xsg_count_async / _status stay XSG_ENOTSUP as for
 *             every list.
 * xsg_scan_kernel_name of such a list ends in " all of", behind " whole words" if both are set.  list_flags == 0 and
 * list_flags == XSG_LIST_WHOLE_WORDS stay, result for result, what they are without this bit.  Like whole words, the option
 * is a property of the pattern: any later set call clears it. */
#define XSG_LIST_ALL_OF 0x4u /* list_flags; every bit but these two, 0x2 among them, stays XSG_EINVAL: 0x2 was refused as an
                                * unknown flag by every build so far, and callers that probe with it keep their answer */
#define XSG_MAX_ALL_OF_LITERALS 64u
int xsg_set_literals_opts(xsg_ctx* ctx, const void* list, size_t n, uint32_t flags, uint32_t list_flags);
/* A ROW LIMIT PER CHUNK (grep --max-count on every chunk of a binding): "the first max_count are enough".  The limit is a
 * property of the PATTERN, like the list options: it is set after xsg_set_pattern, xsg_set_literals or
 * xsg_set_literals_opts, any later set call clears it whether that call succeeds or fails, and without a pattern the call
 * returns XSG_ESTATE.  max_count == 0 means no limit: every entry point is then, result for result, what it is without
 * this call.  Any other value N is accepted, up to UINT64_MAX.
 *
 * For one chunk let R be the list the tag reports for that chunk under the pattern and its flags: XSG_FLAG_INVERT is
 * already applied (R is then the complement I) and the default lossy end-of-chunk behaviour is included -- all this before
 * XSG_FLAG_CONTEXT widens anything and before XSG_LINES drops an unterminated last line.  With the limit R is replaced by
 * its first N entries in file order, per chunk, and everything downstream sees that list.
 *   line list tags   XSG_LINE_BYTE_OFFSETS, XSG_LINE_INDICES, XSG_LINES: the first N selected lines of every chunk; context,
 *                    if set, is taken around those N lines and xsg_result_context_edges describes the limited list;
 *                    XSG_LINES then drops an unterminated last line as always, so a chunk may hand out N - 1 lines.
 *   match list tags  XSG_MATCH_BYTE_OFFSETS, XSG_MATCHES: the first N MATCHES of every chunk -- entries, not lines (grep -o
 *                    --max-count counts lines); lengths and bytes follow their entries.
 *   rows             xsg_result_chunk_ptr and its byte_ptr: the rows of the limited result.
 *   counts           xsg_count, xsg_count_begin / _end: XSG_CTR_MATCHES or XSG_CTR_LINES is the sum over the chunks of
 *                    min(count of chunk c, N); XSG_CTR_NEWLINES, XSG_CTR_BYTES and the non-ASCII refusal are unchanged;
 *                    xsg_count_begin does its work synchronously, as it does for a count that is a list.
 *                    xsg_count_chunks: counts[c] = min(counts[c] without the limit, N), totals as xsg_count gives them
 *                    under the limit, newlines[] unchanged; sum(counts) == totals[...] keeps holding.
 *   refused          XSG_ENOTSUP, never approximated: the stream-ordered counts under a limit (xsg_count_async,
 *                    xsg_count_async_status, xsg_count_chunks_async) and every per-literal entry point under a limit
 *                    (xsg_count_literals*, xsg_find_literals*: a clamp per literal is a different feature).  Every other
 *                    refusal keeps its precedence and its message.
 * xsg_scan_kernel_name names the stage, " + xsg::k_limit_copy (max count)" for a list tag and " + xsg::k_limit_counts (max
 * count)" for a count, behind "(inverted)" and in front of "(context)"; xsg_time_scan_kernel and xsg_shard_tune ignore the
 * limit.  A limited search takes the exact list route, as an inverted one does.
 * Unlike GNU grep: the after-context of the Nth line includes later lines even if they would have been selected themselves
 * (grep ends trailing context at the next selected line once the count is reached). */
int xsg_set_max_count(xsg_ctx* ctx, uint64_t max_count);
/* Would xsg_set_literals accept this list, and what does it compile to?  Host only, needs no device (like
 * xsg_regex_check).  XSG_OK or XSG_EINVAL with the reason in xsg_last_error().  `info` (optional) receives the numbers,
 * `filter` (optional, XSG_LITERAL_FILTER_BYTES) the filter image: bit h of the little-endian uint32 words is set <=> some
 * literal starts with a g-gram whose hash is h; the hash of a gram v (its g bytes, first byte lowest, folded under
 * XSG_FLAG_IGNORE_CASE) is v for g <= 2 and (v * 0x9E3779B1 mod 2^32) >> 16 for g = 3, 4. */
#define XSG_LITERAL_FILTER_BYTES 8192u
typedef struct xsg_literal_list {
  uint32_t count;            /* literals */
  uint32_t min_len, max_len; /* shortest / longest, bytes */
  uint32_t gram;             /* g = min(min_len, 4) */
  uint32_t filter_bits_set;  /* of 65 536 */
} xsg_literal_list;
int xsg_literals_info(const void* list, size_t n, uint32_t flags, xsg_literal_list* info, uint8_t* filter);
/* Would XSG_FLAG_REGEX accept this expression?  XSG_OK, or XSG_ENOTSUP with the
 * reason in xsg_last_error().  Needs no device (callers route on it the way the
 * reference routes on use_str_as_regex, utils/utils.h:17-25).  Optional outputs:
 * the number of byte positions, and their 256-bit sets (room for 32 x 8 uint32;
 * bit b of sets[8*k + b/32] set <=> position k accepts byte b; folded if
 * XSG_FLAG_IGNORE_CASE is in flags).  *positions == 0: an expression of variable
 * length, served by the automaton route below (no position-wise sets; whether it
 * can match a '\n' is xsg_regex_dfa.multiline). */
int xsg_regex_check(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* sets);
/* The same with the whole structure: number of alternatives, whether the expression is exact on ASCII data only
 * ('.', negated classes), and every alternative's sets (room for 64 x 8 uint32, alternative-major).  xsg_regex_check
 * returns the position-wise UNION of the alternatives. */
int xsg_regex_info(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* alternatives,
                   uint32_t* ascii_only, uint32_t* sets);
/* Expressions of VARIABLE length (x* x+ x? x{n,m}, lazy forms, alternatives of different lengths) are served by a
 * second route: the library compiles them into a forward (leftmost-first) and a reverse (longest) byte-class DFA
 * and k_rx_scan walks every line with them (csrc/xsg_regex.h; restrictions there: no empty matches, no anchors; an
 * expression with a set that accepts '\n' is walked chunk by chunk instead and serves the match tags only).
 * xsg_regex_check / xsg_regex_info return XSG_OK with *positions == 0 for such an expression.  This call hands out the automata (for inspection and for the host-side tests, which drive the tables
 * against another regex engine without a GPU): `info` always; `fwd` / `rev` (row-major, states x ncls entries, each
 * the NEXT STATE'S ROW OFFSET = state * ncls; state 0 is dead, states >= *_first_acc hold a match) if they have room
 * for the tables (cap_entries each).  XSG_ENOTSUP: the expression is not served by this route (it may still be a
 * fixed-length one that xsg_regex_info describes). */
typedef struct xsg_regex_dfa {
  uint32_t ncls, minlen, ascii_only;
  uint32_t multiline; /* a set accepts '\n': matches may span lines; the match tags only */
  /* PREFILTER: if prefix_positions != 0, every match starts with that many bytes accepted by one of
   * prefix_alternatives class sequences; the synchronous entry points (xsg_count, xsg_search, the jobs) then find
   * candidate positions with the scan kernel's class-sequence matcher and run the automaton at candidates only. */
  uint32_t prefix_positions, prefix_alternatives;
  /* FACTOR (expressions without a selective start that cannot match across lines): if factor_positions != 0, every match
   * CONTAINS that many consecutive bytes accepted by one class sequence (`\w+ing`: `\wing`); the synchronous entry
   * points mark the tiles in which a line with an occurrence starts, once per binding and pattern, and the line-walking
   * kernel skips every other tile. */
  uint32_t factor_positions;
  uint32_t fwd_states, fwd_start, fwd_first_acc;
  uint32_t rev_states, rev_start, rev_first_acc;
  uint8_t class_of[256];
} xsg_regex_dfa;
int xsg_regex_dfa_info(const void* expr, size_t n, uint32_t flags, xsg_regex_dfa* info, uint16_t* fwd, uint16_t* rev,
                       size_t cap_entries);
/* The prefilter of such an expression in the layout of xsg_regex_info (room for 64 x 8 uint32, alternative-major):
 * every match starts with *positions bytes that one of the *alternatives class sequences accepts.  *positions == 0:
 * the expression has no selective start, every entry point walks all lines (k_rx_scan). */
int xsg_regex_prefix(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* alternatives, uint32_t* sets);
/* ... and its factor (xsg_regex_dfa.factor_positions): one class sequence, room for 32 x 8 uint32. */
int xsg_regex_factor(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* sets);

/* ---- shards ---------------------------------------------------------------- */
/* d_base/capacity: device memory owned by the caller (hipMalloc, a torch
 * tensor's data_ptr(), ...), must stay valid, and its BYTES ARE IMMUTABLE FOR THE LIFETIME OF THE BINDING: the library
 * keeps results derived from them per binding (newline counts per tile, the 4-gram sketch of every tile and whether
 * its gate pays for a pattern, the measured hot filter and filter window of a pattern, the tile marks and density
 * verdicts of the regex prefilters, whether a pattern's lists fit the one-sync route) and every later pass -- the
 * stream-ordered xsg_count_async included -- relies on them.
 * The sketch is 512 bytes of device memory per 16 KiB tile (a
 * binding simply goes without if the allocation fails): one bit per hashed 4-gram that starts in the tile.  It does not
 * depend on the pattern.  A span locator of another 1 KiB per tile is built with it -- 2048 such bits for each of the
 * tile's four 4 KiB spans -- and, with the locator, the sketch's bit planes: the same 4096 bits per tile transposed, one
 * 64-bit word per (bit, group of 64 tiles), another 512 bytes per tile.  The three together take 12.5 % of the text in
 * device memory, 6.25 GiB beside a 50 GiB binding (9.4 % before the planes existed, 3.1 % before the locator); a binding
 * without memory for the locator keeps the sketch alone, one without memory for the planes keeps sketch and locator.  The plain count pass of a case-sensitive literal of 4 bytes and more -- xsg_count,
 * xsg_count_begin, xsg_count_async, the count pass of xsg_search -- is then one launch of a bounded grid: its workgroups
 * test the sketches of 256 tiles at a time for the needle's first grams and scan the tiles that hold every one of them --
 * the candidate tiles -- and read no other text.  A needle whose grams are words of the text passes everywhere: the synchronous
 * entry points find that out first (a sample of the sketch, once per binding and pattern) and keep the full scan.
 * xsg_count_async cannot -- it never waits for the device -- and uses the gate whenever no synchronous call has judged
 * the pattern on this binding; for such a needle every tile is then a candidate and the pass is SLOWER than the full
 * scan (measured 1.07 x on a 50 GiB binding; the wave form's grid of one resident round adds 6 % to
 * that case -- `this`, every tile a candidate: 8.27 -> 8.75 ms, XSG_GATE_GRID=8192 takes it back): call a synchronous entry point once with the pattern,
 * or set XSG_SKETCH=0, where that matters.  A plain match count behind the gate (no XSG_WITH_NEWLINES; a needle of
 * at most 33 bytes, or XSG_FLAG_EXACT_TAIL) is ONE launch: the same kernel sums in registers, walks the end-of-chunk zones
 * that hold an occurrence itself and writes the counters (50 GiB, `Sherlock`: 0.149 -> 0.110 ms per call).  It pays for a
 * needle in a chunk's last plen + 31 bytes with a look back through that chunk for the previous occurrence: data with the
 * needle at the end of EVERY chunk measured 1.6 x slower than the two launches (0.25 against 0.16 ms, 3200 chunks of 16 MiB,
 * DESIGN.md section 5); XSG_GATE_FINISH=0 keeps the two launches.  With the span locator that launch reads, of a
 * candidate tile, only the 4 KiB spans whose own bits hold the needle's grams (XSG_GATE_SPANS=0: the whole tile;
 * xsg_scan_kernel_name says " by 4 KiB spans" in front of " finishing").  With the locator the launch also runs as a wave
 * per sketch group of 64 tiles -- every wave tests its own tiles and reads its own candidates' spans, none waits for
 * another before the kernel's end (50 GiB, `Sherlock`: 0.083 -> 0.076 ms per call; the name says " a wave per group" in
 * front of " by 4 KiB spans").  A wave takes its groups four at a time: the sketch words of all four are requested together,
 * the batch's candidates are looked up in one round trip and then scanned (50 GiB, `Sherlock`: 0.076 -> 0.062 ms per call;
 * the name says " in batches of 4" in front of " a wave per group"; XSG_GATE_BATCH=1 keeps one group at a time).
 * Where the binding holds the bit planes the wave picks a group's candidates from them -- the AND of one 64-bit word per
 * gram of the needle, 40 bytes a group for `Sherlock` where the sketch words are 1280 and a chunk number per tile (50 GiB,
 * `Sherlock`: 0.062 -> 0.058 ms per call; the name says " from bit planes" in front of " in batches of 4";
 * XSG_GATE_PLANES=0 keeps the select from sketch words).  Building them adds 2.3 ms to the sketch's 38 ms on 50 GiB.
 * XSG_GATE_WAVES=0 keeps the workgroup form; XSG_GATE_GRID=N sets the number of workgroups of either form (default 1536
 * for the wave form, 8192 for the workgroup form and the storing pass; never more than one per 256 tiles).  Bindings of
 * 64 MiB and more get the sketch from
 * xsg_shard_tune, or from the second such pass of a synchronous entry point (the build is enqueued on the context's
 * stream); xsg_count_async on a caller's stream never builds, it uses what is there.  XSG_SKETCH=0 switches the feature
 * off, XSG_SKETCH=1 builds before the first pass.  A caller that refills
 * the buffer in place calls xsg_shard_rebind (same pointer and table are fine) or xsg_shard_invalidate before the
 * next search; searching rewritten bytes under an old binding can silently lose matches.
 * Requirements: d_base 16-byte aligned; for every chunk offset % 16 == 0 and
 * offset + round_up(length,16) <= capacity; chunks must not overlap and must
 * be listed in increasing offset order.  The table is copied. */
int xsg_shard_create(xsg_ctx* ctx, const void* d_base, uint64_t capacity, const xsg_chunk* chunks, uint64_t nchunks,
                     xsg_shard** out);
/* Re-point an existing shard at a new chunk table (same or different buffer)
 * without re-allocating its scratch when the new table is not larger. */
int xsg_shard_rebind(xsg_shard* shard, const void* d_base, uint64_t capacity, const xsg_chunk* chunks,
                     uint64_t nchunks);
/* The bytes behind the binding were rewritten in place (same buffer, same chunk table): forget everything derived
 * from the old bytes.  Cheaper than a rebind (no table upload); a rebind implies it. */
int xsg_shard_invalidate(xsg_shard* shard);
void xsg_shard_destroy(xsg_shard* shard);
/* line-index base of the whole shard for XSG_LINE_BASE_AUTO chunks (default 0):
 * the number of '\n' in all shards that precede this one in the file. */
int xsg_shard_set_line_base(xsg_shard* shard, uint64_t line_base);

/* ---- counting (replaces search::count, search_wrappers.h:163-185) ---------- */
/* Asynchronous: enqueues the scan on `stream` (a hipStream_t, NULL = the
 * ctx's own stream) and returns.  d_counters: device memory for
 * XSG_NUM_COUNTERS uint64 values, overwritten by the call.  Serves
 * XSG_COUNT_LINES and XSG_COUNT_MATCHES, each optionally | XSG_WITH_NEWLINES,
 * with one exception.  A pattern that can overlap itself -- a literal with a
 * border (`that`, `aa`, `abab`) or a class sequence two of whose occurrences may
 * overlap (`[a-z]{4}`, `t.e`; the test is conservative) -- needs the greedy
 * non-overlap walk over the ordered occurrence list.  Its XSG_COUNT_MATCHES
 * runs that list route entirely on the device, into arrays whose capacity is
 * twice the number of raw occurrences the last list pass on this shard saw (at
 * least 2^20): if there are more, all four counters read UINT64_MAX and
 * xsg_count (synchronous, sizes exactly, remembers the size) is the call to
 * make; | XSG_WITH_NEWLINES is not served for such a pattern (XSG_ENOTSUP).
 * For a LITERAL with a border the exception lapses once a synchronous call
 * (xsg_count, xsg_search) on this binding has established that its occurrences
 * do not overlap in the bound data -- the usual case in text; see xsg_count.
 * The first pass of a (binding, pattern) on a shard of 64 MiB or more also runs
 * the library's hot-filter probe (a few short launches and one stream sync,
 * DESIGN.md 3.1) -- unless another binding of the same buffer already measured
 * this pattern on this ctx; every later call only enqueues. */
int xsg_count_async(xsg_shard* shard, uint32_t mode, void* stream, uint64_t* d_counters);
/* The same pass with an error channel: *d_status (device memory, one uint64, overwritten by the call) receives 0 or a
 * combination of the XSG_STATUS_* bits below, and when it is not 0 all four counters read ZERO -- so a caller that adds
 * up or all-reduces counters (and the status word with them: the bits of different ranks add up to something non-zero)
 * can never mistake a refusal for a number.  xsg_count_async itself keeps its older convention (UINT64_MAX in all four
 * counters); new callers should use this form. */
#define XSG_STATUS_OK 0u
#define XSG_STATUS_OVERFLOW 1u  /* a self-overlapping pattern's bounded device-side list ran out of capacity: call xsg_count */
#define XSG_STATUS_NONASCII 2u  /* an expression that is exact on ASCII data only met a byte >= 0x80 (see XSG_FLAG_REGEX) */
int xsg_count_async_status(xsg_shard* shard, uint32_t mode, void* stream, uint64_t* d_counters, uint64_t* d_status);
/* Synchronous, any pattern, XSG_COUNT_MATCHES or XSG_COUNT_LINES
 * (| XSG_WITH_NEWLINES): result in host memory.  The first XSG_COUNT_MATCHES
 * (or match-offset search) of a literal with a border on a binding also runs
 * one count pass per border (at most three) for the word two overlapping
 * occurrences would spell: if the data holds none, every occurrence is a
 * match and the pattern is served like one without a border from then on. */
int xsg_count(xsg_shard* shard, uint32_t mode, uint64_t counters[XSG_NUM_COUNTERS]);

/* Split-phase form of xsg_count for host pipelines: _begin enqueues the pass on the ctx's stream and returns,
 * _end blocks until it is done and hands out the counters.  One pass in flight per shard. */
int xsg_count_begin(xsg_shard* shard, uint32_t mode);
int xsg_count_end(xsg_shard* shard, uint64_t counters[XSG_NUM_COUNTERS]);

/* ---- counts per chunk ------------------------------------------------------ */
/* A shard is a table of chunks searched independently; a caller who binds many documents as the chunks of one resident
 * buffer asks here which of them hold the needle and how often (grep -c over many files; grep -l / -L follow), in one pass.
 * counts[c], c in [0, nchunks): what xsg_count(mode) would put into XSG_CTR_MATCHES (XSG_COUNT_MATCHES) or XSG_CTR_LINES
 * (XSG_COUNT_LINES) for a binding that holds chunk c alone -- same pattern, same flags (XSG_FLAG_EXACT_TAIL or the
 * lossy tail, IGNORE_CASE, REGEX, INVERT; CONTEXT bits are ignored as by every count).  Under XSG_FLAG_INVERT the lines
 * of a chunk are those defined there, and counts[c] = lines of chunk c - its matching lines.
 * newlines (optional; requires mode | XSG_WITH_NEWLINES, XSG_EINVAL otherwise; with the flag and without the array only
 * the total is produced): newlines[c] = number of '\n' in chunk c.
 * totals (optional): the four counters exactly as xsg_count(mode) returns them for the binding.
 * Always: sum(counts) == totals[XSG_CTR_MATCHES or XSG_CTR_LINES], sum(newlines) == totals[XSG_CTR_NEWLINES].
 * cap_chunks < the number of bound chunks, counts == NULL, a list mode, unknown mode bits: XSG_EINVAL.  A chunk of length
 * 0 counts 0; a binding of 0 chunks is XSG_OK and writes nothing to counts.  XSG_COUNT_MATCHES under XSG_FLAG_INVERT:
 * XSG_ENOTSUP, as everywhere.  An expression that is exact on ASCII data only, on a binding that holds a byte >= 0x80,
 * is refused for the WHOLE binding as by xsg_count (never per chunk): XSG_ENOTSUP, counts unspecified.
 * Serves every pattern kind and flag xsg_count serves.  Patterns whose count is a list (the prefilter route of an
 * expression, a literal list, a bordered literal whose occurrences do overlap in the data, XSG_COUNT_LINES of a literal
 * that contains '\n') run that list route and sort its entries by chunk on the device; everything else is the scan in
 * its storing form and one finish kernel that keeps the chunk boundaries (a plain xsg_count keeps its one launch). */
int xsg_count_chunks(xsg_shard* shard, uint32_t mode, uint64_t* counts, uint64_t* newlines, uint64_t cap_chunks,
                     uint64_t totals[XSG_NUM_COUNTERS]);
/* Stream-ordered form: every output is DEVICE memory, nothing waits.  d_counts: cap_chunks words; d_newlines optional as
 * above; d_counters (XSG_NUM_COUNTERS words) and d_status (one word) are required and follow xsg_count_async_status:
 * status != 0 => the four counters AND every d_counts[c] / d_newlines[c] read zero (XSG_STATUS_NONASCII for the refusal
 * above).  Serves what xsg_count_async_status serves through scan + finish: not a literal list, not a bordered literal
 * that is not yet known overlap-free on this binding (a synchronous call establishes that), not XSG_COUNT_LINES of a
 * pattern that contains '\n' -- XSG_ENOTSUP for those; xsg_count_chunks serves them. */
int xsg_count_chunks_async(xsg_shard* shard, uint32_t mode, void* stream, uint64_t* d_counts, uint64_t* d_newlines,
                           uint64_t cap_chunks, uint64_t* d_counters, uint64_t* d_status);

/* ---- counts per literal ---------------------------------------------------- */
/* The other axis: which literals of a list (xsg_set_literals) occur in the bound chunks, and how often -- a keyword table
 * in one pass over the text.  Let l_0 .. l_{k-1} be the literals in the order xsg_set_literals parsed them.
 * counts[j] = the number of pairs (chunk c, position p) with p + len(l_j) <= length(c) and the chunk bytes
 * [p, p + len(l_j)) equal to l_j; under XSG_FLAG_IGNORE_CASE both sides are ASCII-lowered first.  These are OCCURRENCES,
 * not the matches of the list's leftmost-first walk: overlapping occurrences all count (`aa` in `aaaa`: 3), a literal
 * covered by another still counts (`ab`, `abc` on `abc`: 1 and 1), duplicates in the list get the same number each, and
 * counts[j] depends on l_j's bytes and the bound data only, never on the rest of the list.  No byte at or beyond a chunk's
 * end decides anything.
 * Relation to the rest of the ABI: counts[j] equals XSG_CTR_MATCHES of xsg_count(XSG_COUNT_MATCHES) under
 * XSG_FLAG_EXACT_TAIL with l_j as the only pattern whenever no two occurrences of l_j overlap in the data -- always, for a
 * literal without a border (no proper prefix of it is also its suffix).
 * Both calls write counts[0 .. k), every entry, zeros included; a binding of 0 chunks is XSG_OK with k zeros.
 * XSG_ESTATE: the ctx holds no pattern.  XSG_ENOTSUP: the pattern is not a list set by xsg_set_literals (a single
 * literal goes in as a list of one); XSG_FLAG_INVERT is set (a count of occurrences has no inverted form); a binding of
 * 2^24 chunks or more, as for every list search.  XSG_EINVAL: counts == NULL, cap_literals < k.  The CONTEXT bits and
 * XSG_FLAG_EXACT_TAIL are accepted and ignored, as by every count of a list.
 * One launch: the candidate scan of the list with the verify step inside its own pass (no candidate list, no size fetched
 * from the device), a histogram per workgroup, 64-bit atomics into counts.  The list tags (xsg_count, xsg_search) are
 * unchanged and may be called before and after on the same binding. */
int xsg_count_literals(xsg_shard* shard, uint64_t* counts, uint64_t cap_literals); /* host memory; waits */
/* Stream-ordered form: d_counts is DEVICE memory (cap_literals words), overwritten; nothing waits and nothing is fetched.
 * Unlike the other stream-ordered counts of a list (XSG_ENOTSUP there) this one needs no size from the device. */
int xsg_count_literals_async(xsg_shard* shard, void* stream, uint64_t* d_counts, uint64_t cap_literals);

/* ---- counts per chunk and literal -------------------------------------------- */
/* Both axes at once: a term-document matrix, the keyword table of every bound chunk from ONE pass.  Let k be the number
 * of literals xsg_set_literals parsed and n the number of bound chunks.  counts[c * k + j], row-major by chunk, is what
 * xsg_count_literals would put into counts[j] for a binding that holds chunk c alone: the same pattern, flags, definition
 * of an occurrence (overlapping ones, covered ones and duplicates of the list all count) and ignore-case folding, and
 * again no byte at or beyond a chunk's end decides anything.  Hence, for every j,
 *     sum over c of counts[c * k + j]  ==  xsg_count_literals' counts[j] on the same binding.
 * chunks_with (optional, NULL: not wanted; cap_literals >= k): chunks_with[j] = the number of chunks c with
 * counts[c * k + j] > 0, the literal's document frequency; duplicates in the list get the same number each.
 * Every one of the n * k words is written, zeros included, and every chunks_with[j]; a chunk of length 0 yields a row of
 * zeros; a binding of 0 chunks is XSG_OK, writes nothing to counts and k zeros to chunks_with.  Words behind n * k and
 * behind k are not touched.
 * XSG_ESTATE: the ctx holds no pattern.  XSG_ENOTSUP: the pattern is no list set by xsg_set_literals; XSG_FLAG_INVERT is
 * set; a binding of 2^24 chunks or more.  XSG_EINVAL: counts == NULL, cap_words < n * k, chunks_with != NULL with
 * cap_literals < k.  The CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and ignored.
 * The matrix is DENSE: n * k words whatever they hold.  The sparse form is xsg_count_literals_csr, below.
 * One launch behind the memsets of both results (k_set_count_literals_chunks): a workgroup owns a contiguous range of
 * tiles, keeps one histogram in LDS and adds it to row c with 64-bit atomics whenever the next tile belongs to another
 * chunk; an add that finds its word 0 is the chunk's first for that literal and counts 1 for chunks_with[j] (exact: every
 * addend is positive, so a word leaves 0 once).  No candidate list, no size fetched from the device.
 * The synchronous form keeps the matrix in device memory of the shard's and a pinned mirror: a matrix of more than 2^28
 * words (2 GiB) is XSG_ENOTSUP there -- the stream-ordered form, whose memory is the caller's, has no such limit. */
int xsg_count_literals_chunks(xsg_shard* shard, uint64_t* counts, uint64_t cap_words,
                              uint64_t* chunks_with, uint64_t cap_literals);               /* host memory; waits */
/* Stream-ordered form: d_counts (cap_words words) and d_chunks_with (cap_literals words, or NULL) are DEVICE memory,
 * overwritten; nothing waits and nothing is fetched. */
int xsg_count_literals_chunks_async(xsg_shard* shard, void* stream, uint64_t* d_counts, uint64_t cap_words,
                                    uint64_t* d_chunks_with, uint64_t cap_literals);       /* device memory; nothing waits */
/* The literals a workgroup of that pass can note between two flushes before a flush sweeps its whole histogram instead
 * of walking the noted ones (results do not depend on it; tests place their lists around it). */
uint32_t xsg_literals_chunks_touched_capacity(void);

/* The same matrix in CSR form, for bindings of many small chunks under a long list, whose matrix is almost all zeros.
 * Let D[c][j] be the word xsg_count_literals_chunks would write to counts[c * k + j].  The result is
 *   row_ptr  n + 1 uint64: row_ptr[0] == 0, row_ptr[c + 1] - row_ptr[c] = the number of j with D[c][j] > 0,
 *            row_ptr[n] == nnz;
 *   cols     nnz uint32: within a row the literal indices j ASCEND STRICTLY;
 *   vals     nnz uint64: vals[e] == D[c][cols[e]], never 0
 * -- what scipy.sparse.csr_matrix((vals, cols, row_ptr)) and torch.sparse_csr_tensor take.  Duplicates in the list get an
 * entry each, as they get a column each in the dense form; a chunk of length 0 is an empty row; a binding of 0 chunks is
 * XSG_OK with row_ptr = {0} and nnz = 0.  The result is a function of the list, the flags and the bound bytes alone:
 * bit-identical from call to call and across grid sizes, no entry's place is left to scheduling.  chunks_with is not
 * produced here: it is the bincount of cols.
 * xsg_count_literals_csr runs the pass, sizes the result exactly and KEEPS it on the shard; *nnz = row_ptr[n].  The kept
 * result is valid until the next xsg_count_literals_csr, xsg_shard_rebind or xsg_shard_invalidate on the shard (calls to
 * other entry points in between do not disturb it: it lives in buffers of its own); xsg_result_literals_csr copies it out
 * and is XSG_ESTATE otherwise -- the xsg_search / xsg_result_u64 pattern.  There: cap_rows >= n + 1 and cap_entries >= nnz;
 * cols and vals may BOTH be NULL (row_ptr alone); words behind n + 1 / nnz are not touched.
 * XSG_ESTATE, XSG_ENOTSUP as for xsg_count_literals_chunks (no pattern; no list, XSG_FLAG_INVERT, 2^24 chunks or more).
 * XSG_EINVAL: nnz == NULL; in xsg_result_literals_csr row_ptr == NULL, cap_rows < n + 1, cap_entries < nnz, exactly one
 * of cols / vals NULL.  The CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and ignored.
 * A result of more than 2^28 entries is XSG_ENOTSUP in the synchronous form -- the stream-ordered form, whose memory is
 * the caller's, has no such limit.  There is NO limit on n * k: the scratch is a word per chunk and at most 64 MiB.
 * Two passes of the dense form's partition around a prefix sum (k_set_count_literals_csr): the first sizes every row, the
 * second writes its entries at row_ptr[c] + rank in ascending j.  The synchronous form fetches row_ptr[n] between them,
 * its one extra wait. */
int xsg_count_literals_csr(xsg_shard* shard, uint64_t* nnz);                                 /* waits; keeps the result */
int xsg_result_literals_csr(xsg_shard* shard, uint64_t* row_ptr, uint64_t cap_rows, uint32_t* cols, uint64_t* vals,
                            uint64_t cap_entries);                                           /* host memory */
/* Stream-ordered form: d_row_ptr (cap_rows >= n + 1 words), d_cols and d_vals (cap_entries entries each) and d_status (one
 * word) are DEVICE memory of the caller's, all required; nothing waits and nothing is fetched.  nnz <= cap_entries:
 * *d_status = 0 and everything is written.  Otherwise *d_status = XSG_STATUS_OVERFLOW; d_row_ptr is still complete and
 * true, so d_row_ptr[n] is the capacity to come back with; every entry with an index below cap_entries is written and
 * correct; nothing at or behind cap_entries is written.  cap_entries == 0 (non-NULL pointers) is a pure sizing pass.
 * XSG_EINVAL: a NULL output, cap_rows < n + 1.  The scratch is the shard's: calls on one shard follow one another. */
int xsg_count_literals_csr_async(xsg_shard* shard, void* stream, uint64_t* d_row_ptr, uint64_t cap_rows,
                                 uint32_t* d_cols, uint64_t* d_vals, uint64_t cap_entries, uint64_t* d_status);

/* ---- occurrences per literal ------------------------------------------------- */
/* Where, and which literal: every occurrence of every literal of the list with its identity, in text order -- what
 * dictionary tagging, positional postings and highlighting need, and the "all matches" output of an Aho-Corasick matcher.
 * (The list tags, xsg_search with XSG_MATCH_BYTE_OFFSETS / XSG_MATCHES, report the winners of the leftmost-first walk only
 * and not which literal won.)  Let l_0 .. l_{k-1} be the list as xsg_set_literals[_opts] parsed it and n the number of
 * bound chunks.  An OCCURRENCE is a triple (c, p, j) with p + len(l_j) <= length(c) and the chunk bytes [p, p + len(l_j))
 * equal to l_j; under XSG_FLAG_IGNORE_CASE both sides are ASCII-lowered first; under XSG_LIST_WHOLE_WORDS only admissible
 * occurrences count.  This is the definition xsg_count_literals uses: overlapping occurrences (`aa` in `aaaa`: 3), covered
 * ones (`ab`, `abc` on `abc`: both, at one position) and duplicates of the list (an entry each) are all included.  No byte
 * at or beyond a chunk's end decides anything.
 * The result is the list of ALL occurrences sorted ascending by (c, p, j), in three arrays:
 *   chunk_ptr  n + 1 uint64: chunk_ptr[0] == 0, the entries [chunk_ptr[c], chunk_ptr[c + 1]) are chunk c's,
 *              chunk_ptr[n] == total;
 *   pos        total uint64: global_offset(c) + p, like every reported byte offset;
 *   lit        total uint32: the listing index j.
 * A chunk of length 0 is an empty range; a binding of 0 chunks is XSG_OK with chunk_ptr = {0} and total = 0.  The result
 * is a function of the list, the flags and the bound bytes alone: bit-identical from call to call and across grid sizes,
 * no entry's place is left to scheduling.  Relations: bincount(lit) == xsg_count_literals' counts; the bincount of chunk
 * c's range == row c of xsg_count_literals_chunks; for a list of one literal without a border, pos equals the
 * XSG_MATCH_BYTE_OFFSETS list under XSG_FLAG_EXACT_TAIL.
 * xsg_find_literals runs the passes, sizes the result exactly and KEEPS it on the shard in buffers of its own (device
 * memory and a pinned mirror); *total = chunk_ptr[n].  The kept result is valid until the next xsg_find_literals,
 * xsg_shard_rebind or xsg_shard_invalidate on the shard; calls to other entry points in between do not disturb it.
 * xsg_result_literal_hits copies it out and is XSG_ESTATE without one.  There: cap_rows >= n + 1; pos and lit are either
 * both given (cap_entries >= total) or both NULL (chunk_ptr alone); words behind n + 1 / total are not touched.
 * XSG_ESTATE: the ctx holds no pattern.  XSG_ENOTSUP: the pattern is no list set by xsg_set_literals, XSG_FLAG_INVERT is
 * set, a binding of 2^24 chunks or more -- the refusals of xsg_count_literals_csr.  XSG_EINVAL: total == NULL; in
 * xsg_result_literal_hits chunk_ptr == NULL, cap_rows < n + 1, cap_entries < total, exactly one of pos / lit NULL.  The
 * CONTEXT bits and XSG_FLAG_EXACT_TAIL are accepted and ignored.  A result of more than 2^28 entries is XSG_ENOTSUP in the
 * synchronous form -- the stream-ordered form, whose memory is the caller's, has no such limit.
 * Two passes of the candidate scan around a prefix sum (k_set_find_literals): the first stores one word per 4 KiB wave
 * span, its occurrences; the second skips the spans without one and stores the others' entries at the span's offset plus
 * their rank.  The scratch is the shard's, 12 bytes per span (0.3 % of the text).  The synchronous form fetches
 * chunk_ptr[n] between the passes, its one extra wait. */
int xsg_find_literals(xsg_shard* shard, uint64_t* total);                                    /* waits; keeps the result */
int xsg_result_literal_hits(xsg_shard* shard, uint64_t* chunk_ptr, uint64_t cap_rows, uint64_t* pos, uint32_t* lit,
                            uint64_t cap_entries);                                           /* host memory */
/* Stream-ordered form: d_chunk_ptr (cap_rows >= n + 1 words), d_pos and d_lit (cap_entries entries each) and d_status (one
 * word) are DEVICE memory of the caller's, all required; nothing waits and nothing is fetched.  total <= cap_entries:
 * *d_status = 0 and everything is written.  Otherwise *d_status = XSG_STATUS_OVERFLOW; d_chunk_ptr is still complete and
 * true, so d_chunk_ptr[n] is the capacity to come back with; every entry with an index below cap_entries is written and
 * correct; nothing at or behind cap_entries is written.  cap_entries == 0 (non-NULL pointers) is a pure sizing pass.
 * XSG_EINVAL: a NULL output, cap_rows < n + 1.  The scratch is the shard's: calls on one shard follow one another. */
int xsg_find_literals_async(xsg_shard* shard, void* stream, uint64_t* d_chunk_ptr, uint64_t cap_rows, uint64_t* d_pos,
                            uint32_t* d_lit, uint64_t cap_entries, uint64_t* d_status);

/* ---- list results (replace byte_offsets_match/_line, line; :136-154,187-207) */
/* Runs the search for one of the list modes on the ctx stream and waits.
 * *n_results = number of elements (offsets / indices / lines).  Results stay
 * in device memory owned by the shard until the next search on it. */
int xsg_search(xsg_shard* shard, uint32_t mode, uint64_t* n_results);
/* Copy the uint64 results of the last XSG_MATCH_BYTE_OFFSETS /
 * XSG_LINE_BYTE_OFFSETS / XSG_LINE_INDICES search, ascending, to host memory. */
int xsg_result_u64(xsg_shard* shard, uint64_t* out, uint64_t cap);
/* The same without the copy into caller memory: *out points at *n values in pinned host memory owned by the shard,
 * valid until the next search on it (a dense needle returns hundreds of MB: D2H into pageable memory runs at a
 * sixth of the pinned rate). */
int xsg_result_u64_view(xsg_shard* shard, const uint64_t** out, uint64_t* n);
/* After an XSG_LINES search: total number of line bytes (no '\n's).  After an XSG_MATCHES search here and in the two
 * calls below: "line" reads "match" (n_lines = |M|, lengths / bytes / offsets of the matched text). */
int xsg_result_lines_size(xsg_shard* shard, uint64_t* n_lines, uint64_t* total_bytes);
/* line i = bytes[ starts[i] .. starts[i] + lengths[i] ), in file order;
 * `offsets` (optional) receives the global byte offset of each line start. */
int xsg_result_lines(xsg_shard* shard, uint64_t* lengths, char* bytes, uint64_t bytes_cap, uint64_t* offsets);

/* The same without copies into caller memory: *lengths / *offsets (n_lines values each) and *bytes (total_bytes, the lines
 * back to back) point into pinned host memory owned by the shard, valid until the next search on it.  A list that fit
 * the one-sync route is already there; a larger one is moved in three pinned D2H copies (a needle in most lines of
 * 10 GiB returns 3 GB: into pageable memory that is 0.3 s, pinned 0.07).  XSG_ENOMEM if the result needs more than
 * 16 GiB of pinned memory (use xsg_result_lines). */
int xsg_result_lines_view(xsg_shard* shard, const uint64_t** lengths, const char** bytes, const uint64_t** offsets,
                          uint64_t* n_lines, uint64_t* total_bytes);

/* newline count of the shard, available after an XSG_LINE_INDICES search (lets a
 * caller chain line-index bases from chunk to chunk without a second pass). */
int xsg_result_newlines(xsg_shard* shard, uint64_t* newlines);

/* What the edges of every chunk cut off under XSG_FLAG_CONTEXT: what a pipeline needs to join the results of chunks
 * that are consecutive pieces of one text (csrc/xsg_context.h holds the seam rule the file pipeline applies).  One
 * entry per chunk of the binding, in chunk order.  Valid after an XSG_LINE_BYTE_OFFSETS / XSG_LINE_INDICES / XSG_LINES
 * search with non-zero context; XSG_ESTATE otherwise, XSG_EINVAL if cap_chunks is below the number of chunks. */
typedef struct xsg_context_edge {
  uint64_t lines;       /* lines of the chunk */
  uint64_t first, last; /* chunk-local index of the first / last line of C (before XSG_LINES drops an unterminated
                           one); UINT64_MAX: C is empty */
  uint32_t open_before; /* max(0, B - index of the first line of R); 0 if R is empty */
  uint32_t open_after;  /* max(0, A - (lines - 1 - index of the last line of R)); 0 if R is empty */
} xsg_context_edge;
int xsg_result_context_edges(xsg_shard* shard, xsg_context_edge* out, uint64_t cap_chunks);

/* The rows of a list result: which of its entries belong to which bound chunk -- what a caller that binds many documents
 * as the chunks of one buffer needs to hand every document its own list (the per-chunk counts of xsg_count_chunks are
 * the rows' lengths).  Valid after a successful xsg_search in any of the five list modes, until the next search, rebind
 * or invalidate on the shard; XSG_ESTATE otherwise, also after a search that failed -- the xsg_result_u64 pattern.
 * With n chunks bound, chunk_ptr receives n + 1 words: chunk_ptr[0] == 0, the entries [chunk_ptr[c], chunk_ptr[c + 1])
 * of the result as xsg_result_u64[_view] and xsg_result_lines[_view] hand it out (for XSG_LINES: after the unterminated
 * last lines were dropped) are chunk c's, and chunk_ptr[n] == *n_results.  Under XSG_FLAG_INVERT the rows are those of
 * I, under XSG_FLAG_CONTEXT those of C, as defined per chunk above; a chunk of length 0 has an empty row, a binding of 0
 * chunks yields {0}.  byte_ptr is optional and allowed only after XSG_LINES / XSG_MATCHES (XSG_EINVAL after a uint64
 * mode): n + 1 words, byte_ptr[c] the sum of the lengths of the entries in front of chunk_ptr[c] -- where chunk c's
 * bytes begin in `bytes` --, byte_ptr[n] == total_bytes.  XSG_EINVAL: chunk_ptr NULL, cap_rows < n + 1.
 * The rows come from the chunk number the device keeps with every entry, never from the reported values: they hold for
 * any global_offset / line_base the chunks were bound with.  A search pays nothing for them: they are computed by this
 * call (a small kernel, one copy of the words, one wait), which leaves the result as it is -- every other accessor works
 * before and after it, and it may be called again. */
int xsg_result_chunk_ptr(xsg_shard* shard, uint64_t* chunk_ptr, uint64_t cap_rows, uint64_t* byte_ptr);

/* ======================================================================== */
/* File searches: the host pipeline behind xs::extern_search                 */
/* ======================================================================== */
/* Replaces, for the literal path, what the reference runs inside
 * include/xsearch/Searcher.h:100-120 (worker loop: read -> search -> result.add)
 * with include/xsearch/tasks/readers.h:29-54 as the reader and
 * include/xsearch/ResultTypes.h:31-130 as the result container:
 *   - chunks are cut at '\n' (>= chunk_bytes, extended to the next newline; the
 *     layout the reference's .meta fixtures show) or taken from a metafile;
 *   - num_max_readers reader threads pread (and LZ4/ZSTD-decode) chunks into
 *     pinned host buffers; num_threads device workers take the filled buffers,
 *     hipMemcpyAsync them on their own HIP stream and run the scan.  The pinned
 *     buffers circulate between the two stages (readers never run ahead by more
 *     than num_threads + 1 chunks);
 *   - partial results are published in chunk order; a consumer may read them
 *     while the search is still running (blocking cursor below).
 *   - under XSG_FLAG_CONTEXT a line-list job reports the context of the WHOLE searched
 *     range, however it was cut: every chunk is searched on its own, its worker keeps
 *     the few lines a neighbour may still want, and the seams are joined when the
 *     partial results are published (csrc/xsg_context.h).  Context crosses ONE seam
 *     between chunks at most: if it would reach across a whole chunk that is not the
 *     first or last of the range, the job fails with XSG_ENOTSUP from xsg_job_join
 *     (search with a larger chunk_bytes), never approximated.  At the ends of the
 *     range -- of [chunk_begin, chunk_end) -- context is clipped.
 * Errors: start fails for an unreadable file / bad metafile / no device; a
 * failure inside a worker stops the job and is returned by xsg_job_join. */
typedef struct xsg_job xsg_job;

typedef struct xsg_job_opts {
  uint32_t struct_size;     /* sizeof(xsg_job_opts), for ABI growth */
  uint32_t mode;            /* enum xsg_mode */
  uint32_t pattern_flags;   /* XSG_FLAG_* */
  int32_t device;           /* HIP device index */
  int32_t num_threads;      /* worker threads, >= 1 */
  int32_t num_max_readers;  /* concurrent reads, >= 1 */
  uint64_t chunk_bytes;     /* target chunk size without a metafile (default 16 MiB) */
  uint64_t chunk_begin;     /* search only chunks [chunk_begin, chunk_end) of the plan; 0,0 = all. */
  uint64_t chunk_end;       /* (how one rank of a multi-GPU job takes its contiguous range) */
  uint32_t pattern_is_list; /* != 0: `pattern` of xsg_job_start is a literal list (xsg_set_literals).  Honoured only when
                               struct_size covers it; xsg_job_opts_init zeroes it. */
} xsg_job_opts;
/* The structure grew by pattern_is_list (48 -> 56 bytes).  xsg_job_start still takes the 48-byte form from a caller that
 * fills struct_size by hand.  xsg_job_opts_init cannot know its caller's size: it clears and stamps sizeof(xsg_job_opts)
 * of the library it is in, so a program compiled against the 48-byte header that calls it must be rebuilt before it runs
 * with this library. */

typedef struct xsg_job_stats {
  uint64_t bytes_scanned;  /* uncompressed bytes handed to the GPU */
  uint64_t bytes_read;     /* bytes read from disk/page cache */
  uint64_t chunks;
  double seconds_total;    /* start -> last worker done */
  double seconds_read;     /* summed over workers */
  double seconds_decompress;
  double seconds_device;   /* H2D + kernels + D2H, summed over workers */
  uint64_t newlines;       /* XSG_LINE_INDICES without metafile bases: '\n' in the searched chunks */
  uint64_t plan_chunks;    /* chunks in the whole plan of the file (before the range was applied) */
} xsg_job_stats;

void xsg_job_opts_init(xsg_job_opts* opts);
/* meta_file_path may be NULL.  Returns immediately; the search runs in the
 * job's own threads. */
int xsg_job_start(const void* pattern, size_t plen, const char* file_path, const char* meta_file_path,
                  const xsg_job_opts* opts, xsg_job** out);
/* xsg_job_start for a literal list with list options (xsg_set_literals_opts: XSG_LIST_WHOLE_WORDS) -- an entry point of
 * its own because xsg_job_opts does not grow again.  It behaves as xsg_job_start with pattern_is_list forced on, whatever
 * `opts` says there; struct_size is read as xsg_job_start reads it.  XSG_FLAG_REGEX in opts->pattern_flags is XSG_EINVAL,
 * as for any list; an unknown bit of list_flags too.  list_flags == 0: xsg_job_start with pattern_is_list = 1. */
int xsg_job_start_list(const void* list, size_t n, uint32_t list_flags, const char* file_path,
                       const char* meta_file_path, const xsg_job_opts* opts, xsg_job** out);
/* xsg_job_start with a LIMIT PER FILE (grep --max-count): the result is the first max_count entries of what the same job
 * reports without a limit, over the searched range [chunk_begin, chunk_end); for the count tags it is min(total, max_count).
 * An entry point of its own because xsg_job_opts does not grow.  `opts` is read exactly as xsg_job_start reads it,
 * pattern_is_list included; list_flags are those of xsg_job_start_list and belong to a list: list_flags != 0 without
 * pattern_is_list is XSG_EINVAL.  max_count == 0 is xsg_job_start / xsg_job_start_list.
 *   The publisher is ordered: it keeps the remaining budget and appends min(remaining, entries of the chunk) of every chunk's
 * result -- for XSG_LINES the entries after an unterminated last line was dropped.  When the budget reaches 0 the job
 * stops reading and finishes normally: xsg_job_join returns XSG_OK, finished = 1; chunks behind that point are neither
 * reported nor, beyond the buffers already in circulation (2 x num_threads + 3 chunks), read.  For the count tags the running
 * totals are clamped to max_count, and the sequence of elements ends with the chunk that reached it.  xsg_job_stats counts
 * what was actually read and searched.  The workers' contexts carry the limit too (xsg_set_max_count): a chunk alone never
 * moves more than max_count rows.
 *   A limit together with non-zero XSG_FLAG_CONTEXT counts is XSG_ENOTSUP from this call (and from
 * xsg_fileset_start_max_count): the budget is only known in file order, and the seam stitcher joins lists that are already
 * widened.  xsg_set_max_count on a binding serves the combination. */
int xsg_job_start_max_count(const void* pattern, size_t plen, uint32_t list_flags, uint64_t max_count, const char* file_path,
                            const char* meta_file_path, const xsg_job_opts* opts, xsg_job** out);
/* Blocks until every worker has finished; returns the first worker error. */
int xsg_job_join(xsg_job* job);
/* Joins, then frees the job and everything it returned pointers into. */
void xsg_job_destroy(xsg_job* job);
/* Count tags: the count so far (final after join).  List tags: elements so far. */
int xsg_job_total(xsg_job* job, uint64_t* total);
/* Blocks until element `index` of the result sequence exists or the job has
 * finished.  *available = number of elements that exist now; *finished = 1 once
 * no more will come.  Count tags: element k = running total after k+1 chunks. */
int xsg_job_wait(xsg_job* job, uint64_t index, uint64_t* available, int* finished);
/* Non-blocking form of xsg_job_wait. */
int xsg_job_poll(xsg_job* job, uint64_t* available, int* finished);
int xsg_job_get_u64(xsg_job* job, uint64_t first, uint64_t n, uint64_t* out);
/* XSG_LINES: line `index`, XSG_MATCHES: match `index`; *data stays valid until xsg_job_destroy. */
int xsg_job_get_line(xsg_job* job, uint64_t index, const char** data, uint64_t* len);
int xsg_job_stats_get(xsg_job* job, xsg_job_stats* stats);

/* ======================================================================== */
/* File sets: a LIST of files searched in a few bindings                     */
/* ======================================================================== */
/* The sibling of the job API for many files: a source tree of 20 000 small files is 20 000 jobs there, each with its own
 * transfer, binding, launches and wait; here the files are the CHUNKS of a few bindings.  xsg_fileset_start returns at once,
 * the search runs in the set's own threads, and results are published per file in path order.
 * File f's result is what a search of that file ALONE reports: byte offsets relative to the file, line indices from 0,
 * context clipped at the file's edges, the default lossy end-of-chunk behaviour applied per chunk of the file's own plan.
 *   - A file of at most chunk_bytes is ONE chunk.  Readers pread it into a pinned batch buffer at the next multiple of 16; a
 *     batch closes when the next file would not fit batch_bytes, or at 2^20 files; it is uploaded, bound by xsg_shard_rebind
 *     (global_offset = 0, line_base = 0 per chunk) and searched with ONE xsg_count_chunks (the two count tags) or ONE
 *     xsg_search + xsg_result_chunk_ptr (the five list tags).  Two batch buffers: reading batch k + 1 overlaps the transfer
 *     and search of batch k; readers never run further ahead.
 *   - A file larger than chunk_bytes goes through xsg_job_start[_list] on the same device with the same chunk_bytes --
 *     that pipeline and its seam stitcher as they are -- and its result is spliced in at the file's place.
 *   - A path that cannot be read, a directory, or a file whose size changes under the read has the status XSG_EIO and an
 *     empty row; the rest are searched.  Only pattern, option and device errors fail xsg_fileset_start or _join.
 *   - xsg_count_chunks / xsg_search refuse a WHOLE binding that holds a byte >= 0x80 under an ASCII-only expression.  The
 *     set then searches that batch again one file per binding, and only the files that hold such a byte get XSG_ENOTSUP.
 *   - Results are a function of pattern, flags and file bytes only: identical for every batch_bytes, num_readers and cut.
 *   - Paths may repeat, each mention is a file; npaths == 0 is XSG_OK with nothing to report.
 * XSG_EINVAL from xsg_fileset_start: NULL paths (or a NULL path), a struct_size that is not sizeof(xsg_fileset_opts), a
 * mode that is no tag, batch_bytes < chunk_bytes, an empty or oversized pattern, unknown list_flags, list_flags without
 * pattern_is_list, num_readers < 0.  Patterns and flags the searches would refuse (xsg_set_pattern, xsg_set_literals_opts,
 * XSG_FLAG_INVERT or XSG_LIST_ALL_OF with a match tag, a pattern that can match '\n' with a line tag) are refused there
 * too, with the code the search would give. */
typedef struct xsg_fileset xsg_fileset;
typedef struct xsg_fileset_opts {
  uint32_t struct_size;     /* sizeof(xsg_fileset_opts) */
  uint32_t mode;            /* enum xsg_mode: any of the seven tags */
  uint32_t pattern_flags;   /* XSG_FLAG_* */
  uint32_t pattern_is_list; /* != 0: `pattern` is a literal list (xsg_set_literals) */
  uint32_t list_flags;      /* XSG_LIST_* (with pattern_is_list) */
  int32_t device;           /* HIP device index */
  int32_t num_readers;      /* 0: auto, never more than 16 */
  uint64_t batch_bytes;     /* 0: 256 MiB */
  uint64_t chunk_bytes;     /* 0: 16 MiB */
} xsg_fileset_opts;
void xsg_fileset_opts_init(xsg_fileset_opts* opts);  /* clears, stamps struct_size, mode = XSG_COUNT_LINES */
int xsg_fileset_start(const void* pattern, size_t plen, const char* const* paths, uint64_t npaths,
                      const xsg_fileset_opts* opts, xsg_fileset** out);
/* ... with a limit per FILE: every file's result is the first max_count entries of what xsg_fileset_start reports for it
 * (count tags: min(count, max_count)), identical for every batch_bytes, chunk_bytes and reader count.  Small files are
 * chunks of a binding under xsg_set_max_count, large ones go through xsg_job_start_max_count; the per-file search behind
 * a non-ASCII refusal carries the limit too.  max_count == 0 is xsg_fileset_start; with non-zero XSG_FLAG_CONTEXT counts
 * the call is XSG_ENOTSUP (see xsg_job_start_max_count). */
int xsg_fileset_start_max_count(const void* pattern, size_t plen, const char* const* paths, uint64_t npaths,
                                const xsg_fileset_opts* opts, uint64_t max_count, xsg_fileset** out);
/* Blocks until file `file_index` is published or the set has finished; *files_done = files published so far (they publish
 * in path order, so the files [0, *files_done) have their results), *finished = 1 once no more will come. */
int xsg_fileset_wait(xsg_fileset* set, uint64_t file_index, uint64_t* files_done, int* finished);
/* Blocks until the set has finished; returns its error (never a single file's: see xsg_fileset_status). */
int xsg_fileset_join(xsg_fileset* set);
/* Per file: XSG_OK or its XSG_E* (cap >= npaths); files not yet published read XSG_OK. */
int xsg_fileset_status(xsg_fileset* set, int32_t* status, uint64_t cap);
/* Per file: the count (count tags) or the number of its entries (list tags); cap >= npaths; not yet published: 0. */
int xsg_fileset_counts(xsg_fileset* set, uint64_t* counts, uint64_t cap);
/* List tags: npaths + 1 words, the entries [file_ptr[f], file_ptr[f + 1]) of the set's flat result are file f's (files
 * not yet published have empty rows at the current end).  XSG_ESTATE for a count tag. */
int xsg_fileset_file_ptr(xsg_fileset* set, uint64_t* file_ptr, uint64_t cap_rows);
/* The flat result, as far as it is published: uint64 tags / XSG_LINES and XSG_MATCHES (*data stays valid until
 * xsg_fileset_destroy). */
int xsg_fileset_get_u64(xsg_fileset* set, uint64_t first, uint64_t n, uint64_t* out);
int xsg_fileset_get_line(xsg_fileset* set, uint64_t index, const char** data, uint64_t* len);
/* Stops what is still running, joins, frees the set and everything it returned pointers into. */
void xsg_fileset_destroy(xsg_fileset* set);

/* ======================================================================== */
/* The lower seam: one chunk held in HOST memory                             */
/* ======================================================================== */
/* What a reference-style searcher functor calls for the chunk its reader just
 * produced (include/xsearch/tasks/searchers.h:38-93: IndexSearcher ->
 * byte_offsets_match, LineIndexSearcher -> byte_offsets_line, LineSearcher ->
 * line; concepts.h:36-39 SearcherC).  Results are CHUNK-LOCAL, exactly what the
 * search_wrappers.h functions return.  Thread-safe like the reference's shared
 * const functor (Searcher.h:110): concurrent callers use separate internal
 * slots (pinned staging buffer + device buffer + stream); callers beyond
 * max_slots wait for a free one.  include/xsearch/tasks/gpu_searchers.h wraps
 * these in functors with the reference's call signature. */
typedef struct xsg_host_searcher xsg_host_searcher;
int xsg_host_searcher_create(int device, const void* pattern, size_t plen, uint32_t flags, int max_slots,
                             xsg_host_searcher** out);
/* The same for a literal list (xsg_set_literals); every xsg_host_* call then works on it. */
int xsg_host_searcher_create_list(int device, const void* list, size_t n, uint32_t flags, int max_slots,
                                  xsg_host_searcher** out);
/* ... with list options (xsg_set_literals_opts); list_flags == 0 is the call above. */
int xsg_host_searcher_create_list_opts(int device, const void* list, size_t n, uint32_t flags, uint32_t list_flags,
                                       int max_slots, xsg_host_searcher** out);
void xsg_host_searcher_destroy(xsg_host_searcher* hs);
/* xsg_set_max_count on every slot's context, from the next call on: xsg_host_count returns min(count, max_count),
 * xsg_host_offsets, xsg_host_lines and xsg_host_matches the chunk's limited lists.  It may be changed between calls (a loop
 * over the chunks of a stream sets what is left of its budget); 0 clears it. */
int xsg_host_searcher_set_max_count(xsg_host_searcher* hs, uint64_t max_count);
/* search::count(data, pattern, skip_to_nl)  (search_wrappers.h:163-185) */
int xsg_host_count(xsg_host_searcher* hs, const void* data, uint64_t len, int skip_to_nl, uint64_t* count);
/* mode = XSG_MATCH_BYTE_OFFSETS / XSG_LINE_BYTE_OFFSETS / XSG_LINE_INDICES; *out is malloc'ed (xsg_free).
 * Under XSG_FLAG_CONTEXT this seam stays chunk-local like everything it returns: the context of xsg_host_offsets and
 * xsg_host_lines is clipped at the edges of the chunk handed in, and nothing joins consecutive calls. */
int xsg_host_offsets(xsg_host_searcher* hs, uint32_t mode, const void* data, uint64_t len, uint64_t** out,
                     uint64_t* n);
/* search::line (:187-207): n lines, lengths[i] bytes each, packed in *bytes; both malloc'ed (xsg_free) */
int xsg_host_lines(xsg_host_searcher* hs, const void* data, uint64_t len, uint64_t** lengths, char** bytes,
                   uint64_t* n, uint64_t* nbytes);
/* XSG_MATCHES of the chunk: n matches, lengths[i] bytes each, packed in *bytes; both malloc'ed (xsg_free) */
int xsg_host_matches(xsg_host_searcher* hs, const void* data, uint64_t len, uint64_t** lengths, char** bytes,
                     uint64_t* n, uint64_t* nbytes);

/* Counts per literal (xsg_count_literals) over chunks in host memory, ACCUMULATED: a reader loop that hands in the
 * newline-aligned chunks of a file gets the file's table -- a literal holds no '\n', so no occurrence straddles a cut.
 * The counter owns a context with the list, two pinned staging slots with device buffers and a stream each: _add copies
 * the chunk into a slot, enqueues its transfer and its pass and returns, so the transfer of one chunk overlaps the pass
 * over the one before; the running sums stay on the device.  _get waits for what is in flight and copies the sums out
 * (counts[0 .. k), cap_literals >= k or XSG_EINVAL; *bytes, optional: the bytes added so far); it may be called between
 * adds.  len == 0 adds nothing.  `flags`: those of xsg_set_literals; XSG_FLAG_INVERT is XSG_ENOTSUP.  One counter is used
 * from one thread at a time. */
typedef struct xsg_literal_counter xsg_literal_counter;
int xsg_literal_counter_create(int device, const void* list, size_t n, uint32_t flags, xsg_literal_counter** out);
/* ... with list options (xsg_set_literals_opts: under XSG_LIST_WHOLE_WORDS the edges of every chunk that is added are word
 * boundaries); list_flags == 0 is the call above. */
int xsg_literal_counter_create_opts(int device, const void* list, size_t n, uint32_t flags, uint32_t list_flags,
                                    xsg_literal_counter** out);
int xsg_literal_counter_add(xsg_literal_counter* lc, const void* data, uint64_t len);
int xsg_literal_counter_get(xsg_literal_counter* lc, uint64_t* counts, uint64_t cap_literals, uint64_t* bytes);
void xsg_literal_counter_destroy(xsg_literal_counter* lc);

/* Occurrences per literal (xsg_find_literals) of ONE chunk in host memory, synchronous: *pos and *lit receive malloc'ed
 * arrays of *n entries (xsg_free each; never NULL on XSG_OK), sorted by (position, listing index), pos[i] = base + p -- a
 * reader loop passes the chunk's offset in its file as `base` and gets file offsets.  len == 0 yields n = 0.  The finder
 * owns a context with the list, a pinned staging block and a device buffer.  `flags`, `list_flags`: those of
 * xsg_set_literals_opts; XSG_FLAG_INVERT is XSG_ENOTSUP; under XSG_LIST_WHOLE_WORDS the chunk's edges are word boundaries.
 * One finder is used from one thread at a time. */
typedef struct xsg_literal_finder xsg_literal_finder;
int xsg_literal_finder_create_opts(int device, const void* list, size_t n, uint32_t flags, uint32_t list_flags,
                                   xsg_literal_finder** out);
int xsg_literal_finder_find(xsg_literal_finder* lf, const void* data, uint64_t len, uint64_t base, uint64_t** pos,
                            uint32_t** lit, uint64_t* n);
void xsg_literal_finder_destroy(xsg_literal_finder* lf);

/* ---- chunk plans and metafiles (host only: usable without a GPU) ------------- */
/* One record of the reference's metafile (decoded from test/files/ *.meta,
 * field names from metafile_cat.cpp:39-49). */
typedef struct xsg_file_chunk {
  uint64_t original_offset; /* offset in the uncompressed stream */
  uint64_t actual_offset;   /* offset in the file on disk */
  uint64_t original_size;
  uint64_t actual_size;     /* == original_size when not compressed */
  uint64_t first_line;      /* global index of the first line of the chunk, or XSG_LINE_BASE_AUTO */
  uint64_t n_mappings;      /* metafile only: number of (byte offset, line index) pairs */
} xsg_file_chunk;

#define XSG_COMPRESSION_NONE 1
#define XSG_COMPRESSION_ZSTD 2
#define XSG_COMPRESSION_LZ4 3

/* Newline-aligned plan of a plain file: every chunk is >= target_bytes long and
 * ends just after a '\n' (the last one ends at EOF).  *chunks is malloc'ed:
 * release with xsg_free. */
int xsg_plan_chunks(const char* file_path, uint64_t target_bytes, xsg_file_chunk** chunks, uint64_t* n);
/* Parse a metafile.  mappings (optional) receives all (globalByteOffset,
 * globalLineIndex) pairs back to back, 2 uint64 each, n_mappings per chunk. */
int xsg_meta_read(const char* meta_path, int32_t* compression, xsg_file_chunk** chunks, uint64_t* n,
                  uint64_t** mappings, uint64_t* n_mapping_pairs);
/* Preprocess `file_path` into the reference's on-disk layout: writes the
 * metafile and, for ZSTD/LZ4, the chunk-wise compressed data file
 * (data_out_path; ignored for XSG_COMPRESSION_NONE).  mapping_gap = minimum
 * distance in bytes between two mapping entries (fixtures: 500). */
int xsg_meta_write(const char* file_path, const char* meta_out_path, const char* data_out_path, int32_t compression,
                   uint64_t chunk_bytes, uint64_t mapping_gap, int hc);
void xsg_free(void* p);
/* Which decoder serves a compression type on this host (loads it if need be): "liblz4" / "libzstd" (the system's
 * shared library, what the reference links: Dockerfile:8), "built-in LZ4 block codec" (csrc/xsg_lz4.h, when the host
 * has no liblz4 or XSG_NO_LIBLZ4=1), "none" for XSG_COMPRESSION_NONE, "" if the type cannot be served here. */
const char* xsg_codec_name(int32_t compression);

/* ======================================================================== */
/* Multi-GPU: the one exchange step, RCCL over xGMI                           */
/* ======================================================================== */
/* The reference's only parallelism is N threads over chunks (include/xsearch/Searcher.h:141-145).  Across GPUs
 * the chunk list is cut into contiguous ranges (xsg_job_opts.chunk_begin/_end, or one shard per device) and
 * searched with no data-path collective; what is exchanged once per search is
 *   - the counter vector (xs::count / xs::count_lines): ncclAllReduce(sum) of XSG_NUM_COUNTERS uint64
 *   - one uint64 per device, its '\n' total (xs::line_indices without a metafile): ncclAllGather
 * 8-32 byte messages: latency-bound.  librccl is bound at run time (the copy the process already carries --
 * e.g. PyTorch-ROCm's -- else the system's); without one the create calls return XSG_ENOTSUP and the caller sums
 * on the host instead (include/xsearch/xsearch.h does exactly that). */
typedef struct xsg_comm xsg_comm;
#define XSG_COMM_ID_BYTES 128
/* rank form (one process per GPU): rank 0 makes an id, hands it to the others by any means (file, socket,
 * torch.distributed store), every rank then creates its end. */
int xsg_comm_unique_id(void* id, size_t cap);
int xsg_comm_create_rank(xsg_ctx* ctx, int nranks, int rank, const void* id, xsg_comm** out);
/* local form (one process, n GPUs): one communicator over the devices of ctxs[0..n), all distinct. */
int xsg_comm_create_local(xsg_ctx* const* ctxs, int n, xsg_comm** out);
/* Destroy a communicator BEFORE the contexts it was made from are used for nothing else: the collectives run on the
 * contexts' streams, so a ctx must outlive every collective still queued on it (destroying the ctx first is tolerated by
 * xsg_comm_destroy itself -- it keeps the device numbers by value -- but not by a collective in flight). */
void xsg_comm_destroy(xsg_comm* comm);
int xsg_comm_size(xsg_comm* comm, int* nranks, int* rank /* -1 in the local form */);
/* path of the librccl in use ("" if none) */
const char* xsg_comm_library(void);
/* rank form: in-place sum over the ranks of k uint64 device words (e.g. what xsg_count_async wrote), enqueued
 * on `stream` (a hipStream_t; NULL = the ctx's own) -- stream-ordered behind the count that produced them. */
int xsg_reduce_counts_async(xsg_comm* comm, uint64_t* d_counters, int k, void* stream);
/* either form, blocking: totals[0..k) = the sums; the device vectors are left summed in place.
 * rank form: d_counters[0] is this rank's vector; local form: d_counters[i] lives on ctxs[i]'s device. */
int xsg_reduce_counts(xsg_comm* comm, uint64_t* const* d_counters, int k, uint64_t* totals);
/* either form, blocking: out[0..nranks) = every rank's / device's value in rank order (mine[0], or mine[i] for
 * ctxs[i]); the exclusive prefix -- the line-index base of each range -- is the caller's to take. */
int xsg_allgather_u64(xsg_comm* comm, const uint64_t* mine, uint64_t* out);

/* NUMA placement of a device: its node (-1 if the platform does not say) and the CPUs next to it (the PCI device's
 * local_cpulist, e.g. "0-63,128-191").  The reader and device-worker threads of a job are bound to those CPUs
 * (XSG_NUMA=0 switches that off); its pinned buffers are allocated on that node by hipHostMalloc. */
int xsg_device_numa(int device, int* node, char* cpulist, size_t cap);

/* The count of a search that fanned out over several devices (one job each, contiguous chunk ranges): the sum of
 * the jobs' totals, exchanged over RCCL (one ncclAllReduce of one uint64 over a per-process communicator of the
 * jobs' devices, created at first use).  *via_rccl (optional) = 1 if it went that way, 0 if the sum was taken on
 * the host instead: no librccl, a device listed twice, a single job, or XS_REDUCE=host.  Call after the joins. */
int xsg_jobs_reduce_total(xsg_job* const* jobs, int n, uint64_t* total, int* via_rccl);

/* ---- diagnostics ------------------------------------------------------------ */
/* Name of the device the ctx is bound to (e.g. "gfx950..."), CU count. */
int xsg_ctx_info(xsg_ctx* ctx, char* arch, size_t arch_cap, int* compute_units, uint64_t* hbm_bytes);
/* Time the dominant kernel alone: runs the bulk scan kernel of the given count
 * mode `iters` times back to back on the ctx stream between two HIP events and
 * returns the average milliseconds per launch (bench.py's roofline figure). */
/* (A literal list: the candidate count pass, xsg::k_set_scan.) */
int xsg_time_scan_kernel(xsg_shard* shard, uint32_t mode, int iters, float* avg_ms);
/* Name of the bulk-kernel instantiation the next pass of `mode` launches on this shard with the current pattern
 * ("xsg::k_scan<KIND, WANT_NL, WANT_LINES, EMIT, LOADS, ICASE> stagger=N"): what a profile of that pass shows.
 * " gated by xsg::k_sketch (512 B/tile)" follows when that pass would run behind the binding's sketch: this
 * instantiation on a bounded grid, which selects the candidate tiles and scans them; " finishing (xsg::k_scan_fin)" in
 * front of it: the count of this mode is that one launch, the finishing form, with no xsg::k_count_finish behind it
 * (xsg_time_scan_kernel and xsg_shard_tune time that form for such a mode).  A literal list:
 * "xsg::k_set_scan<EMIT, ICASE> g=N + xsg::k_set_verify". */
int xsg_scan_kernel_name(xsg_shard* shard, uint32_t mode, char* out, size_t cap);
/* Measure and fix the bulk kernel's wave stagger for this shard, the current pattern and `mode` (a handful of
 * launches; replaces the per-variant default until the shard is destroyed or tuned again).  *chosen (optional)
 * receives the value, or UINT32_MAX when the default was kept (shard under 1 GiB, XSG_TUNE set, an expression of
 * variable length or a literal list: their kernels have no stagger).
 * A caller that tunes is investing in the binding: for a plain count mode and a pattern the sketch serves, the
 * binding's sketch is built first (bindings of 64 MiB and more: about two full scans' worth of time, once), and the
 * sweep then times the kernel the later passes launch, gated where the gate pays. */
int xsg_shard_tune(xsg_shard* shard, uint32_t mode, uint32_t* chosen);
/* (The read-only HBM probes of round 1 -- xsg_time_read_ceiling and friends -- moved to libxsg_diag.so,
 * x-search_amd/csrc/diag/xsg_diag.hip: the product library holds search code only.) */

#ifdef __cplusplus
}
#endif
#endif /* XSG_H */
