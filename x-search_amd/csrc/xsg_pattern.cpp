// xsg_pattern.cpp -- the C ABI of include/xsg.h, part 2: patterns.  Literals, class sequences and the automaton pair
// are compiled on the host and their device images uploaded (xsg_set_pattern); the xsg_regex_* queries report what
// the compilers made of an expression.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "xsg_classseq.h"
#include "xsg_regex.h"
#include "xsg_set.h"
#include "xsg_host.h"
#include "xsg_sketch.h"

using namespace xsg;

static int set_pattern_plain(xsg_ctx* c, const void* pattern, size_t plen, uint32_t flags);  // xsg_set_pattern without XSG_FLAG_INVERT / XSG_FLAG_CONTEXT

static uint32_t le32(const uint8_t* p, size_t n) {
  uint32_t v = 0;
  for (size_t i = 0; i < 4 && i < n; ++i) v |= (uint32_t)p[i] << (8 * i);
  return v;
}
// Which 8 bytes of a long pattern should the hot loop look for?  The slow path runs for
// every wave-load that holds the window somewhere, so the window should be rare in
// text: one that spans a word boundary is (a pair of words is far rarer than either
// word), then upper case / digits / non-ASCII, then the rarer letters.  Static
// heuristic, no look at the data; `detective street` -> "ective s".
static int byte_rarity(uint8_t c, int pos_in_window) {
  const bool lower = c >= 'a' && c <= 'z', upper = c >= 'A' && c <= 'Z', digit = c >= '0' && c <= '9';
  if (c >= 0x80) return 30;
  if (!lower && !upper && !digit) return (pos_in_window >= 1 && pos_in_window <= 6) ? 40 : 10;
  if (upper || digit) return 12;
  if (strchr("jqxzvkwbypgf", c)) return 6;
  return 1;
}

uint32_t xsg::pick_filter_window(const uint8_t* p, size_t plen) {
  if (plen <= 8) return 0;
  uint32_t best = 0;
  int best_score = -1;
  for (size_t k = 0; k + 8 <= plen; ++k) {
    int score = 0;
    for (int i = 0; i < 8; ++i) score += byte_rarity(p[k + i], i);
    if (score > best_score) {
      best_score = score;
      best = (uint32_t)k;
    }
  }
  return best;
}

static uint32_t mask32(size_t n) { return n >= 4 ? 0xffffffffu : (n == 0 ? 0u : ((1u << (8 * n)) - 1u)); }

void xsg::window_fields(const uint8_t* p, size_t plen, uint32_t koff, PatternDev* P) {
  const uint8_t* w = p + koff;
  const size_t wlen = plen - koff;  // >= 8 when koff > 0
  P->koff = koff;
  P->p0 = le32(w, wlen);
  P->m0 = mask32(wlen);
  P->p1 = wlen > 4 ? le32(w + 4, wlen - 4) : 0u;
  P->m1 = wlen > 4 ? mask32(wlen - 4) : 0u;
  P->q0 = (P->p0 | 0x20202020u) & P->m0;
  P->q1 = (P->p1 | 0x20202020u) & P->m1;
  // (x | 0x20) == (p | 0x20) holds exactly for x in {p, p - 32} when p is a lower-case letter (the pattern is
  // already lowered): a window of letters only needs no second look under ignore_case
  bool letters = true;
  for (size_t i = 0; i < 8 && i < wlen; ++i) letters &= w[i] >= 'a' && w[i] <= 'z';
  P->lazy_exact = letters ? 1u : 0u;
}

// Long patterns: the windows worth MEASURING on the data (choose_hot_filter): the static heuristic's pick first, then
// the next best-looking ones -- every position for patterns up to 20 bytes, the eight best scores beyond.
static std::vector<uint32_t> window_candidates(const uint8_t* p, size_t plen) {
  std::vector<uint32_t> out;
  if (plen <= 8) return out;
  std::vector<std::pair<int, uint32_t>> scored;
  for (size_t k = 0; k + 8 <= plen; ++k) {
    int score = 0;
    for (int i = 0; i < 8; ++i) score += byte_rarity(p[k + i], i);
    scored.push_back({-score, (uint32_t)k});
  }
  std::stable_sort(scored.begin(), scored.end());
  const size_t n = plen <= 20 ? scored.size() : std::min<size_t>(scored.size(), 8);
  for (size_t i = 0; i < n; ++i) out.push_back(scored[i].second);
  return out;
}

// The window-filter fields of a class expression and the device image of its sets (alternative-major, 32 bytes per
// set) -- for a pattern of its own (set_class_pattern) and for the prefilter of the automaton route (set_dfa_pattern).
static void class_fields(const xsg::ClassExpr& ex, bool icase, PatternDev* Pout, std::vector<uint8_t>* blob) {
  const size_t plen = ex.npos;
  const std::vector<xsg::ByteSet> seq = xsg::union_sets(ex);
  // What the window compare can know about a position: the bits all members of its set agree on (a literal: all
  // eight; [Ss]: seven; [0-9]: the upper four; [a-z]: the upper three).  (x & agree) == (member & agree) holds for
  // every member x, so it is a superset filter at no cost -- the compare is masked per byte anyway -- and the
  // exact decision against the sets follows for the rare candidate.  With several alternatives the sets are the
  // position-wise unions.
  std::vector<uint8_t> agree(plen), value(plen);
  for (size_t k = 0; k < plen; ++k) {
    int first = -1;
    uint32_t diff = 0;
    for (uint32_t b = 0; b < 256; ++b)
      if (xsg::set_has(seq[k], b)) {
        if (first < 0) first = (int)b;
        diff |= b ^ (uint32_t)first;
      }
    agree[k] = (uint8_t)~diff;
    value[k] = (uint8_t)((uint32_t)first & ~diff);
  }
  // the window that pins the most bits (rarer literal bytes break ties)
  uint32_t koff = 0;
  int best = -1;
  for (size_t k = 0; k < plen; ++k) {
    int score = 0;
    for (int i = 0; i < 8 && k + i < plen; ++i) {
      score += 16 * __builtin_popcount(agree[k + i]);
      if (agree[k + i] == 0xff) score += byte_rarity(value[k + i], i);
    }
    // a window whose positions 0, 1 and 4..7 are single bytes takes the exact 16 + 32 bit filter (PatternDev::cls_fast)
    if (k + 8 <= plen && agree[k] == 0xff && agree[k + 1] == 0xff && agree[k + 4] == 0xff && agree[k + 5] == 0xff &&
        agree[k + 6] == 0xff && agree[k + 7] == 0xff)
      score += 48;
    if (score > best) best = score, koff = (uint32_t)k;
  }
  uint32_t pw[2] = {0, 0}, mw[2] = {0, 0};
  for (int i = 0; i < 8 && koff + i < plen; ++i) {
    pw[i >> 2] |= (uint32_t)value[koff + i] << (8 * (i & 3));
    mw[i >> 2] |= (uint32_t)agree[koff + i] << (8 * (i & 3));
  }
  constexpr size_t kSetBytes = xsg::kMaxAltSets * sizeof(xsg::ByteSet);
  blob->assign(std::max<size_t>(XSG_MAX_REGEX, kSetBytes) + 16, 0);
  for (size_t a = 0; a < ex.alts.size(); ++a)
    memcpy(blob->data() + a * plen * sizeof(xsg::ByteSet), ex.alts[a].data(), plen * sizeof(xsg::ByteSet));
  PatternDev& P = *Pout;
  P = PatternDev{};
  P.plen = (uint32_t)plen;
  P.kind = kClass;
  P.koff = koff;
  P.p0 = pw[0], P.m0 = mw[0], P.p1 = pw[1], P.m1 = mw[1];
  P.q0 = (P.p0 | 0x20202020u) & P.m0, P.q1 = (P.p1 | 0x20202020u) & P.m1;
  {
    const char* cf = XSG_TOGGLE("XSG_CLS_FAST");
    P.cls_fast = (P.m1 == 0xffffffffu && (P.m0 & 0xffffu) == 0xffffu && !(cf && *cf == '0')) ? 1u : 0u;
  }
  P.exact_tail = 1u;
  P.icase = icase ? 1u : 0u;
  P.nalt = (uint32_t)ex.alts.size();
  // Up to 8 positions: the filter window is the whole expression and candidates are decided in registers.  A position
  // needs no look at its set when the hot filter's compare already decides it exactly: one alternative, and the set
  // is precisely the bytes that agree with `value` under `agree` (a literal; [Ss]; [a-z] is not: 0x60-0x7f pass the
  // compare) -- and, under the 16 + 32 bit filter, the position is not one of the two that filter leaves out.
  // With several alternatives only a position that is one byte in all of them is decided (the compare sees the union).
  {
    const char* ir = XSG_TOGGLE("XSG_CLS_INREG");
    P.cls_chk = 0;
    for (size_t k = 0; k < plen && k < 8; ++k) {
      bool decided = true;
      for (uint32_t b = 0; b < 256 && decided; ++b)
        decided = xsg::set_has(seq[k], b) == ((b & agree[k]) == value[k]);
      if (ex.alts.size() > 1 && agree[k] != 0xff) decided = false;
      if (P.cls_fast && (k == 2 || k == 3)) decided = false;  // (the aligned trigger's slow path uses the full masks, but one table serves both)
      if (!decided) P.cls_chk |= 1u << k;
    }
    // Measured on whole calls (scripts/ab_inreg.py, 20 GiB): one alternative with something left to look up wins
    // (`She[r ]lock` 4.38 -> 4.05 ms); several alternatives lose (the candidate scan of `Sherlock|Holmes`, two
    // alternatives, dense candidates: 33 -> 61 ms: a scalar loop per alternative and position); and an expression the
    // compare decides completely (one alternative, nothing to look up: `Sher`, `[Ss]herlock`) needs no verification
    // at all -- its candidate bits ARE its matches (cls_exact).
    const bool one = ex.alts.size() == 1 && plen <= 8 && koff == 0;
    P.cls_inreg = (one && P.cls_chk != 0 && !(ir && *ir == '0')) ? 1u : 0u;
    P.cls_exact = (one && P.cls_chk == 0 && !P.cls_fast && !(ir && *ir == '0')) ? 1u : 0u;
  }
  P.ascii_only = ex.ascii_only ? 1u : 0u;
  P.has_newline = 0;
  for (const xsg::ByteSet& st : seq) P.has_newline |= xsg::set_has(st, '\n') ? 1u : 0u;
}

// A pattern's device image: room for at least `min_cap` bytes, the blob copied in and the copy waited for (the blobs
// are locals of their callers).
static int upload_pattern_blob(xsg_ctx* c, DevBuf& buf, const void* data, size_t bytes, size_t min_cap = 0) {
  XSG_TRY(buf.ensure(std::max(bytes, min_cap)));
  HIP_TRY(hipMemcpyAsync(buf.p, data, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XSG_OK;
}

// The automaton route's compiler for an expression the class-sequence compiler refused or handed over;
// `why_not_class`: what that one said, for the message if this route refuses too.
static int dfa_route_serves(const uint8_t* re, size_t n, uint32_t flags, const std::string& why_not_class, xsg::RegexDfa* out) {
  std::string err;
  if (!xsg::compile_regex_dfa(re, n, (flags & XSG_FLAG_IGNORE_CASE) != 0, out, &err))
    return fail(XSG_ENOTSUP, "regex not supported by the GPU matchers: %s [as a fixed-length expression: %s]", err.c_str(),
                why_not_class.c_str());
  return XSG_OK;
}

// layout of the device copy of a RegexDfa: class_of[256], then the forward table, then (16-byte aligned) the reverse one
static size_t rx_rev_offset(uint32_t fwd_entries) { return (256 + 2 * (size_t)fwd_entries + 15) & ~(size_t)15; }

// XSG_FLAG_REGEX, second route: an expression of variable length, as a pair of byte-class DFAs for k_rx_scan
// (xsg_regex.h).  `why_not_class`: what the class-sequence compiler said, for the message if this route refuses too.
static int set_dfa_pattern(xsg_ctx* c, const uint8_t* re, size_t n, uint32_t flags, const std::string& why_not_class) {
  xsg::RegexDfa dfa;
  XSG_TRY(dfa_route_serves(re, n, flags, why_not_class, &dfa));
  HIP_TRY(hipSetDevice(c->device));
  c->pattern.assign(re, re + n);
  c->flags = flags;
  ++c->pattern_serial;
  c->koff_cands.clear();
  c->sketch_hashes.clear();
  c->span_hashes.clear();
  c->bordered = false;  // the kernel walks every line as the reference does: what it reports is already non-overlapping
  c->overlap_words.clear();
  // The table the line walks step (k_rx_scan / k_rx_count): the anchored automaton for the line-anchor form (`^` walks
  // it; `$` alone walks the reverse automaton and ships `anc` only for its start row), else the forward one.
  const bool anchored = dfa.anchor_begin || dfa.anchor_end;
  const std::vector<uint16_t>& walk = anchored ? dfa.anc : dfa.fwd;
  // a TRIGGER can begin a match: it moves the unanchored automaton out of its start state, or equally takes the
  // anchored one to a live state.  (Anchored walks do not skip, but a span without a trigger still holds no match start.)
  auto trigger = [&](uint32_t b) {
    return anchored ? dfa.anc[(size_t)dfa.anc_start * dfa.ncls + dfa.class_of[b]] != 0
                    : dfa.fwd[(size_t)dfa.fwd_start * dfa.ncls + dfa.class_of[b]] != dfa.fwd_start * dfa.ncls;
  };
  const size_t rev_off = rx_rev_offset((uint32_t)walk.size());
  const size_t anc_off = (rev_off + 2 * dfa.rev.size() + 15) & ~(size_t)15;
  const size_t bytes = anc_off + 2 * dfa.anc.size() + 16;
  std::vector<uint8_t> blob(bytes, 0);
  memcpy(blob.data() + anc_off, dfa.anc.data(), 2 * dfa.anc.size());
  memcpy(blob.data(), dfa.class_of, 256);
  // Trigger bytes: those that move the forward automaton out of its start state (a byte that cannot begin a match
  // leaves it there), and '\n'.  Flagged in bit 7 of the class table; k_rx_scan's walks jump from trigger to trigger.
  const char* skip_env = XSG_TOGGLE("XSG_RX_SKIP");
  bool skip = dfa.ncls <= 128 && !dfa.multiline && !(skip_env && *skip_env == '0');
  if (skip && !(skip_env && *skip_env == '1')) {
    // skipping pays when triggers are rare in the data; an expression that can begin with most letters (`\\w+ing`)
    // triggers at every word and the jumps cost more than the steps they replace (measured: 156 against 201 GB/s)
    uint32_t common = 0;
    for (uint32_t b = 'a'; b <= 'z'; ++b) common += trigger(b);
    if (common >= 9) skip = false;
  }
  if (skip)
    for (uint32_t b = 0; b < 256; ++b)
      if (b == '\n' || trigger(b)) blob[b] |= 0x80u;
  memcpy(blob.data() + 256, walk.data(), 2 * walk.size());
  memcpy(blob.data() + rev_off, dfa.rev.data(), 2 * dfa.rev.size());
  XSG_TRY(upload_pattern_blob(c, c->d_pat, blob.data(), bytes, XSG_MAX_REGEX + 16));
  PatternDev& P = c->pat;
  P = PatternDev{};
  P.plen = dfa.minlen;  // what the list kernels may skip behind a match start before they look for the line's end
  P.kind = kDfa;
  P.d_pat = c->d_pat.as<uint8_t>();
  P.exact_tail = 1u;
  P.icase = 0u;  // the sets are closed under case; the data is not folded
  P.ascii_only = dfa.ascii_only ? 1u : 0u;
  P.has_newline = dfa.multiline ? 1u : 0u;  // a match may span lines: the line tags are refused, as for a literal with '\n'
  P.rx_multiline = dfa.multiline ? 1u : 0u;
  P.rx_ncls = dfa.ncls;
  P.rx_fwd_n = (uint32_t)walk.size();
  P.rx_rev_n = (uint32_t)dfa.rev.size();
  P.rx_fwd_start = (anchored ? dfa.anc_start : dfa.fwd_start) * dfa.ncls;
  P.rx_fwd_acc = (anchored ? dfa.anc_first_acc : dfa.fwd_first_acc) * dfa.ncls;
  P.rx_bol = dfa.anchor_begin ? 1u : 0u;
  P.rx_eol = dfa.anchor_end ? 1u : 0u;
  P.rx_rev_start = dfa.rev_start * dfa.ncls;
  P.rx_rev_acc = dfa.rev_first_acc * dfa.ncls;
  P.rx_skip = skip ? 1u : 0u;
  // few trigger byte values (`Sherlock|Holmes`: S, H; `Sher.*mes`: S; closed under case: up to four): k_rx_scan looks for
  // them with byte-parallel compares on its loads and does not stage a tile that holds none (XSG_RX_TRIG=0 switches it off)
  if (skip) {
    const char* te = XSG_TOGGLE("XSG_RX_TRIG");
    uint32_t n = 0, packed = 0;
    for (uint32_t b = 0; b < 256; ++b)
      if (b != '\n' && (blob[b] & 0x80u)) {
        if (n < 4) packed |= b << (8 * n);
        ++n;
      }
    if (n >= 1 && n <= 4 && !(te && *te == '0')) {
      for (uint32_t k = n; k < 4; ++k) packed |= (packed & 0xffu) << (8 * k);  // unused slots repeat the first value
      P.rx_ntrig = n;
      P.rx_trig4 = packed;
    }
  }
  P.rx_anc_n = (uint32_t)dfa.anc.size();
  P.rx_anc_start = dfa.anc_start * dfa.ncls;
  P.rx_anc_acc = dfa.anc_first_acc * dfa.ncls;
  // A selective start: the synchronous entry points find candidates with the class-sequence matcher and verify them
  // (xsg_list.cpp: prefilter_candidates); xsg_count_async, which may not wait for the host, keeps k_rx_scan.  XSG_RX_PRE=0 switches it off.
  const char* pre_env = XSG_TOGGLE("XSG_RX_PRE");
  c->rx_pre = dfa.prefix.npos != 0 && !(pre_env && *pre_env == '0');
  c->rx_pre_forced = pre_env && *pre_env == '1';  // on shards of any size (tests; by default only where it pays, use_prefilter)
  if (c->rx_pre) {
    std::vector<uint8_t> pblob;
    class_fields(dfa.prefix, false, &c->pre_pat, &pblob);  // the sets are closed under case already: no folding
    XSG_TRY(upload_pattern_blob(c, c->d_pre, pblob.data(), pblob.size()));
    c->pre_pat.d_pat = c->d_pre.as<uint8_t>();
    c->pre_pat.ascii_only = P.ascii_only;  // the candidate scan reads every byte: it raises the refusal flag
  }
  // No selective start, but a factor every match contains (`\\w+ing`: `\\wing`): lines without it have no match, and the
  // synchronous entry points first mark the tiles in which a line with an occurrence starts (ensure_factor_mask).
  const char* fac_env = XSG_TOGGLE("XSG_RX_FAC");
  c->rx_fac = !c->rx_pre && dfa.factor.npos != 0 && !(fac_env && *fac_env == '0');
  c->rx_fac_forced = fac_env && *fac_env == '1';
  if (c->rx_fac) {
    std::vector<uint8_t> fblob;
    class_fields(dfa.factor, false, &c->fac_pat, &fblob);
    XSG_TRY(upload_pattern_blob(c, c->d_fac, fblob.data(), fblob.size()));
    c->fac_pat.d_pat = c->d_fac.as<uint8_t>();
    c->fac_pat.ascii_only = P.ascii_only;
  }
  return XSG_OK;
}

// Where set_class_pattern sends an expression the class-sequence compiler took (and what xsg_test_class_fields answers for):
// (?m)^BODY$ with a fixed-length BODY goes to the automaton route, whose line walks decide the anchors; one alternative
// of single bytes (`a\.b`) is an ordinary literal (*lit), minus the reference's scalar-tail quirk (RE2 has none); the rest
// is class_fields'.
enum ClassRoute { kRouteClass, kRouteAutomaton, kRouteLiteral };
static ClassRoute class_route(const xsg::ClassExpr& ex, const std::vector<xsg::ByteSet>& seq, std::vector<uint8_t>* lit) {
  if (ex.anchor_begin || ex.anchor_end) return kRouteAutomaton;
  bool literal = ex.alts.size() == 1;
  lit->assign(seq.size(), 0);
  for (size_t k = 0; k < seq.size(); ++k) {
    const int b = xsg::set_single(seq[k]);
    literal &= b >= 0;
    (*lit)[k] = (uint8_t)(b >= 0 ? b : 0);
  }
  return literal ? kRouteLiteral : kRouteClass;
}

// XSG_FLAG_REGEX: a fixed-length class sequence (xsg_classseq.h).  RE2 has no lossy tail, so the
// matching is exact up to the end of the chunk (as with XSG_FLAG_EXACT_TAIL).
static int set_class_pattern(xsg_ctx* c, const uint8_t* re, size_t n, uint32_t flags) {
  xsg::ClassExpr ex;
  std::string err;
  const bool icase = (flags & XSG_FLAG_IGNORE_CASE) != 0;
  if (!xsg::compile_class_expr(re, n, icase, &ex, &err)) return set_dfa_pattern(c, re, n, flags, err);
  const size_t plen = ex.npos;
  const std::vector<xsg::ByteSet> seq = xsg::union_sets(ex);  // what the filter, the overlap and '\n' tests look at
  std::vector<uint8_t> lit;
  switch (class_route(ex, seq, &lit)) {
    case kRouteAutomaton: return set_dfa_pattern(c, re, n, flags, "line anchors");
    case kRouteLiteral: return set_pattern_plain(c, lit.data(), plen, (flags & XSG_FLAG_IGNORE_CASE) | XSG_FLAG_EXACT_TAIL);
    case kRouteClass: break;
  }

  HIP_TRY(hipSetDevice(c->device));
  c->pattern.assign(re, re + n);
  c->flags = flags;
  ++c->pattern_serial;
  c->koff_cands.clear();
  c->sketch_hashes.clear();
  c->span_hashes.clear();
  c->bordered = xsg::sequence_can_overlap(seq);
  c->overlap_words.clear();
  std::vector<uint8_t> blob;
  PatternDev P;
  class_fields(ex, icase, &P, &blob);
  XSG_TRY(upload_pattern_blob(c, c->d_pat, blob.data(), blob.size()));
  P.d_pat = c->d_pat.as<uint8_t>();
  c->pat = P;
  c->rx_pre = false;
  c->rx_fac = false;
  return XSG_OK;
}

static int check_expr(const void* expr, size_t n) {
  if (!expr || n == 0) return fail(XSG_EINVAL, "empty expression");
  if (n > XSG_MAX_REGEX) return fail(XSG_EINVAL, "expression longer than %u bytes", XSG_MAX_REGEX);
  return XSG_OK;
}

// What every xsg_regex_* query starts with: the argument checks, then xsg_set_pattern's compile attempts.  `ex` null:
// the automaton route alone (*dfa).  Else the class-sequence compiler first (*fixed: it served, *ex is valid), and the
// automaton route (*dfa) for what it refuses or hands over -- line anchors, as set_class_pattern does.
static int compile_for_query(const void* expr, size_t n, uint32_t flags, xsg::ClassExpr* ex, bool* fixed, xsg::RegexDfa* dfa) {
  XSG_TRY(check_expr(expr, n));
  const uint8_t* re = static_cast<const uint8_t*>(expr);
  const bool icase = (flags & XSG_FLAG_IGNORE_CASE) != 0;
  std::string err;
  if (!ex) {
    if (!xsg::compile_regex_dfa(re, n, icase, dfa, &err))
      return fail(XSG_ENOTSUP, "regex not supported by the automaton route: %s", err.c_str());
    return XSG_OK;
  }
  *fixed = xsg::compile_class_expr(re, n, icase, ex, &err);
  if (*fixed && !ex->anchor_begin && !ex->anchor_end) return XSG_OK;
  return dfa_route_serves(re, n, flags, *fixed ? "line anchors" : err, dfa);
}

extern "C" int xsg_regex_dfa_info(const void* expr, size_t n, uint32_t flags, xsg_regex_dfa* info, uint16_t* fwd,
                                  uint16_t* rev, size_t cap_entries) {
  XSG_TRY(check_expr(expr, n));  // (ahead of `info`: the refusal a call wrong in both ways has always got)
  if (!info) return fail(XSG_EINVAL, "info is null");
  xsg::RegexDfa dfa;
  XSG_TRY(compile_for_query(expr, n, flags, nullptr, nullptr, &dfa));
  info->ncls = dfa.ncls, info->minlen = dfa.minlen, info->ascii_only = dfa.ascii_only ? 1u : 0u;
  info->multiline = dfa.multiline ? 1u : 0u;
  info->prefix_positions = dfa.prefix.npos;
  info->prefix_alternatives = (uint32_t)dfa.prefix.alts.size();
  info->factor_positions = dfa.factor.npos;
  info->fwd_states = dfa.fwd_states, info->fwd_start = dfa.fwd_start, info->fwd_first_acc = dfa.fwd_first_acc;
  info->rev_states = dfa.rev_states, info->rev_start = dfa.rev_start, info->rev_first_acc = dfa.rev_first_acc;
  memcpy(info->class_of, dfa.class_of, 256);
  if (fwd && cap_entries >= dfa.fwd.size()) memcpy(fwd, dfa.fwd.data(), 2 * dfa.fwd.size());
  if (rev && cap_entries >= dfa.rev.size()) memcpy(rev, dfa.rev.data(), 2 * dfa.rev.size());
  return XSG_OK;
}

extern "C" int xsg_regex_prefix(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* alternatives,
                                uint32_t* sets) {
  xsg::RegexDfa dfa;
  XSG_TRY(compile_for_query(expr, n, flags, nullptr, nullptr, &dfa));
  if (positions) *positions = dfa.prefix.npos;
  if (alternatives) *alternatives = (uint32_t)dfa.prefix.alts.size();
  if (sets)
    for (size_t a = 0; a < dfa.prefix.alts.size(); ++a)
      memcpy(sets + a * dfa.prefix.npos * 8, dfa.prefix.alts[a].data(), dfa.prefix.npos * sizeof(xsg::ByteSet));
  return XSG_OK;
}

extern "C" int xsg_regex_factor(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* sets) {
  xsg::RegexDfa dfa;
  XSG_TRY(compile_for_query(expr, n, flags, nullptr, nullptr, &dfa));
  if (positions) *positions = dfa.factor.npos;
  if (sets && dfa.factor.npos) memcpy(sets, dfa.factor.alts[0].data(), dfa.factor.npos * sizeof(xsg::ByteSet));
  return XSG_OK;
}

extern "C" int xsg_regex_check(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* sets) {
  xsg::ClassExpr ex;
  xsg::RegexDfa dfa;
  bool fixed = false;
  XSG_TRY(compile_for_query(expr, n, flags, &ex, &fixed, &dfa));
  if (!fixed) {
    if (positions) *positions = 0;  // variable length: no position-wise sets; such an expression never accepts '\n'
    return XSG_OK;
  }
  const std::vector<xsg::ByteSet> seq = xsg::union_sets(ex);
  if (positions) *positions = (uint32_t)seq.size();
  if (sets) memcpy(sets, seq.data(), seq.size() * sizeof(xsg::ByteSet));
  return XSG_OK;
}

extern "C" int xsg_regex_info(const void* expr, size_t n, uint32_t flags, uint32_t* positions, uint32_t* alternatives,
                              uint32_t* ascii_only, uint32_t* sets) {
  xsg::ClassExpr ex;
  xsg::RegexDfa dfa;
  bool fixed = false;
  XSG_TRY(compile_for_query(expr, n, flags, &ex, &fixed, &dfa));
  if (!fixed) {
    if (positions) *positions = 0;
    if (alternatives) *alternatives = 0;
    if (ascii_only) *ascii_only = dfa.ascii_only ? 1u : 0u;
    return XSG_OK;
  }
  if (positions) *positions = ex.npos;
  if (alternatives) *alternatives = (uint32_t)ex.alts.size();
  if (ascii_only) *ascii_only = ex.ascii_only ? 1u : 0u;
  if (sets)
    for (size_t a = 0; a < ex.alts.size(); ++a)
      memcpy(sets + a * ex.npos * 8, ex.alts[a].data(), ex.npos * sizeof(xsg::ByteSet));
  return XSG_OK;
}

// XSG_TEST_HOOKS=1 only (not part of include/xsg.h): what class_fields decides for an expression -- the fields k_scan
// picks its verification path from -- without a device: out[] = plen, nalt, koff, cls_fast, cls_inreg, cls_exact, cls_chk,
// ascii_only, has_newline, m0, m1, p0, p1 (as many as `cap` holds).  XSG_ENOTSUP for an expression that set_class_pattern
// does not hand to class_fields: the automaton route's, and a plain literal (which becomes an ordinary pattern).
extern "C" int xsg_test_class_fields(const void* expr, size_t n, uint32_t flags, uint32_t* out, size_t cap) {
  if (!test_hooks()) return fail(XSG_ENOTSUP, "xsg_test_class_fields needs XSG_TEST_HOOKS=1");
  if (!out) return fail(XSG_EINVAL, "out is null");
  XSG_TRY(check_expr(expr, n));
  xsg::ClassExpr ex;
  std::string err;
  const bool icase = (flags & XSG_FLAG_IGNORE_CASE) != 0;
  if (!xsg::compile_class_expr(static_cast<const uint8_t*>(expr), n, icase, &ex, &err))
    return fail(XSG_ENOTSUP, "not a class sequence: %s", err.c_str());
  std::vector<uint8_t> lit;
  switch (class_route(ex, xsg::union_sets(ex), &lit)) {  // as set_class_pattern routes it
    case kRouteAutomaton: return fail(XSG_ENOTSUP, "not a class sequence: line anchors");
    case kRouteLiteral: return fail(XSG_ENOTSUP, "a literal: searched as an ordinary pattern");
    case kRouteClass: break;
  }
  PatternDev P;
  std::vector<uint8_t> blob;
  class_fields(ex, icase, &P, &blob);
  const uint32_t v[] = {P.plen, P.nalt, P.koff, P.cls_fast, P.cls_inreg, P.cls_exact, P.cls_chk,
                        P.ascii_only, P.has_newline, P.m0, P.m1, P.p0, P.p1};
  for (size_t i = 0; i < cap && i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
  return XSG_OK;
}

// XSG_FLAG_INVERT and the context counts of XSG_FLAG_CONTEXT are not properties of the compiled pattern (PatternDev and the
// scan kernels never see them): the pattern is set without them, refused if it can match '\n' (the line such a match
// belongs to is not a line of the chunk), and the bits are kept on the context, where the list and count routes read them.
constexpr uint32_t kContextBits = 0xffffff00u;  // XSG_FLAG_CONTEXT(before, after): bits 8-19 and 20-31
extern "C" int xsg_set_pattern(xsg_ctx* c, const void* pattern, size_t plen, uint32_t flags) {
  if (c) c->max_count = 0;  // xsg_set_max_count belongs to the pattern that was set before it: gone, whatever this call returns
  const uint32_t list_bits = flags & (XSG_FLAG_INVERT | kContextBits);
  if (!list_bits || !c) return set_pattern_plain(c, pattern, plen, flags);
  if (flags & ~(XSG_FLAG_EXACT_TAIL | XSG_FLAG_IGNORE_CASE | XSG_FLAG_REGEX | XSG_FLAG_INVERT | kContextBits))
    return fail(XSG_EINVAL, "unknown pattern flags 0x%x", flags);
  XSG_TRY(set_pattern_plain(c, pattern, plen, flags & ~list_bits));
  if (c->pat.has_newline) {
    c->pattern.clear();  // no pattern is set: a search now says so instead of running the plain form
    if (flags & XSG_FLAG_INVERT)
      return fail(XSG_ENOTSUP, "XSG_FLAG_INVERT: an inverted search does not accept a pattern that can match '\\n'");
    return fail(XSG_ENOTSUP, "XSG_FLAG_CONTEXT: a search with context lines does not accept a pattern that can match '\\n'");
  }
  c->flags |= list_bits;
  return XSG_OK;
}

// The limit is a property of the pattern like the list bits above, and no more one of the compiled pattern than they are: it
// is kept on the context, where the limit stage of the list route and the clamp of the count routes read it.
extern "C" int xsg_set_max_count(xsg_ctx* c, uint64_t max_count) {
  if (!c) return fail(XSG_EINVAL, "ctx is null");
  if (c->pattern.empty()) return fail(XSG_ESTATE, "xsg_set_max_count: no pattern is set (the limit belongs to a pattern: set it after the pattern)");
  c->max_count = max_count;
  return XSG_OK;
}

// ---- a literal list (xsg_set.h) ---------------------------------------------------------------------------------------
static int compile_list(const void* list, size_t n, uint32_t flags, xsg::SetProgram* prog) {
  if (flags & XSG_FLAG_REGEX) return fail(XSG_EINVAL, "a literal list does not take XSG_FLAG_REGEX");
  if (flags & ~(XSG_FLAG_EXACT_TAIL | XSG_FLAG_IGNORE_CASE | XSG_FLAG_INVERT | kContextBits))
    return fail(XSG_EINVAL, "unknown pattern flags 0x%x", flags);
  if (!list || n == 0) return fail(XSG_EINVAL, "empty literal list");
  if (n > XSG_MAX_PATTERN) return fail(XSG_EINVAL, "literal list longer than %u bytes", XSG_MAX_PATTERN);
  std::string err;
  if (!xsg::compile_literal_set(static_cast<const uint8_t*>(list), n, (flags & XSG_FLAG_IGNORE_CASE) != 0, prog, &err))
    return fail(XSG_EINVAL, "literal list: %s", err.c_str());
  return XSG_OK;
}

extern "C" int xsg_literals_info(const void* list, size_t n, uint32_t flags, xsg_literal_list* info, uint8_t* filter) {
  xsg::SetProgram prog;
  XSG_TRY(compile_list(list, n, flags, &prog));
  if (info) {
    info->count = prog.count, info->min_len = prog.min_len, info->max_len = prog.max_len;
    info->gram = prog.g, info->filter_bits_set = prog.filter_bits_set;
  }
  if (filter) memcpy(filter, prog.filter.data(), XSG_LITERAL_FILTER_BYTES);
  return XSG_OK;
}

extern "C" int xsg_set_literals(xsg_ctx* c, const void* list, size_t n, uint32_t flags) {
  return xsg_set_literals_opts(c, list, n, flags, 0u);
}

// XSG_LIST_WHOLE_WORDS and XSG_LIST_ALL_OF are properties of the compiled pattern: they live in PatternDev::set_words and
// PatternDev::set_all_of, which every set call rewrites (P = PatternDev{}), and nowhere else -- nothing of them can outlive
// the pattern.  Under XSG_LIST_ALL_OF a line's literals are one 64-bit mask: a longer list is refused here.
extern "C" int xsg_set_literals_opts(xsg_ctx* c, const void* list, size_t n, uint32_t flags, uint32_t list_flags) {
  if (c) c->pattern.clear();  // a failed call leaves the context without a pattern
  if (c) c->max_count = 0;    // ... and without the limit of the pattern before it (xsg_set_max_count)
  if (list_flags & ~(XSG_LIST_WHOLE_WORDS | XSG_LIST_ALL_OF)) return fail(XSG_EINVAL, "unknown list flags 0x%x", list_flags);
  if (!c) return fail(XSG_EINVAL, "ctx is null");
  xsg::SetProgram prog;
  XSG_TRY(compile_list(list, n, flags, &prog));
  if ((list_flags & XSG_LIST_ALL_OF) && prog.count > XSG_MAX_ALL_OF_LITERALS)
    return fail(XSG_EINVAL, "XSG_LIST_ALL_OF: %u literals, at most %u are served", prog.count, XSG_MAX_ALL_OF_LITERALS);
  HIP_TRY(hipSetDevice(c->device));
  uint32_t off[4];
  const std::vector<uint8_t> blob = prog.blob(off);
  XSG_TRY(upload_pattern_blob(c, c->d_pat, blob.data(), blob.size()));
  c->pattern.assign(static_cast<const uint8_t*>(list), static_cast<const uint8_t*>(list) + n);
  c->flags = flags;  // (XSG_FLAG_INVERT and the context counts live here alone: a list cannot match '\n')
  ++c->pattern_serial;
  c->koff_cands.clear();
  c->sketch_hashes.clear();  // the sketch gate serves single literals
  c->span_hashes.clear();
  c->bordered = false;       // k_rx_heads / k_rx_chains walk the candidates as the reference does: no overlap is left
  c->overlap_words.clear();
  c->rx_pre = c->rx_fac = false;
  PatternDev& P = c->pat;
  P = PatternDev{};
  P.plen = prog.min_len;  // what the list kernels may skip behind a match start before they look for the line's end
  P.kind = kSet;
  P.d_pat = c->d_pat.as<uint8_t>();
  P.exact_tail = 1u;
  P.icase = prog.icase ? 1u : 0u;
  P.set_g = prog.g;
  P.set_words = (list_flags & XSG_LIST_WHOLE_WORDS) ? 1u : 0u;
  P.set_all_of = (list_flags & XSG_LIST_ALL_OF) ? 1u : 0u;
  P.set_ngrams = (uint32_t)prog.keys.size();
  P.set_keys = off[0], P.set_first = off[1], P.set_ent = off[2], P.set_bytes = off[3];
  c->set_count = prog.count;
  c->set_idx_off = prog.idx_offset();
  return XSG_OK;
}

static int set_pattern_plain(xsg_ctx* c, const void* pattern, size_t plen, uint32_t flags) {
  if (!c) return fail(XSG_EINVAL, "ctx is null");
  if (!pattern || plen == 0) return fail(XSG_EINVAL, "empty pattern");
  if (plen > XSG_MAX_PATTERN) return fail(XSG_EINVAL, "pattern longer than %u bytes", XSG_MAX_PATTERN);
  if (flags & ~(XSG_FLAG_EXACT_TAIL | XSG_FLAG_IGNORE_CASE | XSG_FLAG_REGEX))
    return fail(XSG_EINVAL, "unknown pattern flags 0x%x", flags);
  if (flags & XSG_FLAG_REGEX) {
    if (plen > XSG_MAX_REGEX) return fail(XSG_EINVAL, "expression longer than %u bytes", XSG_MAX_REGEX);
    return set_class_pattern(c, static_cast<const uint8_t*>(pattern), plen, flags);
  }
  HIP_TRY(hipSetDevice(c->device));
  c->pattern.assign(static_cast<const uint8_t*>(pattern), static_cast<const uint8_t*>(pattern) + plen);
  if (flags & XSG_FLAG_IGNORE_CASE)  // simd::toLower on the pattern (string_utils.cpp:11-33)
    for (uint8_t& b : c->pattern)
      if (b >= 'A' && b <= 'Z') b = (uint8_t)(b + 32);
  const uint8_t* p = c->pattern.data();
  c->flags = flags;
  ++c->pattern_serial;
  // border <=> the pattern can overlap itself (KMP failure function of the last position > 0)
  std::vector<uint32_t> pi(plen, 0);
  for (size_t i = 1, k = 0; i < plen; ++i) {
    while (k > 0 && p[i] != p[k]) k = pi[k - 1];
    if (p[i] == p[k]) ++k;
    pi[i] = (uint32_t)k;
  }
  c->bordered = pi[plen - 1] > 0;
  c->overlap_words.clear();
  for (uint32_t b = pi[plen - 1]; b > 0; b = pi[b - 1]) {
    std::vector<uint8_t> w(p, p + (plen - b));
    w.insert(w.end(), p, p + plen);
    if (c->overlap_words.size() == 3 || w.size() > XSG_MAX_PATTERN) {  // `aaaa`: such a needle overlaps itself wherever it is dense
      c->overlap_words.clear();
      break;
    }
    c->overlap_words.push_back(std::move(w));
  }

  // padded device copy (the long-pattern verify and the tail walk read it)
  // (at least a KiB: the long-pattern kernel stages min(plen, 1 KiB) into LDS, the tail kernels read a few bytes past short patterns)
  const size_t pat_bytes = std::max<size_t>(plen, 1024) + 16;
  std::vector<uint8_t> padded(pat_bytes, 0);
  memcpy(padded.data(), p, plen);
  XSG_TRY(upload_pattern_blob(c, c->d_pat, padded.data(), padded.size()));

  PatternDev& P = c->pat;
  P = PatternDev{};
  P.plen = (uint32_t)plen;
  window_fields(p, plen, pick_filter_window(p, plen), &P);  // koff 0 unless plen > 8
  c->koff_cands = window_candidates(p, plen);
  c->sketch_hashes.clear();  // the gate of the plain count pass: case-sensitive literals of 4 bytes and more
  if (plen >= 4 && !(flags & XSG_FLAG_IGNORE_CASE))
    for (size_t k = 0; k + 4 <= plen; ++k) c->sketch_hashes.push_back((uint16_t)sketch_hash(sketch_gram(p + k)));
  c->span_hashes.clear();  // ... and the same grams' bits in a span's locator (k_scan_fin)
  for (size_t k = 0; k < c->sketch_hashes.size(); ++k) c->span_hashes.push_back((uint16_t)span_hash(sketch_gram(p + k)));
  c->rx_pre = false;
  c->rx_fac = false;
  P.kind = plen < 4 ? kMask1 : plen == 4 ? kOne : plen < 8 ? kMask2 : plen == 8 ? kTwo : kLong;
  P.d_pat = c->d_pat.as<uint8_t>();
  P.exact_tail = (flags & XSG_FLAG_EXACT_TAIL) ? 1u : 0u;
  P.has_newline = memchr(p, '\n', plen) != nullptr;
  P.nl_first = p[0] == '\n' ? 1u : 0u;
  P.icase = (flags & XSG_FLAG_IGNORE_CASE) ? 1u : 0u;
  return XSG_OK;
}
