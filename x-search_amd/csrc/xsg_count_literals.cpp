// xsg_count_literals.cpp -- the C ABI of include/xsg.h, part 4b: one count per literal of a list (xsg_count_literals,
// xsg_count_literals_async).  One launch of k_set_count_literals (xsg_set_kernels.hip) behind a memset of the result:
// no candidate list, no size fetched from the device, none of the list route's scratch read or written.  Behind them the
// chunks x literals matrix (xsg_count_literals_chunks, xsg_count_literals_chunks_async): the same pass with the chunk
// boundaries kept, k_set_count_literals_chunks.  Behind those the matrix in CSR form (xsg_count_literals_csr,
// xsg_result_literals_csr, xsg_count_literals_csr_async): a count pass, a prefix sum of the rows' lengths and a fill pass.
// Last the occurrences themselves (xsg_find_literals, xsg_result_literal_hits, xsg_find_literals_async): a count pass per
// 4 KiB wave span, a prefix sum over the spans and a fill pass of (position, literal) entries.
#include <cstring>

#include "xsg_host.h"
#include "xsg_litfind.h"
#include "xsg_litmatrix.h"

using namespace xsg;

// what every entry point of this file asks of the context: a pattern, a list, no XSG_FLAG_INVERT
static int count_literals_pattern(xsg_shard* s) {
  XSG_TRY(check_ready(s));
  const xsg_ctx* c = s->ctx;
  if (c->pat.kind != kSet)
    return fail(XSG_ENOTSUP, "counts per literal need a literal list as the pattern: xsg_set_literals (a single pattern: a list of one)");
  if (c->flags & XSG_FLAG_INVERT) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  if (c->max_count)  // (a clamp per literal would be a different feature: refused, never approximated)
    return fail(XSG_ENOTSUP, "xsg_set_max_count limits a chunk's entries, not a literal's: the per-literal entry points do not serve a limit");
  return XSG_OK;
}

static int count_literals_args(xsg_shard* s, const uint64_t* counts, uint64_t cap_literals) {
  XSG_TRY(count_literals_pattern(s));
  const xsg_ctx* c = s->ctx;
  if (!counts) return fail(XSG_EINVAL, "counts is null");
  if (cap_literals < c->set_count)
    return fail(XSG_EINVAL, "room for %llu literals, the list holds %u", (unsigned long long)cap_literals, c->set_count);
  return set_route_serves(s);
}

int xsg::enqueue_count_literals(xsg_shard* s, hipStream_t st, uint64_t* d_counts, bool zero) {
  xsg_ctx* c = s->ctx;
  // (a pending chunk-table upload is ordered before work on a foreign stream, as prepare_tiles does for the count passes)
  if (s->table_pending && st != c->stream) HIP_TRY(hipStreamWaitEvent(st, s->table_ev, 0));
  if (zero) HIP_TRY(hipMemsetAsync(d_counts, 0, 8 * (size_t)c->set_count, st));
  const ScanArgs a = scan_args(s);
  LitCountArgs l{};
  l.counts = reinterpret_cast<unsigned long long*>(d_counts);
  l.nlits = c->set_count;
  l.idx_off = c->set_idx_off;
  HIP_TRY(launch_set_count_literals(a, l, st));
  return XSG_OK;
}

extern "C" int xsg_count_literals(xsg_shard* s, uint64_t* counts, uint64_t cap_literals) {
  XSG_TRY(count_literals_args(s, counts, cap_literals));
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = 8 * (size_t)c->set_count;
  XSG_TRY(s->d_lit_counts.ensure(bytes));
  XSG_TRY(s->h_lit_counts.ensure(bytes));
  XSG_TRY(enqueue_count_literals(s, c->stream, s->d_lit_counts.as<uint64_t>(), true));
  HIP_TRY(hipMemcpyAsync(s->h_lit_counts.p, s->d_lit_counts.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  s->table_pending = false;
  memcpy(counts, s->h_lit_counts.p, bytes);
  return XSG_OK;
}

extern "C" int xsg_count_literals_async(xsg_shard* s, void* stream, uint64_t* d_counts, uint64_t cap_literals) {
  XSG_TRY(count_literals_args(s, d_counts, cap_literals));
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_count_literals(s, stream ? static_cast<hipStream_t>(stream) : c->stream, d_counts, true);
}

// ---- the chunks x literals matrix -------------------------------------------------------------------------------------------
// the touched list of DESIGN.md 3.5f and its A/B switch (XSG_LITMATRIX_TOUCHED=0: every flush sweeps the histogram), of the
// dense form and the CSR form alike
static bool litmatrix_touched() {
  const char* t = XSG_TOGGLE("XSG_LITMATRIX_TOUCHED");
  return !(t && *t == '0');
}

static int count_literals_chunks_args(xsg_shard* s, const uint64_t* counts, uint64_t cap_words, const uint64_t* chunks_with,
                                      uint64_t cap_literals) {
  // (count_literals_args' refusals; its room check is the matrix's own here)
  XSG_TRY(count_literals_args(s, counts, UINT64_MAX));
  const xsg_ctx* c = s->ctx;
  const uint64_t need = (uint64_t)s->chunks.size() * c->set_count;
  if (cap_words < need)
    return fail(XSG_EINVAL, "room for %llu words, %llu chunks x %u literals need %llu", (unsigned long long)cap_words,
                (unsigned long long)s->chunks.size(), c->set_count, (unsigned long long)need);
  if (chunks_with && cap_literals < c->set_count)
    return fail(XSG_EINVAL, "chunks_with has room for %llu literals, the list holds %u", (unsigned long long)cap_literals, c->set_count);
  return XSG_OK;
}

int xsg::enqueue_count_literals_chunks(xsg_shard* s, hipStream_t st, uint64_t* d_counts, uint64_t* d_chunks_with) {
  xsg_ctx* c = s->ctx;
  if (s->table_pending && st != c->stream) HIP_TRY(hipStreamWaitEvent(st, s->table_ev, 0));
  const size_t words = s->chunks.size() * (size_t)c->set_count;
  if (words) HIP_TRY(hipMemsetAsync(d_counts, 0, 8 * words, st));
  if (d_chunks_with) HIP_TRY(hipMemsetAsync(d_chunks_with, 0, 8 * (size_t)c->set_count, st));
  const ScanArgs a = scan_args(s);
  LitMatrixArgs l{};
  l.counts = reinterpret_cast<unsigned long long*>(d_counts);
  l.chunks_with = reinterpret_cast<unsigned long long*>(d_chunks_with);
  l.nlits = c->set_count;
  l.idx_off = c->set_idx_off;
  l.touched = litmatrix_touched();
  // tests: a grid of a few workgroups on a dozen tiles (never more workgroups than tiles: litmatrix_grid)
  HIP_TRY(launch_set_count_literals_chunks(a, l, XSG_TOGGLE_GRID("XSG_LITMATRIX_GRID"), st));
  return XSG_OK;
}

extern "C" int xsg_count_literals_chunks(xsg_shard* s, uint64_t* counts, uint64_t cap_words, uint64_t* chunks_with,
                                         uint64_t cap_literals) {
  XSG_TRY(count_literals_chunks_args(s, counts, cap_words, chunks_with, cap_literals));
  xsg_ctx* c = s->ctx;
  const uint64_t k = c->set_count, words = (uint64_t)s->chunks.size() * k;
  if (words > (1ull << 28))
    return fail(XSG_ENOTSUP, "a matrix of %llu words is more than the synchronous form keeps (2^28 words, 2 GiB): use "
                "xsg_count_literals_chunks_async with device memory of the caller's", (unsigned long long)words);
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = 8 * (size_t)(words + k);  // the matrix, then chunks_with
  s->h_lit_matrix.trim(bytes);  // (what a far larger earlier matrix left page-locked)
  XSG_TRY(s->d_lit_matrix.ensure(bytes));
  XSG_TRY(s->h_lit_matrix.ensure(bytes));
  uint64_t* d = s->d_lit_matrix.as<uint64_t>();
  XSG_TRY(enqueue_count_literals_chunks(s, c->stream, d, chunks_with ? d + words : nullptr));
  HIP_TRY(hipMemcpyAsync(s->h_lit_matrix.p, d, chunks_with ? bytes : 8 * (size_t)words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  s->table_pending = false;
  const uint64_t* h = s->h_lit_matrix.as<uint64_t>();
  memcpy(counts, h, 8 * (size_t)words);
  if (chunks_with) memcpy(chunks_with, h + words, 8 * (size_t)k);
  return XSG_OK;
}

extern "C" int xsg_count_literals_chunks_async(xsg_shard* s, void* stream, uint64_t* d_counts, uint64_t cap_words,
                                               uint64_t* d_chunks_with, uint64_t cap_literals) {
  XSG_TRY(count_literals_chunks_args(s, d_counts, cap_words, d_chunks_with, cap_literals));
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_count_literals_chunks(s, stream ? static_cast<hipStream_t>(stream) : c->stream, d_counts, d_chunks_with);
}

extern "C" uint32_t xsg_literals_chunks_touched_capacity(void) { return kLitTouched; }

// ---- a kept ragged result (xsg_objects.h: KeptRagged): what the synchronous CSR and occurrence forms share -----------------------
// The one size such a form fetches, ptr[n]: it sizes the two entry arrays and the mirror exactly.  `async_call`: where the refusal sends the caller.
static int kept_size(xsg_shard* s, KeptRagged& k, const uint64_t* d_ptr, uint64_t n, const char* async_call, DevBuf& d_words8, DevBuf& d_words4) {
  xsg_ctx* c = s->ctx;
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_ptr + n, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  s->table_pending = false;
  if (total > (1ull << 28))
    return fail(XSG_ENOTSUP, "a result of %llu entries is more than the synchronous form keeps (2^28 entries): use "
                "%s with device memory of the caller's", (unsigned long long)total, async_call);
  const size_t bytes = 8 * (size_t)(n + 1) + 12 * (size_t)total;
  k.h.trim(bytes);  // (what a far larger earlier result left page-locked)
  XSG_TRY(d_words8.ensure(8 * (size_t)total));
  XSG_TRY(d_words4.ensure(4 * (size_t)total));
  XSG_TRY(k.h.ensure(bytes));
  k.rows = n;
  k.total = total;
  return XSG_OK;
}
// the copies into the mirror on `st`: the pointer words (d_ptr, or null), the entries (both arrays, or null)
static int kept_mirror(const KeptRagged& k, hipStream_t st, const uint64_t* d_ptr, const void* d_words8, const void* d_words4) {
  uint8_t* const h = k.h.as<uint8_t>();
  const size_t ptr_bytes = 8 * (size_t)(k.rows + 1), bytes8 = 8 * (size_t)k.total;
  if (d_ptr) HIP_TRY(hipMemcpyAsync(h, d_ptr, ptr_bytes, hipMemcpyDeviceToHost, st));
  if (d_words8) HIP_TRY(hipMemcpyAsync(h + ptr_bytes, d_words8, bytes8, hipMemcpyDeviceToHost, st));
  if (d_words8) HIP_TRY(hipMemcpyAsync(h + ptr_bytes + bytes8, d_words4, 4 * (size_t)k.total, hipMemcpyDeviceToHost, st));
  return XSG_OK;
}

// The read-out of a kept result.  `call` produced it; `ptr_name` its pointer array, `pair_name` its two entry arrays.
static int kept_read(const KeptRagged& k, const char* call, const char* ptr_name, const char* pair_name, uint64_t* ptr, uint64_t cap_rows,
                     void* words8, void* words4, uint64_t cap_entries) {
  if (!k.valid)
    return fail(XSG_ESTATE, "no result of %s is kept: none was run on this binding, or a rebind or invalidate dropped it", call);
  if (!ptr) return fail(XSG_EINVAL, "%s is null", ptr_name);
  if (cap_rows < k.rows + 1)
    return fail(XSG_EINVAL, "room for %llu %s words, %llu chunks need %llu", (unsigned long long)cap_rows, ptr_name,
                (unsigned long long)k.rows, (unsigned long long)k.rows + 1);
  if ((words8 == nullptr) != (words4 == nullptr)) return fail(XSG_EINVAL, "%s go together: both, or neither for %s alone", pair_name, ptr_name);
  if (words8 && cap_entries < k.total)
    return fail(XSG_EINVAL, "room for %llu entries, the result holds %llu", (unsigned long long)cap_entries, (unsigned long long)k.total);
  const size_t ptr_bytes = 8 * (size_t)(k.rows + 1), bytes8 = 8 * (size_t)k.total;
  const uint8_t* const h = k.h.as<uint8_t>();
  memcpy(ptr, h, ptr_bytes);
  if (words8 && k.total) {
    memcpy(words8, h + ptr_bytes, bytes8);
    memcpy(words4, h + ptr_bytes + bytes8, 4 * (size_t)k.total);
  }
  return XSG_OK;
}

// ---- the matrix in CSR form ---------------------------------------------------------------------------------------------------
// count_literals_args' refusals (its room checks are the sparse form's own, in the callers)
static int count_literals_csr_args(xsg_shard* s) {
  XSG_TRY(count_literals_pattern(s));
  return set_route_serves(s);
}

namespace {
struct CsrCall {
  ScanArgs a;
  LitCsrArgs l;
  uint32_t grid;
};
}  // namespace

// Steps 1 to 3 of DESIGN.md 3.5g on `st`: the scratch zeroed, the count pass with its seam count, the prefix sum of the
// rows' lengths into d_row_ptr (n + 1 words).  Every size is the host's: chunks, literals, the grid.
static int csr_count_rows(xsg_shard* s, hipStream_t st, uint64_t* d_row_ptr, CsrCall* k) {
  xsg_ctx* c = s->ctx;
  if (s->table_pending && st != c->stream) HIP_TRY(hipStreamWaitEvent(st, s->table_ev, 0));
  const uint64_t n = s->chunks.size();
  k->a = scan_args(s);
  k->grid = set_litcsr_grid(k->a, c->set_count, XSG_TOGGLE_GRID("XSG_LITMATRIX_GRID"));
  const size_t seam_bytes = 8 * (size_t)k->grid * c->set_count;  // (at most 64 MiB: kLitCsrSeamWords)
  XSG_TRY(s->d_csr_row_nnz.ensure(4 * (size_t)n));
  XSG_TRY(s->d_csr_tmp.ensure(8 * (size_t)scan_tmp_elems(n)));
  XSG_TRY(s->d_csr_seam.ensure(seam_bytes));
  if (n) HIP_TRY(hipMemsetAsync(s->d_csr_row_nnz.p, 0, 4 * (size_t)n, st));
  if (seam_bytes) HIP_TRY(hipMemsetAsync(s->d_csr_seam.p, 0, seam_bytes, st));
  LitCsrArgs& l = k->l;
  l = LitCsrArgs{};
  l.row_nnz = s->d_csr_row_nnz.as<uint32_t>();
  l.seam = s->d_csr_seam.as<unsigned long long>();
  l.nchunks = n;
  l.nlits = c->set_count;
  l.idx_off = c->set_idx_off;
  l.touched = litmatrix_touched();
  HIP_TRY(launch_set_count_literals_csr(k->a, l, k->grid, false, st));
  HIP_TRY(launch_exclusive_scan_u32(l.row_nnz, d_row_ptr, n, s->d_csr_tmp.as<uint64_t>(), st));
  return XSG_OK;
}

// Steps 4 and 5: the fill pass and the seam rows into d_cols / d_vals, nothing at or behind cap_entries; *d_status
static int csr_fill_rows(hipStream_t st, CsrCall* k, const uint64_t* d_row_ptr, uint32_t* d_cols, uint64_t* d_vals,
                         uint64_t cap_entries, uint64_t* d_status) {
  LitCsrArgs& l = k->l;
  l.row_ptr = d_row_ptr;
  l.cols = d_cols;
  l.vals = reinterpret_cast<unsigned long long*>(d_vals);
  l.cap_entries = cap_entries;
  l.status = d_status;
  HIP_TRY(launch_set_count_literals_csr(k->a, l, k->grid, true, st));
  return XSG_OK;
}

int xsg::enqueue_count_literals_csr(xsg_shard* s, hipStream_t st, uint64_t* d_row_ptr, uint32_t* d_cols, uint64_t* d_vals,
                                    uint64_t cap_entries, uint64_t* d_status) {
  CsrCall k;
  XSG_TRY(csr_count_rows(s, st, d_row_ptr, &k));
  return csr_fill_rows(st, &k, d_row_ptr, d_cols, d_vals, cap_entries, d_status);
}

extern "C" int xsg_count_literals_csr(xsg_shard* s, uint64_t* nnz) {
  XSG_TRY(count_literals_csr_args(s));
  if (!nnz) return fail(XSG_EINVAL, "nnz is null");
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  KeptRagged& kept = s->kept_csr;
  kept.valid = false;
  const uint64_t n = s->chunks.size();
  XSG_TRY(s->d_csr_row_ptr.ensure(8 * (size_t)(n + 2)));  // row_ptr, then the status word
  uint64_t* const d_row_ptr = s->d_csr_row_ptr.as<uint64_t>();
  CsrCall k;
  XSG_TRY(csr_count_rows(s, c->stream, d_row_ptr, &k));
  XSG_TRY(kept_size(s, kept, d_row_ptr, n, "xsg_count_literals_csr_async", s->d_csr_vals, s->d_csr_cols));
  XSG_TRY(csr_fill_rows(c->stream, &k, d_row_ptr, s->d_csr_cols.as<uint32_t>(), s->d_csr_vals.as<uint64_t>(), kept.total, d_row_ptr + n + 1));
  XSG_TRY(kept_mirror(kept, c->stream, d_row_ptr, kept.total ? s->d_csr_vals.p : nullptr, s->d_csr_cols.p));
  HIP_TRY(hipStreamSynchronize(c->stream));
  kept.valid = true;
  *nnz = kept.total;
  return XSG_OK;
}

extern "C" int xsg_result_literals_csr(xsg_shard* s, uint64_t* row_ptr, uint64_t cap_rows, uint32_t* cols, uint64_t* vals,
                                       uint64_t cap_entries) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  return kept_read(s->kept_csr, "xsg_count_literals_csr", "row_ptr", "cols and vals", row_ptr, cap_rows, vals, cols, cap_entries);
}

extern "C" int xsg_count_literals_csr_async(xsg_shard* s, void* stream, uint64_t* d_row_ptr, uint64_t cap_rows, uint32_t* d_cols,
                                            uint64_t* d_vals, uint64_t cap_entries, uint64_t* d_status) {
  XSG_TRY(count_literals_csr_args(s));
  if (!d_row_ptr || !d_cols || !d_vals || !d_status) return fail(XSG_EINVAL, "d_row_ptr, d_cols, d_vals or d_status is null");
  if (cap_rows < (uint64_t)s->chunks.size() + 1)
    return fail(XSG_EINVAL, "room for %llu row_ptr words, %llu chunks need %llu", (unsigned long long)cap_rows,
                (unsigned long long)s->chunks.size(), (unsigned long long)s->chunks.size() + 1);
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_count_literals_csr(s, stream ? static_cast<hipStream_t>(stream) : c->stream, d_row_ptr, d_cols, d_vals, cap_entries,
                                    d_status);
}

// ---- every occurrence with its identity: xsg_find_literals -------------------------------------------------------------------------
namespace {
struct FindCall {
  ScanArgs a;
  LitFindArgs f;
  uint32_t forced;
};
}  // namespace

// Steps 1 and 2 of DESIGN.md 3.5i on `st`: the count pass into a word per wave span, their prefix sum, and d_chunk_ptr
// (n + 1 words) with *d_status (optional) gathered from it.  Every size is the host's: tiles and chunks.
static int find_count_spans(xsg_shard* s, hipStream_t st, uint64_t* d_chunk_ptr, uint64_t cap_entries, uint64_t* d_status, FindCall* k) {
  xsg_ctx* c = s->ctx;
  if (s->table_pending && st != c->stream) HIP_TRY(hipStreamWaitEvent(st, s->table_ev, 0));
  k->a = scan_args(s);
  const uint64_t words = litfind_words(k->a.ntiles);
  XSG_TRY(s->d_find_occ.ensure(4 * (size_t)words));
  XSG_TRY(s->d_find_off.ensure(8 * (size_t)(words + 1)));
  XSG_TRY(s->d_find_tmp.ensure(8 * (size_t)scan_tmp_elems(words)));
  // tests: a grid of a few workgroups on a dozen tiles (never more workgroups than tiles: set_litfind_grid)
  k->forced = XSG_TOGGLE_GRID("XSG_LITFIND_GRID");
  LitFindArgs& f = k->f;
  f = LitFindArgs{};
  f.wave_occ = s->d_find_occ.as<uint32_t>();
  f.idx_off = c->set_idx_off;
  HIP_TRY(launch_set_find_literals(k->a, f, k->forced, false, st));
  HIP_TRY(launch_exclusive_scan_u32(f.wave_occ, s->d_find_off.as<uint64_t>(), words, s->d_find_tmp.as<uint64_t>(), st));
  HIP_TRY(launch_set_find_chunk_ptr(k->a, s->d_find_off.as<uint64_t>(), d_chunk_ptr, cap_entries, d_status, st));
  return XSG_OK;
}

// Step 3: the fill pass into d_pos / d_lit, nothing at or behind cap_entries
static int find_fill_spans(xsg_shard* s, hipStream_t st, FindCall* k, uint64_t* d_pos, uint32_t* d_lit, uint64_t cap_entries) {
  LitFindArgs& f = k->f;
  f.wave_off = s->d_find_off.as<uint64_t>();
  f.pos = d_pos;
  f.lit = d_lit;
  f.cap_entries = cap_entries;
  HIP_TRY(launch_set_find_literals(k->a, f, k->forced, true, st));
  return XSG_OK;
}

int xsg::enqueue_find_literals(xsg_shard* s, hipStream_t st, uint64_t* d_chunk_ptr, uint64_t* d_pos, uint32_t* d_lit,
                               uint64_t cap_entries, uint64_t* d_status) {
  FindCall k;
  XSG_TRY(find_count_spans(s, st, d_chunk_ptr, cap_entries, d_status, &k));
  if (cap_entries == 0) return XSG_OK;  // a sizing pass: no entry has a place
  return find_fill_spans(s, st, &k, d_pos, d_lit, cap_entries);
}

extern "C" int xsg_find_literals(xsg_shard* s, uint64_t* total_out) {
  XSG_TRY(count_literals_csr_args(s));
  if (!total_out) return fail(XSG_EINVAL, "total is null");
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  KeptRagged& kept = s->kept_find;
  kept.valid = false;
  const uint64_t n = s->chunks.size();
  XSG_TRY(s->d_find_ptr.ensure(8 * (size_t)(n + 1)));
  uint64_t* const d_chunk_ptr = s->d_find_ptr.as<uint64_t>();
  FindCall k;
  XSG_TRY(find_count_spans(s, c->stream, d_chunk_ptr, 0, nullptr, &k));
  XSG_TRY(kept_size(s, kept, d_chunk_ptr, n, "xsg_find_literals_async", s->d_find_pos, s->d_find_lit));
  XSG_TRY(kept_mirror(kept, c->stream, d_chunk_ptr, nullptr, nullptr));
  if (kept.total) {
    XSG_TRY(find_fill_spans(s, c->stream, &k, s->d_find_pos.as<uint64_t>(), s->d_find_lit.as<uint32_t>(), kept.total));
    XSG_TRY(kept_mirror(kept, c->stream, nullptr, s->d_find_pos.p, s->d_find_lit.p));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  kept.valid = true;
  *total_out = kept.total;
  return XSG_OK;
}

extern "C" int xsg_result_literal_hits(xsg_shard* s, uint64_t* chunk_ptr, uint64_t cap_rows, uint64_t* pos, uint32_t* lit,
                                       uint64_t cap_entries) {
  if (!s) return fail(XSG_EINVAL, "shard is null");
  return kept_read(s->kept_find, "xsg_find_literals", "chunk_ptr", "pos and lit", chunk_ptr, cap_rows, pos, lit, cap_entries);
}

extern "C" int xsg_find_literals_async(xsg_shard* s, void* stream, uint64_t* d_chunk_ptr, uint64_t cap_rows, uint64_t* d_pos,
                                       uint32_t* d_lit, uint64_t cap_entries, uint64_t* d_status) {
  XSG_TRY(count_literals_csr_args(s));
  if (!d_chunk_ptr || !d_pos || !d_lit || !d_status) return fail(XSG_EINVAL, "d_chunk_ptr, d_pos, d_lit or d_status is null");
  if (cap_rows < (uint64_t)s->chunks.size() + 1)
    return fail(XSG_EINVAL, "room for %llu chunk_ptr words, %llu chunks need %llu", (unsigned long long)cap_rows,
                (unsigned long long)s->chunks.size(), (unsigned long long)s->chunks.size() + 1);
  xsg_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  return enqueue_find_literals(s, stream ? static_cast<hipStream_t>(stream) : c->stream, d_chunk_ptr, d_pos, d_lit, cap_entries, d_status);
}
