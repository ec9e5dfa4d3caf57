// xsg_count_literals.cpp -- the C ABI of include/xsg.h, part 4b: one count per literal of a list (xsg_count_literals,
// xsg_count_literals_async).  One launch of k_set_count_literals (xsg_set_kernels.hip) behind a memset of the result:
// no candidate list, no size fetched from the device, none of the list route's scratch read or written.  Behind them the
// chunks x literals matrix (xsg_count_literals_chunks, xsg_count_literals_chunks_async): the same pass with the chunk
// boundaries kept, k_set_count_literals_chunks.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "xsg_host.h"
#include "xsg_litmatrix.h"

using namespace xsg;

static int count_literals_args(xsg_shard* s, const uint64_t* counts, uint64_t cap_literals) {
  XSG_TRY(check_ready(s));
  const xsg_ctx* c = s->ctx;
  if (c->pat.kind != kSet)
    return fail(XSG_ENOTSUP, "counts per literal need a literal list as the pattern: xsg_set_literals (a single pattern: a list of one)");
  if (c->flags & XSG_FLAG_INVERT) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
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
  // the touched list of DESIGN.md 3.5f and its A/B switch (XSG_LITMATRIX_TOUCHED=0: every flush sweeps the histogram)
  const char* t = XSG_TOGGLE("XSG_LITMATRIX_TOUCHED");
  l.touched = !(t && *t == '0');
  // tests: a grid of a few workgroups on a dozen tiles (never more workgroups than tiles: litmatrix_grid)
  const char* g = XSG_TOGGLE("XSG_LITMATRIX_GRID");
  const uint32_t forced = g && atoll(g) > 0 ? (uint32_t)std::min<long long>(atoll(g), 1 << 30) : 0u;
  HIP_TRY(launch_set_count_literals_chunks(a, l, forced, st));
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
