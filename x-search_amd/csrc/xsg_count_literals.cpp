// xsg_count_literals.cpp -- the C ABI of include/xsg.h, part 4b: one count per literal of a list (xsg_count_literals,
// xsg_count_literals_async).  One launch of k_set_count_literals (xsg_set_kernels.hip) behind a memset of the result:
// no candidate list, no size fetched from the device, none of the list route's scratch read or written.
#include <cstdlib>
#include <cstring>

#include "xsg_host.h"

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
  // the two design choices of DESIGN.md 3.5e as measured there -- keys in LDS, candidates compacted -- and their A/B
  // switches in the same build (XSG_LITCOUNT_KEYS=0: keys in global memory; XSG_LITCOUNT_COMPACT=0: verify in-lane)
  const char* k = XSG_TOGGLE("XSG_LITCOUNT_KEYS");
  l.keys_lds = !(k && *k == '0');
  const char* q = XSG_TOGGLE("XSG_LITCOUNT_COMPACT");
  l.compact = !(q && *q == '0');
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
