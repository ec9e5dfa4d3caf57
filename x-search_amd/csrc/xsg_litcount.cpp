// xsg_litcount.cpp -- the C ABI of include/xsg.h: xsg_literal_counter_*, the host-memory seam of xsg_count_literals.  A
// reader loop hands in chunk after chunk of a file; the counter stages each through one of two pinned slots, runs the pass
// of xsg_count_literals over it on the slot's stream and keeps the running sums on the device.  The copy of chunk i + 1
// overlaps the pass over chunk i.  (Its own file: xsg_hostsearch.cpp links against tests/cpp/device_double.cpp alone and
// must not reference a chunk-level entry point that double does not have.)  Beside it xsg_literal_finder_*, the same seam
// of xsg_find_literals: one chunk per call, its occurrences handed back in malloc'ed arrays.  Both stage through xsg_stage.h.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

#include "xsg_host.h"
#include "xsg_stage.h"

using namespace xsg;

namespace {
struct LitSlot {
  xsg_shard* shard = nullptr;
  hipStream_t stream = nullptr;
  StagedChunk buf;
};
}  // namespace

struct xsg_literal_counter {
  xsg_ctx* ctx = nullptr;
  LitSlot slot[2];
  DevBuf d_sums;   // one word per literal, added to by every pass
  PinBuf h_sums;
  uint64_t bytes = 0;
  int next = 0;
  ~xsg_literal_counter() {
    if (ctx) (void)hipSetDevice(ctx->device);
    for (LitSlot& s : slot) {
      if (s.stream) (void)hipStreamSynchronize(s.stream);
      if (s.shard) xsg_shard_destroy(s.shard);
      if (s.stream) (void)hipStreamDestroy(s.stream);
      s.buf.release();  // (here, ahead of the context: a member's own destructor runs after this body)
    }
    d_sums.release();
    h_sums.release();
    if (ctx) xsg_ctx_destroy(ctx);
  }
};

extern "C" int xsg_literal_counter_create(int device, const void* list, size_t n, uint32_t flags, xsg_literal_counter** out) {
  return xsg_literal_counter_create_opts(device, list, n, flags, 0u, out);
}

extern "C" int xsg_literal_counter_create_opts(int device, const void* list, size_t n, uint32_t flags, uint32_t list_flags,
                                               xsg_literal_counter** out) {
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  if (list_flags & ~XSG_LIST_WHOLE_WORDS) return fail(XSG_EINVAL, "unknown list flags 0x%x", list_flags);
  if (flags & XSG_FLAG_INVERT) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  XSG_TRY(xsg_literals_info(list, n, flags, nullptr, nullptr));  // a bad list fails before a device is touched
  std::unique_ptr<xsg_literal_counter> lc(new (std::nothrow) xsg_literal_counter());
  if (!lc) return fail(XSG_ENOMEM, "host allocation failed");
  XSG_TRY(xsg_ctx_create(device, &lc->ctx));
  XSG_TRY(xsg_set_literals_opts(lc->ctx, list, n, flags, list_flags));
  HIP_TRY(hipSetDevice(lc->ctx->device));
  for (LitSlot& s : lc->slot) {
    HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    XSG_TRY(xsg_shard_create(lc->ctx, nullptr, 0, nullptr, 0, &s.shard));
  }
  const size_t bytes = 8 * (size_t)lc->ctx->set_count;
  XSG_TRY(lc->d_sums.ensure(bytes));
  XSG_TRY(lc->h_sums.ensure(bytes));
  HIP_TRY(hipMemsetAsync(lc->d_sums.p, 0, bytes, lc->ctx->stream));
  HIP_TRY(hipStreamSynchronize(lc->ctx->stream));  // the slots' streams add to these words
  *out = lc.release();
  return XSG_OK;
}

extern "C" int xsg_literal_counter_add(xsg_literal_counter* lc, const void* data, uint64_t len) {
  if (!lc || (!data && len)) return fail(XSG_EINVAL, "null argument");
  if (len == 0) return XSG_OK;
  if (len >= (1ull << 40)) return fail(XSG_EINVAL, "chunk too large");
  xsg_ctx* c = lc->ctx;
  HIP_TRY(hipSetDevice(c->device));
  LitSlot& s = lc->slot[lc->next];
  lc->next ^= 1;
  HIP_TRY(hipStreamSynchronize(s.stream));  // the slot's last pass has read its buffer and its chunk table
  XSG_TRY(stage(s.buf, c->device, s.stream, s.shard, data, len, 0));  // (the table goes up on the context's stream, behind an event)
  XSG_TRY(enqueue_count_literals(s.shard, s.stream, lc->d_sums.as<uint64_t>(), false));
  lc->bytes += len;
  return XSG_OK;
}

extern "C" int xsg_literal_counter_get(xsg_literal_counter* lc, uint64_t* counts, uint64_t cap_literals, uint64_t* bytes) {
  if (!lc || !counts) return fail(XSG_EINVAL, "null argument");
  xsg_ctx* c = lc->ctx;
  if (cap_literals < c->set_count)
    return fail(XSG_EINVAL, "room for %llu literals, the list holds %u", (unsigned long long)cap_literals, c->set_count);
  HIP_TRY(hipSetDevice(c->device));
  for (LitSlot& s : lc->slot) HIP_TRY(hipStreamSynchronize(s.stream));
  const size_t n = 8 * (size_t)c->set_count;
  HIP_TRY(hipMemcpyAsync(lc->h_sums.p, lc->d_sums.p, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(counts, lc->h_sums.p, n);
  if (bytes) *bytes = lc->bytes;
  return XSG_OK;
}

extern "C" void xsg_literal_counter_destroy(xsg_literal_counter* lc) { delete lc; }

// ---- xsg_literal_finder_*: the host-memory seam of xsg_find_literals --------------------------------------------------------------
// One chunk per call, synchronous: the chunk goes up through a pinned block, is bound as the shard's only chunk with
// global_offset = base, and the kept result of xsg_find_literals comes back in malloc'ed arrays.
struct xsg_literal_finder {
  xsg_ctx* ctx = nullptr;
  xsg_shard* shard = nullptr;
  StagedChunk buf;
  ~xsg_literal_finder() {
    if (ctx) (void)hipSetDevice(ctx->device);
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (shard) xsg_shard_destroy(shard);
    buf.release();  // (behind the shard, ahead of the context)
    if (ctx) xsg_ctx_destroy(ctx);
  }
};

extern "C" int xsg_literal_finder_create_opts(int device, const void* list, size_t n, uint32_t flags, uint32_t list_flags,
                                              xsg_literal_finder** out) {
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  if (list_flags & ~XSG_LIST_WHOLE_WORDS) return fail(XSG_EINVAL, "unknown list flags 0x%x", list_flags);
  if (flags & XSG_FLAG_INVERT) return fail(XSG_ENOTSUP, "%s", kInvertMatchMsg);
  XSG_TRY(xsg_literals_info(list, n, flags, nullptr, nullptr));  // a bad list fails before a device is touched
  std::unique_ptr<xsg_literal_finder> lf(new (std::nothrow) xsg_literal_finder());
  if (!lf) return fail(XSG_ENOMEM, "host allocation failed");
  XSG_TRY(xsg_ctx_create(device, &lf->ctx));
  XSG_TRY(xsg_set_literals_opts(lf->ctx, list, n, flags, list_flags));
  XSG_TRY(xsg_shard_create(lf->ctx, nullptr, 0, nullptr, 0, &lf->shard));
  *out = lf.release();
  return XSG_OK;
}

extern "C" int xsg_literal_finder_find(xsg_literal_finder* lf, const void* data, uint64_t len, uint64_t base, uint64_t** pos,
                                       uint32_t** lit, uint64_t* n) {
  if (!lf || !pos || !lit || !n || (!data && len)) return fail(XSG_EINVAL, "null argument");
  *pos = nullptr;
  *lit = nullptr;
  *n = 0;
  if (len >= (1ull << 40)) return fail(XSG_EINVAL, "chunk too large");
  xsg_ctx* c = lf->ctx;
  HIP_TRY(hipSetDevice(c->device));
  uint64_t total = 0;
  if (len) {
    XSG_TRY(stage(lf->buf, c->device, c->stream, lf->shard, data, len, base));
    XSG_TRY(xsg_find_literals(lf->shard, &total));  // (waits on the context's stream, behind the copy)
  }
  uint64_t* p = static_cast<uint64_t*>(malloc(8 * std::max<uint64_t>(total, 1)));
  uint32_t* l = static_cast<uint32_t*>(malloc(4 * std::max<uint64_t>(total, 1)));
  if (!p || !l) {
    free(p);
    free(l);
    return fail(XSG_ENOMEM, "host allocation failed");
  }
  if (total) {
    uint64_t chunk_ptr[2];
    const int r = xsg_result_literal_hits(lf->shard, chunk_ptr, 2, p, l, total);
    if (r != XSG_OK) {
      free(p);
      free(l);
      return r;
    }
  }
  *pos = p;
  *lit = l;
  *n = total;
  return XSG_OK;
}

extern "C" void xsg_literal_finder_destroy(xsg_literal_finder* lf) { delete lf; }
