// xsg_hostsearch.cpp -- the lower seam of include/xsg.h: chunks in host memory (xsg_host_searcher_*, xsg_host_count /
// offsets / lines / matches; the reference-style searcher functors of include/xsearch/tasks/gpu_searchers.h call them).  A
// searcher keeps up to max_slots slots of context + shard + staging block; a call leases one, stages its chunk (xsg_stage.h)
// and runs the search on the GPU through the shard API -- there is no CPU search path in here.
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>

#include "xsg_pipeline.h"
#include "xsg_stage.h"

using namespace xsg;

struct HostSlot {
  xsg_ctx* ctx = nullptr;
  xsg_shard* shard = nullptr;
  StagedChunk buf;
  uint64_t max_count = 0;  // the limit its context carries now (xsg_host_searcher_set_max_count)
  ~HostSlot() {
    if (shard) xsg_shard_destroy(shard);
    buf.release();  // (behind the shard, ahead of the context: a member's own destructor would run after this body)
    if (ctx) xsg_ctx_destroy(ctx);
  }
};

struct xsg_host_searcher {
  int device = 0;
  std::vector<uint8_t> pattern;
  uint32_t flags = 0;
  bool is_list = false;  // xsg_host_searcher_create_list
  uint32_t list_flags = 0;  // xsg_host_searcher_create_list_opts
  int max_slots = 1;
  uint64_t max_count = 0;  // xsg_host_searcher_set_max_count: what every call from now on searches under; guarded by mu
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::unique_ptr<HostSlot>> all;
  std::vector<HostSlot*> free_slots;
};

static int host_slot_take(xsg_host_searcher* hs, HostSlot** out) {
  std::unique_lock<std::mutex> lk(hs->mu);
  for (;;) {
    if (!hs->free_slots.empty()) {
      *out = hs->free_slots.back();
      hs->free_slots.pop_back();
      return XSG_OK;
    }
    if ((int)hs->all.size() < hs->max_slots) {
      hs->all.emplace_back(new HostSlot());
      HostSlot* s = hs->all.back().get();
      lk.unlock();
      int r = xsg_ctx_create(hs->device, &s->ctx);
      if (r == XSG_OK) r = set_job_pattern(s->ctx, hs->pattern, hs->flags, hs->is_list, hs->list_flags);
      if (r == XSG_OK) r = xsg_shard_create(s->ctx, nullptr, 0, nullptr, 0, &s->shard);
      if (r != XSG_OK) {
        // give the place back, or later callers would wait for a slot that never comes
        lk.lock();
        for (size_t i = 0; i < hs->all.size(); ++i)
          if (hs->all[i].get() == s) {
            hs->all.erase(hs->all.begin() + (ptrdiff_t)i);
            break;
          }
        lk.unlock();
        hs->cv.notify_one();
        return r;
      }
      *out = s;
      return XSG_OK;
    }
    hs->cv.wait(lk);
  }
}

static void host_slot_release(xsg_host_searcher* hs, HostSlot* s) {
  {
    std::lock_guard<std::mutex> g(hs->mu);
    hs->free_slots.push_back(s);
  }
  hs->cv.notify_one();
}

// a slot for one call, its context under the searcher's limit of this moment (a slot that last served another limit is set
// again: the limit is the context's, and the setter may be called between any two calls)
static int host_slot_acquire(xsg_host_searcher* hs, HostSlot** out) {
  HostSlot* s = nullptr;
  XSG_TRY(host_slot_take(hs, &s));
  uint64_t want = 0;
  {
    std::lock_guard<std::mutex> g(hs->mu);
    want = hs->max_count;
  }
  if (s->max_count != want) {
    const int r = xsg_set_max_count ? xsg_set_max_count(s->ctx, want) : fail(XSG_ENOTSUP, "this build holds no device side for a limit");
    if (r != XSG_OK) {
      host_slot_release(hs, s);
      return r;
    }
    s->max_count = want;
  }
  *out = s;
  return XSG_OK;
}

// stage the chunk: host -> pinned -> device, bind it as a 1-chunk shard (local offsets, line base 0)
static int host_stage(HostSlot* s, const void* data, uint64_t len) {
  return stage(s->buf, s->ctx->device, s->ctx->stream, s->shard, data, len, 0);
}

static int host_searcher_create(int device, const void* pattern, size_t plen, uint32_t flags, bool is_list, uint32_t list_flags,
                                int max_slots, xsg_host_searcher** out) {
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  XSG_TRY(check_list_flags(list_flags));
  if (!pattern || plen == 0 || plen > XSG_MAX_PATTERN) return fail(XSG_EINVAL, "pattern must be 1..%u bytes",
                                                                  XSG_MAX_PATTERN);
  if (is_list) {
    if (!xsg_literals_info) return fail(XSG_ENOTSUP, "%s", kNoListMsg);
    xsg_literal_list info;
    XSG_TRY(xsg_literals_info(pattern, plen, flags, &info, nullptr));
    if ((list_flags & XSG_LIST_ALL_OF) && info.count > XSG_MAX_ALL_OF_LITERALS)
      return fail(XSG_EINVAL, "XSG_LIST_ALL_OF: %u literals, at most %u are served", info.count, XSG_MAX_ALL_OF_LITERALS);
  } else if (flags & XSG_FLAG_REGEX) {
    XSG_TRY(xsg_regex_check(pattern, plen, flags & XSG_FLAG_IGNORE_CASE, nullptr, nullptr));
  }
  int ndev = 0;
  XSG_TRY(xsg_device_count(&ndev));
  if (device < 0 || device >= ndev) return fail(XSG_ENODEV, "device %d out of range", device);
  std::unique_ptr<xsg_host_searcher> hs(new (std::nothrow) xsg_host_searcher());
  if (!hs) return fail(XSG_ENOMEM, "host allocation failed");
  hs->device = device;
  hs->pattern.assign((const uint8_t*)pattern, (const uint8_t*)pattern + plen);
  hs->flags = flags;
  hs->is_list = is_list;
  hs->list_flags = list_flags;
  hs->max_slots = max_slots < 1 ? 1 : max_slots;
  // build the first slot now so that a bad pattern / missing GPU fails here, not in the first search
  HostSlot* s = nullptr;
  XSG_TRY(host_slot_acquire(hs.get(), &s));
  host_slot_release(hs.get(), s);
  *out = hs.release();
  return XSG_OK;
}

extern "C" int xsg_host_searcher_create(int device, const void* pattern, size_t plen, uint32_t flags, int max_slots,
                                        xsg_host_searcher** out) {
  return host_searcher_create(device, pattern, plen, flags, false, 0u, max_slots, out);
}

extern "C" int xsg_host_searcher_create_list(int device, const void* list, size_t n, uint32_t flags, int max_slots,
                                             xsg_host_searcher** out) {
  return xsg_host_searcher_create_list_opts(device, list, n, flags, 0u, max_slots, out);
}

extern "C" int xsg_host_searcher_create_list_opts(int device, const void* list, size_t n, uint32_t flags, uint32_t list_flags,
                                                  int max_slots, xsg_host_searcher** out) {
  return host_searcher_create(device, list, n, flags, true, list_flags, max_slots, out);
}

extern "C" void xsg_host_searcher_destroy(xsg_host_searcher* hs) { delete hs; }

extern "C" int xsg_host_searcher_set_max_count(xsg_host_searcher* hs, uint64_t max_count) {
  if (!hs) return fail(XSG_EINVAL, "host searcher is null");
  if (max_count && !xsg_set_max_count) return fail(XSG_ENOTSUP, "this build holds no device side for a limit");
  std::lock_guard<std::mutex> g(hs->mu);
  hs->max_count = max_count;
  return XSG_OK;
}

struct SlotLease {
  xsg_host_searcher* hs;
  HostSlot* s = nullptr;
  explicit SlotLease(xsg_host_searcher* h) : hs(h) {}
  ~SlotLease() {
    if (s) host_slot_release(hs, s);
  }
};

extern "C" int xsg_host_count(xsg_host_searcher* hs, const void* data, uint64_t len, int skip_to_nl,
                              uint64_t* count) {
  if (!hs || !count || (!data && len)) return fail(XSG_EINVAL, "null argument");
  SlotLease l(hs);
  XSG_TRY(host_slot_acquire(hs, &l.s));
  XSG_TRY(host_stage(l.s, data, len));
  uint64_t ctr[XSG_NUM_COUNTERS];
  XSG_TRY(xsg_count(l.s->shard, skip_to_nl ? XSG_COUNT_LINES : XSG_COUNT_MATCHES, ctr));
  *count = ctr[skip_to_nl ? XSG_CTR_LINES : XSG_CTR_MATCHES];
  return XSG_OK;
}

extern "C" int xsg_host_offsets(xsg_host_searcher* hs, uint32_t mode, const void* data, uint64_t len, uint64_t** out,
                                uint64_t* n) {
  if (!hs || !out || !n || (!data && len)) return fail(XSG_EINVAL, "null argument");
  if (mode != XSG_MATCH_BYTE_OFFSETS && mode != XSG_LINE_BYTE_OFFSETS && mode != XSG_LINE_INDICES)
    return fail(XSG_EINVAL, "mode %u has no uint64 list result", mode);
  SlotLease l(hs);
  XSG_TRY(host_slot_acquire(hs, &l.s));
  XSG_TRY(host_stage(l.s, data, len));
  uint64_t cnt = 0;
  XSG_TRY(xsg_search(l.s->shard, mode, &cnt));
  uint64_t* buf = static_cast<uint64_t*>(malloc(8 * std::max<uint64_t>(cnt, 1)));
  if (!buf) return fail(XSG_ENOMEM, "host allocation failed");
  const int r = xsg_result_u64(l.s->shard, buf, cnt);
  if (r != XSG_OK) {
    free(buf);
    return r;
  }
  *out = buf;
  *n = cnt;
  return XSG_OK;
}

static int host_strings(xsg_host_searcher* hs, uint32_t mode, const void* data, uint64_t len, uint64_t** lengths, char** bytes,
                        uint64_t* n, uint64_t* nbytes) {
  if (!hs || !lengths || !bytes || !n || !nbytes || (!data && len)) return fail(XSG_EINVAL, "null argument");
  SlotLease l(hs);
  XSG_TRY(host_slot_acquire(hs, &l.s));
  XSG_TRY(host_stage(l.s, data, len));
  uint64_t cnt = 0, nl = 0, nb = 0;
  const uint64_t* vlens = nullptr;
  const char* vbytes = nullptr;
  XSG_TRY(xsg_search(l.s->shard, mode, &cnt));
  // out of the shard's pinned buffers (a large result arrives there by pinned copies, not by a pageable D2H)
  XSG_TRY(xsg_result_lines_view(l.s->shard, &vlens, &vbytes, nullptr, &nl, &nb));
  uint64_t* lens = static_cast<uint64_t*>(malloc(8 * std::max<uint64_t>(nl, 1)));
  char* buf = static_cast<char*>(malloc(std::max<uint64_t>(nb, 1)));
  if (!lens || !buf) {
    free(lens);
    free(buf);
    return fail(XSG_ENOMEM, "host allocation failed");
  }
  if (nl) memcpy(lens, vlens, 8 * nl);
  if (nb) memcpy(buf, vbytes, nb);
  *lengths = lens;
  *bytes = buf;
  *n = nl;
  *nbytes = nb;
  return XSG_OK;
}

extern "C" int xsg_host_lines(xsg_host_searcher* hs, const void* data, uint64_t len, uint64_t** lengths, char** bytes,
                              uint64_t* n, uint64_t* nbytes) {
  return host_strings(hs, XSG_LINES, data, len, lengths, bytes, n, nbytes);
}

extern "C" int xsg_host_matches(xsg_host_searcher* hs, const void* data, uint64_t len, uint64_t** lengths, char** bytes,
                                uint64_t* n, uint64_t* nbytes) {
  return host_strings(hs, XSG_MATCHES, data, len, lengths, bytes, n, nbytes);
}
