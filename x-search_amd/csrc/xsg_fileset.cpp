// xsg_fileset.cpp -- a LIST of files searched as the chunks of a few bindings (include/xsg.h: xsg_fileset_*), the sibling
// of the job pipeline of xsg_job.cpp, which searches ONE file as many chunks.  Host glue only: the plan of batches is
// xsg_fileset.h's, the searches are xsg_count_chunks and xsg_search + xsg_result_chunk_ptr on one shard, and a file larger
// than chunk_bytes goes through xsg_job_start[_list] unchanged.  No CPU search path.
//
// Threads: one driver (stat, plan, device work, publication in path order) and num_readers readers that fill the batch
// buffer the driver pointed them at.  Two pinned batch buffers: the readers fill batch k + 1 while the driver uploads and
// searches batch k, and never run further ahead -- the buffer of batch k + 2 is the one batch k is uploaded from.
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "xsg_fileio.h"
#include "xsg_fileset.h"
#include "xsg_pipeline.h"

using namespace xsg;
namespace fsp = xsg_fileset_plan;

struct xsg_fileset {
  xsg_fileset_opts opts{};
  std::vector<uint8_t> pattern;
  std::vector<std::string> paths;
  uint64_t max_count = 0;  // xsg_fileset_start_max_count: per file (0: no limit)
  int nreaders = 1;

  std::thread driver;
  std::vector<std::thread> readers;
  std::atomic<bool> stop{false};

  // the plan (the driver's; the readers see it after the first start_fill)
  std::vector<uint64_t> sizes;
  std::vector<uint8_t> kinds;
  fsp::Plan plan;
  std::vector<uint8_t> item_failed;  // a reader could not read the item's file (or its size changed): an empty chunk

  // driver -> readers: the items [next_item, end_item) go into fill_buf; guarded by r_mu
  std::mutex r_mu;
  std::condition_variable r_cv_work, r_cv_done;
  uint64_t next_item = 0, end_item = 0, items_open = 0;  // items_open: handed out or waiting, not yet reported done
  uint8_t* fill_buf = nullptr;
  bool readers_exit = false;

  // results, in path order; guarded by mu
  std::mutex mu;
  std::condition_variable cv;
  std::vector<int32_t> status;
  std::vector<uint64_t> counts;    // count tags: the count; list tags: the file's rows
  std::vector<uint64_t> file_ptr;  // list tags: npaths + 1
  std::vector<uint64_t> values;    // the uint64 list tags
  std::deque<std::string> lines;   // XSG_LINES, XSG_MATCHES (references stay valid while the set lives)
  uint64_t published = 0;
  bool finished = false;
  int error = XSG_OK;
  std::string errmsg;

  // device side (the driver's)
  xsg_ctx* ctx = nullptr;
  xsg_shard* shard = nullptr;
  void* d_buf = nullptr;
  uint64_t d_cap = 0;
  uint8_t* h_buf[2] = {nullptr, nullptr};
};

// what one batch (or one file of it) reported, in the order of its items
struct BatchResult {
  std::vector<uint64_t> rows;    // items + 1 (count tags: unused)
  std::vector<uint64_t> counts;  // count tags: per item
  std::vector<uint64_t> values;
  std::vector<uint64_t> lens;    // string tags: per entry
  std::vector<uint64_t> byte_rows;
  std::string bytes;
};

// ---- readers --------------------------------------------------------------------------------------------------------------
static void read_item(xsg_fileset* fs, uint64_t i, uint8_t* buf) {
  const fsp::Item& it = fs->plan.items[i];
  uint8_t* dst = buf + it.offset;
  bool ok = true;
  if (it.length) {
    int fd = -1;
    uint64_t size = 0;
    ok = open_ro(fs->paths[it.file].c_str(), &fd, &size) == XSG_OK;
    if (ok) {
      ok = size == it.length && pread_full(fd, dst, it.length, 0) == XSG_OK;  // (a file that shrank or grew since the plan)
      close(fd);
    }
  }
  if (!ok) {
    fs->item_failed[i] = 1;
    fs->status[it.file] = XSG_EIO;  // (published by the driver, behind r_mu and mu)
  }
  const uint64_t end = ok ? it.length : 0;
  memset(dst + end, 0, fsp::round_up(it.length) - end);  // the bytes up to the next item decide nothing, and are the same every run
}

static void reader_main(xsg_fileset* fs) {
  constexpr uint64_t kGrab = 8;  // items per visit to the lock
  for (;;) {
    uint64_t lo = 0, hi = 0;
    uint8_t* buf = nullptr;
    {
      std::unique_lock<std::mutex> lk(fs->r_mu);
      fs->r_cv_work.wait(lk, [&] { return fs->next_item < fs->end_item || fs->readers_exit; });
      if (fs->readers_exit) return;
      lo = fs->next_item;
      hi = std::min(lo + kGrab, fs->end_item);
      fs->next_item = hi;
      buf = fs->fill_buf;
    }
    for (uint64_t i = lo; i < hi && !fs->stop.load(); ++i) read_item(fs, i, buf);
    {
      std::lock_guard<std::mutex> lk(fs->r_mu);
      fs->items_open -= hi - lo;
      if (fs->items_open == 0) fs->r_cv_done.notify_all();
    }
  }
}

static void start_fill(xsg_fileset* fs, const fsp::Batch& b, uint8_t* buf) {
  if (b.first_item == b.end_item) return;
  {
    std::lock_guard<std::mutex> lk(fs->r_mu);
    fs->next_item = b.first_item;
    fs->end_item = b.end_item;
    fs->items_open = b.end_item - b.first_item;
    fs->fill_buf = buf;
  }
  fs->r_cv_work.notify_all();
}

static void wait_fill(xsg_fileset* fs) {
  std::unique_lock<std::mutex> lk(fs->r_mu);
  fs->r_cv_done.wait(lk, [&] { return fs->items_open == 0; });
}

static void stop_readers(xsg_fileset* fs) {
  {
    std::lock_guard<std::mutex> lk(fs->r_mu);
    fs->readers_exit = true;
  }
  fs->r_cv_work.notify_all();
  for (std::thread& t : fs->readers)
    if (t.joinable()) t.join();
}

// ---- the device side ------------------------------------------------------------------------------------------------------
static int bind(xsg_fileset* fs, const xsg_chunk* chunks, uint64_t n) {
  if (!fs->shard) return xsg_shard_create(fs->ctx, fs->d_buf, fs->d_cap, chunks, n, &fs->shard);
  return xsg_shard_rebind(fs->shard, fs->d_buf, fs->d_cap, chunks, n);
}

// one search of what is bound (n chunks), appended to `out`: its rows continue where out's rows stand
static int search_bound(xsg_fileset* fs, uint64_t n, BatchResult& out) {
  const uint32_t mode = fs->opts.mode;
  if (count_mode(mode)) {
    const size_t at = out.counts.size();
    out.counts.resize(at + n);
    const int r = xsg_count_chunks(fs->shard, mode, out.counts.data() + at, nullptr, n, nullptr);
    if (r != XSG_OK) out.counts.resize(at);
    return r;
  }
  uint64_t total = 0;
  XSG_TRY(xsg_search(fs->shard, mode, &total));
  std::vector<uint64_t> rows(n + 1), byte_rows(string_mode(mode) ? n + 1 : 0);
  XSG_TRY(xsg_result_chunk_ptr(fs->shard, rows.data(), n + 1, byte_rows.empty() ? nullptr : byte_rows.data()));
  const uint64_t row0 = out.rows.empty() ? 0 : out.rows.back();
  if (out.rows.empty()) out.rows.push_back(0);
  for (uint64_t i = 1; i <= n; ++i) out.rows.push_back(row0 + rows[i]);
  if (!string_mode(mode)) {
    const uint64_t* v = nullptr;
    uint64_t cnt = 0;
    XSG_TRY(xsg_result_u64_view(fs->shard, &v, &cnt));
    if (cnt) out.values.insert(out.values.end(), v, v + cnt);
    return XSG_OK;
  }
  const uint64_t* lens = nullptr;
  const char* bytes = nullptr;
  uint64_t nl = 0, nb = 0;
  XSG_TRY(xsg_result_lines_view(fs->shard, &lens, &bytes, nullptr, &nl, &nb));
  const uint64_t byte0 = out.bytes.size();
  if (out.byte_rows.empty()) out.byte_rows.push_back(0);
  for (uint64_t i = 1; i <= n; ++i) out.byte_rows.push_back(byte0 + byte_rows[i]);
  if (nl) out.lens.insert(out.lens.end(), lens, lens + nl);
  if (nb) out.bytes.append(bytes, nb);
  return XSG_OK;
}

// Batch b is in `host`: upload, bind, ONE search.  A binding that holds a byte >= 0x80 under an ASCII-only expression is
// refused as a whole (XSG_ENOTSUP); the batch is then searched again one file per binding, and only the files that hold
// such a byte keep the refusal, as their status.
static int search_batch(xsg_fileset* fs, const fsp::Batch& b, const uint8_t* host, BatchResult& out) {
  const uint64_t n = b.end_item - b.first_item;
  std::vector<xsg_chunk> chunks(n);
  for (uint64_t i = 0; i < n; ++i) {
    const fsp::Item& it = fs->plan.items[b.first_item + i];
    chunks[i] = xsg_chunk{it.offset, fs->item_failed[b.first_item + i] ? 0 : it.length, 0, 0};
  }
  HIP_TRY(hipMemcpyAsync(fs->d_buf, host, b.bytes, hipMemcpyHostToDevice, fs->ctx->stream));
  XSG_TRY(bind(fs, chunks.data(), n));
  int r = search_bound(fs, n, out);
  if (r != XSG_ENOTSUP) return r;
  out = BatchResult{};
  for (uint64_t i = 0; i < n && !fs->stop.load(); ++i) {
    XSG_TRY(bind(fs, &chunks[i], 1));
    r = search_bound(fs, 1, out);
    if (r == XSG_OK) continue;
    if (r != XSG_ENOTSUP) return r;
    fs->status[fs->plan.items[b.first_item + i].file] = XSG_ENOTSUP;
    if (count_mode(fs->opts.mode)) {
      out.counts.push_back(0);
    } else {  // an empty row
      if (out.rows.empty()) out.rows.push_back(0);
      out.rows.push_back(out.rows.back());
      if (string_mode(fs->opts.mode)) {
        if (out.byte_rows.empty()) out.byte_rows.push_back(0);
        out.byte_rows.push_back(out.byte_rows.back());
      }
    }
  }
  return XSG_OK;
}

// ---- publication ----------------------------------------------------------------------------------------------------------
static void publish_empty(xsg_fileset* fs, uint64_t f) {
  std::lock_guard<std::mutex> g(fs->mu);
  fs->counts[f] = 0;
  fs->file_ptr[f + 1] = fs->file_ptr[f];
  fs->published = f + 1;
  fs->cv.notify_all();
}

// file f is item i of the batch whose result is r; `rows`: its entries, as xsg_fileset.h attributed them (list tags)
static void publish_item(xsg_fileset* fs, uint64_t f, const BatchResult& r, uint64_t i, uint64_t rows) {
  const uint32_t mode = fs->opts.mode;
  std::lock_guard<std::mutex> g(fs->mu);
  if (count_mode(mode)) {
    fs->counts[f] = r.counts[i];
    fs->file_ptr[f + 1] = fs->file_ptr[f];
  } else {
    const uint64_t lo = r.rows[i], hi = lo + rows;
    fs->counts[f] = hi - lo;
    if (string_mode(mode)) {
      uint64_t at = r.byte_rows[i];
      for (uint64_t k = lo; k < hi; ++k) {
        fs->lines.emplace_back(r.bytes.data() + at, r.lens[k]);
        at += r.lens[k];
      }
    } else {
      fs->values.insert(fs->values.end(), r.values.begin() + (ptrdiff_t)lo, r.values.begin() + (ptrdiff_t)hi);
    }
    fs->file_ptr[f + 1] = fs->file_ptr[f] + (hi - lo);
  }
  fs->published = f + 1;
  fs->cv.notify_all();
}

// A file larger than chunk_bytes: the job pipeline, as it is, on the same device with the same chunk_bytes; its result is
// the file's.  What is wrong with the file alone (unreadable, bytes the expression refuses, context across a whole chunk)
// becomes its status; anything else fails the set.
static int run_large(xsg_fileset* fs, uint64_t f) {
  const uint32_t mode = fs->opts.mode;
  xsg_job_opts o;
  xsg_job_opts_init(&o);
  o.mode = mode;
  o.pattern_flags = fs->opts.pattern_flags;
  o.device = fs->opts.device;
  o.num_threads = 1;
  o.num_max_readers = fs->nreaders;
  o.chunk_bytes = fs->opts.chunk_bytes;
  o.pattern_is_list = fs->opts.pattern_is_list;
  xsg_job* j = nullptr;
  int r;
  if (fs->max_count)  // the file's own budget: the job stops reading where it is spent
    r = xsg_job_start_max_count(fs->pattern.data(), fs->pattern.size(), fs->opts.list_flags, fs->max_count, fs->paths[f].c_str(), nullptr, &o, &j);
  else if (fs->opts.pattern_is_list)
    r = xsg_job_start_list(fs->pattern.data(), fs->pattern.size(), fs->opts.list_flags, fs->paths[f].c_str(), nullptr, &o, &j);
  else
    r = xsg_job_start(fs->pattern.data(), fs->pattern.size(), fs->paths[f].c_str(), nullptr, &o, &j);
  if (r == XSG_OK) r = xsg_job_join(j);
  if (r != XSG_OK) {
    if (j) xsg_job_destroy(j);
    if (r != XSG_EIO && r != XSG_ENOTSUP) return r;
    fs->status[f] = r;
    publish_empty(fs, f);
    return XSG_OK;
  }
  uint64_t n = 0;
  int fin = 0;
  if (count_mode(mode)) {
    r = xsg_job_total(j, &n);
  } else {
    r = xsg_job_poll(j, &n, &fin);
  }
  std::vector<uint64_t> vals;
  if (r == XSG_OK && !count_mode(mode) && !string_mode(mode)) {
    vals.resize(n);
    r = xsg_job_get_u64(j, 0, n, vals.data());
  }
  if (r == XSG_OK) {
    std::lock_guard<std::mutex> g(fs->mu);
    fs->counts[f] = n;
    fs->file_ptr[f + 1] = fs->file_ptr[f] + (count_mode(mode) ? 0 : n);
    if (string_mode(mode)) {
      for (uint64_t k = 0; k < n && r == XSG_OK; ++k) {
        const char* d = nullptr;
        uint64_t len = 0;
        r = xsg_job_get_line(j, k, &d, &len);
        if (r == XSG_OK) fs->lines.emplace_back(d, len);
      }
    } else if (!count_mode(mode)) {
      fs->values.insert(fs->values.end(), vals.begin(), vals.end());
    }
    if (r == XSG_OK) {
      fs->published = f + 1;
      fs->cv.notify_all();
    }
  }
  xsg_job_destroy(j);
  return r;
}

// ---- the driver -----------------------------------------------------------------------------------------------------------
static int driver_body(xsg_fileset* fs) {
  const uint64_t n = fs->paths.size();
  for (uint64_t f = 0; f < n; ++f) {
    struct stat st;
    if (stat(fs->paths[f].c_str(), &st) != 0 || !S_ISREG(st.st_mode)) {  // missing, unreadable, a directory
      fs->kinds[f] = fsp::kUnreadable;
      fs->status[f] = XSG_EIO;
    } else {
      fs->sizes[f] = (uint64_t)st.st_size;
      fs->kinds[f] = fs->sizes[f] > fs->opts.chunk_bytes ? fsp::kLarge : fsp::kSmall;
    }
  }
  fs->plan = fsp::make_plan(fs->sizes, fs->kinds, fs->opts.batch_bytes);
  fs->item_failed.assign(fs->plan.items.size(), 0);
  uint64_t max_bytes = 0;
  for (const fsp::Batch& b : fs->plan.batches) max_bytes = std::max(max_bytes, b.bytes);
  HIP_TRY(hipSetDevice(fs->opts.device));
  if (!fs->plan.items.empty()) {  // (a set of large files only is its jobs: no context, no buffers of its own)
    XSG_TRY(xsg_ctx_create(fs->opts.device, &fs->ctx));
    XSG_TRY(set_job_pattern(fs->ctx, fs->pattern, fs->opts.pattern_flags, fs->opts.pattern_is_list != 0, fs->opts.list_flags));
    // a small file is a chunk: the limit per chunk IS the limit per file, in the batch's one search and in the per-file
    // searches behind a refusal alike (the limit stays with the context's pattern)
    if (fs->max_count) XSG_TRY(xsg_set_max_count(fs->ctx, fs->max_count));
    // (a margin behind the last chunk: the scan reads whole 16-byte units, and an empty last file still needs an address)
    fs->d_cap = max_bytes + 256;
    if (hipMalloc(&fs->d_buf, fs->d_cap) != hipSuccess) return fail(XSG_ENOMEM, "hipMalloc(%llu) failed", (unsigned long long)fs->d_cap);
    HIP_TRY(hipMemsetAsync(fs->d_buf, 0, fs->d_cap, fs->ctx->stream));
    for (int k = 0; k < (fs->plan.batches.size() > 1 ? 2 : 1); ++k)
      if (hipHostMalloc((void**)&fs->h_buf[k], max_bytes + 256, hipHostMallocDefault) != hipSuccess)
        return fail(XSG_ENOMEM, "hipHostMalloc(%llu) failed", (unsigned long long)(max_bytes + 256));
    for (int t = 0; t < fs->nreaders; ++t) fs->readers.emplace_back(reader_main, fs);
    start_fill(fs, fs->plan.batches[0], fs->h_buf[0]);
  }
  for (size_t k = 0; k < fs->plan.batches.size() && !fs->stop.load(); ++k) {
    const fsp::Batch& b = fs->plan.batches[k];
    BatchResult res;
    if (b.end_item > b.first_item) {
      wait_fill(fs);
      // batch k + 1 goes into the buffer batch k - 1 was uploaded from: its search has returned, the copy is long done
      if (k + 1 < fs->plan.batches.size()) start_fill(fs, fs->plan.batches[k + 1], fs->h_buf[(k + 1) & 1]);
      if (fs->stop.load()) break;
      XSG_TRY(search_batch(fs, b, fs->h_buf[k & 1], res));
    }
    std::vector<uint64_t> file_rows;
    if (!res.rows.empty()) fsp::attribute_rows(fs->plan, b, res.rows.data(), file_rows);
    uint64_t i = 0;  // the batch's items, in file order
    for (uint64_t f = b.first_file; f < b.end_file && !fs->stop.load(); ++f) {
      if (fs->kinds[f] == fsp::kSmall) {
        publish_item(fs, f, res, i, file_rows.empty() ? 0 : file_rows[f - b.first_file]);
        ++i;
      } else if (fs->kinds[f] == fsp::kLarge) {
        XSG_TRY(run_large(fs, f));
      } else {
        publish_empty(fs, f);
      }
    }
  }
  return XSG_OK;
}

static void driver_main(xsg_fileset* fs) {
  int r;
  try {
    r = driver_body(fs);
  } catch (const std::bad_alloc&) {
    r = fail(XSG_ENOMEM, "host allocation failed in a file set");
  } catch (const std::exception& e) {
    r = fail(XSG_EIO, "file set: %s", e.what());
  }
  const std::string msg = r != XSG_OK ? last_error_message() : "";
  fs->stop.store(r != XSG_OK || fs->stop.load());
  stop_readers(fs);
  if (fs->ctx) (void)hipStreamSynchronize(fs->ctx->stream);  // (an upload behind a call that failed: the buffers go away below)
  if (fs->shard) xsg_shard_destroy(fs->shard);
  if (fs->ctx) xsg_ctx_destroy(fs->ctx);
  if (fs->d_buf) (void)hipFree(fs->d_buf);
  for (uint8_t* h : fs->h_buf)
    if (h) (void)hipHostFree(h);
  fs->shard = nullptr;
  fs->ctx = nullptr;
  fs->d_buf = nullptr;
  fs->h_buf[0] = fs->h_buf[1] = nullptr;
  std::lock_guard<std::mutex> g(fs->mu);
  if (r != XSG_OK && fs->error == XSG_OK) {
    fs->error = r;
    fs->errmsg = msg;
  }
  fs->finished = true;
  fs->cv.notify_all();
}

// ---- the C ABI ------------------------------------------------------------------------------------------------------------
extern "C" void xsg_fileset_opts_init(xsg_fileset_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  o->mode = XSG_COUNT_LINES;
}

static int check_pattern(const void* pattern, size_t plen, const xsg_fileset_opts& o) {
  const uint32_t flags = o.pattern_flags;
  const bool line_mode = !match_mode(o.mode);
  const bool context = context_flags(flags);
  if (o.pattern_is_list) {
    xsg_literal_list info;
    XSG_TRY(xsg_literals_info(pattern, plen, flags, &info, nullptr));
    if (o.list_flags & XSG_LIST_ALL_OF) {
      if (info.count > XSG_MAX_ALL_OF_LITERALS)
        return fail(XSG_EINVAL, "XSG_LIST_ALL_OF: %u literals, at most %u are served", info.count, XSG_MAX_ALL_OF_LITERALS);
      if (!line_mode) return fail(XSG_ENOTSUP, "XSG_LIST_ALL_OF: a conjunction selects lines; the match tags are not served for it");
    }
  }
  if ((flags & XSG_FLAG_INVERT) && !line_mode)
    return fail(XSG_ENOTSUP, "XSG_FLAG_INVERT: an inverted search reports lines without a match; the match tags have no inverted form");
  const bool nl_literal = !o.pattern_is_list && !(flags & XSG_FLAG_REGEX) && memchr(pattern, '\n', plen);
  if (nl_literal && ((flags & XSG_FLAG_INVERT) || context))
    return fail(XSG_ENOTSUP, "XSG_FLAG_INVERT / XSG_FLAG_CONTEXT: not with a pattern that can match '\\n'");
  if (flags & XSG_FLAG_REGEX) {
    if (plen > XSG_MAX_REGEX) return fail(XSG_EINVAL, "expression longer than %u bytes", XSG_MAX_REGEX);
    uint32_t npos = 0;
    std::vector<uint32_t> sets(32 * 8, 0);
    XSG_TRY(xsg_regex_check(pattern, plen, flags & XSG_FLAG_IGNORE_CASE, &npos, sets.data()));
    bool multiline = false;
    for (uint32_t k = 0; k < npos; ++k) multiline |= (sets[8 * k] & (1u << '\n')) != 0;
    if (npos == 0) {
      xsg_regex_dfa info;
      XSG_TRY(xsg_regex_dfa_info(pattern, plen, flags & XSG_FLAG_IGNORE_CASE, &info, nullptr, nullptr, 0));
      multiline = info.multiline != 0;
    }
    if (multiline && (line_mode || context)) return fail(XSG_ENOTSUP, "line modes and context do not accept a pattern that can match '\\n'");
  }
  return XSG_OK;
}

static int fileset_start(const void* pattern, size_t plen, const char* const* paths, uint64_t npaths,
                         const xsg_fileset_opts* opts, uint64_t max_count, xsg_fileset** out) {
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  if (npaths && !paths) return fail(XSG_EINVAL, "paths is null");
  for (uint64_t f = 0; f < npaths; ++f)
    if (!paths[f]) return fail(XSG_EINVAL, "path %llu is null", (unsigned long long)f);
  if (!opts || opts->struct_size != sizeof(xsg_fileset_opts)) return fail(XSG_EINVAL, "bad xsg_fileset_opts (struct_size)");
  xsg_fileset_opts o = *opts;
  if (o.mode > XSG_MATCHES) return fail(XSG_EINVAL, "bad mode %u", o.mode);
  if (!o.batch_bytes) o.batch_bytes = 256ull << 20;
  if (!o.chunk_bytes) o.chunk_bytes = 16ull << 20;
  if (o.batch_bytes < o.chunk_bytes) return fail(XSG_EINVAL, "batch_bytes %llu < chunk_bytes %llu", (unsigned long long)o.batch_bytes,
                                                 (unsigned long long)o.chunk_bytes);
  if (o.batch_bytes >= (1ull << 40)) return fail(XSG_EINVAL, "batch_bytes too large");
  if (o.num_readers < 0) return fail(XSG_EINVAL, "num_readers < 0");
  if (!pattern || plen == 0 || plen > XSG_MAX_PATTERN) return fail(XSG_EINVAL, "pattern must be 1..%u bytes", XSG_MAX_PATTERN);
  XSG_TRY(check_list_flags(o.list_flags));
  if (o.list_flags && !o.pattern_is_list) return fail(XSG_EINVAL, "list_flags without pattern_is_list");
  XSG_TRY(check_pattern(pattern, plen, o));
  if (max_count && context_flags(o.pattern_flags))
    return fail(XSG_ENOTSUP, "a limit (max_count) with XSG_FLAG_CONTEXT is not served for files: a large file's budget is only known "
                             "in file order, and the seams between its chunks join lists that are already widened; "
                             "xsg_set_max_count on a binding serves the combination");
  int ndev = 0;
  XSG_TRY(xsg_device_count(&ndev));  // fail early and loudly without a device: there is no CPU search path
  if (o.device < 0 || o.device >= ndev) return fail(XSG_ENODEV, "device %d out of range", o.device);
  try {
    xsg_fileset* fs = new xsg_fileset();
    fs->opts = o;
    fs->max_count = max_count;
    fs->pattern.assign((const uint8_t*)pattern, (const uint8_t*)pattern + plen);
    fs->paths.assign(paths, paths + npaths);
    fs->nreaders = o.num_readers ? std::min(o.num_readers, 16) : std::min(16, std::max(1, cpu_budget()));
    fs->sizes.assign(npaths, 0);
    fs->kinds.assign(npaths, fsp::kSmall);
    fs->status.assign(npaths, XSG_OK);
    fs->counts.assign(npaths, 0);
    fs->file_ptr.assign(npaths + 1, 0);
    fs->driver = std::thread(driver_main, fs);
    *out = fs;
  } catch (const std::bad_alloc&) {
    return fail(XSG_ENOMEM, "host allocation failed while setting up the file set");
  } catch (const std::exception& e) {
    return fail(XSG_EIO, "xsg_fileset_start: %s", e.what());
  }
  return XSG_OK;
}

extern "C" int xsg_fileset_start(const void* pattern, size_t plen, const char* const* paths, uint64_t npaths,
                                 const xsg_fileset_opts* opts, xsg_fileset** out) {
  return fileset_start(pattern, plen, paths, npaths, opts, 0u, out);
}

// ... with a limit per FILE: every file's result is the first max_count entries of what it is without one (count tags:
// min(count, max_count)), whatever batch_bytes, chunk_bytes and the reader count; 0 is the call above
extern "C" int xsg_fileset_start_max_count(const void* pattern, size_t plen, const char* const* paths, uint64_t npaths,
                                           const xsg_fileset_opts* opts, uint64_t max_count, xsg_fileset** out) {
  return fileset_start(pattern, plen, paths, npaths, opts, max_count, out);
}

extern "C" int xsg_fileset_wait(xsg_fileset* fs, uint64_t file_index, uint64_t* files_done, int* finished) {
  if (!fs) return fail(XSG_EINVAL, "file set is null");
  std::unique_lock<std::mutex> lk(fs->mu);
  fs->cv.wait(lk, [&] { return fs->published > file_index || fs->finished; });
  if (files_done) *files_done = fs->published;
  if (finished) *finished = fs->finished ? 1 : 0;
  if (fs->finished && fs->error != XSG_OK && fs->published <= file_index) return fail(fs->error, "%s", fs->errmsg.c_str());
  return XSG_OK;
}

extern "C" int xsg_fileset_join(xsg_fileset* fs) {
  if (!fs) return fail(XSG_EINVAL, "file set is null");
  if (fs->driver.joinable()) fs->driver.join();
  std::lock_guard<std::mutex> g(fs->mu);
  if (fs->error != XSG_OK) return fail(fs->error, "%s", fs->errmsg.c_str());
  return XSG_OK;
}

extern "C" void xsg_fileset_destroy(xsg_fileset* fs) {
  if (!fs) return;
  fs->stop.store(true);
  if (fs->driver.joinable()) fs->driver.join();
  delete fs;
}

extern "C" int xsg_fileset_status(xsg_fileset* fs, int32_t* status, uint64_t cap) {
  if (!fs) return fail(XSG_EINVAL, "file set is null");
  const uint64_t n = fs->paths.size();
  if (cap < n || (n && !status)) return fail(XSG_EINVAL, "room for %llu files, the set holds %llu", (unsigned long long)cap, (unsigned long long)n);
  std::lock_guard<std::mutex> g(fs->mu);
  for (uint64_t f = 0; f < n; ++f) status[f] = f < fs->published ? fs->status[f] : XSG_OK;
  return XSG_OK;
}

extern "C" int xsg_fileset_counts(xsg_fileset* fs, uint64_t* counts, uint64_t cap) {
  if (!fs) return fail(XSG_EINVAL, "file set is null");
  const uint64_t n = fs->paths.size();
  if (cap < n || (n && !counts)) return fail(XSG_EINVAL, "room for %llu files, the set holds %llu", (unsigned long long)cap, (unsigned long long)n);
  std::lock_guard<std::mutex> g(fs->mu);
  for (uint64_t f = 0; f < n; ++f) counts[f] = f < fs->published ? fs->counts[f] : 0;
  return XSG_OK;
}

extern "C" int xsg_fileset_file_ptr(xsg_fileset* fs, uint64_t* file_ptr, uint64_t cap_rows) {
  if (!fs) return fail(XSG_EINVAL, "file set is null");
  if (count_mode(fs->opts.mode)) return fail(XSG_ESTATE, "a count tag has no list: xsg_fileset_counts holds its results");
  const uint64_t n = fs->paths.size();
  if (cap_rows < n + 1 || !file_ptr) return fail(XSG_EINVAL, "room for %llu words, the set needs %llu", (unsigned long long)cap_rows, (unsigned long long)(n + 1));
  std::lock_guard<std::mutex> g(fs->mu);
  for (uint64_t f = 0; f <= n; ++f) file_ptr[f] = fs->file_ptr[std::min(f, fs->published)];
  return XSG_OK;
}

extern "C" int xsg_fileset_get_u64(xsg_fileset* fs, uint64_t first, uint64_t n, uint64_t* out) {
  if (!fs || (!out && n)) return fail(XSG_EINVAL, "null argument");
  if (count_mode(fs->opts.mode) || string_mode(fs->opts.mode)) return fail(XSG_ESTATE, "not a uint64 list tag");
  std::lock_guard<std::mutex> g(fs->mu);
  if (first + n > fs->values.size() || first + n < first) return fail(XSG_EINVAL, "range beyond the available results");
  if (n) memcpy(out, fs->values.data() + first, 8 * n);
  return XSG_OK;
}

extern "C" int xsg_fileset_get_line(xsg_fileset* fs, uint64_t index, const char** data, uint64_t* len) {
  if (!fs || !data || !len) return fail(XSG_EINVAL, "null argument");
  if (!string_mode(fs->opts.mode)) return fail(XSG_ESTATE, "not an XSG_LINES or XSG_MATCHES file set");
  std::lock_guard<std::mutex> g(fs->mu);
  if (index >= fs->lines.size()) return fail(XSG_EINVAL, "index beyond the available results");
  const std::string& s = fs->lines[index];
  *data = s.data();
  *len = s.size();
  return XSG_OK;
}
