// xsg_job.cpp -- the host pipeline behind xs::extern_search (include/xsg.h: xsg_job_*): ONE file searched as the chunks of
// its plan (xsg_meta.cpp).  Reader threads fill pinned buffers, device workers copy and scan them, an ordered store
// publishes the chunks' results, with the context of XSG_FLAG_CONTEXT stitched across their seams.  C++ on the host (the
// reference's pipeline is C++: include/xsearch/Searcher.h, tasks/readers.h, ResultTypes.h); the scan itself always runs on
// the GPU through the shard API of xsg_count.cpp / xsg_list.cpp -- there is no CPU search path in here.  Last the sum over
// the jobs of several devices (xsg_jobs_reduce_total): it reads a job's device, so it stays beside the struct.
#include <ctype.h>
#include <pthread.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

#include "xsg_context.h"
#include "xsg_fileio.h"
#include "xsg_meta.h"
#include "xsg_pipeline.h"
#include "xsg_stage.h"

using namespace xsg;
using Clock = std::chrono::steady_clock;

static double seconds_since(Clock::time_point t0) {
  return std::chrono::duration<double>(Clock::now() - t0).count();
}

// what one chunk adds to the job's result
struct Partial {
  uint64_t count = 0;     // count tags
  uint64_t newlines = 0;  // line indices without metafile bases
  bool indices_local = false;
  std::vector<uint64_t> u64;
  std::vector<std::string> lines;
  // XSG_FLAG_CONTEXT on a line-list tag: what the chunk's edges cut off, and the lines a neighbouring chunk may still
  // want, in the job's result form (xsg_context.h)
  bool context = false;
  xsg_context_edge edge{};
  std::vector<xsg_context::Extra<uint64_t>> head_u64, tail_u64;
  std::vector<xsg_context::Extra<std::string>> head_lines, tail_lines;
};

static std::atomic<uint64_t> g_job_serial{0};

struct xsg_job {
  const uint64_t serial = ++g_job_serial;
  xsg_job_opts opts{};
  std::vector<uint8_t> pattern;
  uint32_t list_flags = 0;  // xsg_job_start_list
  // xsg_job_start_max_count: the job reports the first max_count entries of the searched range (0: all of them).  The ordered
  // publisher keeps what is left of that budget (guarded by mu); when it is spent the job stops reading and finishes.
  uint64_t max_count = 0, budget = 0;
  bool budget_spent = false;
  // ... and the readers open no chunk further than bufs_max ahead of the publisher (next_piece): what a limited job reads
  // beyond the chunk that spends the budget is bounded by the buffers in circulation, however the workers interleave
  std::atomic<uint64_t> published_chunks{0};
  int fd = -1;
  int32_t compression = XSG_COMPRESSION_NONE;
  std::vector<xsg_file_chunk> plan;
  uint64_t max_orig = 0, max_actual = 0;

  // Two stages.  num_max_readers reader threads (Searcher.h:39,106 num_concurrent_reads)
  // pread -- and decompress -- chunks into pinned buffers; num_threads device workers take
  // the filled buffers, hipMemcpyAsync them on their own stream and run the scan.  The
  // pinned buffers circulate: free -> (reader) -> ready -> (worker) -> free.
  std::vector<std::thread> threads;
  std::atomic<bool> stop{false};
  std::atomic<int> active{0};   // device workers still running
  int readers_running = 0;      // guarded by q_mu
  std::mutex q_mu;
  std::condition_variable q_cv_free, q_cv_ready;
  std::vector<struct HostBuf*> all_bufs, free_bufs;
  std::deque<struct HostBuf*> ready_bufs;
  // Reading is decoupled from the chunk plan: the readers fill ONE chunk at a time together, piece by piece (a plain
  // file's chunk of 16 MiB is read as pieces of 4 MiB by whichever readers are free), so that a file of six chunks keeps
  // eight readers busy and its first chunk is on its way to the device after a quarter of a chunk's read time.  A
  // compressed chunk is one piece (its decoder needs all of it).  All guarded by q_mu.
  uint64_t next_chunk = 0;            // next chunk of the plan to open
  struct HostBuf* open_buf = nullptr; // the chunk being filled
  uint64_t open_next_piece = 0, open_npieces = 0;
  uint64_t piece_bytes = 4u << 20;
  int bufs_max = 0, bufs_created = 0; // the pinned ring grows on demand (readers allocate their buffers in parallel)

  // ordered result store
  std::mutex mu;
  std::condition_variable cv;
  std::map<uint64_t, Partial> pending;
  uint64_t next_publish = 0;
  std::vector<uint64_t> values;   // count tags: running totals; u64 tags: elements
  std::deque<std::string> lines;  // XSG_LINES, XSG_MATCHES
  uint64_t total = 0;             // count so far / elements so far
  uint64_t nl_running = 0;        // '\n' in all published chunks
  // XSG_FLAG_CONTEXT: the seams between the published chunks (xsg_context.h); spent after a refusal
  xsg_context::Stitcher<uint64_t> stitch_u64;
  xsg_context::Stitcher<std::string> stitch_lines;
  bool seam_refused = false;
  bool finished = false;
  int error = XSG_OK;
  std::string errmsg;

  Clock::time_point t_start;
  xsg_job_stats stats{};
  bool joined = false;
};

static void job_fail(xsg_job* j, int code) {
  std::lock_guard<std::mutex> g(j->mu);
  if (j->error == XSG_OK) {
    j->error = code;
    j->errmsg = last_error_message();
  }
  j->stop.store(true);
  { std::lock_guard<std::mutex> lk(j->q_mu); }  // a waiter is either before its predicate check or already blocked
  j->q_cv_free.notify_all();
  j->q_cv_ready.notify_all();
}

// A chunk's result under XSG_FLAG_CONTEXT joins the job's through the seam stitcher: the lines its neighbour's edge left
// open come first.  The one-neighbour rule (xsg_context.h) refuses, never approximates.
template <typename T, typename Out>
static int publish_context(xsg_job* j, xsg_context::Stitcher<T>& st, uint64_t index, const xsg_context_edge& edge, std::vector<T>&& own,
                           std::vector<xsg_context::Extra<T>>&& head, std::vector<xsg_context::Extra<T>>&& tail, Out* out) {
  if (j->seam_refused) return XSG_OK;  // (the job has failed already)
  xsg_context::Part<T> part;
  part.edge = edge;
  part.own = std::move(own);
  part.head = std::move(head);
  part.tail = std::move(tail);
  const xsg_context::SeamVerdict v = st.add(std::move(part), index == 0, index + 1 == j->plan.size(), out);
  if (v == xsg_context::kSeamOk) return XSG_OK;
  j->seam_refused = true;
  const bool before = v == xsg_context::kSeamBeforeTooFar;
  return fail(XSG_ENOTSUP,
              "XSG_FLAG_CONTEXT: the lines %s a match in chunk %llu reach across the whole of chunk %llu; context crosses one "
              "seam between chunks at most: search with a larger chunk_bytes (now %llu)",
              before ? "before" : "after", (unsigned long long)(before ? index : index - 1),
              (unsigned long long)(before ? index - 1 : index), (unsigned long long)j->opts.chunk_bytes);
}

// xsg_job_start_max_count: the chunk's part of the remaining budget -- its first entries, or its count clamped.  The
// publisher is ordered, so this is the cut of the file's result at its first max_count entries.
static void spend_budget(xsg_job* j, Partial& q) {
  const uint32_t mode = j->opts.mode;
  if (count_mode(mode)) {
    q.count = std::min(q.count, j->budget);
    j->budget -= q.count;
  } else if (string_mode(mode)) {
    if (q.lines.size() > j->budget) q.lines.resize((size_t)j->budget);
    j->budget -= q.lines.size();
  } else {
    if (q.u64.size() > j->budget) q.u64.resize((size_t)j->budget);
    j->budget -= q.u64.size();
  }
  j->budget_spent = j->budget == 0;
}

static int publish(xsg_job* j, uint64_t index, Partial&& p) {
  std::lock_guard<std::mutex> g(j->mu);
  if (j->budget_spent) return XSG_OK;  // (a chunk behind the one that spent the budget: not reported)
  j->pending.emplace(index, std::move(p));
  const uint32_t mode = j->opts.mode;
  int rc = XSG_OK;
  for (auto it = j->pending.find(j->next_publish); it != j->pending.end() && !j->budget_spent; it = j->pending.find(j->next_publish)) {
    Partial& q = it->second;
    if (j->max_count) spend_budget(j, q);
    if (q.context) {
      int r = XSG_OK;
      if (string_mode(mode)) {
        r = publish_context(j, j->stitch_lines, it->first, q.edge, std::move(q.lines), std::move(q.head_lines), std::move(q.tail_lines), &j->lines);
        j->total = j->lines.size();
      } else {
        if (q.indices_local) {
          for (uint64_t& v : q.u64) v += j->nl_running;
          for (auto& e : q.head_u64) e.value += j->nl_running;
          for (auto& e : q.tail_u64) e.value += j->nl_running;
        }
        r = publish_context(j, j->stitch_u64, it->first, q.edge, std::move(q.u64), std::move(q.head_u64), std::move(q.tail_u64), &j->values);
        j->total = j->values.size();
      }
      if (rc == XSG_OK) rc = r;
    } else if (count_mode(mode)) {
      j->total += q.count;
      j->values.push_back(j->total);
    } else if (string_mode(mode)) {
      for (std::string& s : q.lines) j->lines.push_back(std::move(s));
      j->total = j->lines.size();
    } else {
      if (q.indices_local)
        for (uint64_t& v : q.u64) v += j->nl_running;
      j->values.insert(j->values.end(), q.u64.begin(), q.u64.end());
      j->total = j->values.size();
    }
    j->nl_running += q.newlines;
    j->pending.erase(it);
    ++j->next_publish;
  }
  if (j->max_count) {
    j->published_chunks.store(j->next_publish);
    if (j->budget_spent) {  // enough: nothing behind this chunk is reported, so nothing more is read or searched
      j->pending.clear();
      j->stop.store(true);
    }
    { std::lock_guard<std::mutex> lk(j->q_mu); }  // a waiter is either before its predicate check or already blocked
    j->q_cv_free.notify_all();  // (readers held back by the publisher's position, next_piece)
    if (j->budget_spent) j->q_cv_ready.notify_all();
  }
  j->cv.notify_all();
  return rc;
}

// A pinned host buffer travelling between the two stages.
struct HostBuf {
  void* pinned = nullptr;
  uint64_t cap = 0;
  std::vector<uint8_t> staging;  // compressed bytes before decode
  uint64_t index = 0;            // chunk it currently holds
  std::atomic<uint64_t> pieces_left{0};  // pieces of that chunk still being read
  ~HostBuf() {
    if (pinned) (void)hipHostFree(pinned);
  }
};

// Device side of a worker: two lanes of ctx (= stream) + shard scratch + device buffer.  Every tag alternates
// between them so that the copy of chunk i+1 is already in the queue (and moving) while chunk i is scanned and
// its result waited for: count tags enqueue copy + scan and collect the counters one chunk later; list tags enqueue
// the copy and run their search (which ends in a stream sync of ITS lane) one chunk later.
struct Lane {
  xsg_ctx* ctx = nullptr;
  xsg_shard* shard = nullptr;
  void* dev = nullptr;
  uint64_t cap = 0;
  uint64_t job_serial = 0;  // the job this lane carries the pattern of (lane_prepare)
};
struct Slot {
  Lane lane[2];
  int device = 0;
  ~Slot() {
    for (Lane& l : lane) {
      if (l.shard) xsg_shard_destroy(l.shard);
      if (l.dev) (void)hipFree(l.dev);
      if (l.ctx) xsg_ctx_destroy(l.ctx);
    }
  }
};

// Slots and pinned buffers are kept in per-process pools between jobs: creating them
// costs ~10 ms of hipHostMalloc / hipMalloc / stream setup, which dominated searches of
// small files.  The pools are never torn down (a static destructor would race the HIP
// runtime's own exit).
static std::mutex g_pool_mu;
static std::vector<Slot*>& slot_pool() {
  static std::vector<Slot*>* pool = new std::vector<Slot*>();
  return *pool;
}
static std::vector<HostBuf*>& buf_pool() {
  static std::vector<HostBuf*>* pool = new std::vector<HostBuf*>();
  return *pool;
}
constexpr size_t kMaxIdleSlots = 64, kMaxIdleBufs = 128;

static Slot* slot_take(int device) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  std::vector<Slot*>& pool = slot_pool();
  for (size_t i = 0; i < pool.size(); ++i) {
    if (pool[i]->device == device) {
      Slot* s = pool[i];
      pool.erase(pool.begin() + (ptrdiff_t)i);
      return s;
    }
  }
  return nullptr;
}

static void slot_give_back(Slot* s) {
  {
    std::lock_guard<std::mutex> g(g_pool_mu);
    if (slot_pool().size() < kMaxIdleSlots) {
      slot_pool().push_back(s);
      return;
    }
  }
  delete s;
}

// One lane of a slot, ready for this job: its context and shard (created on first use), the job's pattern, a device
// buffer that holds the job's largest chunk.  `serial` = the job the lane was last prepared for.
static int lane_prepare(xsg_job* j, Slot& s, int k) {
  Lane& l = s.lane[k];
  if (l.job_serial == j->serial) return XSG_OK;
  HIP_TRY(hipSetDevice(j->opts.device));
  const uint64_t need = staged_bytes(j->max_orig);
  if (!l.ctx) {
    XSG_TRY(xsg_ctx_create(j->opts.device, &l.ctx));
    XSG_TRY(xsg_shard_create(l.ctx, nullptr, 0, nullptr, 0, &l.shard));
    XSG_TRACE("slot: lane %d ctx + shard created", k);
  }
  XSG_TRY(set_job_pattern(l.ctx, j->pattern, j->opts.pattern_flags, j->opts.pattern_is_list != 0, j->list_flags));
  // a chunk alone never contributes more than the job's limit: a dense needle then moves that many rows per chunk, not all
  // (without the device side of the limit the publisher's cut alone is still the result)
  if (j->max_count && xsg_set_max_count) XSG_TRY(xsg_set_max_count(l.ctx, j->max_count));
  if (need > l.cap) {
    if (l.dev) (void)hipFree(l.dev);
    l.dev = nullptr;
    l.cap = 0;
    HIP_TRY(hipMalloc(&l.dev, need));
    l.cap = need;
    XSG_TRACE("slot: lane %d device buffer %llu bytes", k, (unsigned long long)need);
  }
  l.job_serial = j->serial;
  return XSG_OK;
}

// A worker's slot: taken from the pool or new; lane 0 is made ready here, lane 1 when a second chunk arrives while the
// first is in flight (a stream costs 10-20 ms to create in a fresh process, a device buffer up to 5: a file of one
// chunk never pays for the second lane).
static int slot_prepare(xsg_job* j, Slot** out) {
  Slot* s = slot_take(j->opts.device);
  std::unique_ptr<Slot> own(s ? s : new (std::nothrow) Slot());
  if (!own) return fail(XSG_ENOMEM, "host allocation failed");
  own->device = j->opts.device;
  XSG_TRY(lane_prepare(j, *own, 0));
  *out = own.release();
  return XSG_OK;
}

static int buf_prepare(xsg_job* j, HostBuf** out) {
  HostBuf* b = nullptr;
  {
    std::lock_guard<std::mutex> g(g_pool_mu);
    if (!buf_pool().empty()) {
      b = buf_pool().back();
      buf_pool().pop_back();
    }
  }
  std::unique_ptr<HostBuf> own(b ? b : new (std::nothrow) HostBuf());
  if (!own) return fail(XSG_ENOMEM, "host allocation failed");
  const uint64_t need = staged_bytes(j->max_orig);
  if (need > own->cap) {
    if (own->pinned) (void)hipHostFree(own->pinned);
    own->pinned = nullptr;
    own->cap = 0;
    HIP_TRY(hipSetDevice(j->opts.device));
    HIP_TRY(hipHostMalloc(&own->pinned, need, hipHostMallocDefault));
    own->cap = need;
    XSG_TRACE("pinned buffer %llu bytes", (unsigned long long)need);
  }
  if (j->compression != XSG_COMPRESSION_NONE && own->staging.size() < j->max_actual) {
    try {
      own->staging.resize(j->max_actual);  // <= the data file's size (validated)
    } catch (const std::bad_alloc&) {
      return fail(XSG_ENOMEM, "cannot allocate %llu bytes of staging for compressed chunks", (unsigned long long)j->max_actual);
    }
  }
  *out = own.release();
  return XSG_OK;
}

static void bufs_release(xsg_job* j) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  for (HostBuf* b : j->all_bufs) {
    if (buf_pool().size() < kMaxIdleBufs)
      buf_pool().push_back(b);
    else
      delete b;
  }
  j->all_bufs.clear();
}

// ---- NUMA: the feeder threads of a device run on the CPUs next to it -------------------------------
// one reader/feeder group per GPU with NUMA-local pinned buffers.  The pinned buffers already are
// (hipHostMalloc places them on the node nearest the current device unless hipHostMallocNumaUser is given); the
// threads that fill and drain them are bound here to that node's CPUs, read from the PCI device's
// local_cpulist, intersected with what the process may use.  XSG_NUMA=0 switches the binding off.
static bool parse_cpulist(const char* text, cpu_set_t* out) {
  CPU_ZERO(out);
  const char* p = text;
  bool any = false;
  while (*p) {
    char* end = nullptr;
    const long a = strtol(p, &end, 10);
    if (end == p) break;
    long b = a;
    p = end;
    if (*p == '-') {
      b = strtol(p + 1, &end, 10);
      if (end == p + 1) break;
      p = end;
    }
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (c >= 0) CPU_SET((int)c, out), any = true;
    if (*p == ',') ++p;
    else break;
  }
  return any;
}

static int device_pci_file(int device, const char* leaf, char* buf, size_t cap) {
  char bdf[64] = "";
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) return -1;
  for (char* q = bdf; *q; ++q) *q = (char)tolower((unsigned char)*q);
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/%s", bdf, leaf);
  FILE* f = fopen(path, "r");
  if (!f) return -1;
  const size_t n = fread(buf, 1, cap - 1, f);
  fclose(f);
  buf[n] = 0;
  while (n && (buf[strlen(buf) - 1] == '\n' || buf[strlen(buf) - 1] == ' ')) buf[strlen(buf) - 1] = 0;
  return 0;
}

// CPUs local to the device that this process may run on; false = no usable information (or XSG_NUMA=0)
static bool device_cpuset(int device, cpu_set_t* out) {
  static const char* const env = getenv("XSG_NUMA");
  if (env && *env == '0') return false;
  char text[1024];
  if (device_pci_file(device, "local_cpulist", text, sizeof text) != 0) return false;
  cpu_set_t local, mine;
  if (!parse_cpulist(text, &local)) return false;
  if (sched_getaffinity(0, sizeof mine, &mine) != 0) return false;
  CPU_AND(out, &local, &mine);
  return CPU_COUNT(out) > 0 && CPU_COUNT(out) < CPU_COUNT(&mine);  // nothing to do when it is the whole set anyway
}

static void bind_thread_to_device(int device) {
  cpu_set_t set;
  if (device_cpuset(device, &set)) (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
}

extern "C" int xsg_device_numa(int device, int* node, char* cpulist, size_t cap) {
  int n = 0;
  XSG_TRY(xsg_device_count(&n));
  if (device < 0 || device >= n) return fail(XSG_ENODEV, "device %d out of range", device);
  char text[1024] = "";
  if (node) {
    *node = -1;
    if (device_pci_file(device, "numa_node", text, sizeof text) == 0) *node = atoi(text);
  }
  if (cpulist && cap) {
    cpulist[0] = 0;
    if (device_pci_file(device, "local_cpulist", text, sizeof text) == 0) snprintf(cpulist, cap, "%s", text);
  }
  return XSG_OK;
}

static uint64_t env_u64(const char* name, uint64_t dflt) {
  const char* v = getenv(name);
  return v && *v ? strtoull(v, nullptr, 0) : dflt;
}
// reader threads the pipeline runs whatever the caller asked for (see job_start_impl)
static int auto_readers() {
  static const int n = [] {
    const uint64_t e = env_u64("XSG_MIN_READERS", 0);
    if (e) return (int)std::min<uint64_t>(e, 64);
    return std::min(8, std::max(2, cpu_budget() / 2));
  }();
  return n;
}

// ---- stage 1: read (+ decompress) into a pinned buffer ------------------------
static uint64_t pieces_of(const xsg_job* j, const xsg_file_chunk& fc) {
  if (j->compression != XSG_COMPRESSION_NONE) return 1;  // a decoder needs the whole chunk
  return std::max<uint64_t>(1, fc.actual_size / j->piece_bytes);  // the last piece takes the remainder
}

// A reader's next piece of work: (buffer, piece) of the chunk that is open, opening the next chunk of the plan -- in a
// free buffer of the ring, or in one this reader allocates (the ring grows on demand, up to bufs_max: a fresh process
// pays 3-5 ms per 16 MiB of hipHostMalloc, and several readers pay it side by side while the first chunk is already
// being read).  false: nothing left to read, or the job stopped.
static bool next_piece(xsg_job* j, HostBuf** buf, uint64_t* piece) {
  std::unique_lock<std::mutex> lk(j->q_mu);
  HostBuf* mine = nullptr;  // a buffer this reader holds but has not placed yet
  for (;;) {
    if (j->stop.load()) break;
    if (j->open_buf && j->open_next_piece < j->open_npieces) {
      *buf = j->open_buf;
      *piece = j->open_next_piece++;
      if (mine) {
        j->free_bufs.push_back(mine);
        j->q_cv_free.notify_one();
      }
      return true;
    }
    if (j->next_chunk >= j->plan.size()) break;
    if (j->max_count && j->next_chunk >= j->published_chunks.load() + (uint64_t)j->bufs_max) {
      j->q_cv_free.wait(lk);  // a limited job reads no further ahead of its publisher than its ring is long
      continue;
    }
    if (!mine && !j->free_bufs.empty()) {
      mine = j->free_bufs.back();
      j->free_bufs.pop_back();
    }
    if (!mine && j->bufs_created < j->bufs_max) {
      ++j->bufs_created;
      lk.unlock();
      HostBuf* b = nullptr;
      const int r = buf_prepare(j, &b);
      lk.lock();
      if (r != XSG_OK) {
        lk.unlock();
        job_fail(j, r);
        return false;
      }
      j->all_bufs.push_back(b);
      mine = b;
      continue;  // the state may have moved while the lock was released
    }
    if (!mine) {
      j->q_cv_free.wait(lk);
      continue;
    }
    j->open_buf = mine;
    mine = nullptr;
    j->open_buf->index = j->next_chunk++;
    j->open_npieces = pieces_of(j, j->plan[j->open_buf->index]);
    j->open_buf->pieces_left.store(j->open_npieces);
    j->open_next_piece = 0;
    j->q_cv_free.notify_all();  // readers waiting for a buffer: there are pieces to take now
  }
  if (mine) j->free_bufs.push_back(mine);
  return false;
}

static void reader_loop(xsg_job* j, double& t_read, double& t_dec, uint64_t& rbytes) {
  HostBuf* b = nullptr;
  uint64_t piece = 0;
  while (next_piece(j, &b, &piece)) {
    const xsg_file_chunk& fc = j->plan[b->index];
    const uint64_t np = pieces_of(j, fc);
    const uint64_t lo = piece * j->piece_bytes;
    const uint64_t n = piece + 1 == np ? fc.actual_size - lo : j->piece_bytes;
    auto t0 = Clock::now();
    int r = XSG_OK;
    // the plan was validated at start; the buffers were sized from it -- checked again where the bytes land
    if (fc.original_size > b->cap || (j->compression != XSG_COMPRESSION_NONE && fc.actual_size > b->staging.size()) ||
        (j->compression == XSG_COMPRESSION_NONE && fc.actual_size > b->cap))
      r = fail(XSG_EIO, "chunk %llu does not fit its buffers", (unsigned long long)b->index);
    if (r == XSG_OK && n) {
      uint8_t* dst = j->compression == XSG_COMPRESSION_NONE ? static_cast<uint8_t*>(b->pinned) : b->staging.data();
      r = pread_full(j->fd, dst + lo, n, fc.actual_offset + lo);
    }
    t_read += seconds_since(t0);
    if (r == XSG_OK && j->compression != XSG_COMPRESSION_NONE && fc.original_size) {
      t0 = Clock::now();
      r = decompress_chunk(j->compression, b->staging.data(), fc.actual_size, static_cast<uint8_t*>(b->pinned),
                           fc.original_size);
      t_dec += seconds_since(t0);
    }
    if (r != XSG_OK) {
      job_fail(j, r);  // (the buffer stays with the job: other readers may still be writing their pieces of it)
      break;
    }
    rbytes += n;
    if (b->pieces_left.fetch_sub(1) == 1) {  // the chunk is complete
      {
        std::lock_guard<std::mutex> lk(j->q_mu);
        j->ready_bufs.push_back(b);
      }
      j->q_cv_ready.notify_one();
    }
  }
}

// nothing may leave a thread body (or the extern "C" boundary) as an exception: it fails the job
template <typename F>
static void thread_body(xsg_job* j, const char* who, F&& f) {
  try {
    f();
  } catch (const std::bad_alloc&) {
    (void)fail(XSG_ENOMEM, "host allocation failed in a %s", who);
    job_fail(j, XSG_ENOMEM);
  } catch (const std::exception& e) {
    (void)fail(XSG_EIO, "%s: %s", who, e.what());
    job_fail(j, XSG_EIO);
  }
}

static void reader_main(xsg_job* j) {
  double t_read = 0, t_dec = 0;
  uint64_t rbytes = 0;
  bind_thread_to_device(j->opts.device);
  thread_body(j, "reader", [&] { reader_loop(j, t_read, t_dec, rbytes); });
  {
    std::lock_guard<std::mutex> lk(j->q_mu);
    --j->readers_running;
  }
  j->q_cv_ready.notify_all();  // the last reader leaving lets idle workers finish
  std::lock_guard<std::mutex> g(j->mu);
  j->stats.bytes_read += rbytes;
  j->stats.seconds_read += t_read;
  j->stats.seconds_decompress += t_dec;
}

// ---- stage 2: H2D on the worker's stream, scan, publish -------------------------
static int bind_chunk(xsg_job* j, Lane& l, const HostBuf& hb) {
  const xsg_file_chunk& fc = j->plan[hb.index];
  if (fc.original_size > hb.cap || fc.original_size > l.cap) return fail(XSG_EINVAL, "chunk larger than its buffers");
  if (fc.original_size)
    HIP_TRY(hipMemcpyAsync(l.dev, hb.pinned, fc.original_size, hipMemcpyHostToDevice, l.ctx->stream));
  xsg_chunk ch{};
  ch.offset = 0;
  ch.length = fc.original_size;
  ch.global_offset = fc.original_offset;
  ch.line_base = fc.first_line;  // from the metafile, or AUTO (then local indices + running base at publish)
  return xsg_shard_rebind(l.shard, l.dev, l.cap, &ch, 1);
}

// XSG_FLAG_CONTEXT: the chunk's edge from the device, and from its text in the pinned buffer the lines a neighbouring
// chunk may still want -- its first `after` lines ahead of its first reported line, its last `before` lines behind its
// last one -- in the job's result form (xsg_context.h)
static int context_extras(xsg_job* j, Lane& l, const HostBuf& hb, Partial& p) {
  const xsg_file_chunk& fc = j->plan[hb.index];
  const uint32_t mode = j->opts.mode;
  if (!xsg_result_context_edges) return fail(XSG_ENOTSUP, "XSG_FLAG_CONTEXT: this build holds no device side for context lines");
  XSG_TRY(xsg_result_context_edges(l.shard, &p.edge, 1));
  p.context = true;
  const uint8_t* d = static_cast<const uint8_t*>(hb.pinned);
  const uint64_t len = fc.original_size;
  const uint64_t after = XSG_CONTEXT_AFTER(j->opts.pattern_flags), before = XSG_CONTEXT_BEFORE(j->opts.pattern_flags);
  const std::vector<xsg_context::Line> head = xsg_context::first_lines(d, len, std::min(after, xsg_context::lines_ahead(p.edge)));
  const std::vector<xsg_context::Line> tail = xsg_context::last_lines(d, len, p.edge.lines, std::min(before, xsg_context::lines_behind(p.edge)));
  const uint64_t index_base = fc.first_line == XSG_LINE_BASE_AUTO ? 0 : fc.first_line;  // (AUTO: the running base joins at publish)
  for (int side = 0; side < 2; ++side) {
    for (const xsg_context::Line& ln : side ? tail : head) {
      if (mode == XSG_LINES)
        (side ? p.tail_lines : p.head_lines).push_back({ln.index, std::string(reinterpret_cast<const char*>(d) + ln.start, ln.end - ln.start), ln.terminated});
      else
        (side ? p.tail_u64 : p.head_u64).push_back({ln.index, mode == XSG_LINE_INDICES ? index_base + ln.index : fc.original_offset + ln.start, true});
    }
  }
  return XSG_OK;
}

// list tags, second half: the search on the lane whose copy was queued one chunk earlier, then publish
static int list_collect(xsg_job* j, Lane& l, const HostBuf& hb) {
  const xsg_file_chunk& fc = j->plan[hb.index];
  const uint32_t mode = j->opts.mode;
  Partial p;
  if (string_mode(mode)) {
    uint64_t n = 0, nl = 0, nb = 0;
    const uint64_t* lens = nullptr;
    const char* bytes = nullptr;
    XSG_TRY(xsg_search(l.shard, mode, &n));
    XSG_TRY(xsg_result_lines_view(l.shard, &lens, &bytes, nullptr, &nl, &nb));  // the shard's pinned buffers: one copy, into the strings
    p.lines.reserve(nl);
    uint64_t at = 0;
    for (uint64_t i = 0; i < nl; ++i) {
      p.lines.emplace_back(bytes + at, lens[i]);
      at += lens[i];
    }
  } else {
    // the result is read where the search left it: the shard's pinned buffer (stored there by the kernels on the
    // one-sync route, one pinned D2H copy otherwise) -- no second trip through the device queue per chunk
    uint64_t n = 0;
    const uint64_t* view = nullptr;
    XSG_TRY(xsg_search(l.shard, mode, &n));
    XSG_TRY(xsg_result_u64_view(l.shard, &view, &n));
    p.u64.assign(view, view + n);
    if (mode == XSG_LINE_INDICES && fc.first_line == XSG_LINE_BASE_AUTO) {
      p.indices_local = true;
      XSG_TRY(xsg_result_newlines(l.shard, &p.newlines));
    }
  }
  if (context_flags(j->opts.pattern_flags) && context_mode(mode)) XSG_TRY(context_extras(j, l, hb, p));
  // the search synchronised the lane's stream: its pinned buffer is free again
  return publish(j, hb.index, std::move(p));
}

// count tags, first half: copy + scan of the chunk go into lane k's queue; nothing is waited for
static int count_enqueue(xsg_job* j, Slot& s, int k, const HostBuf& hb) {
  XSG_TRY(bind_chunk(j, s.lane[k], hb));
  return xsg_count_begin(s.lane[k].shard, j->opts.mode);
}
// second half: wait for lane k, publish
static int count_collect(xsg_job* j, Slot& s, int k, uint64_t index) {
  uint64_t ctr[XSG_NUM_COUNTERS];
  XSG_TRY(xsg_count_end(s.lane[k].shard, ctr));
  Partial p;
  p.count = ctr[j->opts.mode == XSG_COUNT_MATCHES ? XSG_CTR_MATCHES : XSG_CTR_LINES];
  return publish(j, index, std::move(p));
}

static void give_back(xsg_job* j, HostBuf* b) {
  {
    std::lock_guard<std::mutex> lk(j->q_mu);
    j->free_bufs.push_back(b);
  }
  j->q_cv_free.notify_one();
}

static void worker_body(xsg_job* j, double& t_dev, uint64_t& bytes, uint64_t& chunks) {
  Slot* sp = nullptr;
  int r = slot_prepare(j, &sp);
  if (r != XSG_OK) {
    job_fail(j, r);
    return;
  }
  const bool counting = count_mode(j->opts.mode);
  HostBuf* inflight = nullptr;  // the chunk whose copy (count tags: and pass) is in lane (k ^ 1)'s queue
  int k = 0;
  // The second lane costs a fresh process 10-20 ms (a stream, a device buffer: profiles/r04_cli_start.txt) and buys
  // the ~50 us a chunk that one lane loses between two chunks: made when the job is long enough to pay that back --
  // or used when the slot already has it (a pooled slot of an earlier, larger job).
  const uint64_t per_worker = (j->plan.size() + (uint64_t)j->opts.num_threads - 1) / (uint64_t)std::max(j->opts.num_threads, 1);
  const bool two_lanes = sp->lane[1].ctx != nullptr || per_worker >= env_u64("XSG_LANE2_MIN_CHUNKS", 32);
  for (;;) {
    HostBuf* b = nullptr;
    bool done = false;
    {
      std::unique_lock<std::mutex> lk(j->q_mu);
      // with a chunk in flight, do not sleep on the queue: collect that result first (its pinned buffer goes
      // back to the readers, who may be waiting for exactly that one)
      if (!inflight)
        j->q_cv_ready.wait(lk, [&] { return !j->ready_bufs.empty() || j->readers_running == 0 || j->stop.load(); });
      if (j->stop.load()) {
        done = true;
      } else if (!j->ready_bufs.empty()) {
        b = j->ready_bufs.front();
        j->ready_bufs.pop_front();
      } else if (!inflight) {
        done = true;  // readers are done and nothing is left
      }
    }
    if (done) break;
    const auto t0 = Clock::now();
    if (b) r = lane_prepare(j, *sp, k);
    if (b && r == XSG_OK) r = counting ? count_enqueue(j, *sp, k, *b) : bind_chunk(j, sp->lane[k], *b);
    if (inflight) {
      const int r2 = counting ? count_collect(j, *sp, k ^ 1, inflight->index) : list_collect(j, sp->lane[k ^ 1], *inflight);
      bytes += j->plan[inflight->index].original_size;
      ++chunks;
      if (r2 != XSG_OK) (void)hipDeviceSynchronize();  // the failed lane may still read the pinned buffer
      give_back(j, inflight);
      inflight = nullptr;
      if (r == XSG_OK) r = r2;
    }
    if (b) {
      if (r == XSG_OK) {
        inflight = b;
        if (two_lanes) {
          k ^= 1;
        } else {  // one lane: this chunk's result is collected before the next chunk is looked at
          const int r2 = counting ? count_collect(j, *sp, k, inflight->index) : list_collect(j, sp->lane[k], *inflight);
          bytes += j->plan[inflight->index].original_size;
          ++chunks;
          if (r2 != XSG_OK) (void)hipDeviceSynchronize();
          give_back(j, inflight);
          inflight = nullptr;
          r = r2;
        }
      } else {
        (void)hipDeviceSynchronize();  // the failed lane may still read the pinned buffer
        give_back(j, b);
      }
    }
    t_dev += seconds_since(t0);
    if (r != XSG_OK) {
      job_fail(j, r);
      break;
    }
  }
  if (inflight) {  // stopped with a chunk in flight: let its lane drain before the buffer is handed back
    (void)hipStreamSynchronize(sp->lane[k ^ 1].ctx->stream);
    give_back(j, inflight);
  }
  if (r == XSG_OK)
    slot_give_back(sp);
  else
    delete sp;  // do not recycle a slot whose last operation failed
}

static void worker_main(xsg_job* j) {
  double t_dev = 0;
  uint64_t bytes = 0, chunks = 0;
  bind_thread_to_device(j->opts.device);
  thread_body(j, "device worker", [&] { worker_body(j, t_dev, bytes, chunks); });
  if (j->stop.load()) {  // wake everybody that may still be waiting on a queue
    { std::lock_guard<std::mutex> lk(j->q_mu); }
    j->q_cv_free.notify_all();
    j->q_cv_ready.notify_all();
  }
  std::lock_guard<std::mutex> g(j->mu);
  j->stats.bytes_scanned += bytes;
  j->stats.chunks += chunks;
  j->stats.seconds_device += t_dev;
  if (--j->active == 0) {  // the last worker closes the result (Searcher.h:116-119)
    XSG_TRACE("job: last worker done (%llu chunks)", (unsigned long long)j->stats.chunks);
    j->finished = true;
    j->stats.seconds_total = seconds_since(j->t_start);
    j->cv.notify_all();
  }
}

extern "C" void xsg_job_opts_init(xsg_job_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  o->mode = XSG_COUNT_MATCHES;
  o->device = 0;
  o->num_threads = 1;
  o->num_max_readers = 1;
  o->chunk_bytes = 16u << 20;
}

// force_list: xsg_job_start_list -- the pattern is a list whatever pattern_is_list says, with `list_flags`
static int job_start_impl(const void* pattern, size_t plen, const char* file_path, const char* meta_file_path,
                          const xsg_job_opts* opts, bool force_list, uint32_t list_flags, uint64_t max_count, xsg_job** out) {
  XSG_TRACE("job: start");
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  // the structure grew by pattern_is_list behind chunk_end: the older size is still taken from a caller that stamps
  // struct_size itself (one that goes through xsg_job_opts_init gets this library's size and must be rebuilt: xsg.h)
  constexpr uint32_t kOptsSizeV1 = offsetof(xsg_job_opts, chunk_end) + sizeof(uint64_t);
  if (!opts || (opts->struct_size != sizeof(xsg_job_opts) && opts->struct_size != kOptsSizeV1))
    return fail(XSG_EINVAL, "bad xsg_job_opts (struct_size)");
  xsg_job_opts known;
  memset(&known, 0, sizeof known);
  memcpy(&known, opts, opts->struct_size);
  opts = &known;
  if (force_list) known.pattern_is_list = 1u;
  XSG_TRY(check_list_flags(list_flags));
  const bool is_list = known.pattern_is_list != 0;
  if (list_flags && !is_list) return fail(XSG_EINVAL, "list_flags without pattern_is_list");
  if (is_list) {  // refuse a bad list here, not in a worker
    if (!xsg_literals_info) return fail(XSG_ENOTSUP, "%s", kNoListMsg);
    xsg_literal_list info;
    XSG_TRY(xsg_literals_info(pattern, plen, opts->pattern_flags, &info, nullptr));
    if (list_flags & XSG_LIST_ALL_OF) {  // (xsg.h: XSG_LIST_ALL_OF -- what the set call and the searches would refuse, here)
      if (info.count > XSG_MAX_ALL_OF_LITERALS)
        return fail(XSG_EINVAL, "XSG_LIST_ALL_OF: %u literals, at most %u are served", info.count, XSG_MAX_ALL_OF_LITERALS);
      if (match_mode(opts->mode))
        return fail(XSG_ENOTSUP, "XSG_LIST_ALL_OF: a conjunction selects lines; it has no single match, and the match tags are not served for it");
    }
  }
  if (!pattern || plen == 0 || plen > XSG_MAX_PATTERN) return fail(XSG_EINVAL, "pattern must be 1..%u bytes",
                                                                  XSG_MAX_PATTERN);
  if ((opts->pattern_flags & XSG_FLAG_REGEX) && plen > XSG_MAX_REGEX) return fail(XSG_EINVAL, "expression longer than %u bytes", XSG_MAX_REGEX);
  if (opts->mode > XSG_MATCHES) return fail(XSG_EINVAL, "bad mode %u", opts->mode);
  if (opts->num_threads < 1 || opts->num_max_readers < 1) return fail(XSG_EINVAL, "num_threads/num_max_readers < 1");
  const bool line_mode = !match_mode(opts->mode);
  if (opts->pattern_flags & XSG_FLAG_INVERT) {  // (xsg.h: the line tags only, and no pattern that can match '\n')
    if (!line_mode) return fail(XSG_ENOTSUP, "XSG_FLAG_INVERT: an inverted search reports lines without a match; the match tags have no inverted form");
    if (!is_list && !(opts->pattern_flags & XSG_FLAG_REGEX) && memchr(pattern, '\n', plen))
      return fail(XSG_ENOTSUP, "XSG_FLAG_INVERT: an inverted search does not accept a pattern that can match '\\n'");
  }
  const bool context = context_flags(opts->pattern_flags);
  static const char kContextNlMsg[] = "XSG_FLAG_CONTEXT: a search with context lines does not accept a pattern that can match '\\n'";
  if (context) {  // (xsg.h: xsg_set_pattern refuses such a pattern whatever the tag; here, not in a worker)
    if (!is_list && !(opts->pattern_flags & XSG_FLAG_REGEX) && memchr(pattern, '\n', plen)) return fail(XSG_ENOTSUP, "%s", kContextNlMsg);
    if (context_mode(opts->mode) && !xsg_result_context_edges)
      return fail(XSG_ENOTSUP, "XSG_FLAG_CONTEXT: this build holds no device side for context lines");
    if (max_count)
      return fail(XSG_ENOTSUP, "a limit (max_count) with XSG_FLAG_CONTEXT is not served for a file: the budget is only known in file "
                               "order, and the seams between chunks join lists that are already widened; xsg_set_max_count on a "
                               "binding serves the combination");
  }
  if (opts->pattern_flags & XSG_FLAG_REGEX) {  // refuse an expression the kernel cannot decide here, not in a worker
    uint32_t npos = 0;
    std::vector<uint32_t> sets(32 * 8, 0);
    XSG_TRY(xsg_regex_check(pattern, plen, opts->pattern_flags & XSG_FLAG_IGNORE_CASE, &npos, sets.data()));
    for (uint32_t k = 0; (line_mode || context) && k < npos; ++k)
      if (sets[8 * k] & (1u << '\n'))
        return line_mode ? fail(XSG_ENOTSUP, "line modes do not accept a pattern that can match '\\n'") : fail(XSG_ENOTSUP, "%s", kContextNlMsg);
    if ((line_mode || context) && npos == 0) {  // the automaton route: does a set of the expression accept '\n'?
      xsg_regex_dfa info;
      XSG_TRY(xsg_regex_dfa_info(pattern, plen, opts->pattern_flags & XSG_FLAG_IGNORE_CASE, &info, nullptr, nullptr, 0));
      if (info.multiline)
        return line_mode ? fail(XSG_ENOTSUP, "line modes do not accept a pattern that can match '\\n'") : fail(XSG_ENOTSUP, "%s", kContextNlMsg);
    }
  }  // (a LITERAL that contains '\n' is served by every tag since round 4: xsg.h, xsg_set_pattern)
  std::unique_ptr<xsg_job> j(new (std::nothrow) xsg_job());
  if (!j) return fail(XSG_ENOMEM, "host allocation failed");
  j->opts = *opts;
  if (!j->opts.chunk_bytes) j->opts.chunk_bytes = 16u << 20;
  j->pattern.assign((const uint8_t*)pattern, (const uint8_t*)pattern + plen);
  j->list_flags = list_flags;
  j->max_count = j->budget = max_count;
  uint64_t fsize = 0;
  XSG_TRY(open_ro(file_path, &j->fd, &fsize));
  int r = XSG_OK;
  if (meta_file_path && *meta_file_path) {
    r = read_meta(meta_file_path, &j->compression, j->plan, nullptr);
    // A metafile is input like any other: every record is checked BEFORE a buffer is sized from it or a byte is
    // read or decoded through it (sizes < 2^40 were enforced by read_meta).
    for (size_t i = 0; r == XSG_OK && i < j->plan.size(); ++i) {
      const xsg_file_chunk& c = j->plan[i];
      if (c.actual_size > fsize || c.actual_offset > fsize - c.actual_size)
        r = fail(XSG_EIO, "metafile '%s': chunk %zu lies beyond the end of '%s'", meta_file_path, i, file_path);
      else if (j->compression == XSG_COMPRESSION_NONE && c.actual_size != c.original_size)
        r = fail(XSG_EIO, "metafile '%s': chunk %zu of an uncompressed file has actual_size != original_size",
                 meta_file_path, i);
      else if (j->compression == XSG_COMPRESSION_LZ4 && (c.original_size > INT32_MAX || c.actual_size > INT32_MAX))
        r = fail(XSG_EIO, "metafile '%s': chunk %zu is too large for an LZ4 block", meta_file_path, i);
      else if (j->compression != XSG_COMPRESSION_NONE && c.original_size && !c.actual_size)
        r = fail(XSG_EIO, "metafile '%s': chunk %zu has no compressed bytes", meta_file_path, i);
    }
    if (r == XSG_OK && j->compression == XSG_COMPRESSION_LZ4) r = need_lz4();
    if (r == XSG_OK && j->compression == XSG_COMPRESSION_ZSTD) r = need_zstd();
  } else {
    r = plan_plain(j->fd, fsize, j->opts.chunk_bytes, j->plan);
  }
  if (r != XSG_OK) {
    close(j->fd);
    return r;
  }
  // fail early and loudly without a device: there is no CPU search path (after the file checks, so that a bad
  // path or metafile is reported as such on any host)
  int ndev = 0;
  r = xsg_device_count(&ndev);
  if (r == XSG_OK && (opts->device < 0 || opts->device >= ndev)) r = fail(XSG_ENODEV, "device %d out of range", opts->device);
  if (r != XSG_OK) {
    close(j->fd);
    return r;
  }
  j->stats.plan_chunks = j->plan.size();
  XSG_TRACE("job: plan of %zu chunks, device count %d", j->plan.size(), ndev);
  if (opts->chunk_begin || opts->chunk_end) {
    if (opts->chunk_begin > opts->chunk_end || opts->chunk_end > j->plan.size()) {
      close(j->fd);
      return fail(XSG_EINVAL, "chunk range [%llu, %llu) outside the plan of %zu chunks",
                  (unsigned long long)opts->chunk_begin, (unsigned long long)opts->chunk_end, j->plan.size());
    }
    j->plan = std::vector<xsg_file_chunk>(j->plan.begin() + (ptrdiff_t)opts->chunk_begin,
                                          j->plan.begin() + (ptrdiff_t)opts->chunk_end);
  }
  for (const xsg_file_chunk& c : j->plan) {
    j->max_orig = std::max(j->max_orig, c.original_size);
    j->max_actual = std::max(j->max_actual, c.actual_size);
  }
  j->t_start = Clock::now();
  const uint64_t nch = std::max<uint64_t>(j->plan.size(), 1);
  const int nworkers = (int)std::min<uint64_t>((uint64_t)opts->num_threads, nch);
  // How many threads READ is the pipeline's business, not the caller's: num_threads = 1, num_max_readers = 1 is what the
  // reference's one-call API defaults to (README.md:37), and one thread copying page-cache bytes into pinned memory
  // moves 6-10 GiB/s where the link to the device takes 50.  The caller's number is a floor; the pipeline adds readers
  // up to half the CPUs the process may use (2..8; XSG_MIN_READERS overrides), and they share the chunks piece by piece.
  j->piece_bytes = std::max<uint64_t>(env_u64("XSG_READ_PIECE", 4u << 20), 1u << 16);
  uint64_t pieces = 0;
  for (const xsg_file_chunk& c : j->plan) pieces += pieces_of(j.get(), c);
  // (readers of a compressed file DECODE: that is what its rate is made of -- 3.5 GiB/s of text per LZ4 thread -- and the device
  // workers mostly sleep, so they get the whole CPU budget, 16 at most)
  const int want_readers = j->compression != XSG_COMPRESSION_NONE && !env_u64("XSG_MIN_READERS", 0)
                               ? (int)std::min<uint64_t>(std::max<uint64_t>(cpu_budget(), 2), 16)
                               : auto_readers();
  const int nreaders = (int)std::min<uint64_t>((uint64_t)std::max(opts->num_max_readers, want_readers), std::max<uint64_t>(pieces, 1));
  // the ring: two chunks per worker (one being scanned, one whose copy is queued behind it), the one the readers are
  // filling, and two complete ones in between -- never more buffers than chunks.  Allocated on demand by the readers.
  // A COMPRESSED chunk is one piece: every reader decodes a whole chunk into a buffer of its own, so the ring also needs one
  // buffer per reader -- with 2 * workers + 3 twelve LZ4 decoders found three to seven buffers free and ran at 25 GiB/s of
  // text where 12 x 3.5 GiB/s were there (bench.py e2e.lz4, profiles/r04_lz4_threads.txt).
  const uint64_t ring = j->compression != XSG_COMPRESSION_NONE ? (uint64_t)(2 * nworkers + nreaders + 1) : (uint64_t)(2 * nworkers + 3);
  j->bufs_max = (int)std::min<uint64_t>(ring, nch);
  j->active = nworkers;
  j->readers_running = nreaders;
  XSG_TRACE("job: starting %d readers + %d workers, ring of up to %d pinned buffers, %llu pieces", nreaders, nworkers,
            j->bufs_max, (unsigned long long)pieces);
  xsg_job* raw = j.release();
  for (int t = 0; t < nreaders; ++t) raw->threads.emplace_back(reader_main, raw);
  for (int t = 0; t < nworkers; ++t) raw->threads.emplace_back(worker_main, raw);
  *out = raw;
  return XSG_OK;
}

static int job_start_guarded(const void* pattern, size_t plen, const char* file_path, const char* meta_file_path,
                             const xsg_job_opts* opts, bool force_list, uint32_t list_flags, uint64_t max_count, xsg_job** out) {
  try {
    return job_start_impl(pattern, plen, file_path, meta_file_path, opts, force_list, list_flags, max_count, out);
  } catch (const std::bad_alloc&) {  // e.g. a plan with millions of records
    return fail(XSG_ENOMEM, "host allocation failed while setting up the job");
  } catch (const std::exception& e) {
    return fail(XSG_EIO, "xsg_job_start: %s", e.what());
  }
}

extern "C" int xsg_job_start(const void* pattern, size_t plen, const char* file_path, const char* meta_file_path,
                             const xsg_job_opts* opts, xsg_job** out) {
  return job_start_guarded(pattern, plen, file_path, meta_file_path, opts, false, 0u, 0u, out);
}

// ... with a limit: the first max_count entries of what the same job reports without one (count tags: min(total, max_count)).
// opts is read as xsg_job_start reads it, pattern_is_list included; list_flags belong to a list.
extern "C" int xsg_job_start_max_count(const void* pattern, size_t plen, uint32_t list_flags, uint64_t max_count, const char* file_path,
                                       const char* meta_file_path, const xsg_job_opts* opts, xsg_job** out) {
  return job_start_guarded(pattern, plen, file_path, meta_file_path, opts, false, list_flags, max_count, out);
}

extern "C" int xsg_job_start_list(const void* list, size_t n, uint32_t list_flags, const char* file_path,
                                  const char* meta_file_path, const xsg_job_opts* opts, xsg_job** out) {
  return job_start_guarded(list, n, file_path, meta_file_path, opts, true, list_flags, 0u, out);
}

extern "C" int xsg_job_join(xsg_job* j) {
  if (!j) return fail(XSG_EINVAL, "job is null");
  for (std::thread& t : j->threads)
    if (t.joinable()) t.join();
  j->joined = true;
  std::lock_guard<std::mutex> g(j->mu);
  if (j->error != XSG_OK) return fail(j->error, "%s", j->errmsg.c_str());
  return XSG_OK;
}

extern "C" void xsg_job_destroy(xsg_job* j) {
  if (!j) return;
  j->stop.store(true);
  { std::lock_guard<std::mutex> lk(j->q_mu); }
  j->q_cv_free.notify_all();
  j->q_cv_ready.notify_all();
  for (std::thread& t : j->threads)
    if (t.joinable()) t.join();
  bufs_release(j);
  if (j->fd >= 0) close(j->fd);
  delete j;
}

extern "C" int xsg_job_total(xsg_job* j, uint64_t* total) {
  if (!j || !total) return fail(XSG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(j->mu);
  *total = j->total;
  return XSG_OK;
}

extern "C" int xsg_job_wait(xsg_job* j, uint64_t index, uint64_t* available, int* finished) {
  if (!j) return fail(XSG_EINVAL, "job is null");
  std::unique_lock<std::mutex> lk(j->mu);
  const bool is_lines = string_mode(j->opts.mode);
  auto avail = [&] { return is_lines ? (uint64_t)j->lines.size() : (uint64_t)j->values.size(); };
  j->cv.wait(lk, [&] { return avail() > index || j->finished; });
  if (available) *available = avail();
  if (finished) *finished = j->finished ? 1 : 0;
  if (j->finished && j->error != XSG_OK && avail() <= index) return fail(j->error, "%s", j->errmsg.c_str());
  return XSG_OK;
}

extern "C" int xsg_job_poll(xsg_job* j, uint64_t* available, int* finished) {
  if (!j) return fail(XSG_EINVAL, "job is null");
  std::lock_guard<std::mutex> g(j->mu);
  if (available) *available = string_mode(j->opts.mode) ? (uint64_t)j->lines.size() : (uint64_t)j->values.size();
  if (finished) *finished = j->finished ? 1 : 0;
  return XSG_OK;
}

extern "C" int xsg_job_get_u64(xsg_job* j, uint64_t first, uint64_t n, uint64_t* out) {
  if (!j || (!out && n)) return fail(XSG_EINVAL, "null argument");
  if (string_mode(j->opts.mode)) return fail(XSG_ESTATE, "XSG_LINES / XSG_MATCHES results are strings: use xsg_job_get_line");
  std::lock_guard<std::mutex> g(j->mu);
  if (first + n > j->values.size()) return fail(XSG_EINVAL, "range beyond the available results");
  if (n) memcpy(out, j->values.data() + first, 8 * n);
  return XSG_OK;
}

extern "C" int xsg_job_get_line(xsg_job* j, uint64_t index, const char** data, uint64_t* len) {
  if (!j || !data || !len) return fail(XSG_EINVAL, "null argument");
  if (!string_mode(j->opts.mode)) return fail(XSG_ESTATE, "not an XSG_LINES or XSG_MATCHES job");
  std::lock_guard<std::mutex> g(j->mu);
  if (index >= j->lines.size()) return fail(XSG_EINVAL, "index beyond the available results");
  const std::string& s = j->lines[index];  // deque: references stay valid while the job lives
  *data = s.data();
  *len = s.size();
  return XSG_OK;
}

extern "C" int xsg_job_stats_get(xsg_job* j, xsg_job_stats* stats) {
  if (!j || !stats) return fail(XSG_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(j->mu);
  *stats = j->stats;
  stats->newlines = j->nl_running;
  if (!j->finished) stats->seconds_total = seconds_since(j->t_start);
  return XSG_OK;
}

// ---------------------------------------------------------------------------
// several jobs of one search (one per device): the count is the sum of their totals.  That sum is the search's one
// exchange step and goes over RCCL: every job's total is put into a word on its own GPU, one ncclAllReduce over a
// per-process communicator of those devices (ncclCommInitAll, kept for the life of the process: creating one costs
// far more than the 8-byte exchange), and the result is read back from the first device.  Falls back to adding on
// the host -- and says so through *via_rccl -- when there is no librccl, when a device is listed twice (RCCL
// wants one rank per GPU), or when XS_REDUCE=host.
// ---------------------------------------------------------------------------
namespace {
struct LocalClique {
  std::vector<int> devices;
  std::vector<xsg_ctx*> ctxs;
  std::vector<uint64_t*> d_word;
  xsg_comm* comm = nullptr;
};
std::mutex g_clique_mu;
std::vector<LocalClique*>& cliques() {
  static std::vector<LocalClique*>* v = new std::vector<LocalClique*>();  // never torn down (see slot_pool)
  return *v;
}

int clique_for(const std::vector<int>& devices, LocalClique** out) {
  for (LocalClique* c : cliques())
    if (c->devices == devices) {
      *out = c;
      return XSG_OK;
    }
  std::unique_ptr<LocalClique> c(new LocalClique());
  c->devices = devices;
  int r = XSG_OK;
  for (int d : devices) {
    xsg_ctx* x = nullptr;
    r = xsg_ctx_create(d, &x);
    if (r != XSG_OK) break;
    c->ctxs.push_back(x);
    void* p = nullptr;
    if (hipSetDevice(d) != hipSuccess || hipMalloc(&p, 64) != hipSuccess) {
      r = fail(XSG_ENOMEM, "hipMalloc on device %d failed", d);
      break;
    }
    c->d_word.push_back(static_cast<uint64_t*>(p));
  }
  if (r == XSG_OK) r = xsg_comm_create_local(c->ctxs.data(), (int)c->ctxs.size(), &c->comm);
  if (r != XSG_OK) {
    for (size_t i = 0; i < c->d_word.size(); ++i) {
      (void)hipSetDevice(devices[i]);
      (void)hipFree(c->d_word[i]);
    }
    for (xsg_ctx* x : c->ctxs) xsg_ctx_destroy(x);
    return r;
  }
  cliques().push_back(c.get());
  *out = c.release();
  return XSG_OK;
}
}  // namespace

extern "C" int xsg_jobs_reduce_total(xsg_job* const* jobs, int n, uint64_t* total, int* via_rccl) {
  if (!jobs || n < 1 || !total) return fail(XSG_EINVAL, "bad argument");
  return guarded("xsg_jobs_reduce_total", [&]() -> int {
    if (via_rccl) *via_rccl = 0;
    uint64_t host_sum = 0;
    std::vector<int> devices;
    std::vector<uint64_t> totals;
    bool distinct = true;
    for (int i = 0; i < n; ++i) {
      if (!jobs[i]) return fail(XSG_EINVAL, "job %d is null", i);
      uint64_t t = 0;
      XSG_TRY(xsg_job_total(jobs[i], &t));
      host_sum += t;
      totals.push_back(t);
      for (int d : devices) distinct &= d != jobs[i]->opts.device;
      devices.push_back(jobs[i]->opts.device);
    }
    *total = host_sum;
    const char* how = getenv("XS_REDUCE");
    if (n < 2 || !distinct || (how && strcmp(how, "host") == 0)) return XSG_OK;
    std::lock_guard<std::mutex> g(g_clique_mu);
    LocalClique* c = nullptr;
    if (clique_for(devices, &c) != XSG_OK) return XSG_OK;  // no librccl / init refused: the host sum stands
    for (int i = 0; i < n; ++i) {
      HIP_TRY(hipSetDevice(devices[i]));
      HIP_TRY(hipMemcpyAsync(c->d_word[i], &totals[i], 8, hipMemcpyHostToDevice, c->ctxs[i]->stream));
    }
    uint64_t sum = 0;
    XSG_TRY(xsg_reduce_counts(c->comm, c->d_word.data(), 1, &sum));
    if (sum != host_sum)
      return fail(XSG_EHIP, "RCCL sum %llu differs from the host sum %llu", (unsigned long long)sum,
                  (unsigned long long)host_sum);
    if (via_rccl) *via_rccl = 1;
    return XSG_OK;
  });
}
