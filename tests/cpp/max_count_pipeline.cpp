// max_count_pipeline.cpp -- the per-file budget of the job pipeline (x-search_amd/csrc/xsg_job.cpp: xsg_job_start_max_count)
// on a box without a GPU, plainly and under ThreadSanitizer: the device is tests/cpp/device_double.cpp, which knows nothing
// of xsg_set_max_count, so every cut seen here is the ordered publisher's alone.
//
// Cases: (1) every list tag the double serves and both count tags, 1 and 2 workers, limits that cut in the first chunk, in
// a middle one, in the last one and beyond the total: the result is the first N entries of the same job without a limit, the count sequence
// the clamped running totals up to the chunk that reached N; (2) the early stop: hits in chunk k only, N = 1, and
// xsg_job_stats.chunks <= k + 1 + (2 x workers + 3) on a file four times longer than that; (3) start calls that are
// refused; (4) join and destroy while the readers are still running, 200 times; (5) the host searcher's setter without a
// device side.
#include <xsg.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                                    \
    }                                                                              \
  } while (0)

constexpr uint64_t kChunk = 65536;

// words and newlines; `needle_from`, `needle_to`: the byte range in which "Sherlock" may appear
static std::string make_corpus(const std::string& path, size_t bytes, unsigned seed, size_t needle_from, size_t needle_to) {
  static const char* words[] = {"the", "of", "and", "Holmes", "she", "lock", "a", "to", "in", "that", "street", "She"};
  std::mt19937 rng(seed);
  std::string s;
  s.reserve(bytes + 64);
  while (s.size() < bytes) {
    const unsigned r = rng();
    s += (r % 211 == 0 && s.size() >= needle_from && s.size() + 16 < needle_to) ? "Sherlock" : words[r % 12];
    s += ((r >> 16) % 6 == 0) ? '\n' : ' ';
  }
  s.back() = 'x';  // the last line lacks its newline: XSG_LINES drops it if it is selected
  std::ofstream(path, std::ios::binary).write(s.data(), (std::streamsize)s.size());
  return s;
}

struct Run {
  int rc = XSG_OK;
  std::vector<uint64_t> values;     // uint64 tags: the elements; count tags: the running totals
  std::vector<std::string> lines;   // XSG_LINES, XSG_MATCHES
  uint64_t total = 0;
  xsg_job_stats stats{};
};

static Run run_job(const std::string& pat, const std::string& file, uint32_t mode, uint32_t flags, int threads, uint64_t max_count) {
  Run out;
  xsg_job_opts o;
  xsg_job_opts_init(&o);
  o.mode = mode;
  o.pattern_flags = flags;
  o.num_threads = threads;
  o.num_max_readers = threads;
  o.chunk_bytes = kChunk;
  xsg_job* j = nullptr;
  out.rc = xsg_job_start_max_count(pat.data(), pat.size(), 0, max_count, file.c_str(), nullptr, &o, &j);
  if (out.rc != XSG_OK) return out;
  out.rc = xsg_job_join(j);
  uint64_t n = 0;
  int fin = 0;
  CHECK(xsg_job_poll(j, &n, &fin) == XSG_OK && fin == 1);
  CHECK(xsg_job_total(j, &out.total) == XSG_OK);
  if (mode == XSG_LINES || mode == XSG_MATCHES) {
    for (uint64_t i = 0; i < n; ++i) {
      const char* d = nullptr;
      uint64_t len = 0;
      CHECK(xsg_job_get_line(j, i, &d, &len) == XSG_OK);
      out.lines.emplace_back(d, len);
    }
  } else {
    out.values.resize(n);
    CHECK(xsg_job_get_u64(j, 0, n, out.values.data()) == XSG_OK);
  }
  CHECK(xsg_job_stats_get(j, &out.stats) == XSG_OK);
  xsg_job_destroy(j);
  return out;
}

template <class T>
static std::vector<T> first_n(const std::vector<T>& v, uint64_t n) {
  return std::vector<T>(v.begin(), v.begin() + (ptrdiff_t)std::min<uint64_t>(n, v.size()));
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string file = dir + "/xsg_max_count_corpus.txt", sparse = dir + "/xsg_max_count_sparse.txt";
  const std::string pat = "Sherlock";
  const size_t bytes = 72 * kChunk;
  make_corpus(file, bytes, 4321, 0, bytes);

  // ---- (1) the publisher's cut
  // (the double serves plain literals on the four list tags of the reference and the two counts: XSG_MATCHES and
  // XSG_FLAG_INVERT are the GPU tests')
  const uint32_t list_modes[] = {XSG_MATCH_BYTE_OFFSETS, XSG_LINE_BYTE_OFFSETS, XSG_LINE_INDICES, XSG_LINES};
  {
    const uint32_t flags = 0;
    for (const uint32_t mode : list_modes) {
      const Run full = run_job(pat, file, mode, flags, 1, 0);
      CHECK(full.rc == XSG_OK && full.stats.plan_chunks >= 64 && full.stats.chunks == full.stats.plan_chunks);
      const bool strings = mode == XSG_LINES;
      const uint64_t total = strings ? full.lines.size() : full.values.size();
      CHECK(total > 200);
      // the first chunk's entries, a middle one's, the last one's, beyond the total
      for (const uint64_t n : {(uint64_t)1, (uint64_t)2, total / 2, total - 1, total, total + 5, (uint64_t)UINT64_MAX}) {
        for (int threads = 1; threads <= 2; ++threads) {
          const Run cut = run_job(pat, file, mode, flags, threads, n);
          CHECK(cut.rc == XSG_OK);
          CHECK(cut.total == std::min(n, total));
          if (strings)
            CHECK(cut.lines == first_n(full.lines, n));
          else
            CHECK(cut.values == first_n(full.values, n));
          if (n >= total) CHECK(cut.stats.chunks == cut.stats.plan_chunks);
        }
      }
    }
    for (const uint32_t mode : {(uint32_t)XSG_COUNT_MATCHES, (uint32_t)XSG_COUNT_LINES}) {
      const Run full = run_job(pat, file, mode, flags, 1, 0);
      CHECK(full.rc == XSG_OK && full.values.size() == full.stats.plan_chunks && full.total == full.values.back());
      for (const uint64_t n : {(uint64_t)1, full.total / 2, full.total, full.total + 5}) {
        for (int threads = 1; threads <= 2; ++threads) {
          const Run cut = run_job(pat, file, mode, flags, threads, n);
          std::vector<uint64_t> want;  // the running totals clamped, ending with the chunk that reached n
          for (const uint64_t x : full.values) {
            want.push_back(std::min(x, n));
            if (x >= n) break;
          }
          CHECK(cut.rc == XSG_OK && cut.total == std::min(n, full.total));
          CHECK(cut.values == want);
        }
      }
    }
  }

  // ---- (2) the early stop: the only hits lie in chunk k
  {
    const uint64_t k = 5;
    make_corpus(sparse, bytes, 99, k * kChunk + 2000, (k + 1) * kChunk - 2000);
    const Run full = run_job(pat, sparse, XSG_LINE_BYTE_OFFSETS, 0, 1, 0);
    // (the plan cuts at newlines, a line from the multiples of chunk_bytes: the hits keep 2000 bytes from both)
    CHECK(full.rc == XSG_OK && !full.values.empty() && full.values.front() / kChunk == k && full.values.back() / kChunk == k);
    for (int threads = 1; threads <= 2; ++threads) {
      const uint64_t ring = 2 * (uint64_t)threads + 3;
      CHECK(full.stats.plan_chunks >= 4 * (k + 1 + ring));
      for (const uint32_t mode : {(uint32_t)XSG_LINE_BYTE_OFFSETS, (uint32_t)XSG_COUNT_LINES, (uint32_t)XSG_LINES}) {
        const Run cut = run_job(pat, sparse, mode, 0, threads, 1);
        CHECK(cut.rc == XSG_OK && cut.total == 1);
        CHECK(cut.stats.chunks >= k + 1 && cut.stats.chunks <= k + 1 + ring);
        if (cut.stats.chunks > k + 1 + ring)
          std::fprintf(stderr, "early stop: %llu chunks searched, bound %llu\n", (unsigned long long)cut.stats.chunks, (unsigned long long)(k + 1 + ring));
      }
    }
  }

  // ---- (3) refusals of the start call
  {
    xsg_job_opts o;
    xsg_job_opts_init(&o);
    o.mode = XSG_LINES;
    o.chunk_bytes = kChunk;
    xsg_job* j = nullptr;
    CHECK(xsg_job_start_max_count(pat.data(), pat.size(), XSG_LIST_WHOLE_WORDS, 3, file.c_str(), nullptr, &o, &j) == XSG_EINVAL && !j);
    o.pattern_flags = XSG_FLAG_CONTEXT(1, 2);
    CHECK(xsg_job_start_max_count(pat.data(), pat.size(), 0, 3, file.c_str(), nullptr, &o, &j) == XSG_ENOTSUP && !j);
    CHECK(std::strstr(xsg_last_error(), "XSG_FLAG_CONTEXT") != nullptr);
    o.mode = XSG_COUNT_LINES;  // (a tag that ignores the context bits: refused all the same, the bits are not zero)
    CHECK(xsg_job_start_max_count(pat.data(), pat.size(), 0, 3, file.c_str(), nullptr, &o, &j) == XSG_ENOTSUP && !j);
    CHECK(xsg_job_start_max_count(pat.data(), pat.size(), 0, 0, file.c_str(), nullptr, nullptr, &j) == XSG_EINVAL);
  }

  // ---- (4) join and destroy while readers are still running
  for (int round = 0; round < 200; ++round) {
    xsg_job_opts o;
    xsg_job_opts_init(&o);
    o.mode = round % 3 == 0 ? XSG_COUNT_LINES : round % 3 == 1 ? XSG_LINES : XSG_LINE_INDICES;
    o.num_threads = 1 + round % 2;
    o.num_max_readers = 1 + round % 3;
    o.chunk_bytes = kChunk;
    xsg_job* j = nullptr;
    CHECK(xsg_job_start_max_count(pat.data(), pat.size(), 0, 1 + (uint64_t)(round % 7), file.c_str(), nullptr, &o, &j) == XSG_OK);
    if (!j) break;
    if (round & 1) {
      uint64_t total = 0;
      CHECK(xsg_job_join(j) == XSG_OK);
      CHECK(xsg_job_total(j, &total) == XSG_OK && total == 1 + (uint64_t)(round % 7));
    }
    xsg_job_destroy(j);  // (even rounds: while readers and workers run)
  }

  // ---- (5) the host searcher without a device side for the limit: the setter says so, 0 is always accepted
  {
    xsg_host_searcher* hs = nullptr;
    CHECK(xsg_host_searcher_create(0, pat.data(), pat.size(), 0, 2, &hs) == XSG_OK);
    CHECK(xsg_host_searcher_set_max_count(hs, 0) == XSG_OK);
    CHECK(xsg_host_searcher_set_max_count(hs, 3) == XSG_ENOTSUP);
    CHECK(xsg_host_searcher_set_max_count(nullptr, 3) == XSG_EINVAL);
    uint64_t c = 0;
    CHECK(xsg_host_count(hs, "a Sherlock\n", 11, 1, &c) == XSG_OK && c == 1);
    xsg_host_searcher_destroy(hs);
  }
  std::remove(file.c_str());
  std::remove(sparse.c_str());
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("max count pipeline: ok\n");
  return 0;
}
