// xsearch/tasks/gpu_searchers.h -- MI355X-backed searcher functors with the call
// signature of the reference's task adapters
// (include/xsearch/tasks/searchers.h:38-93):
//
//   std::optional<PartRes> operator()(const DataT& data) const
//
// so they satisfy the reference's SearcherC concept (include/xsearch/concepts.h:36-39)
// and plug into its worker loop (include/xsearch/Searcher.h:100-120) in place of
// IndexSearcher / LineIndexSearcher / LineSearcher.  Like those, they return
// CHUNK-LOCAL results and std::nullopt when the chunk has no hit
// (searchers.h:51-53), and one shared const instance may be called from many
// threads at once (Searcher.h:110): each concurrent call uses its own pinned
// staging buffer, device buffer and HIP stream inside libxsg.
// Context lines (XSG_FLAG_CONTEXT in `flags`) are CHUNK-LOCAL like everything here: the context of the line functors is
// clipped at the edges of the chunk handed in, and nothing joins consecutive calls (xs::extern_search does, xsg.h).
//
// A trailing `literal_list = true` makes `pattern` a list of literals separated by '\n' (xsg.h: xsg_set_literals); behind
// it `list_flags` takes the list's options (XSG_LIST_WHOLE_WORDS: whole words only; the edges of every chunk handed in are
// word boundaries; XSG_LIST_ALL_OF: the line functors and GpuCountSearcher(skip_to_nl = true) select the lines of the chunk
// that hold every literal, and the match functors -- GpuIndexSearcher, GpuMatchSearcher, GpuCountSearcher(skip_to_nl =
// false) -- throw std::runtime_error on every call, with XSG_ENOTSUP's message, which names XSG_LIST_ALL_OF).
//
// DataT: anything with data() -> convertible to const char* and size()
// (the reference's DefaultDataC, concepts.h:17-22; xs::strtype = std::vector<char>).
#pragma once

#include <xsg.h>

#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

namespace xs {

namespace gpu_detail {

struct Handle {
  xsg_host_searcher* hs = nullptr;
  // literal_list: `pattern` holds several literals separated by '\n' (xsg.h: xsg_set_literals)
  Handle(const std::string& pattern, int device, int max_slots, uint32_t flags, bool literal_list = false, uint32_t list_flags = 0) {
    if (list_flags && !literal_list) throw std::invalid_argument("xs::Gpu*Searcher: list_flags need literal_list = true");
    const int r = literal_list ? xsg_host_searcher_create_list_opts(device, pattern.data(), pattern.size(), flags, list_flags, max_slots, &hs)
                               : xsg_host_searcher_create(device, pattern.data(), pattern.size(), flags, max_slots, &hs);
    if (r != XSG_OK)
      throw std::runtime_error(std::string("xs::Gpu*Searcher: ") + xsg_strerror(r) + " (" + xsg_last_error() + ")");
  }
  ~Handle() { xsg_host_searcher_destroy(hs); }
  // xsg_host_searcher_set_max_count: every later call reports the chunk's first n entries (a count: min(count, n)); 0: all
  void set_max_count(uint64_t n) const {
    const int r = xsg_host_searcher_set_max_count(hs, n);
    if (r != XSG_OK)
      throw std::runtime_error(std::string("xs::Gpu*Searcher: ") + xsg_strerror(r) + " (" + xsg_last_error() + ")");
  }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
};

[[noreturn]] inline void raise(int r) {
  throw std::runtime_error(std::string("xs::Gpu*Searcher: ") + xsg_strerror(r) + " (" + xsg_last_error() + ")");
}

template <class T>
std::optional<std::vector<uint64_t>> offsets(const Handle& h, uint32_t mode, const T& data) {
  uint64_t* out = nullptr;
  uint64_t n = 0;
  const int r = xsg_host_offsets(h.hs, mode, data.data(), data.size(), &out, &n);
  if (r != XSG_OK) raise(r);
  if (n == 0) {
    xsg_free(out);
    return {};
  }
  std::vector<uint64_t> v(out, out + n);
  xsg_free(out);
  return std::make_optional(std::move(v));
}

// xsg_host_lines / xsg_host_matches: n strings as lengths + packed bytes
template <class T>
std::optional<std::vector<std::string>> strings(const Handle& h, decltype(&xsg_host_lines) call, const T& data) {
  uint64_t* lens = nullptr;
  char* bytes = nullptr;
  uint64_t n = 0, nb = 0;
  const int r = call(h.hs, data.data(), data.size(), &lens, &bytes, &n, &nb);
  if (r != XSG_OK) raise(r);
  std::vector<std::string> v;
  v.reserve(n);
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; ++i) {
    v.emplace_back(bytes + at, lens[i]);
    at += lens[i];
  }
  xsg_free(lens);
  xsg_free(bytes);
  if (v.empty()) return {};
  return v;
}

}  // namespace gpu_detail

// replaces IndexSearcher (searchers.h:38-59): search::byte_offsets_match(data, pattern, false)
template <class T = std::vector<char>>
class GpuIndexSearcher {
 public:
  explicit GpuIndexSearcher(std::string pattern, int device = 0, int max_concurrent = 8, uint32_t flags = 0,
           bool literal_list = false, uint32_t list_flags = 0)
      : _h(std::make_shared<gpu_detail::Handle>(pattern, device, max_concurrent, flags, literal_list, list_flags)) {}
  std::optional<std::vector<uint64_t>> operator()(const T& data) const {
    return gpu_detail::offsets(*_h, XSG_MATCH_BYTE_OFFSETS, data);
  }

  // optional: a limit for the calls that follow (a loop over the chunks of a stream hands in what is left of its budget)
  void set_max_count(uint64_t n) const { _h->set_max_count(n); }

 private:
  std::shared_ptr<gpu_detail::Handle> _h;
};

// replaces LineIndexSearcher (searchers.h:61-76): search::byte_offsets_line(data, pattern)
template <class T = std::vector<char>>
class GpuLineIndexSearcher {
 public:
  explicit GpuLineIndexSearcher(std::string pattern, int device = 0, int max_concurrent = 8, uint32_t flags = 0,
           bool literal_list = false, uint32_t list_flags = 0)
      : _h(std::make_shared<gpu_detail::Handle>(pattern, device, max_concurrent, flags, literal_list, list_flags)) {}
  std::optional<std::vector<uint64_t>> operator()(const T& data) const {
    return gpu_detail::offsets(*_h, XSG_LINE_BYTE_OFFSETS, data);
  }

  // optional: a limit for the calls that follow (a loop over the chunks of a stream hands in what is left of its budget)
  void set_max_count(uint64_t n) const { _h->set_max_count(n); }

 private:
  std::shared_ptr<gpu_detail::Handle> _h;
};

// replaces LineSearcher (searchers.h:78-93): search::line(data, pattern)
template <class T = std::vector<char>>
class GpuLineSearcher {
 public:
  explicit GpuLineSearcher(std::string pattern, int device = 0, int max_concurrent = 8, uint32_t flags = 0,
           bool literal_list = false, uint32_t list_flags = 0)
      : _h(std::make_shared<gpu_detail::Handle>(pattern, device, max_concurrent, flags, literal_list, list_flags)) {}
  std::optional<std::vector<std::string>> operator()(const T& data) const {
    return gpu_detail::strings(*_h, xsg_host_lines, data);
  }

  // optional: a limit for the calls that follow (a loop over the chunks of a stream hands in what is left of its budget)
  void set_max_count(uint64_t n) const { _h->set_max_count(n); }

 private:
  std::shared_ptr<gpu_detail::Handle> _h;
};

// the matched text of every match IndexSearcher reports (grep -o; no reference adapter exists for it): XSG_MATCHES
template <class T = std::vector<char>>
class GpuMatchSearcher {
 public:
  explicit GpuMatchSearcher(std::string pattern, int device = 0, int max_concurrent = 8, uint32_t flags = 0,
           bool literal_list = false, uint32_t list_flags = 0)
      : _h(std::make_shared<gpu_detail::Handle>(pattern, device, max_concurrent, flags, literal_list, list_flags)) {}
  std::optional<std::vector<std::string>> operator()(const T& data) const {
    return gpu_detail::strings(*_h, xsg_host_matches, data);
  }

  // optional: a limit for the calls that follow (a loop over the chunks of a stream hands in what is left of its budget)
  void set_max_count(uint64_t n) const { _h->set_max_count(n); }

 private:
  std::shared_ptr<gpu_detail::Handle> _h;
};

// search::count(data, pattern, skip_to_nl) as a functor (no reference adapter exists for it)
template <class T = std::vector<char>>
class GpuCountSearcher {
 public:
  explicit GpuCountSearcher(std::string pattern, bool skip_to_nl = true, int device = 0, int max_concurrent = 8,
                            uint32_t flags = 0, bool literal_list = false, uint32_t list_flags = 0)
      : _h(std::make_shared<gpu_detail::Handle>(pattern, device, max_concurrent, flags, literal_list, list_flags)), _skip(skip_to_nl) {}
  std::optional<uint64_t> operator()(const T& data) const {
    uint64_t c = 0;
    const int r = xsg_host_count(_h->hs, data.data(), data.size(), _skip ? 1 : 0, &c);
    if (r != XSG_OK) gpu_detail::raise(r);
    if (c == 0) return {};
    return c;
  }

  // optional: a limit for the calls that follow (a loop over the chunks of a stream hands in what is left of its budget)
  void set_max_count(uint64_t n) const { _h->set_max_count(n); }

 private:
  std::shared_ptr<gpu_detail::Handle> _h;
  bool _skip;
};

}  // namespace xs
