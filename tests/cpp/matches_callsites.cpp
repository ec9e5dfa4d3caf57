// Compile-only: the call shapes of xs::matches (the matched text of every match, grep -o) against
// include/xsearch/xsearch.h and include/xsearch/tasks/gpu_searchers.h -- those of xs::lines / GpuLineSearcher.
#include <xsearch/xsearch.h>
#include <xsearch/tasks/gpu_searchers.h>

#include <algorithm>
#include <iostream>
#include <type_traits>

static const std::string pattern("colou?r");
static const std::string file_path("test/files/sample.txt");
static const std::string meta_file_path("test/files/sample.meta");

static_assert(XSG_MATCHES == 6, "the tag's value");
static_assert(xs::detail::traits<xs::matches>::mode == XSG_MATCHES, "xs::matches -> XSG_MATCHES");
static_assert(std::is_same<xs::detail::traits<xs::matches>::value_type, xs::detail::traits<xs::lines>::value_type>::value,
              "the result type of xs::lines");

int callsites(int argc, char** argv) {
  (void)argc;
  {  // live iteration, four arguments
    auto searcher = xs::extern_search<xs::matches>(argv[1], argv[2], false, 1);
    for (auto const& m : *searcher->getResult()) std::cout << m << '\n';
  }
  {  // join / getResult / copyResultSafe, with a metafile (five and six arguments)
    auto res = xs::extern_search<xs::matches>(pattern, file_path, meta_file_path, 4, 2);
    res->join();
    auto all = res->getResult()->copyResultSafe();
    static_assert(std::is_same<decltype(all), std::vector<std::string>>::value, "matches are strings");
    std::sort(all.begin(), all.end());
    auto six = xs::extern_search<xs::matches>(pattern, file_path, meta_file_path, true, 4, 4);
    if (six->getResult()->size() != all.size()) return 1;
  }
  {  // the functor beside GpuLineSearcher (SearcherC, concepts.h:36-39)
    using strtype = std::vector<char>;
    xs::GpuMatchSearcher<strtype> m(pattern, 0, 1, XSG_FLAG_REGEX);
    static_assert(std::is_move_constructible<xs::GpuMatchSearcher<strtype>>::value, "SearcherC");
    strtype data;
    static_assert(std::is_same<decltype(m(data)), std::optional<std::vector<std::string>>>::value, "as GpuLineSearcher");
    static_assert(std::is_same<decltype(m(data)), decltype(xs::GpuLineSearcher<strtype>(pattern)(data))>::value, "as GpuLineSearcher");
  }
  return 0;
}
