// xsgrep -- the reference's example/grep.cpp (PATTERN FILE, -c, -i; lines 23-82)
// on the MI355X engine, without boost::program_options.
//
//   xsgrep [-c] [-i] [-o] [-v] [-E|-F] [-x] [-A N] [-B N] [-C N] [-j THREADS] [-m METAFILE] PATTERN FILE|-
//   xsgrep -F [-c] [-i] [-o] [-v] [-w] [-A N] [-B N] [-C N] [-j THREADS] [-m METAFILE] (-e PATTERN)... [-f FILE]... FILE|-
//   xsgrep -F --all-of [-c] [-i] [-v] [-w] [-A N] [-B N] [-C N] [-j THREADS] [-m METAFILE] (-e PATTERN)... [-f FILE]... FILE|-
//   xsgrep -F [-i] [-w] --count-each (-e PATTERN)... [-f FILE]... FILE|-
//   xsgrep -F [-i] [-w] --find-each (-e PATTERN)... [-f FILE]... FILE|-
//   xsgrep [the options of the first three forms but -m] [-r] [-l|-L] [-H|--no-filename] PATTERN FILE FILE...
//
// -c  print only a count of matching lines   (grep.cpp:45-46 -> xs::count_lines)
// -i  ignore ASCII case                      (grep.cpp:47-48)
// -E  read PATTERN as a regex (RE2 syntax) whatever the reference's routing says (XS_FORCE_REGEX)
// -F  read PATTERN as plain text (XS_FORCE_LITERAL)
// -x  whole lines only: searches the regex (?m)^(?:PATTERN)$ (with -F, PATTERN escaped into an RE2 literal first;
//     otherwise a leading `^` and a trailing `$` of PATTERN are dropped, redundant under -x).  An empty PATTERN is
//     refused (it would match empty lines only), as is a PATTERN with anchors elsewhere (`^a|^b`).
// -v  the lines WITHOUT a match (XS_INVERT_MATCH -> XSG_FLAG_INVERT); with -c their number.  Like the reference's
//     xs::lines, a last line that lacks its newline is not printed.
// -o  print only the matched text, every match on its own line (xs::matches -> XSG_MATCHES).  With -c the count stays
//     the count of matching lines, as in grep.  Not with -v: a line without a match has no matched text.
// -A N, -B N, -C N  also print N lines after / before / around every selected line (XS_CONTEXT_AFTER / XS_CONTEXT_BEFORE ->
//     XSG_FLAG_CONTEXT), every line once, in file order, as GNU grep does with --no-group-separator: no `--` lines.
//     N is at most 4095.  With -c or -o the numbers are accepted and change nothing, as in grep.  Not with `-` (stdin):
//     the chunks read from a pipe are searched on their own.  (-m is the METAFILE here, not grep's --max-count.)
// -e PATTERN (repeatable), -f FILE (one literal per line, repeatable)  search for ANY of several literals (XS_PATTERN_LIST ->
//     xsg_set_literals).  They take PATTERN's place.  More than one pattern requires -F and excludes -x; a single -e equals
//     the positional PATTERN.  They combine with -c -i -o -v -A/-B/-C and with stdin.  -o with several patterns is
//     leftmost-FIRST in listing order: at a position where several literals occur the first-listed one is printed (-e ab
//     -e abc prints `ab` for `abc`); GNU grep prints the longest.  An empty pattern among several is refused (grep lets
//     it match every line).
// --count-each  a keyword table: one line per literal in listing order, COUNT<TAB>LITERAL, where COUNT is the number of the
//     literal's OCCURRENCES in the input (xsg_literal_counter_* -> xsg_count_literals: overlapping occurrences, literals
//     covered by another one and duplicates all count; under -i both sides are ASCII-lowered).  One pass over the input
//     however many literals there are.  Requires -F; a single -e or the positional PATTERN is a list of one.  Excludes
//     -c -o -v -x -A -B -C -m: it prints no lines and counts no lines.  The input is read in newline-aligned chunks, FILE
//     and stdin alike; a literal holds no newline, so no occurrence straddles a cut and the sums are the input's.
// --find-each  every occurrence with its identity: one line per occurrence, OFFSET:LITERAL -- the shape of grep -b -o -- in
//     file order and, at one offset, in listing order (xsg_literal_finder_* -> xsg_find_literals).  These are the occurrences
//     --count-each counts: overlapping ones, covered ones and duplicates of the list all appear.  OFFSET is the byte offset
//     in the input; LITERAL is printed as listed, not in the text's case.  Requires -F; reads the input in the same
//     newline-aligned chunks; excludes what --count-each excludes, and --count-each itself.
// -w  whole words only (grep -w; XS_WHOLE_WORDS -> XSG_LIST_WHOLE_WORDS): an occurrence counts only between two bytes that
//     are no word bytes (0-9 A-Z a-z _), the ends of the input's chunks counting as such.  Served with -F only -- the
//     literals go as a list, a single PATTERN as a list of one -- and never dropped: without -F it is an error.  Combines
//     with -c -i -o -v -A -B -C -e -f and --count-each, on FILE and on `-`; excludes -x.  As everywhere with a list, the
//     FIRST-listed literal that stands as a whole word at a position is the match.
// --all-of  the lines that hold EVERY pattern of the list (grep -F a | grep -F b | ...; XS_ALL_OF -> XSG_LIST_ALL_OF), in one
//     pass over the input.  Occurrences may overlap or cover one another (-e ab -e abc selects `abc`), duplicates are one
//     requirement, and under -w only whole-word occurrences count.  Requires -F; at most 64 patterns; a single PATTERN is a
//     list of one.  Combines with -c -i -v -w -A -B -C -e -f -j -m, on FILE and on `-`; with -v it selects the lines that
//     lack at least one pattern.  Excludes -o (a conjunction has no single matched text), -x, --count-each and --find-each.
// FILE FILE..., -r / --recursive  several files in one run (xsg_fileset_*: the files are the chunks of a few bindings, not
//     one job each).  -r walks directories depth-first, entries in byte-wise sorted order, regular files only; symbolic links
//     met during the walk are not followed.  Every file's result is what a search of that file alone gives.
// -l / --files-with-matches, -L / --files-without-match  print only the names of the files with / without a selected line
//     (a count of lines through the file set; no line is printed).  -c prints PATH:COUNT per file.
// -H / --with-filename, --no-filename  the prefix PATH: on every printed line; on by default with more than one FILE operand
//     or -r, off otherwise (-h stays help).  Under -A/-B/-C EVERY printed line carries PATH: -- GNU grep marks context lines
//     with PATH- instead, a deviation like the missing `--` separators.
//     Several FILE operands go with the positional PATTERN; with -e / -f there is one FILE operand, as before this mode
//     existed (a second one stays "unexpected argument"): a list of patterns reaches many files through -r DIR.
//     This mode combines with -i -v -o -w -x -E -F -e -f --all-of -A -B -C -j; it refuses `-` among the files, -m,
//     --count-each and --find-each (exit 2, before a device is touched).  Its exit status is grep's: 0 if something was
//     selected (under -L: listed), 1 if nothing was, 2 if a file failed -- `xsgrep: PATH: reason` on stderr, the other files
//     are still printed.  Output comes per published file, in operand / walk order.  A single FILE without any of -r -l -L
//     -H --no-filename takes the single-file path above, output and exit status unchanged.
// --max-count=N, --max-count N  stop after N selected lines PER FILE (grep --max-count; -m stays the METAFILE): under -v
//     after N lines without a match, under -c the count is min(count, N).  N takes digits only.  Served for one FILE, for
//     several (each file has its own N) and for `-`, where the loop over the pipe's chunks hands what is left of the budget
//     to the searchers and stops reading at 0; a large FILE is read no further than its Nth line and the buffers in flight.
//     Combines with -c -i -v -w -x -E -F -e -f --all-of -l -L -r -H.  --max-count=0 prints nothing and exits 1 without
//     touching a device.  Refused (exit 2, before a device is touched): with -o (grep counts LINES there, the engine's match
//     tags count matches), with -A -B -C (the budget of a file is spent in file order, its context is widened per chunk),
//     with --count-each and --find-each.
// -q / --quiet / --silent  print nothing; exit 0 if a line was selected, 1 if none, 2 on error.  Runs as --max-count=1 with a
//     count of lines, in every form but --count-each / --find-each (exit 2).  Without -q the single-file form's exit status
//     stays what it was.
// -l and -L pass a limit of 1 to the file set: a large file is read up to its first selected line.
// The one-letter options without an argument may be bundled (-vc, -ci, -oi, -wc, -rl, -qi).
// otherwise print the matching lines, live, as they are found (grep.cpp:74-79).
#include <xsearch/tasks/gpu_searchers.h>
#include <xsearch/xsearch.h>

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static const char kUsage[] =
    "usage: %s [-c] [-i] [-o] [-v] [-E|-F] [-x] [-A N] [-B N] [-C N] [-j THREADS] [-m METAFILE] PATTERN FILE|-\n"
    "       %s -F [-c] [-i] [-o] [-v] [-w] [-A N] [-B N] [-C N] [-j THREADS] [-m METAFILE] (-e PATTERN)... [-f FILE]... FILE|-\n"
    "       %s -F --all-of [-c] [-i] [-v] [-w] [-A N] [-B N] [-C N] [-j THREADS] [-m METAFILE] (-e PATTERN)... [-f FILE]... FILE|-\n"
    "       %s -F [-i] [-w] --count-each (-e PATTERN)... [-f FILE]... FILE|-\n"
    "       %s -F [-i] [-w] --find-each (-e PATTERN)... [-f FILE]... FILE|-\n"
    "       %s [options of the first three forms but -m] [-r] [-l|-L] [-H|--no-filename] PATTERN FILE FILE...\n"
    "  --max-count=N stop after N selected lines per file (-m is the METAFILE); N in digits; 0 prints nothing, exit 1; combines\n"
    "     with -c -i -v -w -x -E -F -e -f --all-of -l -L -r -H, on FILE, FILEs and -; not with -o -A -B -C --count-each --find-each\n"
    "  -q, --quiet print nothing: exit 0 if a line was selected, 1 if none, 2 on error (runs as --max-count=1 with -c)\n"
    "  FILE FILE..., -r / --recursive search several files in one run (directories depth-first, sorted byte-wise, regular files\n"
    "     only, links met on the walk not followed); -l / -L print only the names of files with / without a selected line;\n"
    "     -c prints PATH:COUNT; -H / --no-filename force the PATH: prefix on / off (default: on with several FILEs or -r;\n"
    "     context lines carry PATH: too, where GNU grep prints PATH-); exit status 0 selected, 1 nothing, 2 a file failed;\n"
    "     not with FILE = -, -m, --count-each, --find-each; with -e / -f one FILE operand only (use -r DIR)\n"
    "  -e PATTERN, -f FILE (one literal per line) search for any of several literals; both may repeat, need -F and exclude -x\n"
    "     when they give more than one pattern; -o then prints the FIRST-listed literal that occurs at a position (GNU grep: the longest)\n"
    "  -A N, -B N, -C N also print N lines after / before / around every selected line (N <= 4095), each line once and\n"
    "     without group separators; nothing changes under -c and -o; not with FILE = -\n"
    "  -o, --only-matching prints only the matched text, every match on its own line (not with -v)\n"
    "  -v, --invert-match selects the lines WITHOUT a match (with -c: counts them)\n"
    "  -w, --word-regexp whole words only: an occurrence counts only between bytes that are none of 0-9 A-Z a-z _ (or at the\n"
    "     ends of the input); needs -F (a single PATTERN goes as a list of one), excludes -x; works with --count-each too\n"
    "  --all-of selects the lines that hold EVERY pattern of the list (grep -F a | grep -F b), in one pass; needs -F, at most 64\n"
    "     patterns, a single PATTERN is a list of one; with -v the lines that lack at least one; excludes -o -x --count-each --find-each\n"
    "  -x searches (?m)^(?:PATTERN)$; PATTERN must not be empty\n"
    "  --count-each prints COUNT<TAB>LITERAL for every literal in listing order: its occurrences in the input, overlapping\n"
    "     ones and those inside another literal's included; needs -F, excludes -c -o -v -x -A -B -C -m\n"
    "  --find-each prints OFFSET:LITERAL for every occurrence of every literal, in file order and then listing order (the shape\n"
    "     of grep -b -o, with overlapping and covered occurrences); the literal as listed; needs -F, excludes what --count-each\n"
    "     excludes and --count-each itself\n";

// PATTERN without a leading `^` and a trailing unescaped `$`: under -x they say what the wrap says already
static std::string strip_edge_anchors(std::string p) {
  if (!p.empty() && p[0] == '^') p.erase(0, 1);
  if (!p.empty() && p.back() == '$') {
    size_t bs = 0;
    while (bs + 1 < p.size() && p[p.size() - 2 - bs] == '\\') ++bs;
    if (bs % 2 == 0) p.pop_back();
  }
  return p;
}

// PATTERN as an RE2 expression that matches exactly its bytes: ASCII punctuation gets a backslash
static std::string re2_literal(const std::string& p) {
  std::string r;
  for (unsigned char c : p) {
    const bool alnum = (c >= '0' && c <= '9') || ((c | 0x20) >= 'a' && (c | 0x20) <= 'z');
    if (c > 0x20 && c < 0x7f && !alnum) r += '\\';
    r += (char)c;
  }
  return r;
}

// N of -A / -B / -C: digits only, at most XSG_CONTEXT_MAX
static bool context_number(const std::string& text, long* out) {
  if (text.empty() || text.size() > 9 || text.find_first_not_of("0123456789") != std::string::npos) return false;
  *out = std::atol(text.c_str());
  return *out <= (long)XSG_CONTEXT_MAX;
}

// The input in newline-aligned chunks of about 16 MiB: each is cut behind its last newline and the rest opens the next
// one; a line longer than the target grows the chunk; the last chunk ends where the input does.  XSGREP_CHUNK_BYTES sets
// another target (the tests cut a small input into many chunks with it).
// `stop` (optional): set by f when it has seen enough; nothing more is read then.
template <typename F>
static void for_each_aligned_chunk(std::FILE* in, F&& f, const bool* stop = nullptr) {
  size_t target = 16u << 20;
  if (const char* e = std::getenv("XSGREP_CHUNK_BYTES"))
    if (std::atoll(e) > 0) target = (size_t)std::atoll(e);
  const size_t step = std::min<size_t>(target, 1u << 20);
  std::vector<char> buf;  // bytes read and not handed out yet
  size_t want = target;
  bool eof = false;
  for (;;) {
    if (stop && *stop) break;
    while (!eof && buf.size() < want) {
      const size_t at = buf.size();
      buf.resize(at + step);
      const size_t got = std::fread(buf.data() + at, 1, step, in);
      buf.resize(at + got);
      if (got == 0) eof = true;
    }
    if (buf.empty()) break;
    size_t cut = buf.size();
    if (!eof) {  // cut after the last newline; the rest opens the next chunk
      while (cut > 0 && buf[cut - 1] != '\n') --cut;
      if (cut == 0) {  // one line longer than the chunk target: keep reading
        want = buf.size() + target;
        continue;
      }
    }
    std::vector<char> chunk(buf.begin(), buf.begin() + (ptrdiff_t)cut);
    buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)cut);
    want = target;
    f(chunk);
  }
}

// --count-each: the table of xsg_literal_counter_* over the input's chunks; -> the exit status
static int count_each(const std::vector<std::string>& lits, bool icase, bool words, const std::string& file) {
  std::string list;
  for (const std::string& l : lits) list += (list.empty() ? "" : "\n") + l;
  std::FILE* in = file == "-" ? stdin : std::fopen(file.c_str(), "rb");
  if (!in) {
    std::fprintf(stderr, "xsgrep: cannot read '%s'\n", file.c_str());
    return 2;
  }
  xsg_literal_counter* lc = nullptr;
  int rc = xsg_literal_counter_create_opts(0, list.data(), list.size(), icase ? XSG_FLAG_IGNORE_CASE : 0u,
                                           words ? XSG_LIST_WHOLE_WORDS : 0u, &lc);
  if (rc == XSG_OK)
    for_each_aligned_chunk(in, [&](const std::vector<char>& chunk) {
      if (rc == XSG_OK) rc = xsg_literal_counter_add(lc, chunk.data(), chunk.size());
    });
  std::vector<uint64_t> counts(lits.size(), 0);
  if (rc == XSG_OK) rc = xsg_literal_counter_get(lc, counts.data(), counts.size(), nullptr);
  if (rc != XSG_OK) {
    std::fprintf(stderr, "xsgrep: %s\n", xsg_last_error());
    return rc == XSG_EINVAL ? 2 : 1;
  }
  for (size_t j = 0; j < lits.size(); ++j) std::cout << counts[j] << '\t' << lits[j] << '\n';
  std::cout.flush();
  return 0;
}

// --find-each: OFFSET:LITERAL for every occurrence (xsg_literal_finder_*), chunk after chunk; -> the exit status
static int find_each(const std::vector<std::string>& lits, bool icase, bool words, const std::string& file) {
  std::string list;
  for (const std::string& l : lits) list += (list.empty() ? "" : "\n") + l;
  std::FILE* in = file == "-" ? stdin : std::fopen(file.c_str(), "rb");
  if (!in) {
    std::fprintf(stderr, "xsgrep: cannot read '%s'\n", file.c_str());
    return 2;
  }
  xsg_literal_finder* lf = nullptr;
  int rc = xsg_literal_finder_create_opts(0, list.data(), list.size(), icase ? XSG_FLAG_IGNORE_CASE : 0u,
                                          words ? XSG_LIST_WHOLE_WORDS : 0u, &lf);
  uint64_t base = 0;  // the chunk's offset in the input
  if (rc == XSG_OK)
    for_each_aligned_chunk(in, [&](const std::vector<char>& chunk) {
      if (rc != XSG_OK) return;
      uint64_t* pos = nullptr;
      uint32_t* lit = nullptr;
      uint64_t n = 0;
      rc = xsg_literal_finder_find(lf, chunk.data(), chunk.size(), base, &pos, &lit, &n);
      if (rc == XSG_OK) {
        for (uint64_t i = 0; i < n; ++i) std::cout << pos[i] << ':' << lits[lit[i]] << '\n';
        xsg_free(pos);
        xsg_free(lit);
      }
      base += chunk.size();
    });
  if (rc != XSG_OK) {
    std::fprintf(stderr, "xsgrep: %s\n", xsg_last_error());
    return rc == XSG_EINVAL ? 2 : 1;
  }
  std::cout.flush();
  return 0;
}

// -r: the regular files under `dir`, depth-first, entries in byte-wise sorted order; links are not followed
static void walk(const std::string& dir, std::vector<std::string>& out) {
  std::vector<std::string> names;
  if (DIR* d = opendir(dir.c_str())) {
    while (const dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n != "." && n != "..") names.push_back(n);
    }
    closedir(d);
  } else {
    out.push_back(dir);  // (unreadable: the file set reports it)
    return;
  }
  std::sort(names.begin(), names.end());
  for (const std::string& n : names) {
    const std::string path = dir.empty() || dir.back() == '/' ? dir + n : dir + "/" + n;
    struct stat st;
    if (lstat(path.c_str(), &st) != 0) continue;
    if (S_ISDIR(st.st_mode)) walk(path, out);
    else if (S_ISREG(st.st_mode)) out.push_back(path);
  }
}

struct FileSetRun {
  bool count = false, only = false, list_with = false, list_without = false, prefix = false, is_list = false;
  uint32_t list_flags = 0;
  int threads = 2;
  uint64_t max_count = 0;  // per file (0: no limit)
  bool quiet = false;      // -q: nothing is printed
};

// several files (xsg_fileset_*): prints per published file; -> grep's exit status
static int search_files(const std::string& pattern, bool icase, const std::vector<std::string>& files, const FileSetRun& run) {
  xsg_fileset_opts o;
  xsg_fileset_opts_init(&o);
  const bool counting = run.count || run.list_with || run.list_without;
  o.mode = counting ? XSG_COUNT_LINES : run.only ? XSG_MATCHES : XSG_LINES;
  o.pattern_flags = xs::detail::pattern_flags(pattern, icase) | xs::detail::context_flags(o.mode);
  o.pattern_is_list = run.is_list ? 1u : 0u;
  o.list_flags = run.list_flags;
  o.device = (int32_t)xs::detail::env_u64("XS_DEVICE", 0);
  o.num_readers = run.threads > 2 ? std::min(run.threads, 16) : 0;  // (-j beyond its default asks for that many readers)
  o.chunk_bytes = xs::detail::env_u64("XS_CHUNK_BYTES", 0);
  o.batch_bytes = xs::detail::env_u64("XS_BATCH_BYTES", 0);
  std::vector<const char*> paths;
  for (const std::string& f : files) paths.push_back(f.c_str());
  xsg_fileset* set = nullptr;
  if (xsg_fileset_start_max_count(pattern.data(), pattern.size(), paths.data(), paths.size(), &o, run.max_count, &set) != XSG_OK) {
    std::fprintf(stderr, "xsgrep: %s\n", xsg_last_error());
    return 2;
  }
  const uint64_t n = files.size();
  std::vector<int32_t> status(n);
  std::vector<uint64_t> counts(n), file_ptr(n + 1);
  bool selected = false, failed = false;
  uint64_t next = 0;
  while (next < n) {
    uint64_t done = 0;
    int fin = 0;
    if (xsg_fileset_wait(set, next, &done, &fin) != XSG_OK) break;  // (the set failed: reported by the join below)
    if (done == next) break;
    xsg_fileset_status(set, status.data(), n);
    xsg_fileset_counts(set, counts.data(), n);
    if (!counting) xsg_fileset_file_ptr(set, file_ptr.data(), n + 1);
    for (uint64_t f = next; f < done; ++f) {
      const std::string& path = files[f];
      if (status[f] != XSG_OK) {
        std::cout.flush();
        std::fprintf(stderr, "xsgrep: %s: %s\n", path.c_str(),
                     status[f] == XSG_ENOTSUP ? "not searched: it holds bytes this expression does not accept (>= 0x80), or context that crosses a whole chunk"
                                              : "cannot be read (missing, unreadable, no regular file, or changed while it was read)");
        failed = true;
        continue;
      }
      if (run.quiet) {
        selected |= run.list_without ? counts[f] == 0 : counts[f] != 0;
      } else if (run.list_with || run.list_without) {
        if ((counts[f] != 0) == run.list_with) {
          std::cout << path << '\n';
          selected = true;
        }
      } else if (run.count) {
        if (run.prefix) std::cout << path << ':';
        std::cout << counts[f] << '\n';
        selected |= counts[f] != 0;
      } else {
        for (uint64_t k = file_ptr[f]; k < file_ptr[f + 1]; ++k) {
          const char* d = nullptr;
          uint64_t len = 0;
          if (xsg_fileset_get_line(set, k, &d, &len) != XSG_OK) break;
          if (run.prefix) std::cout << path << ':';
          std::cout.write(d, (std::streamsize)len);
          std::cout << '\n';
        }
        selected |= file_ptr[f + 1] != file_ptr[f];
      }
    }
    std::cout.flush();
    next = done;
  }
  if (xsg_fileset_join(set) != XSG_OK) {
    std::cout.flush();
    std::fprintf(stderr, "xsgrep: %s\n", xsg_last_error());
    return 2;
  }
  return failed ? 2 : selected ? 0 : 1;
}

int main(int argc, char** argv) {
  bool count = false, icase = false, fixed = false, extended = false, whole_lines = false, invert = false, only = false;
  bool each = false, find = false, context_given = false, words = false, all_of = false;
  bool recursive = false, list_with = false, list_without = false, with_filename = false, no_filename = false;
  bool quiet = false, max_given = false;
  std::string max_text;
  std::vector<std::string> files;  // every FILE operand (`file` is the first)
  int threads = 2;  // grep.cpp:21
  long before = 0, after = 0;
  std::string meta, pattern, file;
  std::vector<std::string> patterns;  // -e / -f: they take PATTERN's place
  bool have_patterns = false;
  int pos = 0;
  std::vector<std::string> args;
  for (int i = 1; i < argc; ++i) {  // -vc -> -v -c (only letters that take no argument; anything else stays one word)
    const std::string a = argv[i];
    if (a.size() > 2 && a[0] == '-' && a[1] != '-' && a.find_first_not_of("ciEFxvowlLrHq", 1) == std::string::npos) {
      for (size_t k = 1; k < a.size(); ++k) args.push_back(std::string("-") + a[k]);
    } else {
      args.push_back(a);
    }
  }
  const int nargs = (int)args.size();
  for (int i = 0; i < nargs; ++i) {
    const std::string a = args[i];
    if (a == "-v" || a == "--invert-match") {
      invert = true;
    } else if (a == "-o" || a == "--only-matching") {
      only = true;
    } else if (a == "-w" || a == "--word-regexp") {
      words = true;
    } else if (a == "--all-of") {
      all_of = true;
    } else if (a == "-r" || a == "--recursive") {
      recursive = true;
    } else if (a == "-l" || a == "--files-with-matches") {
      list_with = true;
    } else if (a == "-L" || a == "--files-without-match") {
      list_without = true;
    } else if (a == "-H" || a == "--with-filename") {
      with_filename = true;
    } else if (a == "--no-filename") {
      no_filename = true;
    } else if (a == "-q" || a == "--quiet" || a == "--silent") {
      quiet = true;
    } else if (a.rfind("--max-count=", 0) == 0) {
      max_text = a.substr(12);
      max_given = true;
    } else if (a == "--max-count" && i + 1 < nargs) {
      max_text = args[++i];
      max_given = true;
    } else if (a == "--count-each") {
      each = true;
    } else if (a == "--find-each") {
      find = true;
    } else if (a == "-c" || a == "--count") {
      count = true;
    } else if (a == "-i" || a == "--ignore-case") {
      icase = true;
    } else if (a == "-F" || a == "--fixed-strings") {
      fixed = true;  // like grep -F: never read the pattern as a regex
    } else if (a == "-E" || a == "--extended-regexp") {
      extended = true;
    } else if (a == "-x" || a == "--line-regexp") {
      whole_lines = true;
    } else if ((a == "-A" || a == "-B" || a == "-C") && i + 1 < nargs) {
      long n = 0;
      if (!context_number(args[++i], &n)) {
        std::fprintf(stderr, "xsgrep: %s takes a number of lines from 0 to %u, not '%s'\n", a.c_str(), (unsigned)XSG_CONTEXT_MAX, args[i].c_str());
        return 2;
      }
      if (a != "-A") before = n;
      if (a != "-B") after = n;
      context_given = true;
    } else if ((a == "-j" || a == "--threads") && i + 1 < nargs) {
      threads = std::atoi(args[++i].c_str());
    } else if ((a == "-m" || a == "--meta") && i + 1 < nargs) {
      meta = args[++i];
    } else if ((a == "-e" || a == "--regexp") && i + 1 < nargs) {
      patterns.push_back(args[++i]);
      have_patterns = true;
    } else if ((a == "-f" || a == "--file") && i + 1 < nargs) {
      std::ifstream in(args[++i], std::ios::binary);
      if (!in) {
        std::fprintf(stderr, "xsgrep: cannot read the pattern file '%s'\n", args[i].c_str());
        return 2;
      }
      std::stringstream all;
      all << in.rdbuf();
      std::string text = all.str();
      if (!text.empty() && text.back() == '\n') text.pop_back();  // the last line's newline ends it, it opens no empty pattern
      for (size_t at = 0;;) {  // (an empty file holds no pattern: grep -f /dev/null matches nothing)
        if (text.empty()) break;
        const size_t nl = text.find('\n', at);
        patterns.push_back(text.substr(at, nl == std::string::npos ? std::string::npos : nl - at));
        if (nl == std::string::npos) break;
        at = nl + 1;
      }
      have_patterns = true;
    } else if (a == "-h" || a == "--help") {
      std::printf(kUsage, argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
      return 0;
    } else if (pos == 0 && !have_patterns) {
      pattern = a;
      ++pos;
    } else {
      files.push_back(a);
      pos = 2;
    }
  }
  if (have_patterns && !pattern.empty()) {  // (PATTERN was read before the first -e / -f: it is the first FILE)
    files.insert(files.begin(), pattern);
    pattern.clear();
    pos = 2;
  }
  if (have_patterns && files.size() > 1) {  // with -e / -f there is ONE FILE operand, as there always was (under -r: a directory)
    std::fprintf(stderr, "unexpected argument '%s'\n", files[1].c_str());
    return 2;
  }
  if (pos != 2) {
    std::fprintf(stderr, kUsage, argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
    return 2;
  }
  file = files[0];
  uint64_t max_count = 0;
  if (max_given) {  // digits only; refused where grep's lines and the engine's entries part ways
    if (max_text.empty() || max_text.size() > 19 || max_text.find_first_not_of("0123456789") != std::string::npos) {
      std::fprintf(stderr, "xsgrep: --max-count takes a number of lines in digits, not '%s'\n", max_text.c_str());
      return 2;
    }
    max_count = std::strtoull(max_text.c_str(), nullptr, 10);
    const char* clash = only && !quiet ? "excludes -o (grep counts lines there, the match tags count matches)"
                        : context_given ? "excludes -A, -B and -C (a file's budget is spent in file order, its context is widened per chunk)"
                        : each ? "excludes --count-each (that counts per literal, it selects no lines)"
                        : find ? "excludes --find-each (that prints occurrences, it selects no lines)" : nullptr;
    if (clash) {
      std::fprintf(stderr, "xsgrep: --max-count %s\n", clash);
      return 2;
    }
  }
  if (quiet && (each || find)) {
    std::fprintf(stderr, "xsgrep: -q excludes --count-each and --find-each (they select no lines)\n");
    return 2;
  }
  if (quiet) count = true, only = false;  // -q: a count of lines under a limit of 1, nothing printed
  // several files, or an option that only the file-set mode knows; a single FILE without them goes the way it always went
  const bool multi = files.size() > 1 || recursive || list_with || list_without || with_filename || no_filename;
  if (multi) {
    const char* clash = std::find(files.begin(), files.end(), "-") != files.end() ? "`-` (stdin) is not served among several files or with -r -l -L -H --no-filename"
                        : !meta.empty() ? "-m METAFILE belongs to one FILE: it is not served with several files or -r -l -L -H --no-filename"
                        : each ? "--count-each reads one input: it is not served with several files or -r -l -L -H --no-filename"
                        : find ? "--find-each reads one input: it is not served with several files or -r -l -L -H --no-filename"
                        : list_with && list_without ? "-l and -L exclude each other"
                        : with_filename && no_filename ? "-H and --no-filename exclude each other" : nullptr;
    if (clash) {
      std::fprintf(stderr, "xsgrep: %s\n", clash);
      return 2;
    }
  }
  if (words && (!fixed || whole_lines)) {  // never a silent substring search
    std::fprintf(stderr, "xsgrep: -w (whole words) is served for literals only: it needs -F and excludes -x\n");
    return 2;
  }
  if (all_of) {  // never a silent any-of search
    const char* clash = !fixed ? "needs -F: it selects the lines that hold every one of a list of literals"
                        : only ? "excludes -o (a conjunction has no single matched text)"
                        : whole_lines ? "excludes -x" : each ? "excludes --count-each (that counts per literal, it selects no lines)"
                        : find ? "excludes --find-each (that prints occurrences, it selects no lines)" : extended ? "excludes -E" : nullptr;
    if (clash) {
      std::fprintf(stderr, "xsgrep: --all-of %s\n", clash);
      return 2;
    }
    if (have_patterns && patterns.size() > XSG_MAX_ALL_OF_LITERALS) {
      std::fprintf(stderr, "xsgrep: --all-of: %zu patterns, at most %u are served\n", patterns.size(), (unsigned)XSG_MAX_ALL_OF_LITERALS);
      return 2;
    }
  }
  if (find) {  // every occurrence with its literal: no lines are selected, printed or counted
    const char* clash = !fixed ? "needs -F: it finds literals" : each ? "excludes --count-each (one prints occurrences, the other their number)"
                        : count ? "excludes -c (it prints occurrences, it counts no lines)"
                        : only ? "excludes -o (it prints every occurrence, not the matches of the leftmost-first walk)"
                        : invert ? "excludes -v (an occurrence has no inverted form)"
                        : whole_lines ? "excludes -x (it finds occurrences, not whole lines)"
                        : context_given ? "excludes -A, -B and -C (it prints no lines)"
                        : !meta.empty() ? "excludes -m (it reads the input in chunks of its own)" : extended ? "excludes -E" : nullptr;
    if (clash) {
      std::fprintf(stderr, "xsgrep: --find-each %s\n", clash);
      return 2;
    }
    if (!have_patterns) patterns.push_back(pattern);
    if (patterns.empty()) {
      std::fprintf(stderr, "xsgrep: -f: the pattern file holds no pattern\n");
      return 2;
    }
    for (const std::string& p : patterns)
      if (p.empty() || p.find('\n') != std::string::npos) {
        std::fprintf(stderr, "xsgrep: --find-each: an empty pattern (or one with a newline) is not served\n");
        return 2;
      }
    const int rc = find_each(patterns, icase, words, file);
    std::fflush(stdout);
    std::_Exit(rc);  // (as at the end of main: the runtime's teardown is left to the kernel)
  }
  if (each) {  // a keyword table: no lines are selected, printed or counted
    const char* clash = !fixed ? "needs -F: it counts literals" : count ? "excludes -c (it counts occurrences per literal, not lines)"
                        : only ? "excludes -o (it prints counts, not matched text)" : invert ? "excludes -v (an occurrence count has no inverted form)"
                        : whole_lines ? "excludes -x (it counts occurrences, not whole lines)"
                        : context_given ? "excludes -A, -B and -C (it prints no lines)"
                        : !meta.empty() ? "excludes -m (it reads the input in chunks of its own)" : extended ? "excludes -E" : nullptr;
    if (clash) {
      std::fprintf(stderr, "xsgrep: --count-each %s\n", clash);
      return 2;
    }
    if (!have_patterns) patterns.push_back(pattern);
    if (patterns.empty()) {
      std::fprintf(stderr, "xsgrep: -f: the pattern file holds no pattern\n");
      return 2;
    }
    for (const std::string& p : patterns)
      if (p.empty() || p.find('\n') != std::string::npos) {
        std::fprintf(stderr, "xsgrep: --count-each: an empty pattern (or one with a newline) is not served\n");
        return 2;
      }
    const int rc = count_each(patterns, icase, words, file);
    std::fflush(stdout);
    std::_Exit(rc);  // (as at the end of main: the runtime's teardown is left to the kernel)
  }
  bool list = false;
  if (have_patterns) {
    if (patterns.empty()) {
      std::fprintf(stderr, "xsgrep: -f: the pattern file holds no pattern\n");
      return 2;
    }
    if (patterns.size() == 1) {
      pattern = patterns[0];  // a single -e equals the positional PATTERN
    } else {
      if (!fixed || whole_lines) {
        std::fprintf(stderr, "xsgrep: more than one pattern (-e / -f) is served as a list of literals: it needs -F and excludes -x\n");
        return 2;
      }
      for (const std::string& p : patterns) {
        if (p.empty() || p.find('\n') != std::string::npos) {
          std::fprintf(stderr, "xsgrep: an empty pattern (or one with a newline) among several is not served\n");
          return 2;
        }
        pattern += (pattern.empty() ? "" : "\n") + p;
      }
      list = true;
    }
  }
  if (fixed && extended) {
    std::fprintf(stderr, "xsgrep: -E and -F exclude each other\n");
    return 2;
  }
  if ((words || all_of) && !list) {  // a single PATTERN under -F -w or -F --all-of: a list of one
    if (pattern.empty() || pattern.find('\n') != std::string::npos) {
      std::fprintf(stderr, "xsgrep: %s: an empty pattern (or one with a newline) is not served\n", words ? "-w" : "--all-of");
      return 2;
    }
    list = true;
  }
  if (only && invert) {
    std::fprintf(stderr, "xsgrep: -o and -v exclude each other (a line without a match has no matched text)\n");
    return 2;
  }
  const bool context = (before != 0 || after != 0) && !count && !only;  // (grep -c -C and grep -o -C ignore the numbers)
  if (context && file == "-") {
    std::fprintf(stderr, "xsgrep: -A, -B and -C are not served on stdin: the chunks of a pipe are searched on their own\n");
    return 2;
  }
  if (whole_lines) {  // a line-anchored regex (xsg.h, XSG_FLAG_REGEX): the whole line is one match of PATTERN
    const std::string body = fixed ? re2_literal(pattern) : strip_edge_anchors(pattern);
    if (body.empty()) {
      std::fprintf(stderr, "xsgrep: -x with an empty pattern (it matches empty lines only) is not supported\n");
      return 2;
    }
    pattern = "(?m)^(?:" + body + ")$";
    if (pattern.size() > XSG_MAX_REGEX) {
      std::fprintf(stderr, "xsgrep: -x: the expression is longer than %u bytes\n", (unsigned)XSG_MAX_REGEX);
      return 2;
    }
    extended = true, fixed = false;
  }
  if (max_given && max_count == 0) return 1;  // nothing can be selected: no device is touched
  const uint64_t limit = quiet ? 1 : max_count;
  if (limit) setenv("XS_MAX_COUNT", std::to_string(limit).c_str(), 1);
  if (list) setenv("XS_PATTERN_LIST", "1", 1);
  if (words) setenv("XS_WHOLE_WORDS", "1", 1);
  if (all_of) setenv("XS_ALL_OF", "1", 1);
  const uint32_t list_flags = (words ? XSG_LIST_WHOLE_WORDS : 0u) | (all_of ? XSG_LIST_ALL_OF : 0u);
  if (fixed) setenv("XS_FORCE_LITERAL", "1", 1);
  if (extended) setenv("XS_FORCE_REGEX", "1", 1);
  if (invert) setenv("XS_INVERT_MATCH", "1", 1);
  setenv("XS_CONTEXT_BEFORE", context ? std::to_string(before).c_str() : "0", 1);
  setenv("XS_CONTEXT_AFTER", context ? std::to_string(after).c_str() : "0", 1);
  try {
    std::ios::sync_with_stdio(false);
    if (multi) {
      std::vector<std::string> paths;
      for (const std::string& f : files) {
        struct stat st;
        if (recursive && stat(f.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) walk(f, paths);
        else paths.push_back(f);
      }
      FileSetRun run;
      run.count = count, run.only = only, run.list_with = list_with, run.list_without = list_without;
      run.prefix = with_filename || (!no_filename && (files.size() > 1 || recursive));
      run.is_list = list, run.list_flags = list_flags, run.threads = threads;
      run.quiet = quiet;
      run.max_count = list_with || list_without ? 1 : limit;  // (a name is decided by the file's first selected line)
      const int rc = search_files(pattern, icase, paths, run);
      std::cout.flush();
      std::fflush(stdout);
      std::_Exit(rc);  // (as at the end of main: the runtime's teardown is left to the kernel)
    }
    if (file == "-") {
      // stdin (grep.cpp:37: "input file, stdin if '-' or empty"): no file to plan chunks on, so
      // read newline-aligned chunks here and hand each to the reference-style searcher functors
      // (include/xsearch/tasks/gpu_searchers.h), like Searcher::run_thread does with a reader.
      const uint32_t flags = xs::detail::pattern_flags(pattern, icase);
      xs::GpuLineSearcher<std::vector<char>> lines(pattern, 0, 1, flags, list, list_flags);
      xs::GpuMatchSearcher<std::vector<char>> matches(pattern, 0, 1, flags, list, list_flags);
      xs::GpuCountSearcher<std::vector<char>> counter(pattern, true, 0, 1, flags, list, list_flags);
      uint64_t total = 0, left = limit;  // left: what remains of the budget (limit != 0)
      bool enough = false;
      for_each_aligned_chunk(stdin, [&](const std::vector<char>& chunk) {
        if (count) {
          if (limit) counter.set_max_count(left);
          if (auto c = counter(chunk)) total += *c, left -= limit ? *c : 0;
        } else if (only) {
          if (auto ms = matches(chunk))
            for (const auto& m : *ms) std::cout << m << '\n';
        } else {
          if (limit) lines.set_max_count(left);
          if (auto ls = lines(chunk)) {
            for (const auto& l : *ls) std::cout << l << '\n';
            left -= limit ? ls->size() : 0;
          }
        }
        enough = limit != 0 && left == 0;
      }, &enough);
      if (quiet) {
        std::fflush(stdout);
        std::_Exit(total ? 0 : 1);
      }
      if (count) std::cout << total << std::endl;
      return 0;
    }
    if (count) {
      auto searcher = meta.empty() ? xs::extern_search<xs::count_lines>(pattern, file, icase, threads)
                                   : xs::extern_search<xs::count_lines>(pattern, file, meta, icase, threads, threads);
      searcher->join();
      if (quiet) {
        std::fflush(stdout);
        std::_Exit(searcher->getResult()->size() ? 0 : 1);
      }
      std::cout << searcher->getResult()->size() << std::endl;
    } else if (only) {
      auto searcher = meta.empty() ? xs::extern_search<xs::matches>(pattern, file, icase, threads)
                                   : xs::extern_search<xs::matches>(pattern, file, meta, icase, threads, threads);
      for (auto const& match : *searcher->getResult()) {
        std::cout << match << '\n';
      }
    } else {
      auto searcher = meta.empty() ? xs::extern_search<xs::lines>(pattern, file, icase, threads)
                                   : xs::extern_search<xs::lines>(pattern, file, meta, icase, threads, threads);
      for (auto const& line : *searcher->getResult()) {
        std::cout << line << '\n';
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "xsgrep: %s\n", e.what());
    return quiet ? 2 : 1;
  }
  // Everything is printed; what is left is tearing the HIP runtime down (streams, pinned memory, the device context):
  // 40-90 ms of a process that lives 0.2 s on a small file (profiles/r04_cli_start.txt).  A command-line tool leaves that
  // to the kernel, as grep leaves its buffers: flush and go.  (tools/my_grep.cpp, the README's program, returns normally.)
  std::cout.flush();
  std::fflush(stdout);
  std::_Exit(0);
}
