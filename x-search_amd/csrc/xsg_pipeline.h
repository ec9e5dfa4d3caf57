// xsg_pipeline.h -- what the host pipelines share above the chunk-level ABI (xsg_job.cpp: one file per job;
// xsg_hostsearch.cpp: chunks in host memory; xsg_fileset.cpp: a list of files per set): the result tags by kind, the pattern
// of a worker's context, and the device-side entry points that are reached through weak references.  The first two files are
// also linked without the device library (tests/cpp: the sanitizer binaries, against a stand-in that knows nothing of context
// or literal lists), and what needs one of them is then refused at its start.  Not installed.
#pragma once
#include "xsg_objects.h"

// the device side of XSG_FLAG_CONTEXT, and of a literal list (xsg_job_opts.pattern_is_list, xsg_host_searcher_create_list)
extern "C" int xsg_result_context_edges(xsg_shard* shard, xsg_context_edge* out, uint64_t cap_chunks) __attribute__((weak));
extern "C" int xsg_set_literals_opts(xsg_ctx* ctx, const void* list, size_t n, uint32_t flags, uint32_t list_flags) __attribute__((weak));
extern "C" int xsg_set_max_count(xsg_ctx* ctx, uint64_t max_count) __attribute__((weak));  // (absent: the publishers cut alone)
extern "C" int xsg_literals_info(const void* list, size_t n, uint32_t flags, xsg_literal_list* info, uint8_t* filter) __attribute__((weak));

namespace xsg {
static const char kNoListMsg[] = "this build holds no device side for literal lists";
// the pattern of a worker, a slot or a set: a literal list where the caller said so, with its list flags (XSG_LIST_WHOLE_WORDS)
static int set_job_pattern(xsg_ctx* ctx, const std::vector<uint8_t>& pattern, uint32_t flags, bool is_list, uint32_t list_flags) {
  if (!is_list) return xsg_set_pattern(ctx, pattern.data(), pattern.size(), flags);
  if (!xsg_set_literals_opts) return fail(XSG_ENOTSUP, "%s", kNoListMsg);
  return xsg_set_literals_opts(ctx, pattern.data(), pattern.size(), flags, list_flags);
}
static int check_list_flags(uint32_t list_flags) {
  return (list_flags & ~(XSG_LIST_WHOLE_WORDS | XSG_LIST_ALL_OF)) ? fail(XSG_EINVAL, "unknown list flags 0x%x", list_flags) : XSG_OK;
}
static bool context_flags(uint32_t flags) { return XSG_CONTEXT_BEFORE(flags) != 0 || XSG_CONTEXT_AFTER(flags) != 0; }

static bool string_mode(uint32_t mode) { return mode == XSG_LINES || mode == XSG_MATCHES; }  // results are strings
static bool count_mode(uint32_t mode) { return mode == XSG_COUNT_MATCHES || mode == XSG_COUNT_LINES; }
// the tags that report matches; every other tag reports lines (what XSG_FLAG_INVERT and XSG_LIST_ALL_OF are served for)
static bool match_mode(uint32_t mode) { return mode == XSG_COUNT_MATCHES || mode == XSG_MATCH_BYTE_OFFSETS || mode == XSG_MATCHES; }
// the tags whose list context widens (every other tag ignores the bits)
static bool context_mode(uint32_t mode) { return mode == XSG_LINE_BYTE_OFFSETS || mode == XSG_LINE_INDICES || mode == XSG_LINES; }
}  // namespace xsg
