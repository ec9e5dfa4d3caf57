// xsg_meta.h -- what the job pipeline (xsg_job.cpp) needs from xsg_meta.cpp: the chunk plan of a plain file, the metafile
// reader, the codecs of compressed chunks, and the guard that keeps C++ exceptions behind the C ABI.  Not installed.
#pragma once
#include <exception>
#include <new>
#include <vector>

#include "xsg_objects.h"

namespace xsg {
// No C++ exception may cross the C ABI: host-side containers sized from file contents can throw.
template <typename F>
static int guarded(const char* what, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(XSG_ENOMEM, "%s: host allocation failed", what);
  } catch (const std::exception& e) {
    return fail(XSG_EIO, "%s: %s", what, e.what());
  }
}

int plan_plain(int fd, uint64_t size, uint64_t target, std::vector<xsg_file_chunk>& out);
int read_meta(const char* path, int32_t* compression, std::vector<xsg_file_chunk>& chunks, std::vector<uint64_t>* mappings);
int need_lz4();  // the codec of a compression type, loaded on first use
int need_zstd();
int decompress_chunk(int32_t type, const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n);
}  // namespace xsg
