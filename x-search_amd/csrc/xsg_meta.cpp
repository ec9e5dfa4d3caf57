// xsg_meta.cpp -- the files of a search before a device is involved: the chunk plan of a plain file (xsg_plan_chunks), the
// metafile reader and writer (xsg_meta_read, xsg_meta_write: the preprocessor) and the LZ4 / ZSTD codecs of compressed
// chunks, loaded on demand.  Plain host code: no HIP call in here.  The job pipeline (xsg_job.cpp) takes what it needs
// through xsg_meta.h.
#include <dlfcn.h>

#include <mutex>

#include "xsg_fileio.h"
#include "xsg_lz4.h"
#include "xsg_meta.h"

using namespace xsg;

extern "C" void xsg_free(void* p) { free(p); }

// ---------------------------------------------------------------------------
// chunk plan of a plain file: >= target bytes, extended to just past the next '\n'
// (the layout of the reference's fixtures: SURVEY 5.1)
// ---------------------------------------------------------------------------
int xsg::plan_plain(int fd, uint64_t size, uint64_t target, std::vector<xsg_file_chunk>& out) {
  if (target < 1) target = 1;
  uint64_t pos = 0;
  std::vector<uint8_t> probe(1 << 16);
  while (pos < size) {
    uint64_t end = pos + target;
    if (end >= size) {
      end = size;
    } else {
      // first '\n' at or after end-1
      uint64_t q = end - 1;
      bool found = false;
      while (q < size) {
        const uint64_t n = std::min<uint64_t>(probe.size(), size - q);
        XSG_TRY(pread_full(fd, probe.data(), n, q));
        const void* hit = memchr(probe.data(), '\n', n);
        if (hit) {
          end = q + (uint64_t)((const uint8_t*)hit - probe.data()) + 1;
          found = true;
          break;
        }
        q += n;
      }
      if (!found) end = size;
    }
    xsg_file_chunk c{};
    c.original_offset = pos;
    c.actual_offset = pos;
    c.original_size = end - pos;
    c.actual_size = end - pos;
    c.first_line = XSG_LINE_BASE_AUTO;
    c.n_mappings = 0;
    out.push_back(c);
    pos = end;
  }
  return XSG_OK;
}

static int to_malloc(const std::vector<xsg_file_chunk>& v, xsg_file_chunk** chunks, uint64_t* n) {
  *n = v.size();
  *chunks = static_cast<xsg_file_chunk*>(malloc(sizeof(xsg_file_chunk) * std::max<size_t>(v.size(), 1)));
  if (!*chunks) return fail(XSG_ENOMEM, "host allocation failed");
  if (!v.empty()) memcpy(*chunks, v.data(), sizeof(xsg_file_chunk) * v.size());
  return XSG_OK;
}

extern "C" int xsg_plan_chunks(const char* file_path, uint64_t target_bytes, xsg_file_chunk** chunks, uint64_t* n) {
  if (!chunks || !n) return fail(XSG_EINVAL, "null output");
  int fd;
  uint64_t size;
  XSG_TRY(open_ro(file_path, &fd, &size));
  return guarded("xsg_plan_chunks", [&]() -> int {
    std::vector<xsg_file_chunk> v;
    int r;
    try {
      r = plan_plain(fd, size, target_bytes ? target_bytes : (16u << 20), v);
    } catch (...) {
      close(fd);
      throw;
    }
    close(fd);
    if (r != XSG_OK) return r;
    return to_malloc(v, chunks, n);
  });
}

// ---------------------------------------------------------------------------
// metafile (little-endian, packed):
//   int32 compression_type, then per chunk
//   u64 original_offset, actual_offset, original_size, actual_size, n, n x {u64 byte offset, u64 line index}
// ---------------------------------------------------------------------------
int xsg::read_meta(const char* path, int32_t* compression, std::vector<xsg_file_chunk>& chunks,
                   std::vector<uint64_t>* mappings) {
  // The mapping tables are ~3 % of the corpus size (one entry per >= 500 bytes): a
  // search only needs the 40-byte record headers and each chunk's first entry, so
  // the file is walked with small preads and the tables are read only on request.
  int fd;
  uint64_t size;
  XSG_TRY(open_ro(path, &fd, &size));
  struct Closer {
    int fd;
    ~Closer() { close(fd); }
  } closer{fd};
  if (size < 4) return fail(XSG_EIO, "metafile '%s' is too short", path);
  int32_t ct;
  XSG_TRY(pread_full(fd, &ct, 4, 0));
  if (ct != XSG_COMPRESSION_NONE && ct != XSG_COMPRESSION_ZSTD && ct != XSG_COMPRESSION_LZ4)
    return fail(XSG_EIO, "metafile '%s': unknown compression type %d", path, ct);
  *compression = ct;
  uint64_t pos = 4;
  uint64_t expect_orig = 0;
  while (pos < size) {
    if (size - pos < 40) return fail(XSG_EIO, "metafile '%s': truncated chunk record at byte %llu", path,
                                     (unsigned long long)pos);
    uint64_t f[7] = {0, 0, 0, 0, 0, 0, 0};  // 5 header words + the first mapping entry
    const uint64_t want = std::min<uint64_t>(56, size - pos);
    XSG_TRY(pread_full(fd, f, want, pos));
    pos += 40;
    const uint64_t n = f[4];
    if (n > (size - pos) / 16) return fail(XSG_EIO, "metafile '%s': mapping table of chunk %zu overruns the file", path,
                                           chunks.size());
    xsg_file_chunk c{};
    c.original_offset = f[0];
    c.actual_offset = f[1];
    c.original_size = f[2];
    c.actual_size = f[3];
    c.n_mappings = n;
    c.first_line = XSG_LINE_BASE_AUTO;
    if (c.original_offset != expect_orig)
      return fail(XSG_EIO, "metafile '%s': chunk %zu does not start where its predecessor ends", path, chunks.size());
    if (c.original_size >= (1ull << 40) || c.actual_size >= (1ull << 40))
      return fail(XSG_EIO, "metafile '%s': chunk %zu has an implausible size", path, chunks.size());
    expect_orig += c.original_size;  // < 2^40 each and at most size/40 records: no wrap
    if (n) {
      // the first mapping entry of a chunk is the chunk start
      if (f[5] == c.original_offset) c.first_line = f[6];
      if (mappings) {
        const size_t at = mappings->size();
        mappings->resize(at + 2 * n);
        XSG_TRY(pread_full(fd, mappings->data() + at, 16 * n, pos));
      }
    }
    pos += 16 * n;
    chunks.push_back(c);
  }
  return XSG_OK;
}

extern "C" int xsg_meta_read(const char* meta_path, int32_t* compression, xsg_file_chunk** chunks, uint64_t* n,
                             uint64_t** mappings, uint64_t* n_mapping_pairs) {
  if (!compression || !chunks || !n) return fail(XSG_EINVAL, "null output");
  return guarded("xsg_meta_read", [&]() -> int {
    std::vector<xsg_file_chunk> v;
    std::vector<uint64_t> maps;
    XSG_TRY(read_meta(meta_path, compression, v, mappings ? &maps : nullptr));
    XSG_TRY(to_malloc(v, chunks, n));
    if (mappings) {
      *mappings = static_cast<uint64_t*>(malloc(8 * std::max<size_t>(maps.size(), 1)));
      if (!*mappings) return fail(XSG_ENOMEM, "host allocation failed");
      if (!maps.empty()) memcpy(*mappings, maps.data(), 8 * maps.size());
      if (n_mapping_pairs) *n_mapping_pairs = maps.size() / 2;
    }
    return XSG_OK;
  });
}

// ---------------------------------------------------------------------------
// LZ4 / ZSTD through the system libraries (the reference links liblz4 / libzstd,
// Dockerfile:8).  Loaded on demand so that plain-text searches need neither.
// ---------------------------------------------------------------------------
struct Codecs {
  void* lz4 = nullptr;
  void* zstd = nullptr;
  int (*LZ4_decompress_safe)(const char*, char*, int, int) = nullptr;
  int (*LZ4_compress_default)(const char*, char*, int, int) = nullptr;
  int (*LZ4_compress_HC)(const char*, char*, int, int, int) = nullptr;
  int (*LZ4_compressBound)(int) = nullptr;
  size_t (*ZSTD_decompress)(void*, size_t, const void*, size_t) = nullptr;
  size_t (*ZSTD_compress)(void*, size_t, const void*, size_t, int) = nullptr;
  size_t (*ZSTD_compressBound)(size_t) = nullptr;
  unsigned (*ZSTD_isError)(size_t) = nullptr;
};

static Codecs& codecs() {
  static Codecs c;
  return c;
}
static std::mutex g_codec_mu;

static void* open_any(const char* const* names) {
  for (; *names; ++names) {
    void* h = dlopen(*names, RTLD_NOW | RTLD_LOCAL);
    if (h) return h;
  }
  return nullptr;
}

// the built-in block codec (xsg_lz4.h) behind liblz4's signatures
static int builtin_lz4_decompress_safe(const char* src, char* dst, int src_n, int dst_cap) {
  if (src_n < 0 || dst_cap < 0) return -1;
  const int64_t r = xsg::lz4_block_decode((const uint8_t*)src, (size_t)src_n, (uint8_t*)dst, (size_t)dst_cap);
  return r < 0 ? -1 : (int)r;
}
static int builtin_lz4_compress_default(const char* src, char* dst, int src_n, int dst_cap) {
  return xsg::lz4_block_encode((const uint8_t*)src, src_n, (uint8_t*)dst, dst_cap);
}
static int builtin_lz4_compress_bound(int n) { return xsg::lz4_compress_bound(n); }
static char g_builtin_lz4_token;  // non-null marker for Codecs::lz4 when the built-in codec is in use

// liblz4 if the host has one, else the built-in codec (XSG_NO_LIBLZ4=1 forces the built-in one: tests)
int xsg::need_lz4() {
  std::lock_guard<std::mutex> g(g_codec_mu);
  Codecs& c = codecs();
  if (c.lz4) return XSG_OK;
  static const char* names[] = {"liblz4.so.1", "liblz4.so", "/opt/conda/lib/liblz4.so.1", nullptr};
  const char* no = getenv("XSG_NO_LIBLZ4");
  void* h = (no && *no && *no != '0') ? nullptr : open_any(names);
  if (h) {
    c.LZ4_decompress_safe = (int (*)(const char*, char*, int, int))dlsym(h, "LZ4_decompress_safe");
    c.LZ4_compress_default = (int (*)(const char*, char*, int, int))dlsym(h, "LZ4_compress_default");
    c.LZ4_compress_HC = (int (*)(const char*, char*, int, int, int))dlsym(h, "LZ4_compress_HC");
    c.LZ4_compressBound = (int (*)(int))dlsym(h, "LZ4_compressBound");
    if (c.LZ4_decompress_safe && c.LZ4_compress_default && c.LZ4_compressBound) {
      c.lz4 = h;
      return XSG_OK;
    }
  }
  c.LZ4_decompress_safe = builtin_lz4_decompress_safe;
  c.LZ4_compress_default = builtin_lz4_compress_default;
  c.LZ4_compress_HC = nullptr;
  c.LZ4_compressBound = builtin_lz4_compress_bound;
  c.lz4 = &g_builtin_lz4_token;
  return XSG_OK;
}

int xsg::need_zstd() {
  std::lock_guard<std::mutex> g(g_codec_mu);
  Codecs& c = codecs();
  if (c.zstd) return XSG_OK;
  static const char* names[] = {"libzstd.so.1", "libzstd.so", "/opt/conda/lib/libzstd.so.1", nullptr};
  void* h = open_any(names);
  if (!h) return fail(XSG_ENOTSUP, "libzstd not found on this host (needed for ZSTD metafiles)");
  c.ZSTD_decompress = (size_t(*)(void*, size_t, const void*, size_t))dlsym(h, "ZSTD_decompress");
  c.ZSTD_compress = (size_t(*)(void*, size_t, const void*, size_t, int))dlsym(h, "ZSTD_compress");
  c.ZSTD_compressBound = (size_t(*)(size_t))dlsym(h, "ZSTD_compressBound");
  c.ZSTD_isError = (unsigned (*)(size_t))dlsym(h, "ZSTD_isError");
  if (!c.ZSTD_decompress || !c.ZSTD_compress || !c.ZSTD_compressBound || !c.ZSTD_isError)
    return fail(XSG_ENOTSUP, "libzstd lacks the expected symbols");
  c.zstd = h;
  return XSG_OK;
}

extern "C" const char* xsg_codec_name(int32_t compression) {
  if (compression == XSG_COMPRESSION_NONE) return "none";
  if (compression == XSG_COMPRESSION_LZ4) {
    if (need_lz4() != XSG_OK) return "";
    return codecs().lz4 == &g_builtin_lz4_token ? "built-in LZ4 block codec" : "liblz4";
  }
  if (compression == XSG_COMPRESSION_ZSTD) return need_zstd() == XSG_OK ? "libzstd" : "";
  return "";
}

int xsg::decompress_chunk(int32_t type, const uint8_t* src, uint64_t src_n, uint8_t* dst, uint64_t dst_n) {
  if (type == XSG_COMPRESSION_LZ4) {
    // raw LZ4 block per chunk, decoded to exactly original_size bytes
    if (src_n > INT32_MAX || dst_n > INT32_MAX) return fail(XSG_EIO, "LZ4 chunk too large");
    const int r = codecs().LZ4_decompress_safe((const char*)src, (char*)dst, (int)src_n, (int)dst_n);
    if (r < 0 || (uint64_t)r != dst_n) return fail(XSG_EIO, "LZ4 chunk does not decode to its recorded size");
    return XSG_OK;
  }
  if (type == XSG_COMPRESSION_ZSTD) {
    const size_t r = codecs().ZSTD_decompress(dst, dst_n, src, src_n);
    if (codecs().ZSTD_isError(r) || r != dst_n) return fail(XSG_EIO, "ZSTD chunk does not decode to its recorded size");
    return XSG_OK;
  }
  return fail(XSG_EINVAL, "bad compression type %d", type);
}

// ---------------------------------------------------------------------------
// metafile writer / preprocessor
// ---------------------------------------------------------------------------
static int meta_write_impl(const char* file_path, const char* meta_out_path, const char* data_out_path,
                           int32_t compression, uint64_t chunk_bytes, uint64_t mapping_gap, int hc) {
  if (!meta_out_path) return fail(XSG_EINVAL, "meta_out_path is null");
  if (compression != XSG_COMPRESSION_NONE && compression != XSG_COMPRESSION_ZSTD && compression != XSG_COMPRESSION_LZ4)
    return fail(XSG_EINVAL, "bad compression type %d", compression);
  if (compression != XSG_COMPRESSION_NONE && !data_out_path) return fail(XSG_EINVAL, "data_out_path is null");
  if (compression == XSG_COMPRESSION_LZ4) XSG_TRY(need_lz4());
  if (compression == XSG_COMPRESSION_ZSTD) XSG_TRY(need_zstd());
  if (!chunk_bytes) chunk_bytes = 16u << 20;
  if (!mapping_gap) mapping_gap = 500;
  int fd;
  uint64_t size;
  XSG_TRY(open_ro(file_path, &fd, &size));
  std::vector<xsg_file_chunk> plan;
  int r = plan_plain(fd, size, chunk_bytes, plan);
  if (r != XSG_OK) {
    close(fd);
    return r;
  }
  FILE* mf = fopen(meta_out_path, "wb");
  FILE* df = compression != XSG_COMPRESSION_NONE ? fopen(data_out_path, "wb") : nullptr;
  if (!mf || (compression != XSG_COMPRESSION_NONE && !df)) {
    if (mf) fclose(mf);
    if (df) fclose(df);
    close(fd);
    return fail(XSG_EIO, "cannot create output files: %s", strerror(errno));
  }
  fwrite(&compression, 4, 1, mf);
  std::vector<uint8_t> raw, packed;
  std::vector<uint64_t> maps;
  uint64_t line = 0, actual_off = 0;
  for (const xsg_file_chunk& pc : plan) {
    raw.resize(pc.original_size);
    r = pread_full(fd, raw.data(), pc.original_size, pc.original_offset);
    if (r != XSG_OK) break;
    // mapping: the chunk start, then the first line start >= previous entry + gap
    maps.clear();
    maps.push_back(pc.original_offset);
    maps.push_back(line);
    uint64_t last_entry = 0;
    for (uint64_t i = 0; i < pc.original_size; ++i) {
      if (raw[i] == '\n') {
        ++line;
        const uint64_t ls = i + 1;
        if (ls < pc.original_size && ls >= last_entry + mapping_gap) {
          maps.push_back(pc.original_offset + ls);
          maps.push_back(line);
          last_entry = ls;
        }
      }
    }
    uint64_t actual_size = pc.original_size;
    if (compression == XSG_COMPRESSION_LZ4) {
      if (pc.original_size > INT32_MAX) {
        r = fail(XSG_EINVAL, "chunk too large for an LZ4 block");
        break;
      }
      packed.resize((size_t)codecs().LZ4_compressBound((int)pc.original_size));
      const int n = hc && codecs().LZ4_compress_HC
                        ? codecs().LZ4_compress_HC((const char*)raw.data(), (char*)packed.data(), (int)raw.size(),
                                                   (int)packed.size(), 9)
                        : codecs().LZ4_compress_default((const char*)raw.data(), (char*)packed.data(), (int)raw.size(),
                                                        (int)packed.size());
      if (n <= 0 && pc.original_size) {
        r = fail(XSG_EIO, "LZ4 compression failed");
        break;
      }
      actual_size = (uint64_t)n;
    } else if (compression == XSG_COMPRESSION_ZSTD) {
      packed.resize(codecs().ZSTD_compressBound(raw.size()));
      const size_t n = codecs().ZSTD_compress(packed.data(), packed.size(), raw.data(), raw.size(), 3);
      if (codecs().ZSTD_isError(n)) {
        r = fail(XSG_EIO, "ZSTD compression failed");
        break;
      }
      actual_size = n;
    }
    if (df && actual_size && fwrite(packed.data(), 1, actual_size, df) != actual_size) {
      r = fail(XSG_EIO, "short write to '%s'", data_out_path);
      break;
    }
    const uint64_t rec[5] = {pc.original_offset, compression == XSG_COMPRESSION_NONE ? pc.original_offset : actual_off,
                             pc.original_size, actual_size, maps.size() / 2};
    fwrite(rec, 8, 5, mf);
    fwrite(maps.data(), 8, maps.size(), mf);
    actual_off += actual_size;
  }
  if (fclose(mf) != 0 && r == XSG_OK) r = fail(XSG_EIO, "cannot write '%s'", meta_out_path);
  if (df && fclose(df) != 0 && r == XSG_OK) r = fail(XSG_EIO, "cannot write '%s'", data_out_path);
  close(fd);
  return r;
}

extern "C" int xsg_meta_write(const char* file_path, const char* meta_out_path, const char* data_out_path,
                              int32_t compression, uint64_t chunk_bytes, uint64_t mapping_gap, int hc) {
  return guarded("xsg_meta_write", [&]() -> int {
    return meta_write_impl(file_path, meta_out_path, data_out_path, compression, chunk_bytes, mapping_gap, hc);
  });
}
