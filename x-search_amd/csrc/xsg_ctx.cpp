// xsg_ctx.cpp -- the C ABI of include/xsg.h, part 1: errors, trace marks and contexts.  Host glue only; the kernels
// are in the .hip files.  There is no CPU fallback anywhere in the host files of the ABI (this one, xsg_pattern.cpp,
// xsg_shard.cpp, xsg_count.cpp, xsg_list.cpp): every compute entry point needs a HIP device and fails with
// XSG_ENODEV/XSG_EHIP otherwise.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "xsg_host.h"

using namespace xsg;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

namespace xsg {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
const char* last_error_message() { return g_err; }

static const std::chrono::steady_clock::time_point g_loaded = std::chrono::steady_clock::now();
bool test_hooks() {
  static const bool on = [] { const char* e = getenv("XSG_TEST_HOOKS"); return e && *e == '1'; }();
  return on;
}
bool trace_on() {
  static const bool on = [] { const char* e = getenv("XSG_TRACE"); return e && *e && *e != '0'; }();
  return on;
}
void trace(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  const auto now = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(now - g_loaded).count();
  // (the second figure is CLOCK_MONOTONIC in seconds: a launcher that prints the same clock before it starts the
  // process and after it has exited -- scripts/cli_trace.py -- shows what lies before the library is loaded and behind
  // the last mark: the process's start and its teardown)
  fprintf(stderr, "[xsg +%10.3f ms | %.6f] %s\n", ms, std::chrono::duration<double>(now.time_since_epoch()).count(), buf);
}
}  // namespace xsg

extern "C" int xsg_abi_version(void) { return XSG_ABI_VERSION; }

extern "C" const char* xsg_strerror(int code) {
  switch (code) {
    case XSG_OK: return "ok";
    case XSG_EINVAL: return "invalid argument";
    case XSG_ENODEV: return "no usable HIP device";
    case XSG_EHIP: return "HIP runtime error";
    case XSG_ENOMEM: return "out of memory";
    case XSG_ENOTSUP: return "not supported by this entry point";
    case XSG_EIO: return "I/O error";
    case XSG_ESTATE: return "call sequence error";
    default: return "unknown error";
  }
}
extern "C" const char* xsg_last_error(void) { return g_err; }

extern "C" int xsg_device_count(int* count) {
  if (!count) return fail(XSG_EINVAL, "count is null");
  int n = 0;
  XSG_TRACE("hipGetDeviceCount ...");
  hipError_t e = hipGetDeviceCount(&n);
  XSG_TRACE("hipGetDeviceCount -> %d", n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(XSG_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return XSG_OK;
}

extern "C" int xsg_ctx_create(int device, xsg_ctx** out) {
  if (!out) return fail(XSG_EINVAL, "out is null");
  *out = nullptr;
  int n = 0;
  XSG_TRY(xsg_device_count(&n));
  if (n <= 0) return fail(XSG_ENODEV, "no HIP device visible");
  if (device < 0 || device >= n) return fail(XSG_ENODEV, "device %d out of range (0..%d)", device, n - 1);
  HIP_TRY(hipSetDevice(device));
  XSG_TRACE("ctx_create: hipSetDevice(%d) done", device);
  xsg_ctx* c = new (std::nothrow) xsg_ctx();
  if (!c) return fail(XSG_ENOMEM, "host allocation failed");
  c->device = device;
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  XSG_TRACE("ctx_create: device properties");
  if (e != hipSuccess) {
    delete c;
    return fail(XSG_EHIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
  }
  snprintf(c->arch, sizeof c->arch, "%s", prop.gcnArchName);
  c->cus = prop.multiProcessorCount;
  c->hbm = prop.totalGlobalMem;
  if (strncmp(c->arch, "gfx950", 6) != 0) {
    // the code objects in this library are gfx950 only
    std::string a = c->arch;
    delete c;
    return fail(XSG_ENODEV, "device %d is %s; this library carries gfx950 (MI355X) code only", device, a.c_str());
  }
  if (const char* tn = getenv("XSG_TUNE")) c->tune = (uint32_t)strtoul(tn, nullptr, 0);
  if (const char* hf = getenv("XSG_HOT")) c->hot_env = (*hf == '0' || *hf == '1') ? *hf - '0' : -1;
  if (const char* pm = getenv("XSG_PROBE_MIN_BYTES")) c->probe_min_bytes = strtoull(pm, nullptr, 0);
  if (const char* sm = getenv("XSG_SKETCH_MIN_BYTES")) c->sketch_min_bytes = strtoull(sm, nullptr, 0);
  if (const char* tk = getenv("XSG_TILE_KIB")) {
    const int v = atoi(tk);
    if (v == 16) c->tile_bytes = (uint32_t)v * 1024u;
  }
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(XSG_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  XSG_TRACE("ctx_create: stream");
  // The code object of the scan kernels (3.5 MB, ~5 ms the first time in a process) is loaded now rather than inside
  // the first search -- every search launches one of them.  The list kernels' (1.1 ms) and the automaton route's
  // (0.5 ms) are loaded by the first search that needs them: a count of a literal needs neither
  // (profiles/r04_cli_start.txt; XSG_WARM_ALL=1 loads all three here, as round 3 did).
  e = warm_scan_kernels(c->stream);
  XSG_TRACE("ctx_create: scan kernels launched");
  static const bool warm_all = [] { const char* w = getenv("XSG_WARM_ALL"); return w && *w == '1'; }();
  if (warm_all) {
    if (e == hipSuccess) e = warm_list_kernels(c->stream);
    if (e == hipSuccess) e = warm_rx_kernels(c->stream);
    if (e == hipSuccess) e = warm_set_kernels(c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  XSG_TRACE("ctx_create: warm-up synchronised");
  if (e != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    delete c;
    return fail(XSG_EHIP, "loading the kernels failed: %s", hipGetErrorString(e));
  }
  *out = c;
  return XSG_OK;
}

extern "C" void xsg_ctx_destroy(xsg_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  c->d_pat.release();
  c->d_pre.release();
  c->d_fac.release();
  c->d_aux_pat.release();
  delete c;
}

extern "C" int xsg_ctx_info(xsg_ctx* c, char* arch, size_t arch_cap, int* compute_units, uint64_t* hbm_bytes) {
  if (!c) return fail(XSG_EINVAL, "ctx is null");
  if (arch && arch_cap) snprintf(arch, arch_cap, "%s", c->arch);
  if (compute_units) *compute_units = c->cus;
  if (hbm_bytes) *hbm_bytes = c->hbm;
  return XSG_OK;
}
