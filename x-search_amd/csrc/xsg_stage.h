// xsg_stage.h -- a chunk in host memory on its way to the device: a pinned block and a device block of one capacity, and the
// one operation on them.  The host-memory seams stage through it (xsg_hostsearch.cpp, xsg_litcount.cpp) with the HIP entry
// points and the one chunk-level call that tests/cpp/device_double.cpp provides, nothing else.  Not installed.
#pragma once
#include "xsg_objects.h"

namespace xsg {
// what a buffer must hold to carry a chunk of `len` bytes: whole 16-byte units, and the margin the scan may read behind them
inline uint64_t staged_bytes(uint64_t len) { return ((len + 15u) & ~(uint64_t)15u) + 256u; }

// Grow-only.  Its owner releases it where its own teardown says so: behind the shard bound to `dev`, ahead of the context.
struct StagedChunk {
  void* pinned = nullptr;
  void* dev = nullptr;
  uint64_t cap = 0;
  void release() {
    if (pinned) (void)hipHostFree(pinned);
    if (dev) (void)hipFree(dev);
    pinned = dev = nullptr;
    cap = 0;
  }
  ~StagedChunk() { release(); }
};

// host -> pinned -> device on `st`, then `shard` holds the one chunk (offset 0, `len` bytes, line base 0) at global_offset.
// The caller knows that nothing in flight still reads the blocks.  No bytes: nothing is copied, the chunk is bound all the same.
inline int stage(StagedChunk& b, int device, hipStream_t st, xsg_shard* shard, const void* data, uint64_t len, uint64_t global_offset) {
  const uint64_t need = staged_bytes(len);
  if (need > b.cap) {
    b.release();
    const uint64_t cap = std::max<uint64_t>(need, 1u << 20);
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipHostMalloc(&b.pinned, cap, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&b.dev, cap));
    b.cap = cap;
  }
  if (len) {
    memcpy(b.pinned, data, len);
    HIP_TRY(hipMemcpyAsync(b.dev, b.pinned, len, hipMemcpyHostToDevice, st));
  }
  const xsg_chunk ch{0, len, global_offset, 0};  // offset, length, global_offset, line_base
  return xsg_shard_rebind(shard, b.dev, b.cap, &ch, 1);
}
}  // namespace xsg
