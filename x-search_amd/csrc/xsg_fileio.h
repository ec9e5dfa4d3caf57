// xsg_fileio.h -- the file helpers shared by the host pipelines (xsg_meta.cpp, xsg_job.cpp: one file per job; xsg_fileset.cpp: a list
// of files per set): open a regular file read-only, read exactly n bytes, and the CPUs the process may use.  Not installed.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "xsg_objects.h"

namespace {
using xsg::fail;

static int pread_full(int fd, void* buf, uint64_t n, uint64_t off) {
  uint8_t* p = static_cast<uint8_t*>(buf);
  while (n) {
    const ssize_t r = pread(fd, p, n > (1u << 30) ? (1u << 30) : n, (off_t)off);
    if (r < 0) {
      if (errno == EINTR) continue;
      return fail(XSG_EIO, "pread failed: %s", strerror(errno));
    }
    if (r == 0) return fail(XSG_EIO, "unexpected end of file at offset %llu", (unsigned long long)off);
    p += r;
    off += (uint64_t)r;
    n -= (uint64_t)r;
  }
  return XSG_OK;
}

static int open_ro(const char* path, int* fd, uint64_t* size) {
  if (!path || !*path) return fail(XSG_EINVAL, "empty file path");
  const int f = open(path, O_RDONLY | O_CLOEXEC);
  if (f < 0) return fail(XSG_EIO, "cannot open '%s': %s", path, strerror(errno));
  struct stat st;
  if (fstat(f, &st) != 0) {
    close(f);
    return fail(XSG_EIO, "cannot stat '%s': %s", path, strerror(errno));
  }
  if (!S_ISREG(st.st_mode)) {
    close(f);
    return fail(XSG_EIO, "'%s' is not a regular file", path);
  }
  *fd = f;
  *size = (uint64_t)st.st_size;
  return XSG_OK;
}

// CPUs this process may use: its affinity mask, capped by the cgroup's CPU quota (cpu.max)
static int cpu_budget() {
  int n = 1;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::max(1, CPU_COUNT(&set));
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = "";
    long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
      const long long quota = atoll(q);
      if (quota > 0) n = (int)std::min<long long>(n, std::max<long long>(1, quota / period));
    }
    fclose(f);
  }
  return n;
}
}  // namespace
