// sdb_hip_rc.h — the error path of the columnar scan entries (sdb_scan.hip):
// one hipError_t -> SDB_ERR_* mapping, one early-return macro on top of it,
// and the owner of a call's temporary device allocations.
//
// Include after <hip/hip_runtime.h>. The header names hipError_t, its three
// codes below, hipMalloc and hipFree and nothing else of HIP, so
// tools/devbuf_selftest.cpp includes it after host stubs of those names and
// checks on the CPU that every early return frees what it allocated.
#pragma once
#include <cstddef>

#include "../../../include/sdb_gpu.h"

static inline int sdb_hip_rc(hipError_t e) {
  if (e == hipSuccess) return SDB_OK;
  if (e == hipErrorNoDevice) return SDB_ERR_NO_GPU;
  return e == hipErrorOutOfMemory ? SDB_ERR_OOM : SDB_ERR_HIP;
}

#define HIP_CHECK(x)               \
  do {                             \
    const int _rc = sdb_hip_rc(x); \
    if (_rc) return _rc;           \
  } while (0)

// One temporary device allocation, freed when the call returns, however it
// returns. Move-less on purpose: a buffer has one owner for its whole life.
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};
