// devbuf_selftest.cpp — stand-alone leak check of the columnar scan's error
// path, serenedb_amd/csrc/hip/sdb_hip_rc.h: sdb_hip_rc, HIP_CHECK and DevBuf.
// Host code only, no GPU and no HIP: hipMalloc / hipFree are the stubs below,
// which fail at the n-th call on request and track every live pointer. Meant
// to be built with sanitizers:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined
//       -fno-sanitize-recover=all tools/devbuf_selftest.cpp -o devbuf_selftest
//   ./devbuf_selftest
//
// Each scenario has the shape of one of the library's callers (three buffers
// and a run of stream calls, as the hash aggregate; one buffer handed to a
// callee with buffers of its own, as the string-key aggregate; a buffer
// inside a loop body, as table load). For every n, the n-th HIP call of the
// scenario fails, with each of three error codes: the scenario must return
// that code's SDB_ERR_*, and every allocation made before the failure must
// have been freed exactly once. Exit 0 and "devbuf_selftest: ok" on success.

#include <cstdio>
#include <cstdlib>
#include <set>

// ---- the names sdb_hip_rc.h takes from HIP ----
enum hipError_t {
  hipSuccess = 0,
  hipErrorOutOfMemory = 2,
  hipErrorNoDevice = 100,
  hipErrorUnknown = 999,
};

static std::set<void*> live;      // allocated and not yet freed
static int calls, fail_at;        // HIP calls so far; which one fails (0 = none)
static hipError_t fail_with;
static int mallocs, frees, bad_frees;

static bool fails_now() { return ++calls == fail_at; }

static hipError_t hipMalloc(void** p, size_t bytes) {
  if (fails_now()) return fail_with;  // a failed hipMalloc leaves *p alone
  *p = std::malloc(bytes ? bytes : 1);
  live.insert(*p);
  ++mallocs;
  return hipSuccess;
}

static hipError_t hipFree(void* p) {
  if (!live.erase(p)) {  // never allocated, or freed before
    ++bad_frees;
    return hipErrorUnknown;
  }
  std::free(p);
  ++frees;
  return hipSuccess;
}

// any other HIP call of a caller: memset, launch check, copy, synchronize
static hipError_t hip_step() { return fails_now() ? fail_with : hipSuccess; }

#include "../serenedb_amd/csrc/hip/sdb_hip_rc.h"

// ---- scenarios ----
static int three_buffers() {  // scan_agg_hash_core
  DevBuf keys, acc, misc;
  HIP_CHECK(keys.alloc(64));
  HIP_CHECK(acc.alloc(128));
  HIP_CHECK(misc.alloc(8));
  for (int i = 0; i < 3; ++i) HIP_CHECK(hip_step());  // memsets
  HIP_CHECK(hip_step());                              // launch check
  for (int i = 0; i < 3; ++i) HIP_CHECK(hip_step());  // copies back
  HIP_CHECK(hip_step());                              // synchronize
  keys.as<unsigned char>()[63] = 1;  // the buffers are still owned here
  return SDB_OK;
}

static int outer_and_callee() {  // sdb_gpu_scan_agg_hash_str
  DevBuf hash;
  HIP_CHECK(hash.alloc(40));
  HIP_CHECK(hip_step());
  return three_buffers();
}

static int buffer_per_trip() {  // sdb_gpu_table_load's min/max reduction
  for (int c = 0; c < 3; ++c) {
    DevBuf mm;
    HIP_CHECK(mm.alloc(16));
    HIP_CHECK(hip_step());
    HIP_CHECK(hip_step());
  }
  return SDB_OK;
}

static int reseeded_workspace() {  // sdb_gpu_scan_agg_hash_multi
  DevBuf ws;
  HIP_CHECK(ws.alloc(256));
  for (int seed = 0; seed < 4; ++seed) {
    for (int i = 0; i < 5; ++i) HIP_CHECK(hip_step());
    if (seed == 1) return SDB_ERR_OOM;  // a return that is no HIP failure
  }
  return SDB_OK;
}

static int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s (n=%d)\n", __FILE__, __LINE__, \
                   #cond, fail_at);                                  \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static void reset(int n, hipError_t e) {
  calls = mallocs = frees = bad_frees = 0;
  fail_at = n;
  fail_with = e;
}

static size_t sweep(int (*scenario)(), int clean_rc) {
  reset(0, hipSuccess);
  CHECK(scenario() == clean_rc);
  const int ncalls = calls;
  CHECK(ncalls > 0 && mallocs > 0 && frees == mallocs);
  CHECK(live.empty() && bad_frees == 0);
  const hipError_t codes[3] = {hipErrorOutOfMemory, hipErrorNoDevice,
                               hipErrorUnknown};
  const int want[3] = {SDB_ERR_OOM, SDB_ERR_NO_GPU, SDB_ERR_HIP};
  size_t runs = 0;
  for (int n = 1; n <= ncalls; ++n)
    for (int k = 0; k < 3; ++k, ++runs) {
      reset(n, codes[k]);
      CHECK(scenario() == want[k]);
      CHECK(calls == n);           // nothing ran after the failure
      CHECK(frees == mallocs);     // each allocation freed ...
      CHECK(bad_frees == 0);       // ... exactly once
      CHECK(live.empty());
    }
  return runs;
}

int main() {
  CHECK(sdb_hip_rc(hipSuccess) == SDB_OK);
  CHECK(sdb_hip_rc(hipErrorNoDevice) == SDB_ERR_NO_GPU);
  CHECK(sdb_hip_rc(hipErrorOutOfMemory) == SDB_ERR_OOM);
  CHECK(sdb_hip_rc(hipErrorUnknown) == SDB_ERR_HIP);
  {  // an empty holder frees nothing
    reset(0, hipSuccess);
    { DevBuf none; }
    CHECK(frees == 0 && bad_frees == 0);
  }
  size_t runs = 0;
  runs += sweep(three_buffers, SDB_OK);
  runs += sweep(outer_and_callee, SDB_OK);
  runs += sweep(buffer_per_trip, SDB_OK);
  runs += sweep(reseeded_workspace, SDB_ERR_OOM);
  std::printf("devbuf_selftest: %zu failing runs\n", runs);
  if (failures) {
    std::fprintf(stderr, "devbuf_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("devbuf_selftest: ok\n");
  return 0;
}
