// Shared host-side helpers for libproqa_hip.so (error plumbing, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/proqa_hip.h"

namespace proqa {

// thread-local last-error message, surfaced through proqa_last_error()
char* error_buffer();
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// one line on stderr ("[proqa] ...") when the environment variable PROQA_LOG is set to anything but "" / "0": decisions the
// library takes on its own (which scan a search ran on, a suspended / resumed int8 copy); silent otherwise
bool log_enabled();
void log_line(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

inline int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  return fail(PROQA_EHIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}

#define PROQA_HIP(call)                                                          \
  do {                                                                           \
    hipError_t _e = (call);                                                      \
    if (_e != hipSuccess) return ::proqa::hip_fail(_e, #call, __FILE__, __LINE__); \
  } while (0)

#define PROQA_LAUNCH_CHECK()                                                              \
  do {                                                                                    \
    hipError_t _e = hipGetLastError();                                                    \
    if (_e != hipSuccess) return ::proqa::hip_fail(_e, "kernel launch", __FILE__, __LINE__); \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Makes `want` the current HIP device for the lifetime of the guard and restores the caller's device afterwards: a
// handle that lives on another GPU than the caller's current one must not change the device under the caller (its
// later allocations and stream look-ups would land on the wrong GPU).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int want) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != want) {
      err = hipSetDevice(want);
      switched = err == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define PROQA_ON_DEVICE(dev)                   \
  ::proqa::DeviceGuard _device_guard(dev);     \
  PROQA_HIP(_device_guard.err)

// hipMalloc whose failure is an expected, recoverable condition (the caller falls back or reports PROQA_ENOMEM): HIP's
// last-error slot is sticky until read, so it is cleared here -- otherwise the next launch wrapper's hipGetLastError()
// would report this allocation failure as its own.
inline hipError_t try_malloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}

// An allocation that is grown on demand and never shrinks: the pointer, its capacity and its release live here and
// nowhere else.  Device memory, or pinned host memory when `pinned_host` is set.  Growing keeps nothing of the contents.
struct GrowBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  bool pinned_host = false;
  // At least `want` bytes (exactly `want` when it has to grow).  `wait_on`: work enqueued on that stream may still use
  // the old allocation -- it is waited for before the allocation goes.  On failure the buffer is left empty.
  hipError_t grow(size_t want, const hipStream_t* wait_on = nullptr) {
    if (want <= bytes) return hipSuccess;
    if (wait_on)
      if (hipError_t e = hipStreamSynchronize(*wait_on)) return e;
    if (hipError_t e = release()) return e;
    hipError_t e = pinned_host ? hipHostMalloc(&ptr, want, hipHostMallocDefault) : try_malloc(&ptr, want);
    if (e != hipSuccess) {
      if (pinned_host) (void)hipGetLastError();   // (as try_malloc)
      ptr = nullptr;
      return e;
    }
    bytes = want;
    return hipSuccess;
  }
  hipError_t release() {
    void* p = ptr;
    ptr = nullptr;
    bytes = 0;
    if (!p) return hipSuccess;
    return pinned_host ? hipHostFree(p) : hipFree(p);
  }
};

template <typename T>
inline T ceil_div(T a, T b) {
  return (a + b - 1) / b;
}
template <typename T>
inline T round_up(T a, T b) {
  return ceil_div(a, b) * b;
}

// The row blocks of the block-diagonal in-batch objective (proqa_inbatch_loss_blocks_f16 and its gradient): block m owns
// the rows [o[m], o[m + 1]) of q AND of c.  The offsets travel by value in the kernel arguments: no device copy.
struct BlockOffsets {
  int o[PROQA_INBATCH_MAX_BLOCKS + 1];
};
// The geometry both entry points refuse, before the device is touched; on success `offs` holds the offsets and `widest`
// the rows of the largest block.
inline int check_inbatch_blocks(const char* who, const int32_t* block_offsets, int n_blocks, int n, int dim, BlockOffsets* offs,
                                int* widest) {
  if (dim != PROQA_EMBED_DIM) return fail(PROQA_EINVAL, "%s: dim=%d, only %d is supported", who, dim, PROQA_EMBED_DIM);
  if (n_blocks < 1 || n_blocks > PROQA_INBATCH_MAX_BLOCKS)
    return fail(PROQA_EINVAL, "%s: n_blocks=%d must be in [1, %d]", who, n_blocks, PROQA_INBATCH_MAX_BLOCKS);
  if (n < n_blocks || n > (1 << 24)) return fail(PROQA_EINVAL, "%s: n=%d rows for %d blocks (at most 2^24 rows)", who, n, n_blocks);
  if (!block_offsets) return fail(PROQA_EINVAL, "%s: NULL block_offsets", who);
  if (block_offsets[0] != 0 || block_offsets[n_blocks] != n)
    return fail(PROQA_EINVAL, "%s: block_offsets must run from 0 to n=%d (they run from %d to %d)", who, n, block_offsets[0],
                block_offsets[n_blocks]);
  *offs = BlockOffsets{};
  *widest = 0;
  for (int m = 0; m < n_blocks; ++m) {
    const int rows = block_offsets[m + 1] - block_offsets[m];
    if (rows < 1 || block_offsets[m + 1] > n)
      return fail(PROQA_EINVAL, "%s: block %d is [%d, %d): every block needs at least one row inside [0, n]", who, m,
                  block_offsets[m], block_offsets[m + 1]);
    offs->o[m + 1] = block_offsets[m + 1];
    if (rows > *widest) *widest = rows;
  }
  return PROQA_OK;
}

// number of compute units of the current device (256 on MI355X); cached
int device_cu_count();

#if defined(__HIPCC__)
// Barrier that publishes LDS-DMA'd data.  `global_load_lds` completion is tracked by vmcnt only, and
// hipcc does NOT reliably drain vmcnt at __syncthreads() (observed: `s_waitcnt lgkmcnt(0); s_barrier`
// inside a loop), so a stage could be read before its DMA had landed -- rare, data-dependent garbage.
// Every barrier that makes a DMA'd LDS stage readable goes through this.
__device__ __forceinline__ void dma_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
#endif

}  // namespace proqa
