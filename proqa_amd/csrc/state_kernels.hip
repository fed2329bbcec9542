// Trainer-state snapshot (proqa_state_snapshot, include/proqa_hip.h): every fp32 tensor of the optimizer (masters, exp_avg,
// exp_avg_sq) is read once, written to a flat buffer and folded into one 64-bit digest per tensor, in two launches whatever
// the number of tensors:
//   state_copy_digest   one workgroup per fixed chunk of one tensor: copy, and one uint64 partial per chunk (no atomics)
//   state_digest_finish one wave per tensor adds that tensor's partials
// The pass is bound by HBM (4 bytes read, 4 written per element); the digest costs one xor, one index update and one
// 32 x 32 + 64 -> 64 bit multiply-add per element.
#include "common.h"

namespace proqa {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = PROQA_STATE_CHUNK;     // elements of one tensor per workgroup; a multiple of 4 * kThreads
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is a whole number of float4 rounds of the workgroup");
static_assert(sizeof(proqa_state_tensor) == 32 && sizeof(proqa_state_chunk) == 8, "plan layouts are part of the ABI");

constexpr int64_t kMaxNumel = (int64_t)1 << 31;     // 2 i + 1 of every index fits 32 bits: one v_mad_u64_u32 per element

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

// mix(bits, i) = (bits ^ PROQA_STATE_MIX_XOR) * (2 i + 1) mod 2^64; i < 2^31, so both factors fit 32 bits
__device__ __forceinline__ unsigned long long mix(unsigned int bits, unsigned int i) {
  return (unsigned long long)(bits ^ PROQA_STATE_MIX_XOR) * (unsigned long long)(2u * i + 1u);
}

// sum over the workgroup, valid in thread 0: wave64 shuffles, the four wave sums through LDS (integer: any order gives the
// same bits; the order is fixed all the same)
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long x, unsigned long long* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = x;
  __syncthreads();
  unsigned long long s = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += lds[w];
  }
  return s;
}

// One chunk: elements [start, start + n) of tensor t.  The source is only 4-byte aligned: `head` scalar elements up to the
// first 16-byte boundary, 16-byte loads over the body, scalar loads over the tail.  The destination of a tensor starts on
// a 256-byte boundary and a chunk is 64 KiB, so the body's stores are 16-byte aligned exactly when head == 0; a shifted
// body (a source that is a row slice of a flat buffer) is stored as four dwords.
template <bool kCopy>
__global__ __launch_bounds__(kThreads) void state_copy_digest(const void* const* __restrict__ src, const proqa_state_tensor* __restrict__ tensors,
                                                              const proqa_state_chunk* __restrict__ chunks,
                                                              unsigned char* __restrict__ dst_flat,
                                                              unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long lds[kThreads / 64];
  const proqa_state_chunk ck = chunks[blockIdx.x];
  const proqa_state_tensor t = tensors[ck.tensor];
  const long long start = (long long)ck.index * kChunk;
  const int n = (int)(t.numel - start < kChunk ? t.numel - start : kChunk);
  const unsigned int* __restrict__ s = static_cast<const unsigned int*>(src[ck.tensor]) + start;
  unsigned int* __restrict__ d = nullptr;
  if (kCopy) d = reinterpret_cast<unsigned int*>(dst_flat + t.dst_offset) + start;
  const unsigned int base = (unsigned int)start;      // index of the chunk's first element inside its tensor (< 2^31)

  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(s) & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int n4 = (n - head) >> 2;
  const int tail0 = head + (n4 << 2);

  unsigned long long acc = 0;
  if ((int)threadIdx.x < head) {
    const unsigned int x = s[threadIdx.x];
    if (kCopy) d[threadIdx.x] = x;
    acc += mix(x, base + threadIdx.x);
  }
  const uint4v* __restrict__ s4 = reinterpret_cast<const uint4v*>(s + head);
  if (head == 0) {
    uint4v* __restrict__ d4 = reinterpret_cast<uint4v*>(d);
#pragma unroll 4
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const uint4v x = s4[i];
      if (kCopy) d4[i] = x;
      const unsigned int e = base + 4u * i;
      acc += mix(x.x, e);
      acc += mix(x.y, e + 1);
      acc += mix(x.z, e + 2);
      acc += mix(x.w, e + 3);
    }
  } else {
#pragma unroll 2
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const uint4v x = s4[i];
      const int o = head + 4 * i;
      if (kCopy) {
        d[o] = x.x;
        d[o + 1] = x.y;
        d[o + 2] = x.z;
        d[o + 3] = x.w;
      }
      const unsigned int e = base + (unsigned int)o;
      acc += mix(x.x, e);
      acc += mix(x.y, e + 1);
      acc += mix(x.z, e + 2);
      acc += mix(x.w, e + 3);
    }
  }
  const int i_tail = tail0 + (int)threadIdx.x;      // at most 3 elements
  if (i_tail < n) {
    const unsigned int x = s[i_tail];
    if (kCopy) d[i_tail] = x;
    acc += mix(x, base + i_tail);
  }
  acc = block_sum_u64(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// digests[t] = sum of tensor t's partials: one wave per tensor, lane-strided in ascending chunk order, then the shuffles.
// A tensor without elements has no chunk: 0.
__global__ __launch_bounds__(kThreads) void state_digest_finish(const proqa_state_tensor* __restrict__ tensors, int n_tensors,
                                                                const unsigned long long* __restrict__ partial,
                                                                unsigned long long* __restrict__ digests) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= n_tensors) return;      // whole waves leave; no barrier follows
  const long long first = tensors[t].first_chunk, count = tensors[t].n_chunks;
  unsigned long long acc = 0;
  for (long long i = lane; i < count; i += 64) acc += partial[first + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) digests[t] = acc;
}

// validates the sizes and counts the chunks; negative on error
int64_t count_chunks(const char* who, const int64_t* numel, int n_tensors) {
  if (n_tensors < 0) return fail(PROQA_EINVAL, "%s: negative tensor count", who);
  if (n_tensors > 0 && !numel) return fail(PROQA_EINVAL, "%s: NULL numel", who);
  int64_t n = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (numel[t] < 0) return fail(PROQA_EINVAL, "%s: tensor %d has a negative size", who, t);
    if (numel[t] > kMaxNumel)
      return fail(PROQA_EINVAL, "%s: tensor %d has %lld elements, more than 2^31", who, t, (long long)numel[t]);
    n += ceil_div<int64_t>(numel[t], kChunk);
    if (n > INT32_MAX) return fail(PROQA_EINVAL, "%s: too many chunks", who);
  }
  return n;
}

size_t plan_bytes_of(int n_tensors, int64_t n_chunks) {
  const size_t b = (size_t)n_tensors * sizeof(proqa_state_tensor) + (size_t)n_chunks * sizeof(proqa_state_chunk);
  return b > 0 ? round_up<size_t>(b, 16) : 16;
}

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

size_t proqa_state_snapshot_plan_bytes(const int64_t* numel, int n_tensors) {
  const int64_t n_chunks = count_chunks("state_snapshot_plan_bytes", numel, n_tensors);
  return n_chunks < 0 ? 0 : plan_bytes_of(n_tensors, n_chunks);
}

size_t proqa_state_snapshot_workspace_bytes(const int64_t* numel, int n_tensors) {
  const int64_t n_chunks = count_chunks("state_snapshot_workspace_bytes", numel, n_tensors);
  if (n_chunks < 0) return 0;
  return plan_bytes_of(n_tensors, n_chunks) + (n_chunks > 0 ? (size_t)n_chunks * sizeof(uint64_t) : 16);
}

int proqa_state_snapshot_plan(const int64_t* numel, const int64_t* dst_offsets, int n_tensors, void* plan_host,
                              size_t plan_bytes) {
  const int64_t n_chunks = count_chunks("state_snapshot_plan", numel, n_tensors);
  if (n_chunks < 0) return (int)n_chunks;
  if (!plan_host || plan_bytes < plan_bytes_of(n_tensors, n_chunks))
    return fail(PROQA_EINVAL, "state_snapshot_plan: the plan needs %zu bytes", plan_bytes_of(n_tensors, n_chunks));
  proqa_state_tensor* tensors = static_cast<proqa_state_tensor*>(plan_host);
  proqa_state_chunk* chunks = reinterpret_cast<proqa_state_chunk*>(tensors + n_tensors);
  int64_t c = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const int64_t off = dst_offsets ? dst_offsets[t] : 0;
    if (off < 0 || off % PROQA_STATE_DST_ALIGN != 0)
      return fail(PROQA_EINVAL, "state_snapshot_plan: destination offset %lld of tensor %d is not a multiple of %d",
                  (long long)off, t, PROQA_STATE_DST_ALIGN);
    const int64_t here = ceil_div<int64_t>(numel[t], kChunk);
    tensors[t] = proqa_state_tensor{numel[t], off, c, here};
    for (int64_t i = 0; i < here; ++i) chunks[c + i] = proqa_state_chunk{t, (int32_t)i};
    c += here;
  }
  return PROQA_OK;
}

int proqa_state_snapshot(const void* const* src_dev_ptrs, const int64_t* numel, int n_tensors, void* dst_flat_dev,
                         const int64_t* dst_offsets, uint64_t* digests_dev, void* ws, size_t ws_bytes, void* stream) {
  const int64_t n_chunks = count_chunks("state_snapshot", numel, n_tensors);
  if (n_chunks < 0) return (int)n_chunks;
  if (n_tensors == 0) return PROQA_OK;
  if (!src_dev_ptrs || !digests_dev) return fail(PROQA_EINVAL, "state_snapshot: NULL source table or digests");
  if (dst_flat_dev) {
    if (!dst_offsets) return fail(PROQA_EINVAL, "state_snapshot: a destination without offsets");
    if (reinterpret_cast<uintptr_t>(dst_flat_dev) % PROQA_STATE_DST_ALIGN != 0)
      return fail(PROQA_EINVAL, "state_snapshot: the destination is not %d-byte aligned", PROQA_STATE_DST_ALIGN);
    for (int t = 0; t < n_tensors; ++t)
      if (dst_offsets[t] < 0 || dst_offsets[t] % PROQA_STATE_DST_ALIGN != 0)
        return fail(PROQA_EINVAL, "state_snapshot: destination offset %lld of tensor %d is not a multiple of %d",
                    (long long)dst_offsets[t], t, PROQA_STATE_DST_ALIGN);
  }
  const size_t plan = plan_bytes_of(n_tensors, n_chunks);
  if (!ws || reinterpret_cast<uintptr_t>(ws) % 16 != 0 || ws_bytes < plan + (n_chunks > 0 ? (size_t)n_chunks * sizeof(uint64_t) : 16))
    return fail(PROQA_EINVAL, "state_snapshot: workspace missing, not 16-byte aligned or too small");
  const proqa_state_tensor* tensors = static_cast<const proqa_state_tensor*>(ws);
  const proqa_state_chunk* chunks = reinterpret_cast<const proqa_state_chunk*>(tensors + n_tensors);
  unsigned long long* partial = reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(ws) + plan);
  hipStream_t st = as_stream(stream);
  if (n_chunks > 0) {
    if (dst_flat_dev)
      hipLaunchKernelGGL(state_copy_digest<true>, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, src_dev_ptrs, tensors, chunks,
                         static_cast<unsigned char*>(dst_flat_dev), partial);
    else
      hipLaunchKernelGGL(state_copy_digest<false>, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, src_dev_ptrs, tensors, chunks,
                         static_cast<unsigned char*>(nullptr), partial);
    PROQA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(state_digest_finish, dim3((unsigned)ceil_div(n_tensors, kThreads / 64)), dim3(kThreads), 0, st, tensors,
                     n_tensors, partial, reinterpret_cast<unsigned long long*>(digests_dev));
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // extern "C"
