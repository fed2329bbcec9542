// The optimizer step of retriever training (retrieval/train_retriever.py:207-214: amp unscale, clip_grad_norm_, AdamW.step,
// scheduler-driven learning rates) as three launches over ALL parameter tensors at once:
//   adamw_grad_sumsq  one workgroup per fixed chunk of one tensor -> one fp32 partial per chunk (no atomics)
//   adamw_finalize    one workgroup: norm, overflow flag, clip coefficient, step counter, bias corrections, loss scale
//   adamw_update      the same chunks: g, p, m, v read once, p, m, v written once
//   adamw_update_half the same, and every p written is also written as fp16 to the tensor's working copy (2 more bytes)
//   adamw_cast_half   p -> the working copies alone, over the same chunk map (construction, load_state_dict)
// The kernels are bound by HBM (32 bytes per parameter); the arithmetic is a dozen fp32 operations per element with
// correctly rounded sqrt and division (hipcc's default for HIP).
#include <cmath>

#include "common.h"

namespace proqa {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = PROQA_ADAMW_CHUNK;     // elements of one tensor per workgroup; a multiple of 4 * kThreads
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is a whole number of float4 rounds of the workgroup");

// caller-owned device scalars (PROQA_ADAMW_STATE_BYTES; the offsets are part of the ABI, see proqa_hip.h)
struct AdamwState {
  long long step;          //  0  optimizer steps taken (skipped ones not counted)
  long long skipped;       //  8  steps skipped because the gradient norm was not finite
  long long clean_steps;   // 16  steps since the loss scale last changed (dynamic scale)
  float loss_scale;        // 24
  float last_norm;         // 28  unscaled global gradient norm of the last step (what clip_grad_norm_ returns)
  int found_inf;           // 32  1 when the last step was skipped
  float factor;            // 36  inv_scale * clip: what every gradient element is multiplied by
  double bc1;              // 40  1 - beta1^step
  double bc2;              // 48  1 - beta2^step
  float clip;              // 56  clip coefficient of the last step (exactly 1 when nothing was clipped)
  int reserved;            // 60
};
static_assert(sizeof(AdamwState) == PROQA_ADAMW_STATE_BYTES, "state layout is part of the ABI");
static_assert(sizeof(proqa_adamw_tensor) == 56 && sizeof(proqa_adamw_chunk) == 8, "table layouts are part of the ABI");

__device__ __forceinline__ float block_sum(float x, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = x;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += lds[w];
  }
  return s;   // valid in thread 0
}

// partial[chunk] = sum over the chunk of (g * inv_scale)^2, in a fixed order: thread-strided, wave64 shuffles, four wave
// sums through LDS.  A tensor without a gradient contributes 0.
__global__ __launch_bounds__(kThreads) void adamw_grad_sumsq(const proqa_adamw_tensor* __restrict__ table,
                                                             const proqa_adamw_chunk* __restrict__ chunks,
                                                             const AdamwState* __restrict__ state,
                                                             float* __restrict__ partial) {
  __shared__ float lds[kThreads / 64];
  const proqa_adamw_chunk ck = chunks[blockIdx.x];
  const proqa_adamw_tensor t = table[ck.tensor];
  const float* __restrict__ g = static_cast<const float*>(t.g);
  float acc = 0.f;
  if (g != nullptr) {
    const float inv_scale = 1.0f / state->loss_scale;
    const long long start = (long long)ck.index * kChunk;
    const int n = (int)(t.n - start < kChunk ? t.n - start : kChunk);
    g += start;
    if ((reinterpret_cast<uintptr_t>(t.g) & 15) == 0) {
      const int n4 = n >> 2;
      const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 4
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        const float4 x = g4[i];
        const float a = x.x * inv_scale, b = x.y * inv_scale, c = x.z * inv_scale, d = x.w * inv_scale;
        acc += (a * a + b * b) + (c * c + d * d);
      }
      for (int i = (n4 << 2) + threadIdx.x; i < n; i += kThreads) {
        const float a = g[i] * inv_scale;
        acc += a * a;
      }
    } else {
      for (int i = threadIdx.x; i < n; i += kThreads) {
        const float a = g[i] * inv_scale;
        acc += a * a;
      }
    }
  }
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

struct FinalizeArgs {
  long long n_chunks;
  double beta1, beta2;
  float max_grad_norm;     // <= 0: no clipping
  int scale_mode;          // PROQA_ADAMW_SCALE_*
  float backoff_factor, growth_factor;
  int growth_interval;
};

// The partials are added in ascending chunk order in double: thread t owns the t-th contiguous run of chunks, thread 0
// then adds the 256 run sums in ascending order.  One fixed association, whatever the hardware does.
__global__ __launch_bounds__(kThreads) void adamw_finalize(const float* __restrict__ partial, AdamwState* __restrict__ state,
                                                           FinalizeArgs a) {
  __shared__ double run[kThreads];
  const long long per = (a.n_chunks + kThreads - 1) / kThreads;
  const long long lo = per * threadIdx.x;
  const long long hi = lo + per < a.n_chunks ? lo + per : a.n_chunks;
  double s = 0.0;
  for (long long i = lo; i < hi; ++i) s += (double)partial[i];
  run[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < kThreads; ++i) total += run[i];
  const double norm = sqrt(total);
  const bool bad = !(norm <= 1.7976931348623157e308);     // inf or NaN
  const float scale = state->loss_scale;
  double clip = 1.0;
  if (a.max_grad_norm > 0.f) {
    clip = (double)a.max_grad_norm / (norm + 1e-6);        // torch.nn.utils.clip_grad_norm_
    if (!(clip < 1.0)) clip = 1.0;
  }
  state->last_norm = (float)norm;
  state->found_inf = bad ? 1 : 0;
  state->clip = (float)clip;
  // with clip == 1 this is the correctly rounded 1 / scale, the factor adamw_grad_sumsq used
  state->factor = (float)((1.0 / (double)scale) * clip);
  if (bad) {
    state->skipped += 1;
    if (a.scale_mode == PROQA_ADAMW_SCALE_DYNAMIC) {
      state->loss_scale = scale * a.backoff_factor;
      state->clean_steps = 0;
    }
    return;
  }
  const long long t = state->step + 1;
  state->step = t;
  state->bc1 = 1.0 - pow(a.beta1, (double)t);
  state->bc2 = 1.0 - pow(a.beta2, (double)t);
  if (a.scale_mode == PROQA_ADAMW_SCALE_DYNAMIC) {
    const long long clean = state->clean_steps + 1;
    if (clean >= a.growth_interval) {
      state->loss_scale = scale * a.growth_factor;
      state->clean_steps = 0;
    } else {
      state->clean_steps = clean;
    }
  }
}

struct UpdateArgs {
  float beta1, beta2;          // the double hyper-parameters rounded once, as torch rounds a Python scalar
  float one_minus_beta1, one_minus_beta2;
  float eps;
  int torch_semantics;
  // without device state (no clipping, no loss scale): the bias corrections of the host-counted step
  double bc1, bc2;
};

struct ElementCoefs {
  float factor, b1, omb1, b2, omb2, eps;
  float step_size;     // reference: lr * sqrt(bc2) / bc1;  torch: lr / bc1
  float decay;         // reference: lr * wd (p -= decay * p, after);  torch: 1 - lr * wd (p *= decay, before)
  float sqrt_bc2;      // torch: sqrt(v) / sqrt(bc2) + eps
};

template <bool kTorch>
__device__ __forceinline__ void adamw_element(float g, float& p, float& m, float& v, const ElementCoefs& c) {
  g *= c.factor;
  m = c.b1 * m + c.omb1 * g;
  v = c.b2 * v + c.omb2 * (g * g);
  if (kTorch) {
    p *= c.decay;
    p -= c.step_size * (m / (sqrtf(v) / c.sqrt_bc2 + c.eps));
  } else {
    p -= c.step_size * (m / (sqrtf(v) + c.eps));
    p -= c.decay * p;
  }
}

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

template <bool kTorch>
__device__ __forceinline__ void adamw_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int n, bool vec, const ElementCoefs& c) {
  int done = 0;
  if (vec) {
    const int n4 = n >> 2;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
#pragma unroll 2
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const float4 gg = g4[i];
      float4 pp = p4[i], mm = m4[i], vv = v4[i];
      adamw_element<kTorch>(gg.x, pp.x, mm.x, vv.x, c);
      adamw_element<kTorch>(gg.y, pp.y, mm.y, vv.y, c);
      adamw_element<kTorch>(gg.z, pp.z, mm.z, vv.z, c);
      adamw_element<kTorch>(gg.w, pp.w, mm.w, vv.w, c);
      p4[i] = pp;
      m4[i] = mm;
      v4[i] = vv;
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += kThreads) {
    float pp = p[i], mm = m[i], vv = v[i];
    adamw_element<kTorch>(g[i], pp, mm, vv, c);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

// h[i] = (fp16) p[i] over one chunk: round to nearest even, beyond +-65504 -> +-inf (v_cvt_f16_f32 in the default mode,
// what p.to(float16) does).  Thread-strided exactly as adamw_chunk, so that in the update a thread converts the elements
// it has just written itself (its own stores: no barrier), still in the cache.  With p 16-byte and h 8-byte aligned a
// lane packs four results into one 8-byte store; any other pair takes the scalar loop.
__device__ __forceinline__ void cast_chunk(const float* p, _Float16* __restrict__ h, int n, bool vec) {
  int done = 0;
  if (vec) {
    const int n4 = n >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p);
    half4* __restrict__ h4 = reinterpret_cast<half4*>(h);
#pragma unroll 4
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const float4 pp = p4[i];
      half4 hh;
      hh.x = (_Float16)pp.x;
      hh.y = (_Float16)pp.y;
      hh.z = (_Float16)pp.z;
      hh.w = (_Float16)pp.w;
      h4[i] = hh;
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += kThreads) h[i] = (_Float16)p[i];
}

// state == nullptr: no skip rule, factor 1, bias corrections from the arguments.  kHalf: half_table[t] (or NULL) is the
// fp16 working copy of tensor t; a tensor without one runs exactly the code of the kHalf = false instantiation.
template <bool kHalf>
__device__ __forceinline__ void adamw_update_body(const proqa_adamw_tensor* __restrict__ table,
                                                  const proqa_adamw_chunk* __restrict__ chunks,
                                                  const AdamwState* __restrict__ state, UpdateArgs a,
                                                  void* const* __restrict__ half_table) {
  double bc1 = a.bc1, bc2 = a.bc2;
  float factor = 1.0f;
  if (state != nullptr) {
    if (state->found_inf) return;
    bc1 = state->bc1;
    bc2 = state->bc2;
    factor = state->factor;
  }
  const proqa_adamw_chunk ck = chunks[blockIdx.x];
  const proqa_adamw_tensor t = table[ck.tensor];
  if (t.g == nullptr) return;       // `if p.grad is None: continue`: p, m and v stay as they are
  ElementCoefs c;
  c.factor = factor;
  c.b1 = a.beta1;
  c.omb1 = a.one_minus_beta1;
  c.b2 = a.beta2;
  c.omb2 = a.one_minus_beta2;
  c.eps = a.eps;
  c.sqrt_bc2 = (float)sqrt(bc2);
  if (a.torch_semantics) {
    c.step_size = (float)(t.lr / bc1);
    c.decay = (float)(1.0 - t.lr * t.weight_decay);
  } else {
    c.step_size = (float)(t.lr * sqrt(bc2) / bc1);
    c.decay = (float)(t.lr * t.weight_decay);
  }
  const long long start = (long long)ck.index * kChunk;
  const int n = (int)(t.n - start < kChunk ? t.n - start : kChunk);
  const bool vec = ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                     reinterpret_cast<uintptr_t>(t.v)) & 15) == 0;
  float* p = static_cast<float*>(t.p) + start;
  const float* g = static_cast<const float*>(t.g) + start;
  float* m = static_cast<float*>(t.m) + start;
  float* v = static_cast<float*>(t.v) + start;
  // the loops of p, g, m, v are the same code with and without copies, chosen by THEIR alignment alone: the compiler
  // contracts the 16-byte loop and the scalar loop differently, and a tensor keeps the bits proqa_adamw_step gives it
  if (a.torch_semantics)
    adamw_chunk<true>(p, g, m, v, n, vec, c);
  else
    adamw_chunk<false>(p, g, m, v, n, vec, c);
  if (kHalf) {
    _Float16* h = static_cast<_Float16*>(half_table[ck.tensor]);
    if (h == nullptr) return;
    // vec: a thread reads back the float4s it wrote; otherwise the scalars it wrote, or (p 16-byte aligned, the copy not
    // 8-byte aligned) scalars of the float4s and of the tail that other threads wrote: those wait for the workgroup
    const bool hvec = vec && (reinterpret_cast<uintptr_t>(h) & 7) == 0;
    if (vec && !hvec) __syncthreads();
    cast_chunk(p, h + start, n, hvec);       // (kChunk keeps the alignment of the tensor's start)
  }
}

__global__ __launch_bounds__(kThreads) void adamw_update(const proqa_adamw_tensor* __restrict__ table,
                                                         const proqa_adamw_chunk* __restrict__ chunks,
                                                         const AdamwState* __restrict__ state, UpdateArgs a) {
  adamw_update_body<false>(table, chunks, state, a, nullptr);
}

__global__ __launch_bounds__(kThreads) void adamw_update_half(const proqa_adamw_tensor* __restrict__ table,
                                                              const proqa_adamw_chunk* __restrict__ chunks,
                                                              const AdamwState* __restrict__ state, UpdateArgs a,
                                                              void* const* __restrict__ half_table) {
  adamw_update_body<true>(table, chunks, state, a, half_table);
}

// half_table[t][i] = (fp16) p[i] over the same chunk map; a tensor without a copy is left alone
__global__ __launch_bounds__(kThreads) void adamw_cast_half(const proqa_adamw_tensor* __restrict__ table,
                                                            const proqa_adamw_chunk* __restrict__ chunks,
                                                            void* const* __restrict__ half_table) {
  const proqa_adamw_chunk ck = chunks[blockIdx.x];
  _Float16* h = static_cast<_Float16*>(half_table[ck.tensor]);
  if (h == nullptr) return;
  const proqa_adamw_tensor t = table[ck.tensor];
  const long long start = (long long)ck.index * kChunk;
  const int n = (int)(t.n - start < kChunk ? t.n - start : kChunk);
  const bool vec = (reinterpret_cast<uintptr_t>(t.p) & 15) == 0 && (reinterpret_cast<uintptr_t>(h) & 7) == 0;
  cast_chunk(static_cast<const float*>(t.p) + start, h + start, n, vec);
}

__global__ void adamw_state_init(AdamwState* state, long long step, float loss_scale, long long clean_steps,
                                 long long skipped) {
  AdamwState s = {};
  s.step = step;
  s.skipped = skipped;
  s.clean_steps = clean_steps;
  s.loss_scale = loss_scale;
  s.factor = 1.0f / loss_scale;
  s.bc1 = 1.0;
  s.bc2 = 1.0;
  s.clip = 1.0f;
  *state = s;
}

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

int64_t proqa_adamw_chunk_map(const int64_t* sizes, int n_tensors, proqa_adamw_chunk* out, int64_t capacity) {
  if (n_tensors < 0) return fail(PROQA_EINVAL, "adamw_chunk_map: negative tensor count");
  if (n_tensors > 0 && !sizes) return fail(PROQA_EINVAL, "adamw_chunk_map: NULL sizes");
  int64_t n = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes[t] < 0) return fail(PROQA_EINVAL, "adamw_chunk_map: tensor %d has a negative size", t);
    const int64_t here = ceil_div<int64_t>(sizes[t], kChunk);
    if (here > INT32_MAX || n + here > INT32_MAX) return fail(PROQA_EINVAL, "adamw_chunk_map: too many chunks");
    if (out) {
      if (n + here > capacity) return fail(PROQA_EINVAL, "adamw_chunk_map: output holds %lld chunks, more are needed", (long long)capacity);
      for (int64_t i = 0; i < here; ++i) out[n + i] = proqa_adamw_chunk{t, (int32_t)i};
    }
    n += here;
  }
  return n;
}

size_t proqa_adamw_workspace_bytes(int64_t n_chunks) {
  return n_chunks > 0 ? round_up<size_t>((size_t)n_chunks * sizeof(float), 16) : 16;
}

int proqa_adamw_state_init(void* state_dev, int64_t step, float loss_scale, int64_t clean_steps, int64_t skipped_steps,
                           void* stream) {
  if (!state_dev) return fail(PROQA_EINVAL, "adamw_state_init: NULL state");
  if (step < 0 || clean_steps < 0 || skipped_steps < 0) return fail(PROQA_EINVAL, "adamw_state_init: negative counter");
  if (!(loss_scale > 0.f) || std::isinf(loss_scale))
    return fail(PROQA_EINVAL, "adamw_state_init: loss scale %g must be positive and finite", (double)loss_scale);
  hipLaunchKernelGGL(adamw_state_init, dim3(1), dim3(1), 0, as_stream(stream), (AdamwState*)state_dev, (long long)step,
                     loss_scale, (long long)clean_steps, (long long)skipped_steps);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

static int adamw_step_impl(const proqa_adamw_tensor* table_dev, void* const* half_dev, int n_tensors,
                           const proqa_adamw_chunk* chunks_dev, int64_t n_chunks, const proqa_adamw_hyper* hyper, void* state_dev,
                           void* ws, size_t ws_bytes, void* stream) {
  if (n_tensors < 0 || n_chunks < 0 || n_chunks > INT32_MAX)
    return fail(PROQA_EINVAL, "adamw_step: n_tensors=%d n_chunks=%lld", n_tensors, (long long)n_chunks);
  if (!hyper) return fail(PROQA_EINVAL, "adamw_step: NULL hyper-parameters");
  if (!table_dev || (n_chunks > 0 && !chunks_dev)) return fail(PROQA_EINVAL, "adamw_step: NULL tensor table or chunk map");
  if (n_chunks > 0 && n_tensors == 0) return fail(PROQA_EINVAL, "adamw_step: chunks without tensors");
  const proqa_adamw_hyper& h = *hyper;
  if (!(h.beta1 >= 0.0 && h.beta1 < 1.0) || !(h.beta2 >= 0.0 && h.beta2 < 1.0))
    return fail(PROQA_EINVAL, "adamw_step: betas (%g, %g) must lie in [0, 1)", h.beta1, h.beta2);
  if (!(h.eps >= 0.0)) return fail(PROQA_EINVAL, "adamw_step: eps %g must not be negative", h.eps);
  if (h.scale_mode < PROQA_ADAMW_SCALE_NONE || h.scale_mode > PROQA_ADAMW_SCALE_DYNAMIC)
    return fail(PROQA_EINVAL, "adamw_step: scale_mode %d", h.scale_mode);
  if (std::isnan(h.max_grad_norm)) return fail(PROQA_EINVAL, "adamw_step: max_grad_norm is NaN");
  if (h.scale_mode == PROQA_ADAMW_SCALE_DYNAMIC &&
      (!(h.backoff_factor > 0.f && h.backoff_factor < 1.f) || !(h.growth_factor >= 1.f) || std::isinf(h.growth_factor) ||
       h.growth_interval < 1))
    return fail(PROQA_EINVAL, "adamw_step: dynamic scale needs 0 < backoff < 1 <= growth and growth_interval >= 1");
  const bool plain = !(h.max_grad_norm > 0.f) && h.scale_mode == PROQA_ADAMW_SCALE_NONE;
  if (plain && h.host_step < 1) return fail(PROQA_EINVAL, "adamw_step: without clipping and loss scale host_step must be >= 1");
  if (!plain && !state_dev) return fail(PROQA_EINVAL, "adamw_step: NULL state");
  if (!plain && (!ws || ws_bytes < proqa_adamw_workspace_bytes(n_chunks)))
    return fail(PROQA_EINVAL, "adamw_step: workspace too small");
  hipStream_t st = as_stream(stream);
  const AdamwState* state = plain ? nullptr : (const AdamwState*)state_dev;
  if (!plain) {
    if (n_chunks > 0) {
      hipLaunchKernelGGL(adamw_grad_sumsq, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, table_dev, chunks_dev, state,
                         (float*)ws);
      PROQA_LAUNCH_CHECK();
    }
    FinalizeArgs fa;
    fa.n_chunks = n_chunks;
    fa.beta1 = h.beta1;
    fa.beta2 = h.beta2;
    fa.max_grad_norm = h.max_grad_norm;
    fa.scale_mode = h.scale_mode;
    fa.backoff_factor = h.backoff_factor;
    fa.growth_factor = h.growth_factor;
    fa.growth_interval = h.growth_interval;
    hipLaunchKernelGGL(adamw_finalize, dim3(1), dim3(kThreads), 0, st, (const float*)ws, (AdamwState*)state_dev, fa);
    PROQA_LAUNCH_CHECK();
  }
  if (n_chunks == 0) return PROQA_OK;
  UpdateArgs ua;
  ua.beta1 = (float)h.beta1;
  ua.beta2 = (float)h.beta2;
  ua.one_minus_beta1 = (float)(1.0 - h.beta1);
  ua.one_minus_beta2 = (float)(1.0 - h.beta2);
  ua.eps = (float)h.eps;
  ua.torch_semantics = h.torch_semantics ? 1 : 0;
  ua.bc1 = plain ? 1.0 - std::pow(h.beta1, (double)h.host_step) : 1.0;
  ua.bc2 = plain ? 1.0 - std::pow(h.beta2, (double)h.host_step) : 1.0;
  if (half_dev)
    hipLaunchKernelGGL(adamw_update_half, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, table_dev, chunks_dev, state, ua,
                       half_dev);
  else
    hipLaunchKernelGGL(adamw_update, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, table_dev, chunks_dev, state, ua);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

int proqa_adamw_step(const proqa_adamw_tensor* table_dev, int n_tensors, const proqa_adamw_chunk* chunks_dev, int64_t n_chunks,
                     const proqa_adamw_hyper* hyper, void* state_dev, void* ws, size_t ws_bytes, void* stream) {
  return adamw_step_impl(table_dev, nullptr, n_tensors, chunks_dev, n_chunks, hyper, state_dev, ws, ws_bytes, stream);
}

int proqa_adamw_step_half(const proqa_adamw_tensor* table_dev, void* const* half_dev, int n_tensors,
                          const proqa_adamw_chunk* chunks_dev, int64_t n_chunks, const proqa_adamw_hyper* hyper, void* state_dev,
                          void* ws, size_t ws_bytes, void* stream) {
  return adamw_step_impl(table_dev, half_dev, n_tensors, chunks_dev, n_chunks, hyper, state_dev, ws, ws_bytes, stream);
}

int proqa_cast_half_tensors(const proqa_adamw_tensor* table_dev, void* const* half_dev, int n_tensors,
                            const proqa_adamw_chunk* chunks_dev, int64_t n_chunks, void* stream) {
  if (n_tensors < 0 || n_chunks < 0 || n_chunks > INT32_MAX)
    return fail(PROQA_EINVAL, "cast_half_tensors: n_tensors=%d n_chunks=%lld", n_tensors, (long long)n_chunks);
  if (!table_dev || !half_dev || (n_chunks > 0 && !chunks_dev))
    return fail(PROQA_EINVAL, "cast_half_tensors: NULL tensor table, copy table or chunk map");
  if (n_chunks > 0 && n_tensors == 0) return fail(PROQA_EINVAL, "cast_half_tensors: chunks without tensors");
  if (n_chunks == 0) return PROQA_OK;
  hipLaunchKernelGGL(adamw_cast_half, dim3((unsigned)n_chunks), dim3(kThreads), 0, as_stream(stream), table_dev, chunks_dev,
                     half_dev);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // extern "C"
