// Reader head of BertRetrieveQA on the last hidden state: qa_outputs = Linear(hidden, 2) -> start / end logits, the
// paragraph mask, and the best span with 0 <= end - start <= max_answer_len (qa/bert_retrieve_qa.py:58-77,
// qa/train_retrieve_qa.py:300-313), plus select_outputs = Linear(hidden, 1) on the pooled output (--add-select).
//
// The reference forms the whole masked [B, L, L] span-score tensor (1 MB per 512-token passage in fp32).  Here one
// workgroup owns one sequence: its waves stream the sequence's hidden rows once (16-byte loads, one row per wave at a
// time, two rows in flight), form both logits as fp32 dot products + bias rounded to fp16 (the arithmetic of a
// half-precision nn.Linear), keep them in LDS, and then every thread scans the max_answer_len + 1 ends of its starts.
// The kernel's cost is the T x hidden x 2 bytes it reads; the [L, L] matrix never exists.
// reader_span_nbest is the same launch with the first n_best spans of every sequence and the log-sum-exps of its paragraph
// logits (the training objective's Z^s, Z^e), for marginal answer decoding; both come from the logits in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "common.h"
#include "reader_head.h"

namespace proqa {
namespace {

constexpr int kSpanThreads = 512;      // 8 waves per sequence
constexpr int kSpanWaves = kSpanThreads / 64;
constexpr int kMaxChunks = kHeadMaxChunks;   // hidden <= 64 lanes * 2 chunks * 8 = 1024
constexpr int kMaxSpanSeqLen = 4096;   // 2 x 4096 fp32 logits = 32 KiB of LDS
constexpr int kMaxNBest = 32;
constexpr int kEndsInFlight = 4;      // ends of one start the n-best scan reads from LDS before it compares them

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// (score, start, end) order of the span search: higher score first, then lower start (a start owns one end)
__device__ __forceinline__ bool better(float s, int i, float s_other, int i_other) {
  return s > s_other || (s == s_other && i >= 0 && (i_other < 0 || i < i_other));
}

// Rows of sequence b: padded layout (cu_seqlens == null) rows b * seq_len .. + len(b), len(b) = seq_lens[b]; packed layout
// rows cu_seqlens[b] .. cu_seqlens[b + 1].  seq_len caps len (it sizes the LDS).
__device__ __forceinline__ void span_rows(const int* __restrict__ seq_lens, const int* __restrict__ cu_seqlens, int b,
                                          int seq_len, long long& row0, int& len) {
  if (cu_seqlens) {
    row0 = cu_seqlens[b];
    len = cu_seqlens[b + 1] - cu_seqlens[b];
  } else {
    row0 = (long long)b * seq_len;
    len = seq_lens[b];
  }
  len = len < 0 ? 0 : (len > seq_len ? seq_len : len);
}

// phase 1 of both span kernels: the logits of rows row0 .. row0 + len into lg ([0, seq_len): start, [seq_len, 2 seq_len):
// end) and, optionally, logits_out; two rows per wave in flight.  The caller's barrier follows.
__device__ __forceinline__ void span_logits(const _Float16* __restrict__ hidden, long long row0, int len, int seq_len, int hsize,
                                            const _Float16* __restrict__ qa_w, const _Float16* __restrict__ qa_b,
                                            _Float16* __restrict__ logits_out, float* lg) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_chunks = hsize >> 3;

  // the two weight rows stay in registers for the whole sequence
  f16x8 w0[kMaxChunks], w1[kMaxChunks];
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    const int chunk = lane + 64 * c;
    if (chunk < n_chunks) {
      w0[c] = *(const f16x8*)(qa_w + chunk * 8);
      w1[c] = *(const f16x8*)(qa_w + hsize + chunk * 8);
    }
  }
  const float b0 = (float)qa_b[0], b1 = (float)qa_b[1];

  for (int r = wave; r < len; r += 2 * kSpanWaves) {
    const int r2 = r + kSpanWaves;
    const bool two = r2 < len;
    const _Float16* x = hidden + (row0 + r) * hsize;
    const _Float16* y = hidden + (row0 + (two ? r2 : r)) * hsize;
    f16x8 xa[kMaxChunks], ya[kMaxChunks];
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
        xa[c] = *(const f16x8*)(x + chunk * 8);
        ya[c] = *(const f16x8*)(y + chunk * 8);
      }
    }
    // the head's arithmetic lives in reader_head.h (the training objective forms the same bits)
    const DropoutParams no_drop = {};
    float s0, e0, s1, e1;
    head_row_dots<false>(xa, w0, w1, lane, n_chunks, no_drop, 0u, s0, e0);
    head_row_dots<false>(ya, w0, w1, lane, n_chunks, no_drop, 0u, s1, e1);
    const _Float16 hs0 = head_logit(s0, b0), he0 = head_logit(e0, b1);
    const _Float16 hs1 = head_logit(s1, b0), he1 = head_logit(e1, b1);
    if (lane == 0) {
      lg[r] = (float)hs0;
      lg[seq_len + r] = (float)he0;
      if (logits_out) {
        f16x2 o = {hs0, he0};
        *(f16x2*)(logits_out + (row0 + r) * 2) = o;
      }
      if (two) {
        lg[r2] = (float)hs1;
        lg[seq_len + r2] = (float)he1;
        if (logits_out) {
          f16x2 o = {hs1, he1};
          *(f16x2*)(logits_out + (row0 + r2) * 2) = o;
        }
      }
    }
  }
}

// One workgroup per sequence.
__global__ __launch_bounds__(kSpanThreads) void reader_span(const _Float16* __restrict__ hidden, const int* __restrict__ seq_lens,
                                                            const int* __restrict__ cu_seqlens, int seq_len, int hsize,
                                                            const int* __restrict__ para_offset,
                                                            const _Float16* __restrict__ qa_w, const _Float16* __restrict__ qa_b,
                                                            int max_answer_len, int* __restrict__ start_out,
                                                            int* __restrict__ end_out, float* __restrict__ score_out,
                                                            _Float16* __restrict__ logits_out) {
  extern __shared__ float lg[];   // [0, seq_len): start logits, [seq_len, 2 seq_len): end logits
  __shared__ float red_s[kSpanWaves];
  __shared__ int red_i[kSpanWaves], red_j[kSpanWaves];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long row0;
  int len;
  span_rows(seq_lens, cu_seqlens, b, seq_len, row0, len);
  span_logits(hidden, row0, len, seq_len, hsize, qa_w, qa_b, logits_out, lg);
  __syncthreads();

  // phase 2: every start of the paragraph [para_offset, len - 1) against its max_answer_len + 1 ends; a thread walks its
  // starts in increasing order and keeps the first of equal scores, the reductions below keep the lowest start
  int p0 = para_offset[b];
  p0 = p0 < 0 ? 0 : p0;
  const int last = len - 1;   // first position after the paragraph (the final [SEP])
  float best = -INFINITY;
  int bi = -1, bj = -1;
  for (int i = p0 + tid; i < last; i += kSpanThreads) {
    const float s = lg[i];
    const int jmax = min(i + max_answer_len, last - 1);
    float rb = -INFINITY;
    int rj = -1;
    for (int j = i; j <= jmax; ++j) {
      const float v = s + lg[seq_len + j];
      if (v > rb) {
        rb = v;
        rj = j;
      }
    }
    if (rj >= 0 && better(rb, i, best, bi)) {
      best = rb;
      bi = i;
      bj = rj;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float os = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64), oj = __shfl_xor(bj, off, 64);
    if (oi >= 0 && better(os, oi, best, bi)) {
      best = os;
      bi = oi;
      bj = oj;
    }
  }
  if (lane == 0) {
    red_s[wave] = best;
    red_i[wave] = bi;
    red_j[wave] = bj;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSpanWaves; ++w)
      if (red_i[w] >= 0 && better(red_s[w], red_i[w], best, bi)) {
        best = red_s[w];
        bi = red_i[w];
        bj = red_j[w];
      }
    // no paragraph token: no span (the reference would raise IndexError); the host maps it to the answer ""
    start_out[b] = bi;
    end_out[b] = bi >= 0 ? bj : -1;
    score_out[b] = bi >= 0 ? best : -INFINITY;
  }
}

// A candidate (score, i, j) of the n-best search as one 64-bit key whose unsigned order is the search's total order --
// score descending, then start ascending, then end ascending: bits 55..24 the score's bits made monotone (-0 counts as
// +0, as `==` has it in reader_span), bits 23..12 4095 - i, bits 11..0 4095 - j (i, j < kMaxSpanSeqLen = 4096).  A
// candidate's score is above -inf, so its key is above 0, which stands for "no candidate".
__device__ __forceinline__ unsigned long long span_key(float score, int i, int j) {
  unsigned u = __float_as_uint(score);
  u = u == 0x80000000u ? 0u : u;
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((unsigned long long)u << 24) | (unsigned)(((kMaxSpanSeqLen - 1 - i) << 12) | (kMaxSpanSeqLen - 1 - j));
}

// reader_span with the first n_best candidates of every sequence and the two log-sum-exps of its paragraph logits; same
// phase 1.  Round r of phase 3 takes the workgroup's best candidate that comes strictly after round r - 1's winner in the
// total order (every thread rescans the ends of its starts in LDS), so nothing is stored per candidate and no candidate is
// excluded by a list; the order is total, so the result does not depend on which thread or wave held a candidate.
__global__ __launch_bounds__(kSpanThreads) void reader_span_nbest(
    const _Float16* __restrict__ hidden, const int* __restrict__ seq_lens, const int* __restrict__ cu_seqlens, int seq_len,
    int hsize, const int* __restrict__ para_offset, const _Float16* __restrict__ qa_w, const _Float16* __restrict__ qa_b,
    int max_answer_len, int n_best, int* __restrict__ start_out, int* __restrict__ end_out, float* __restrict__ score_out,
    float* __restrict__ lse_out, _Float16* __restrict__ logits_out) {
  extern __shared__ float lg[];   // [0, seq_len): start logits, [seq_len, 2 seq_len): end logits
  __shared__ unsigned long long red_k[2][kSpanWaves];   // by the round's parity: one barrier per round
  __shared__ float red_m[kSpanWaves][2], red_z[kSpanWaves][2];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long row0;
  int len;
  span_rows(seq_lens, cu_seqlens, b, seq_len, row0, len);
  span_logits(hidden, row0, len, seq_len, hsize, qa_w, qa_b, logits_out, lg);
  __syncthreads();

  int p0 = para_offset[b];
  p0 = p0 < 0 ? 0 : p0;
  const int last = len - 1;   // first position after the paragraph (the final [SEP])

  // phase 2: Z^s, Z^e = log-sum-exp of the paragraph's start / end logits, as max-shifted sums in a fixed order: a thread
  // adds its rows in increasing order, the lanes of a wave add by the xor butterfly, thread 0 adds the waves in order
  float ms = -INFINITY, me = -INFINITY;
  for (int i = p0 + tid; i < last; i += kSpanThreads) {
    ms = fmaxf(ms, lg[i]);
    me = fmaxf(me, lg[seq_len + i]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ms = fmaxf(ms, __shfl_xor(ms, off, 64));
    me = fmaxf(me, __shfl_xor(me, off, 64));
  }
  if (lane == 0) {
    red_m[wave][0] = ms;
    red_m[wave][1] = me;
  }
  __syncthreads();
  ms = red_m[0][0];
  me = red_m[0][1];
  for (int w = 1; w < kSpanWaves; ++w) {
    ms = fmaxf(ms, red_m[w][0]);
    me = fmaxf(me, red_m[w][1]);
  }
  // an infinite maximum is not subtracted: all -inf (or empty) sums to 0 -> -inf, a +inf logit sums to +inf -> +inf
  const float shift_s = fabsf(ms) == INFINITY ? 0.f : ms, shift_e = fabsf(me) == INFINITY ? 0.f : me;
  float zs = 0.f, ze = 0.f;
  for (int i = p0 + tid; i < last; i += kSpanThreads) {
    zs += expf(lg[i] - shift_s);
    ze += expf(lg[seq_len + i] - shift_e);
  }
  zs = wave_sum(zs);
  ze = wave_sum(ze);
  if (lane == 0) {
    red_z[wave][0] = zs;
    red_z[wave][1] = ze;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSpanWaves; ++w) {
      zs += red_z[w][0];
      ze += red_z[w][1];
    }
    lse_out[2 * b] = zs > 0.f || zs != zs ? shift_s + logf(zs) : -INFINITY;
    lse_out[2 * b + 1] = ze > 0.f || ze != ze ? shift_e + logf(ze) : -INFINITY;
  }

  // phase 3: n_best rounds over the starts [para_offset, len - 1) and their max_answer_len + 1 ends
  unsigned long long prev = ~0ull;   // above every key
  for (int r = 0; r < n_best; ++r) {
    unsigned long long best = 0;
    for (int i = p0 + tid; i < last; i += kSpanThreads) {
      const float s = lg[i];
      const int jmax = min(i + max_answer_len, last - 1);
      // four ends at a time, so that four LDS reads are in flight (a round is latency, not volume); the clamp keeps the
      // reads of a short tail inside the paragraph and `j <= jmax` drops what it repeats
      for (int j0 = i; j0 <= jmax; j0 += kEndsInFlight) {
        float v[kEndsInFlight];
#pragma unroll
        for (int u = 0; u < kEndsInFlight; ++u) v[u] = s + lg[seq_len + min(j0 + u, jmax)];
#pragma unroll
        for (int u = 0; u < kEndsInFlight; ++u) {
          const int j = j0 + u;
          const unsigned long long k = span_key(v[u], i, j);
          // a candidate is neither -inf nor NaN (fp16 logits that overflowed), as in reader_span
          const bool take = j <= jmax && v[u] > -INFINITY && k < prev && k > best;
          best = take ? k : best;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)best, off, 64), hi = __shfl_xor((unsigned)(best >> 32), off, 64);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      best = o > best ? o : best;
    }
    if (lane == 0) red_k[r & 1][wave] = best;
    __syncthreads();
    best = red_k[r & 1][0];
    for (int w = 1; w < kSpanWaves; ++w) best = red_k[r & 1][w] > best ? red_k[r & 1][w] : best;
    if (best == 0) {
      // fewer than n_best candidates (none at all without a paragraph token): the rest of the row is (-1, -1, -inf)
      for (int q = r + tid; q < n_best; q += kSpanThreads) {
        start_out[(long long)b * n_best + q] = -1;
        end_out[(long long)b * n_best + q] = -1;
        score_out[(long long)b * n_best + q] = -INFINITY;
      }
      break;   // every thread read the same key
    }
    if (tid == 0) {
      const int i = kMaxSpanSeqLen - 1 - (int)((best >> 12) & 4095), j = kMaxSpanSeqLen - 1 - (int)(best & 4095);
      start_out[(long long)b * n_best + r] = i;
      end_out[(long long)b * n_best + r] = j;
      score_out[(long long)b * n_best + r] = lg[i] + lg[seq_len + j];   // the sum itself: its bits, -0 included
    }
    prev = best;
  }
}

// out[b] = fp16(pooled[b] . w + bias) as fp32: select_outputs = Linear(hidden, 1) in half precision, one wave per row
__global__ __launch_bounds__(256) void reader_select(const _Float16* __restrict__ pooled, int batch, int hsize,
                                                     const _Float16* __restrict__ w, const _Float16* __restrict__ bias,
                                                     float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= batch) return;
  const int n_chunks = hsize >> 3;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    const int chunk = lane + 64 * c;
    if (chunk < n_chunks) {
      const f16x8 x = *(const f16x8*)(pooled + (long long)row * hsize + chunk * 8);
      const f16x8 v = *(const f16x8*)(w + chunk * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += (float)x[i] * (float)v[i];
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) out[row] = (float)(_Float16)(acc + (float)bias[0]);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the argument checks of both span entry points, before the device is touched
int span_sizes_ok(int batch, int seq_len, int hidden_size, int max_answer_len) {
  if (batch < 0 || seq_len <= 0 || max_answer_len < 0) return fail(PROQA_EINVAL, "reader_span: bad sizes");
  if (seq_len > kMaxSpanSeqLen) return fail(PROQA_EINVAL, "reader_span: seq_len=%d exceeds %d", seq_len, kMaxSpanSeqLen);
  if (hidden_size <= 0 || hidden_size % 8 || hidden_size > 64 * kMaxChunks * 8)
    return fail(PROQA_EINVAL, "reader_span: hidden=%d must be a multiple of 8 and <= %d", hidden_size, 64 * kMaxChunks * 8);
  return PROQA_OK;
}

int span_pointers_ok(const void* hidden, const void* seq_lens_dev, const void* cu_seqlens_dev, const void* para_offset_dev,
                     const void* qa_w, const void* qa_b, bool outputs, const void* logits_out) {
  if (!hidden || !para_offset_dev || !qa_w || !qa_b || !outputs) return fail(PROQA_EINVAL, "reader_span: NULL argument");
  if ((seq_lens_dev == nullptr) == (cu_seqlens_dev == nullptr))
    return fail(PROQA_EINVAL, "reader_span: exactly one of seq_lens (padded) and cu_seqlens (packed) must be given");
  if (!aligned16(hidden) || !aligned16(qa_w) || (logits_out && ((uintptr_t)logits_out & 3)))
    return fail(PROQA_EINVAL, "reader_span: hidden / qa_w must be 16-byte aligned, logits 4-byte aligned");
  return PROQA_OK;
}

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

int proqa_reader_span_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                          int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w, const void* qa_b,
                          int max_answer_len, int32_t* start_out, int32_t* end_out, float* score_out, void* logits_out,
                          void* stream) {
  if (int rc = span_sizes_ok(batch, seq_len, hidden_size, max_answer_len)) return rc;
  if (batch == 0) return PROQA_OK;
  if (int rc = span_pointers_ok(hidden, seq_lens_dev, cu_seqlens_dev, para_offset_dev, qa_w, qa_b,
                                start_out && end_out && score_out, logits_out))
    return rc;
  const size_t lds = (size_t)2 * seq_len * sizeof(float);
  hipLaunchKernelGGL(reader_span, dim3((unsigned)batch), dim3(kSpanThreads), lds, as_stream(stream), (const _Float16*)hidden,
                     (const int*)seq_lens_dev, (const int*)cu_seqlens_dev, seq_len, hidden_size, (const int*)para_offset_dev,
                     (const _Float16*)qa_w, (const _Float16*)qa_b, max_answer_len, (int*)start_out, (int*)end_out, score_out,
                     (_Float16*)logits_out);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

int proqa_reader_span_nbest_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                                int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w,
                                const void* qa_b, int max_answer_len, int n_best, int32_t* start_out, int32_t* end_out,
                                float* score_out, float* lse_out, void* logits_out, void* stream) {
  if (int rc = span_sizes_ok(batch, seq_len, hidden_size, max_answer_len)) return rc;
  if (n_best < 1 || n_best > kMaxNBest) return fail(PROQA_EINVAL, "reader_span: n_best=%d outside [1, %d]", n_best, kMaxNBest);
  if (batch == 0) return PROQA_OK;
  if (int rc = span_pointers_ok(hidden, seq_lens_dev, cu_seqlens_dev, para_offset_dev, qa_w, qa_b,
                                start_out && end_out && score_out && lse_out, logits_out))
    return rc;
  const size_t lds = (size_t)2 * seq_len * sizeof(float);
  // no span is longer than the sequence: the cap keeps i + max_answer_len inside an int
  const int cap = max_answer_len < seq_len ? max_answer_len : seq_len;
  hipLaunchKernelGGL(reader_span_nbest, dim3((unsigned)batch), dim3(kSpanThreads), lds, as_stream(stream),
                     (const _Float16*)hidden, (const int*)seq_lens_dev, (const int*)cu_seqlens_dev, seq_len, hidden_size,
                     (const int*)para_offset_dev, (const _Float16*)qa_w, (const _Float16*)qa_b, cap, n_best, (int*)start_out,
                     (int*)end_out, score_out, lse_out, (_Float16*)logits_out);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

int proqa_reader_select_f16(const void* pooled, int batch, int hidden_size, const void* select_w, const void* select_b,
                            float* out, void* stream) {
  if (batch < 0 || hidden_size <= 0 || hidden_size % 8 || hidden_size > 64 * kMaxChunks * 8)
    return fail(PROQA_EINVAL, "reader_select: bad sizes");
  if (batch == 0) return PROQA_OK;
  if (!pooled || !select_w || !select_b || !out) return fail(PROQA_EINVAL, "reader_select: NULL argument");
  if (!aligned16(pooled) || !aligned16(select_w)) return fail(PROQA_EINVAL, "reader_select: operands must be 16-byte aligned");
  hipLaunchKernelGGL(reader_select, dim3((unsigned)ceil_div(batch, 4)), dim3(256), 0, as_stream(stream),
                     (const _Float16*)pooled, batch, hidden_size, (const _Float16*)select_w, (const _Float16*)select_b, out);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // extern "C"
