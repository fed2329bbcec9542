// Reader head of BertRetrieveQA on the last hidden state: qa_outputs = Linear(hidden, 2) -> start / end logits, the
// paragraph mask, and the best span with 0 <= end - start <= max_answer_len (qa/bert_retrieve_qa.py:58-77,
// qa/train_retrieve_qa.py:300-313), plus select_outputs = Linear(hidden, 1) on the pooled output (--add-select).
//
// The reference forms the whole masked [B, L, L] span-score tensor (1 MB per 512-token passage in fp32).  Here one
// workgroup owns one sequence: its waves stream the sequence's hidden rows once (16-byte loads, one row per wave at a
// time, two rows in flight), form both logits as fp32 dot products + bias rounded to fp16 (the arithmetic of a
// half-precision nn.Linear), keep them in LDS, and then every thread scans the max_answer_len + 1 ends of its starts.
// The kernel's cost is the T x hidden x 2 bytes it reads; the [L, L] matrix never exists.
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

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// (score, start, end) order of the span search: higher score first, then lower start (a start owns one end)
__device__ __forceinline__ bool better(float s, int i, float s_other, int i_other) {
  return s > s_other || (s == s_other && i >= 0 && (i_other < 0 || i < i_other));
}

// One workgroup per sequence.  Rows of sequence b: padded layout (cu_seqlens == null) rows b * seq_len .. + len(b),
// len(b) = seq_lens[b]; packed layout rows cu_seqlens[b] .. cu_seqlens[b + 1].  seq_len caps len (it sizes the LDS).
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
  if (cu_seqlens) {
    row0 = cu_seqlens[b];
    len = cu_seqlens[b + 1] - cu_seqlens[b];
  } else {
    row0 = (long long)b * seq_len;
    len = seq_lens[b];
  }
  len = len < 0 ? 0 : (len > seq_len ? seq_len : len);
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

  // phase 1: logits, two rows per wave in flight
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

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

int proqa_reader_span_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                          int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w, const void* qa_b,
                          int max_answer_len, int32_t* start_out, int32_t* end_out, float* score_out, void* logits_out,
                          void* stream) {
  if (batch < 0 || seq_len <= 0 || max_answer_len < 0) return fail(PROQA_EINVAL, "reader_span: bad sizes");
  if (seq_len > kMaxSpanSeqLen) return fail(PROQA_EINVAL, "reader_span: seq_len=%d exceeds %d", seq_len, kMaxSpanSeqLen);
  if (hidden_size <= 0 || hidden_size % 8 || hidden_size > 64 * kMaxChunks * 8)
    return fail(PROQA_EINVAL, "reader_span: hidden=%d must be a multiple of 8 and <= %d", hidden_size, 64 * kMaxChunks * 8);
  if (batch == 0) return PROQA_OK;
  if (!hidden || !para_offset_dev || !qa_w || !qa_b || !start_out || !end_out || !score_out)
    return fail(PROQA_EINVAL, "reader_span: NULL argument");
  if ((seq_lens_dev == nullptr) == (cu_seqlens_dev == nullptr))
    return fail(PROQA_EINVAL, "reader_span: exactly one of seq_lens (padded) and cu_seqlens (packed) must be given");
  if (!aligned16(hidden) || !aligned16(qa_w) || (logits_out && ((uintptr_t)logits_out & 3)))
    return fail(PROQA_EINVAL, "reader_span: hidden / qa_w must be 16-byte aligned, logits 4-byte aligned");
  const size_t lds = (size_t)2 * seq_len * sizeof(float);
  hipLaunchKernelGGL(reader_span, dim3((unsigned)batch), dim3(kSpanThreads), lds, as_stream(stream), (const _Float16*)hidden,
                     (const int*)seq_lens_dev, (const int*)cu_seqlens_dev, seq_len, hidden_size, (const int*)para_offset_dev,
                     (const _Float16*)qa_w, (const _Float16*)qa_b, max_answer_len, (int*)start_out, (int*)end_out, score_out,
                     (_Float16*)logits_out);
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
