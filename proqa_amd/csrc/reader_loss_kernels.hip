// The reader's training objective (qa/bert_retrieve_qa.py:64-171 as qa/train_dense_qa.sh trains it: --shared-norm, joint
// loss, early loss over the sampler's top-5000) and its gradient: proqa_reader_loss_f16 and
// proqa_reader_loss_backward_f16 in proqa_hip.h, where the objective is written out.
//
// The reference runs two Python loops of CrossEntropyLoss calls and three nonzero() host waits, and its fp16 d_logits
// reach inf at a loss scale of 2^16 whenever a probability is near 1.  Here the forward is three launches and the
// backward four; nothing waits for the host, and the [T, 2] logit gradient exists only in fp32 registers.
//
//   forward   reader_loss_rows      a workgroup owns 32 rows of one sequence: both logits (reader_head.h, the bits of
//                                   proqa_reader_span_f16) and the (max, sum exp) of its rows inside the paragraph mask
//             reader_loss_rank      a workgroup owns 64 rows of para_embed: x_j = q . para_embed[j] in fp32 and the
//                                   (max, sum exp) of all its rows and of its gold rows
//             reader_loss_finish    one workgroup: the normalisers from the partials in ascending order, then the
//                                   log-sum-exp over the answer pairs; writes stats and loss_out
//   backward  reader_loss_pairs     a wave per sequence: w_ba = exp(l_ba + joint) and omega_b
//             reader_loss_bwd_rows  the forward's row ownership: dlogit in fp32, d_hidden, and the workgroup's slab of
//                                   d_qa_w / d_qa_b
//             reader_loss_bwd_rank  the forward's row ownership: drank_j, and the workgroup's slab of d_q
//             reader_loss_bwd_sum   the slabs in ascending order (compensated, as reduce_slabs of train_kernels.hip)
//
// Every kernel has a question dimension (struct Questions): proqa_reader_loss_multi_f16 / _backward_f16 run the same seven
// launches over the sequences and para rows of Q questions, cut by two device CSR arrays; the single-question entry points
// pass no arrays and are the Q = 1 case of the same bodies, index for index.  The row kernels and reader_loss_pairs keep
// their grids over the sequences of all questions, the rank kernels run Q x (blocks of the largest question),
// reader_loss_finish one workgroup per question; reader_loss_bwd_sum adds the questions' d_qa_w / d_qa_b in ascending order.
//
// Determinism: no atomics; a wave adds by the xor butterfly, a workgroup adds its waves in a fixed order, workgroups meet
// only in the ascending sums of reader_loss_finish and reader_loss_bwd_sum.  The T x H passes read every hidden row of
// the paragraph once (16-byte loads, a wave per row, two rows in flight); para_embed is read once per pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>

#include "common.h"
#include "dropout_rng.h"
#include "reader_head.h"

namespace proqa {
namespace {

constexpr int kRowThreads = 512;                 // row kernels: 8 waves
constexpr int kRowWaves = kRowThreads / 64;
constexpr int kRowsPerBlock = 4 * kRowWaves;     // a wave owns rows wave, wave + 8, wave + 16, wave + 24 of its block
constexpr int kRankThreads = 256;                // rank kernels: 4 waves, 16 lanes per row of 128 columns
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankRows = 64;
constexpr int kFinishThreads = 256;
constexpr int kMaxSeqLen = 4096;
constexpr int kMaxAnswers = 1024;
constexpr int kMaxParas = 65536;
constexpr int kStatsHead = 8;                    // stats: 8 scalars, then (Z^s_b, Z^e_b) per sequence

// ---- a running log-sum-exp: the pair (max, sum of exp(. - max)) -------------------------------------------------------------
struct Lse {
  float m, s;
};
__device__ __forceinline__ Lse lse_empty() { return Lse{-INFINITY, 0.f}; }
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
  const float m = fmaxf(a.m, b.m);
  if (m == -INFINITY) return Lse{m, a.s + b.s};   // both empty (or only -inf terms): exp(-inf - -inf) must not be taken
  return Lse{m, a.s * expf(a.m - m) + b.s * expf(b.m - m)};
}
__device__ __forceinline__ Lse lse_of(float v) { return Lse{v, v == -INFINITY ? 0.f : 1.f}; }
__device__ __forceinline__ float lse_value(Lse a) { return a.s > 0.f || a.s != a.s ? a.m + logf(a.s) : -INFINITY; }
__device__ __forceinline__ Lse lse_wave(Lse a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const Lse o = {__shfl_xor(a.m, off, 64), __shfl_xor(a.s, off, 64)};
    a = lse_merge(a, o);
  }
  return a;   // (lane 0's value is the one that is used)
}
// the workgroup's value in thread 0: waves in ascending order; red holds one Lse per wave
__device__ __forceinline__ Lse lse_block(Lse a, Lse* red, int n_waves) {
  a = lse_wave(a);
  __syncthreads();   // red may still be read from the previous use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  Lse t = red[0];
  for (int w = 1; w < n_waves; ++w) t = lse_merge(t, red[w]);
  return t;
}
__device__ __forceinline__ float block_sum(float v, float* red, int n_waves) {
  v = head_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
  for (int w = 1; w < n_waves; ++w) t += red[w];
  return t;
}

// ---- the batch's geometry ----------------------------------------------------------------------------------------------------
struct Layout {
  const int* seq_lens;     // padded layout: sequence b is rows b * seq_len .. + seq_lens[b]
  const int* cu_seqlens;   // packed layout: rows cu_seqlens[b] .. cu_seqlens[b + 1]
  const int* para_offset;
  int seq_len;
};
struct Extent {
  long long row0;   // first row of the sequence in hidden / logits
  int len;          // its length, clamped to [0, seq_len]
  int p0, p1;       // the paragraph mask [p0, p1) = [para_offset, len - 1)
};
__device__ __forceinline__ int clamp_len(int len, int seq_len) { return len < 0 ? 0 : (len > seq_len ? seq_len : len); }
__device__ __forceinline__ Extent extent_of(const Layout& g, int b) {
  Extent e;
  if (g.cu_seqlens) {
    e.row0 = g.cu_seqlens[b];
    e.len = g.cu_seqlens[b + 1] - g.cu_seqlens[b];
  } else {
    e.row0 = (long long)b * g.seq_len;
    e.len = g.seq_lens[b];
  }
  e.len = clamp_len(e.len, g.seq_len);
  const int p0 = g.para_offset[b];
  e.p0 = p0 < 0 ? 0 : p0;
  e.p1 = e.len - 1;
  return e;
}
__device__ __forceinline__ bool in_mask(const Extent& e, int t) { return t >= e.p0 && t < e.p1; }
// the packed row of the sequence's first token (the dropout coordinate is the packed row in both layouts); every lane of
// the wave calls it
__device__ __forceinline__ uint32_t packed_row0(const Layout& g, int b, int lane) {
  if (g.cu_seqlens) return (uint32_t)g.cu_seqlens[b];
  int n = 0;
  for (int i = lane; i < b; i += 64) n += clamp_len(g.seq_lens[i], g.seq_len);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  return (uint32_t)n;
}

// ---- the questions of a pass ----------------------------------------------------------------------------------------------
// Question i owns the sequences seq[i] .. seq[i + 1] and the rows para[i] .. para[i + 1] of para_embed / labels (CSR, on the
// device).  seq == nullptr is the single-question call: one question that owns everything, and every index below is the
// index the single-question kernels have always formed.  The arrays are not trusted: every bound is clamped into
// [0, batch] / [0, n_paras] and made ascending, so that arrays which are not a cover give wrong sums and no stray access.
struct Questions {
  const int* seq;
  const int* para;
  int n;             // the number of questions
  int batch;         // sequences of all questions
  int n_paras;       // rows of para_embed of all questions
  int rank_blocks;   // blocks of 64 para rows the rank grids hold per question
};
struct QSpan {
  int b0, nb;   // the question's first sequence and their number
  int p0, np;   // its first para row and their number
};
__device__ __forceinline__ int clamp_to(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ QSpan question_span(const Questions& qs, int qi) {
  if (!qs.seq) return QSpan{0, qs.batch, 0, qs.n_paras};
  QSpan s;
  s.b0 = clamp_to(qs.seq[qi], 0, qs.batch);
  s.nb = clamp_to(qs.seq[qi + 1], s.b0, qs.batch) - s.b0;
  s.p0 = clamp_to(qs.para[qi], 0, qs.n_paras);
  s.np = clamp_to(qs.para[qi + 1], s.p0, qs.n_paras) - s.p0;
  return s;
}
// the question's blocks of 64 para rows, never more than the rank grids hold
__device__ __forceinline__ int rank_blocks_of(const Questions& qs, const QSpan& s) {
  const int n = (s.np + 63) / 64;
  return n < qs.rank_blocks ? n : qs.rank_blocks;
}
// the last question whose first sequence is <= b (bisection; the loads are uniform over the wave)
__device__ __forceinline__ int question_of_seq(const Questions& qs, int b) {
  if (!qs.seq) return 0;
  int lo = 0, hi = qs.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (qs.seq[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// the question's stats: the single-question layout (8 scalars, then 2 per sequence), question after question
__device__ __forceinline__ size_t stats_at(int qi, const QSpan& s) { return (size_t)kStatsHead * qi + 2 * (size_t)s.b0; }

__device__ __forceinline__ void load_head_weights(const _Float16* qa_w, int hsize, int lane, int n_chunks,
                                                  f16x8 (&w0)[kHeadMaxChunks], f16x8 (&w1)[kHeadMaxChunks]) {
#pragma unroll
  for (int c = 0; c < kHeadMaxChunks; ++c) {
    const int chunk = lane + 64 * c;
    if (chunk < n_chunks) {
      w0[c] = *(const f16x8*)(qa_w + chunk * 8);
      w1[c] = *(const f16x8*)(qa_w + hsize + chunk * 8);
    }
  }
}
__device__ __forceinline__ void load_row(const _Float16* x, int lane, int n_chunks, f16x8 (&xa)[kHeadMaxChunks]) {
#pragma unroll
  for (int c = 0; c < kHeadMaxChunks; ++c) {
    const int chunk = lane + 64 * c;
    if (chunk < n_chunks) xa[c] = *(const f16x8*)(x + chunk * 8);
  }
}

// ---- forward: logits and the partial normalisers of 32 rows ----------------------------------------------------------------
// grid batch * n_blocks (sequence-major).  span_part[(b * n_blocks + block) * 4] = (max, sum) of the start logits, (max, sum)
// of the end logits of the block's rows inside the mask; every workgroup writes its entry.
template <bool kDrop>
__global__ __launch_bounds__(kRowThreads) void reader_loss_rows(const _Float16* __restrict__ hidden, Layout g, int n_blocks,
                                                                 int hsize,
                                                                 const _Float16* __restrict__ qa_w,
                                                                 const _Float16* __restrict__ qa_b, DropoutParams drop,
                                                                 _Float16* __restrict__ logits_out,
                                                                 float* __restrict__ span_part) {
  __shared__ float lg_s[kRowsPerBlock], lg_e[kRowsPerBlock];
  const int b = blockIdx.x / n_blocks;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Extent ext = extent_of(g, b);
  const int base = (blockIdx.x - b * n_blocks) * kRowsPerBlock;
  const int n_chunks = hsize >> 3;
  if (tid < kRowsPerBlock) {
    lg_s[tid] = -INFINITY;
    lg_e[tid] = -INFINITY;
  }
  __syncthreads();
  if (base < ext.len) {
    f16x8 w0[kHeadMaxChunks], w1[kHeadMaxChunks];
    load_head_weights(qa_w, hsize, lane, n_chunks, w0, w1);
    const float b0 = (float)qa_b[0], b1 = (float)qa_b[1];
    const uint32_t prow0 = kDrop ? packed_row0(g, b, lane) : 0u;
    for (int r = base + wave; r < ext.len && r < base + kRowsPerBlock; r += 2 * kRowWaves) {
      const int r2 = r + kRowWaves;
      const bool two = r2 < ext.len;
      const int ry = two ? r2 : r;
      f16x8 xa[kHeadMaxChunks], ya[kHeadMaxChunks];
      load_row(hidden + (ext.row0 + r) * hsize, lane, n_chunks, xa);
      load_row(hidden + (ext.row0 + ry) * hsize, lane, n_chunks, ya);
      float s0, e0, s1, e1;
      head_row_dots<kDrop>(xa, w0, w1, lane, n_chunks, drop, prow0 + (uint32_t)r, s0, e0);
      head_row_dots<kDrop>(ya, w0, w1, lane, n_chunks, drop, prow0 + (uint32_t)ry, s1, e1);
      const _Float16 hs0 = head_logit(s0, b0), he0 = head_logit(e0, b1);
      const _Float16 hs1 = head_logit(s1, b0), he1 = head_logit(e1, b1);
      if (lane == 0) {
        const f16x2 o0 = {hs0, he0};
        *(f16x2*)(logits_out + (ext.row0 + r) * 2) = o0;
        if (in_mask(ext, r)) {
          lg_s[r - base] = (float)hs0;
          lg_e[r - base] = (float)he0;
        }
        if (two) {
          const f16x2 o1 = {hs1, he1};
          *(f16x2*)(logits_out + (ext.row0 + r2) * 2) = o1;
          if (in_mask(ext, r2)) {
            lg_s[r2 - base] = (float)hs1;
            lg_e[r2 - base] = (float)he1;
          }
        }
      }
    }
  }
  // the padded layout's rows past the sequence: zeros, so that every row of logits_out is defined
  if (!g.cu_seqlens && tid < kRowsPerBlock && base + tid >= ext.len && base + tid < g.seq_len)
    *(f16x2*)(logits_out + (ext.row0 + base + tid) * 2) = f16x2{};
  __syncthreads();
  if (wave == 0) {
    const Lse s = lse_wave(lane < kRowsPerBlock ? lse_of(lg_s[lane]) : lse_empty());
    const Lse e = lse_wave(lane < kRowsPerBlock ? lse_of(lg_e[lane]) : lse_empty());
    if (lane == 0) {
      float* out = span_part + (size_t)blockIdx.x * 4;
      out[0] = s.m;
      out[1] = s.s;
      out[2] = e.m;
      out[3] = e.s;
    }
  }
}

// ---- rank scores ---------------------------------------------------------------------------------------------------------------
// 16 lanes own a row of 128 columns, 8 columns each: fp16 rows one 16-byte load, fp32 rows two.  The dot product is fp32:
// products in column order within the lane, then the butterfly over the row's 16 lanes.
struct RankRow {
  float v[8];
};
template <bool kF32>
__device__ __forceinline__ RankRow load_rank_row(const void* para, long long row, int col0) {
  RankRow r;
  if (kF32) {
    const float4* p = (const float4*)((const float*)para + row * PROQA_EMBED_DIM + col0);
    const float4 a = p[0], b = p[1];
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  } else {
    const f16x8 h = *(const f16x8*)((const _Float16*)para + row * PROQA_EMBED_DIM + col0);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = (float)h[i];
  }
  return r;
}
__device__ __forceinline__ float rank_score(const RankRow& r, const float (&qv)[8]) {
  float x = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) x += qv[i] * r.v[i];
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ void load_q(const _Float16* q, int col0, float (&qv)[8]) {
  const f16x8 h = *(const f16x8*)(q + col0);
#pragma unroll
  for (int i = 0; i < 8; ++i) qv[i] = (float)h[i];
}

// grid n_questions * rank_blocks (question-major): a workgroup owns 64 rows of ONE question's para_embed, counted from the
// question's first row; a workgroup past the question's rows does nothing, and nothing reads its outputs.
// x_out[j] = q . para_embed[j]; rank_part[block * 8] = (max, sum) over the block's rows, (max, sum) over its gold rows, the
// number of its gold rows.
template <bool kF32>
__global__ __launch_bounds__(kRankThreads) void reader_loss_rank(const _Float16* __restrict__ q, const void* __restrict__ para_all,
                                                                  const int* __restrict__ labels_all, Questions qs,
                                                                  float* __restrict__ x_all, float* __restrict__ rank_part) {
  __shared__ float xs[kRankRows];
  __shared__ int gold[kRankRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col0 = (lane & 15) * 8;
  const int qi = blockIdx.x / qs.rank_blocks;
  const QSpan span = question_span(qs, qi);
  const int n_paras = span.np;
  const int base = (blockIdx.x - qi * qs.rank_blocks) * kRankRows;
  if (base >= n_paras) return;
  const void* para = kF32 ? (const void*)((const float*)para_all + (size_t)span.p0 * PROQA_EMBED_DIM)
                          : (const void*)((const _Float16*)para_all + (size_t)span.p0 * PROQA_EMBED_DIM);
  const int* labels = labels_all + span.p0;
  float* x_out = x_all + span.p0;
  float qv[8];
  load_q(q + (size_t)qi * PROQA_EMBED_DIM, col0, qv);
  RankRow rows[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = base + wave * 16 + it * 4 + (lane >> 4);
    rows[it] = load_rank_row<kF32>(para, j < n_paras ? j : n_paras - 1, col0);
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int local = wave * 16 + it * 4 + (lane >> 4);
    const int j = base + local;
    const float x = rank_score(rows[it], qv);
    if ((lane & 15) == 0) {
      const bool live = j < n_paras;
      xs[local] = live ? x : -INFINITY;
      gold[local] = live && labels[j] != 0;
      if (live) x_out[j] = x;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const bool is_gold = gold[lane] != 0;
    const Lse all = lse_wave(lse_of(xs[lane]));
    const Lse gl = lse_wave(is_gold ? lse_of(xs[lane]) : lse_empty());
    const float n_gold = head_wave_sum(is_gold ? 1.f : 0.f);
    if (lane == 0) {
      float* out = rank_part + (size_t)blockIdx.x * 8;
      out[0] = all.m;
      out[1] = all.s;
      out[2] = gl.m;
      out[3] = gl.s;
      out[4] = n_gold;
      out[5] = out[6] = out[7] = 0.f;
    }
  }
}

// ---- forward: normalisers, pairs, loss -------------------------------------------------------------------------------------
// l_ba of a pair, or -inf when a position lies outside the paragraph mask; stats holds the normalisers
__device__ __forceinline__ float pair_logprob(const Extent& e, int sp, int ep, const _Float16* __restrict__ logits, float zs,
                                              float ze, float log_r) {
  if (!in_mask(e, sp) || !in_mask(e, ep)) return -INFINITY;
  const float s = (float)logits[(e.row0 + sp) * 2], t = (float)logits[(e.row0 + ep) * 2 + 1];
  return s - zs + t - ze + log_r;
}

// grid n_questions: one workgroup per question; b below counts the question's own sequences
__global__ __launch_bounds__(kFinishThreads) void reader_loss_finish(Layout g_all, Questions qs, int n_blocks, int n_answers,
                                                                      const int* __restrict__ start_all,
                                                                      const int* __restrict__ end_all,
                                                                      int flags, const _Float16* __restrict__ logits,
                                                                      float* span_all,
                                                                      const float* __restrict__ rank_all,
                                                                      const float* __restrict__ x_all, float* __restrict__ stats_all,
                                                                      float* __restrict__ loss_all) {
  __shared__ Lse red[kFinishThreads / 64];
  __shared__ float redf[kFinishThreads / 64];
  __shared__ float bc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kFinishThreads / 64;
  const int qi = blockIdx.x;
  const QSpan span = question_span(qs, qi);
  const int batch = span.nb;
  const int n_rank_blocks = rank_blocks_of(qs, span);
  if (batch < 1 || span.np < batch) {   // only CSR arrays that are not a cover come here: a zero loss and no gradient
    if (tid < kStatsHead) stats_all[stats_at(qi, span) + tid] = 0.f;
    if (tid < 3) loss_all[3 * (size_t)qi + tid] = 0.f;
    return;
  }
  Layout g = g_all;  // the question's sequences: cu_seqlens keeps the rows of the whole pack
  if (g.seq_lens) g.seq_lens += span.b0;
  if (g.cu_seqlens) g.cu_seqlens += span.b0;
  g.para_offset += span.b0;
  const int* start_pos = start_all + (size_t)span.b0 * n_answers;
  const int* end_pos = end_all + (size_t)span.b0 * n_answers;
  float* span_part = span_all + (size_t)span.b0 * n_blocks * 4;
  const float* rank_part = rank_all + (size_t)qi * qs.rank_blocks * 8;
  const float* x = x_all + span.p0;
  float* stats = stats_all + stats_at(qi, span);
  float* loss_out = loss_all + 3 * (size_t)qi;
  float* z = stats + kStatsHead;

  // the normalisers of every sequence: a wave per sequence, its blocks' partials lane by lane
  for (int b = wave; b < batch; b += kWaves) {
    Lse s = lse_empty(), e = lse_empty();
    for (int k = lane; k < n_blocks; k += 64) {
      const float* p = span_part + ((size_t)b * n_blocks + k) * 4;
      s = lse_merge(s, Lse{p[0], p[1]});
      e = lse_merge(e, Lse{p[2], p[3]});
    }
    s = lse_wave(s);
    e = lse_wave(e);
    if (lane == 0) {
      if (flags & PROQA_READER_LOSS_SHARED_NORM) {   // kept as (max, sum) until the sequences have met
        float* p = span_part + (size_t)b * n_blocks * 4;
        p[0] = s.m;
        p[1] = s.s;
        p[2] = e.m;
        p[3] = e.s;
      } else {
        z[2 * b] = lse_value(s);
        z[2 * b + 1] = lse_value(e);
      }
    }
  }
  __syncthreads();
  if (flags & PROQA_READER_LOSS_SHARED_NORM) {
    Lse s = lse_empty(), e = lse_empty();
    for (int b = tid; b < batch; b += kFinishThreads) {
      const float* p = span_part + (size_t)b * n_blocks * 4;
      s = lse_merge(s, Lse{p[0], p[1]});
      e = lse_merge(e, Lse{p[2], p[3]});
    }
    s = lse_block(s, red, kWaves);
    e = lse_block(e, red, kWaves);
    const float zs = lse_value(s), ze = lse_value(e);
    for (int b = tid; b < batch; b += kFinishThreads) {
      z[2 * b] = zs;
      z[2 * b + 1] = ze;
    }
    __syncthreads();
  }

  // the rank normaliser and the gold rows' log-sum-exp
  Lse all = lse_empty(), gl = lse_empty();
  float n_gold = 0.f;
  for (int k = tid; k < n_rank_blocks; k += kFinishThreads) {
    const float* p = rank_part + (size_t)k * 8;
    all = lse_merge(all, Lse{p[0], p[1]});
    gl = lse_merge(gl, Lse{p[2], p[3]});
    n_gold += p[4];
  }
  all = lse_block(all, red, kWaves);
  gl = lse_block(gl, red, kWaves);
  n_gold = block_sum(n_gold, redf, kWaves);
  if (tid == 0) {
    bc[0] = lse_value(all);
    bc[1] = lse_value(gl);
    bc[2] = n_gold;
  }
  __syncthreads();
  const float zr = bc[0], zg = bc[1];
  const bool has_gold = bc[2] > 0.f && !(flags & PROQA_READER_LOSS_NO_EARLY);

  // the answer pairs
  Lse joint = lse_empty();
  float n_valid = 0.f;
  const long long n_pairs = (long long)batch * n_answers;
  for (long long i = tid; i < n_pairs; i += kFinishThreads) {
    const int b = (int)(i / n_answers);
    const Extent e = extent_of(g, b);
    const float l = pair_logprob(e, start_pos[i], end_pos[i], logits, z[2 * b], z[2 * b + 1], x[b] - zr);
    if (in_mask(e, start_pos[i]) && in_mask(e, end_pos[i])) {
      joint = lse_merge(joint, lse_of(l));
      n_valid += 1.f;
    }
  }
  joint = lse_block(joint, red, kWaves);
  n_valid = block_sum(n_valid, redf, kWaves);
  if (tid == 0) {
    const bool has_pair = n_valid > 0.f;
    const float joint_loss = has_pair ? -lse_value(joint) : 0.f;
    const float early_loss = has_gold ? -(zg - zr) : 0.f;
    stats[0] = joint_loss;
    stats[1] = zr;
    stats[2] = zg;
    stats[3] = has_pair ? 1.f : 0.f;
    stats[4] = has_gold ? 1.f : 0.f;
    stats[5] = stats[6] = stats[7] = 0.f;
    loss_out[0] = joint_loss + early_loss;
    loss_out[1] = joint_loss;
    loss_out[2] = early_loss;
  }
}

// ---- backward: pair weights ------------------------------------------------------------------------------------------------
// a wave per sequence: w[b * A + a] = exp(l_ba + joint) (0 for an invalid pair), omega[b] = their sum
// (b counts the sequences of all questions; the wave looks its question up)
__global__ __launch_bounds__(256) void reader_loss_pairs(Layout g, Questions qs, int n_answers, const int* __restrict__ start_pos,
                                                         const int* __restrict__ end_pos,
                                                         const _Float16* __restrict__ q, const void* __restrict__ para,
                                                         int para_f32, const _Float16* __restrict__ logits,
                                                         const float* __restrict__ stats_all, float* __restrict__ w,
                                                         float* __restrict__ omega) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= qs.batch) return;
  const int qi = question_of_seq(qs, b);
  const QSpan span = question_span(qs, qi);
  const int lb = b - span.b0;   // the sequence within its question, and its row of the question's para_embed
  if (lb < 0 || lb >= span.nb || lb >= span.np) {   // only CSR arrays that are not a cover come here
    for (int a = lane; a < n_answers; a += 64) w[(size_t)b * n_answers + a] = 0.f;
    if (lane == 0) omega[b] = 0.f;
    return;
  }
  const float* stats = stats_all + stats_at(qi, span);
  // x_b as the forward formed it: the row's 16 lanes (here lanes 0..15; the other lanes repeat them)
  const int col0 = (lane & 15) * 8;
  float qv[8];
  load_q(q + (size_t)qi * PROQA_EMBED_DIM, col0, qv);
  const long long prow = (long long)span.p0 + lb;
  const RankRow row = para_f32 ? load_rank_row<true>(para, prow, col0) : load_rank_row<false>(para, prow, col0);
  const float log_r = rank_score(row, qv) - stats[1];
  const Extent e = extent_of(g, b);
  const float joint = stats[0], zs = stats[kStatsHead + 2 * lb], ze = stats[kStatsHead + 2 * lb + 1];
  float sum = 0.f;
  for (int a = lane; a < n_answers; a += 64) {
    const size_t i = (size_t)b * n_answers + a;
    const float l = pair_logprob(e, start_pos[i], end_pos[i], logits, zs, ze, log_r);
    const float v = l == -INFINITY ? 0.f : expf(l + joint);
    w[i] = v;
    sum += v;
  }
  sum = head_wave_sum(sum);
  if (lane == 0) omega[b] = sum;
}

// ---- backward: the rows ----------------------------------------------------------------------------------------------------
// grid batch * n_blocks (sequence-major), dynamic LDS 4 * slab_stride floats.  Every row of the block that exists in d_hidden is written
// (zeros outside the mask); the workgroup's sums go to slabs[(b * n_blocks + block) * slab_stride]: d_qa_w [2][H], then
// d_qa_b [2].  slab_stride = 2 H + 8.
template <bool kDrop>
__global__ __launch_bounds__(kRowThreads) void reader_loss_bwd_rows(const _Float16* __restrict__ hidden, Layout g,
                                                                     Questions qs, int n_blocks, int hsize,
                                                                     const _Float16* __restrict__ qa_w, int n_answers,
                                                                     const int* __restrict__ start_pos,
                                                                     const int* __restrict__ end_pos, int flags,
                                                                     DropoutParams drop, const _Float16* __restrict__ logits,
                                                                     const float* __restrict__ stats_all,
                                                                     const float* __restrict__ grad_in,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ omega,
                                                                     _Float16* __restrict__ d_hidden,
                                                                     float* __restrict__ slabs) {
  extern __shared__ float lds[];   // [4][slab_stride]: the waves' sums on their way to wave 0
  __shared__ int sp_s[kMaxAnswers], ep_s[kMaxAnswers];
  __shared__ float w_s[kMaxAnswers];
  const int b = blockIdx.x / n_blocks;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Extent ext = extent_of(g, b);
  const int base = (blockIdx.x - b * n_blocks) * kRowsPerBlock;
  const int n_chunks = hsize >> 3;
  const int slab_stride = 2 * hsize + 8;
  const int n_rows = g.cu_seqlens ? ext.len : g.seq_len;   // rows of the sequence that d_hidden has
  // the sequence's question: its incoming gradient and its stats (b counts the sequences of all questions)
  const int qi = question_of_seq(qs, b);
  const QSpan span = question_span(qs, qi);
  const int lb = b - span.b0;
  const bool owned = lb >= 0 && lb < span.nb;   // false only under CSR arrays that are not a cover: the rows get zeros
  const float* stats = stats_all + stats_at(qi, span);
  const float gin = grad_in[qi];
  const bool has_pair = owned && stats[3] != 0.f;
  const float cb = (flags & PROQA_READER_LOSS_SHARED_NORM) ? 1.f : omega[b];
  const float zs = owned ? stats[kStatsHead + 2 * lb] : 0.f, ze = owned ? stats[kStatsHead + 2 * lb + 1] : 0.f;

  for (int a = tid; a < n_answers; a += kRowThreads) {
    const size_t i = (size_t)b * n_answers + a;
    sp_s[a] = start_pos[i];
    ep_s[a] = end_pos[i];
    w_s[a] = w[i];
  }
  __syncthreads();

  float acc0[kHeadMaxChunks][8], acc1[kHeadMaxChunks][8];
#pragma unroll
  for (int c = 0; c < kHeadMaxChunks; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc0[c][i] = acc1[c][i] = 0.f;
  float db0 = 0.f, db1 = 0.f;

  f16x8 w0[kHeadMaxChunks], w1[kHeadMaxChunks];
  load_head_weights(qa_w, hsize, lane, n_chunks, w0, w1);
  const uint32_t prow0 = kDrop ? packed_row0(g, b, lane) : 0u;

  for (int r = base + wave; r < n_rows && r < base + kRowsPerBlock; r += 2 * kRowWaves) {
    const int r2 = r + kRowWaves;
    const bool two = r2 < n_rows;
    const int rr[2] = {r, two ? r2 : r};
    const bool live[2] = {in_mask(ext, r), two && in_mask(ext, r2)};
    f16x8 xa[2][kHeadMaxChunks];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (live[k]) {
        load_row(hidden + (ext.row0 + rr[k]) * hsize, lane, n_chunks, xa[k]);
      } else {
#pragma unroll
        for (int c = 0; c < kHeadMaxChunks; ++c) xa[k][c] = f16x8{};
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k == 1 && !two) break;
      const int t = rr[k];
      _Float16* out = d_hidden + (ext.row0 + t) * hsize;
      if (!live[k]) {   // a row outside the mask, or a padding row: zeros
#pragma unroll
        for (int c = 0; c < kHeadMaxChunks; ++c) {
          const int chunk = lane + 64 * c;
          if (chunk < n_chunks) *(f16x8*)(out + chunk * 8) = f16x8{};
        }
        continue;
      }
      // W^s[t], W^e[t]: the pairs lane by lane, then the butterfly
      float ws_t = 0.f, we_t = 0.f;
      for (int a = lane; a < n_answers; a += 64) {
        const float v = w_s[a];
        ws_t += sp_s[a] == t ? v : 0.f;
        we_t += ep_s[a] == t ? v : 0.f;
      }
      ws_t = head_wave_sum(ws_t);
      we_t = head_wave_sum(we_t);
      const f16x2 lg = *(const f16x2*)(logits + (ext.row0 + t) * 2);
      float ds = cb * expf((float)lg[0] - zs) - ws_t;
      float de = cb * expf((float)lg[1] - ze) - we_t;
      ds = has_pair ? gin * ds : 0.f;
      de = has_pair ? gin * de : 0.f;
      db0 += ds;
      db1 += de;
      const uint32_t prow = prow0 + (uint32_t)t;
#pragma unroll
      for (int c = 0; c < kHeadMaxChunks; ++c) {
        const int chunk = lane + 64 * c;
        if (chunk < n_chunks) {
          Philox4 bits = {};
          if (kDrop) bits = dropout_hidden_call(drop, prow, (uint32_t)chunk);
          f16x8 o;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float xd = head_element<kDrop>(xa[k][c][i], drop, bits, i);
            acc0[c][i] += ds * xd;
            acc1[c][i] += de * xd;
            float dh = ds * (float)w0[c][i] + de * (float)w1[c][i];
            if (kDrop) dh = dropout_hidden_keep(drop, bits, i) ? dh * drop.factor : 0.f;
            o[i] = (_Float16)dh;
          }
          *(f16x8*)(out + chunk * 8) = o;
        }
      }
    }
  }

  // the waves' sums: 4..7 into 0..3, 2..3 into 0..1, 1 into 0
  for (int half = kRowWaves / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) {
      float* dst = lds + (size_t)(wave - half) * slab_stride;
#pragma unroll
      for (int c = 0; c < kHeadMaxChunks; ++c) {
        const int chunk = lane + 64 * c;
        if (chunk < n_chunks) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            dst[chunk * 8 + i] = acc0[c][i];
            dst[hsize + chunk * 8 + i] = acc1[c][i];
          }
        }
      }
      if (lane == 0) {
        dst[2 * hsize] = db0;
        dst[2 * hsize + 1] = db1;
      }
    }
    __syncthreads();
    if (wave < half) {
      const float* src = lds + (size_t)wave * slab_stride;
#pragma unroll
      for (int c = 0; c < kHeadMaxChunks; ++c) {
        const int chunk = lane + 64 * c;
        if (chunk < n_chunks) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            acc0[c][i] += src[chunk * 8 + i];
            acc1[c][i] += src[hsize + chunk * 8 + i];
          }
        }
      }
      db0 += src[2 * hsize];       // (every lane of the wave carries the same db0 / db1: the rows' ds / de are wave-uniform)
      db1 += src[2 * hsize + 1];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* dst = slabs + (size_t)blockIdx.x * slab_stride;
#pragma unroll
    for (int c = 0; c < kHeadMaxChunks; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dst[chunk * 8 + i] = acc0[c][i];
          dst[hsize + chunk * 8 + i] = acc1[c][i];
        }
      }
    }
    if (lane == 0) {
      dst[2 * hsize] = db0;
      dst[2 * hsize + 1] = db1;
    }
  }
}

// ---- backward: the rank rows -----------------------------------------------------------------------------------------------
// grid ceil(P / 64): drank_j = [pair](r_j - omega_j [j < B]) + [early](r_j - g_j), times the incoming gradient; the
// workgroup's sum of drank_j para_embed[j] goes to dq_slabs[block * 128].
template <bool kF32>
__global__ __launch_bounds__(kRankThreads) void reader_loss_bwd_rank(const _Float16* __restrict__ q, const void* __restrict__ para_all,
                                                                      const int* __restrict__ labels_all, Questions qs,
                                                                      const float* __restrict__ stats_all,
                                                                      const float* __restrict__ grad_in,
                                                                      const float* __restrict__ omega_all,
                                                                      float* __restrict__ dq_slabs) {
  __shared__ float part[kRankWaves][PROQA_EMBED_DIM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col0 = (lane & 15) * 8;
  // the forward's ownership: the grid is question-major, the rows count from the question's first
  const int qi = blockIdx.x / qs.rank_blocks;
  const QSpan span = question_span(qs, qi);
  const int n_paras = span.np, batch = span.nb;
  const int base = (blockIdx.x - qi * qs.rank_blocks) * kRankRows;
  if (base >= n_paras) return;
  const void* para = kF32 ? (const void*)((const float*)para_all + (size_t)span.p0 * PROQA_EMBED_DIM)
                          : (const void*)((const _Float16*)para_all + (size_t)span.p0 * PROQA_EMBED_DIM);
  const int* labels = labels_all + span.p0;
  const float* omega = omega_all + span.b0;
  const float* stats = stats_all + stats_at(qi, span);
  float qv[8];
  load_q(q + (size_t)qi * PROQA_EMBED_DIM, col0, qv);
  const float zr = stats[1], zg = stats[2];
  const bool has_pair = stats[3] != 0.f, has_gold = stats[4] != 0.f;
  const float gin = grad_in[qi];
  RankRow rows[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = base + wave * 16 + it * 4 + (lane >> 4);
    rows[it] = load_rank_row<kF32>(para, j < n_paras ? j : n_paras - 1, col0);
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = base + wave * 16 + it * 4 + (lane >> 4);
    const float x = rank_score(rows[it], qv);
    if (j < n_paras) {
      const float r = expf(x - zr);
      float d = 0.f;
      if (has_pair) d += r - (j < batch ? omega[j] : 0.f);
      if (has_gold) d += r - (labels[j] != 0 ? expf(x - zg) : 0.f);
      d = (has_pair || has_gold) ? gin * d : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += d * rows[it].v[i];
    }
  }
  // the wave's four row groups, then the waves in ascending order
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc[i] += __shfl_xor(acc[i], 16, 64);
    acc[i] += __shfl_xor(acc[i], 32, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int i = 0; i < 8; ++i) part[wave][col0 + i] = acc[i];
  }
  __syncthreads();
  if (tid < PROQA_EMBED_DIM) {
    float s = part[0][tid];
#pragma unroll
    for (int k = 1; k < kRankWaves; ++k) s += part[k][tid];
    dq_slabs[(size_t)blockIdx.x * PROQA_EMBED_DIM + tid] = s;
  }
}

// ---- backward: slabs -> sums -------------------------------------------------------------------------------------------------
// one thread per output: 2 H weights, 2 biases, 128 columns of d_q; the slabs in ascending order, compensated (Kahan)
__device__ __forceinline__ void kahan_add(float v, float& s, float& comp) {
  const float y = v - comp;
  const float t = s + y;
  comp = (t - s) - y;
  s = t;
}
// (eight loads in flight, then the eight additions in slab order: the order of the sum does not depend on the batching)
__device__ __forceinline__ float sum_slabs(const float* __restrict__ p, long long n, size_t stride) {
  float s = 0.f, comp = 0.f;
  long long k = 0;
  for (; k + 8 <= n; k += 8) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[(size_t)(k + i) * stride];
#pragma unroll
    for (int i = 0; i < 8; ++i) kahan_add(v[i], s, comp);
  }
  for (; k < n; ++k) kahan_add(p[(size_t)k * stride], s, comp);
  return s;
}
// d_qa_w / d_qa_b: the compensated sum of EACH question's slabs (what the single-question call returns for it), then the
// questions in ascending order by plain fp32 additions, starting from question 0's value.  d_q: 128 columns per question.
__global__ __launch_bounds__(256) void reader_loss_bwd_sum(const float* __restrict__ slabs, Questions qs, int n_blocks, int hsize,
                                                           const float* __restrict__ dq_slabs,
                                                           float* __restrict__ d_qa_w, float* __restrict__ d_qa_b,
                                                           _Float16* __restrict__ d_q) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_w = 2 * hsize;
  const size_t stride = (size_t)n_w + 8;
  if (t < n_w + 2) {
    QSpan span = question_span(qs, 0);
    float s = sum_slabs(slabs + (size_t)span.b0 * n_blocks * stride + t, (long long)span.nb * n_blocks, stride);
    for (int qi = 1; qi < qs.n; ++qi) {
      span = question_span(qs, qi);
      s += sum_slabs(slabs + (size_t)span.b0 * n_blocks * stride + t, (long long)span.nb * n_blocks, stride);
    }
    if (t < n_w) d_qa_w[t] = s;
    else d_qa_b[t - n_w] = s;
  } else if (t < n_w + 2 + qs.n * PROQA_EMBED_DIM) {
    const int qi = (t - n_w - 2) / PROQA_EMBED_DIM, c = (t - n_w - 2) % PROQA_EMBED_DIM;
    const QSpan span = question_span(qs, qi);
    d_q[(size_t)qi * PROQA_EMBED_DIM + c] = (_Float16)sum_slabs(
        dq_slabs + (size_t)qi * qs.rank_blocks * PROQA_EMBED_DIM + c, rank_blocks_of(qs, span), PROQA_EMBED_DIM);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// the caps of a multi-question pass (proqa_hip.h)
constexpr int kMaxQuestions = 4096;
constexpr int kMaxPackSeqs = 65536;
constexpr int kMaxPackParas = 1 << 22;
const int kPackedOnly = 0;   // stands for cu_seqlens in check_sizes: the multi calls take the packed layout only

// the regions of the caller's scratch (bytes from its start); forward and backward overlay each other.  n_rank: the rank
// grids' blocks over all questions (n_questions * blocks of the largest question).
struct Scratch {
  size_t span_part, rank_part, x;             // forward
  size_t w, omega, slabs, dq_slabs;           // backward
  size_t bytes;
};
Scratch scratch_of(int batch, int seq_len, int hsize, int n_answers, int n_paras, size_t n_rank) {
  const size_t n_blocks = (size_t)ceil_div(seq_len, kRowsPerBlock);
  Scratch s;
  size_t at = 0;
  s.span_part = at, at += up16((size_t)batch * n_blocks * 4 * sizeof(float));
  s.rank_part = at, at += up16(n_rank * 8 * sizeof(float));
  s.x = at, at += up16((size_t)n_paras * sizeof(float));
  const size_t fwd = at;
  at = 0;
  s.w = at, at += up16((size_t)batch * n_answers * sizeof(float));
  s.omega = at, at += up16((size_t)batch * sizeof(float));
  s.slabs = at, at += up16((size_t)batch * n_blocks * (2 * (size_t)hsize + 8) * sizeof(float));
  s.dq_slabs = at, at += up16(n_rank * PROQA_EMBED_DIM * sizeof(float));
  s.bytes = at > fwd ? at : fwd;
  return s;
}

// what every entry point checks before the device is touched; paras_cap: the most rows of para_embed the call takes
int check_sizes(const char* who, int batch, int seq_len, int hsize, int n_answers, int n_paras, int paras_cap, int dim,
                int para_dtype, int flags, const void* seq_lens, const void* cu_seqlens) {
  if (dim != PROQA_EMBED_DIM) return fail(PROQA_EINVAL, "%s: dim=%d, only %d is supported", who, dim, PROQA_EMBED_DIM);
  if (hsize <= 0 || hsize % 8 || hsize > 64 * kHeadMaxChunks * 8)
    return fail(PROQA_EINVAL, "%s: hidden=%d must be a multiple of 8 and <= %d", who, hsize, 64 * kHeadMaxChunks * 8);
  if (batch < 1 || seq_len < 1 || seq_len > kMaxSeqLen)
    return fail(PROQA_EINVAL, "%s: batch=%d must be >= 1 and seq_len=%d in [1, %d]", who, batch, seq_len, kMaxSeqLen);
  if (n_answers < 1 || n_answers > kMaxAnswers)
    return fail(PROQA_EINVAL, "%s: %d answer positions per sequence, must be in [1, %d]", who, n_answers, kMaxAnswers);
  if (n_paras < batch || n_paras > paras_cap)
    return fail(PROQA_EINVAL, "%s: para_embed has %d rows; the first %d belong to the sequences and at most %d are taken", who,
                n_paras, batch, paras_cap);
  if (para_dtype != PROQA_F16 && para_dtype != PROQA_F32) return fail(PROQA_EINVAL, "%s: para_dtype=%d", who, para_dtype);
  if (flags & ~(PROQA_READER_LOSS_SHARED_NORM | PROQA_READER_LOSS_NO_EARLY)) return fail(PROQA_EINVAL, "%s: flags=%d", who, flags);
  if ((seq_lens == nullptr) == (cu_seqlens == nullptr))
    return fail(PROQA_EINVAL, "%s: exactly one of seq_lens (padded) and cu_seqlens (packed) must be given", who);
  return PROQA_OK;
}

// the questions of a multi call: the integers, and the host copies of the CSR arrays when the caller has them
int check_questions(const char* who, int n_questions, int batch, int n_paras, int max_seqs, int max_paras,
                    const int32_t* seq_host, const int32_t* para_host) {
  if (n_questions < 1 || n_questions > kMaxQuestions)
    return fail(PROQA_EINVAL, "%s: %d questions, must be in [1, %d]", who, n_questions, kMaxQuestions);
  if (batch < n_questions || batch > kMaxPackSeqs)
    return fail(PROQA_EINVAL, "%s: %d sequences for %d questions; every question has one, and at most %d are taken", who, batch,
                n_questions, kMaxPackSeqs);
  if (max_seqs < 1 || max_seqs > batch - (n_questions - 1) || (long long)max_seqs * n_questions < batch)
    return fail(PROQA_EINVAL, "%s: max_seqs=%d cannot be the largest of %d questions' counts that sum to %d", who, max_seqs,
                n_questions, batch);
  if (max_paras < max_seqs || max_paras > kMaxParas || max_paras > n_paras - (n_questions - 1) ||
      (long long)max_paras * n_questions < n_paras)
    return fail(PROQA_EINVAL, "%s: max_paras=%d cannot be the largest of %d questions' counts that sum to %d (each >= its "
                "sequences, <= %d)", who, max_paras, n_questions, n_paras, kMaxParas);
  if ((seq_host == nullptr) != (para_host == nullptr))
    return fail(PROQA_EINVAL, "%s: the host copies of question_seq and question_para come together or not at all", who);
  if (!seq_host) return PROQA_OK;
  if (seq_host[0] != 0 || seq_host[n_questions] != batch || para_host[0] != 0 || para_host[n_questions] != n_paras)
    return fail(PROQA_EINVAL, "%s: question_seq must run from 0 to %d and question_para from 0 to %d", who, batch, n_paras);
  for (int i = 0; i < n_questions; ++i) {
    const long long nb = (long long)seq_host[i + 1] - seq_host[i], np = (long long)para_host[i + 1] - para_host[i];
    if (nb < 1 || nb > max_seqs || np < nb || np > max_paras)
      return fail(PROQA_EINVAL, "%s: question %d has %lld sequences and %lld rows of para_embed; 1 <= sequences <= rows, at most "
                  "max_seqs=%d and max_paras=%d", who, i, nb, np, max_seqs, max_paras);
  }
  return PROQA_OK;
}

// the operands both passes share
struct Operands {
  const void* hidden;
  Layout g;
  Questions qs;
  int hsize;
  const void* qa_w;
  const int* start_pos;
  const int* end_pos;
  int n_answers;
  const void* q;
  const void* para;
  int para_dtype;
  const int* labels;
  int flags;
  DropoutParams drop;
};

int launch_forward(const Operands& o, const void* qa_b, void* logits_out, float* stats, float* loss_out, void* ws,
                   const Scratch& sc, hipStream_t st) {
  const int n_blocks = ceil_div(o.g.seq_len, kRowsPerBlock);
  const unsigned n_rank = (unsigned)((size_t)o.qs.n * o.qs.rank_blocks);
  float* span_part = (float*)((char*)ws + sc.span_part);
  float* rank_part = (float*)((char*)ws + sc.rank_part);
  float* x = (float*)((char*)ws + sc.x);
  const dim3 row_grid((unsigned)((size_t)n_blocks * o.qs.batch));
  if (o.drop.thr > 0) {
    hipLaunchKernelGGL(reader_loss_rows<true>, row_grid, dim3(kRowThreads), 0, st, (const _Float16*)o.hidden, o.g, n_blocks, o.hsize,
                       (const _Float16*)o.qa_w, (const _Float16*)qa_b, o.drop, (_Float16*)logits_out, span_part);
  } else {
    hipLaunchKernelGGL(reader_loss_rows<false>, row_grid, dim3(kRowThreads), 0, st, (const _Float16*)o.hidden, o.g, n_blocks, o.hsize,
                       (const _Float16*)o.qa_w, (const _Float16*)qa_b, o.drop, (_Float16*)logits_out, span_part);
  }
  PROQA_LAUNCH_CHECK();
  if (o.para_dtype == PROQA_F32) {
    hipLaunchKernelGGL(reader_loss_rank<true>, dim3(n_rank), dim3(kRankThreads), 0, st, (const _Float16*)o.q, o.para, o.labels,
                       o.qs, x, rank_part);
  } else {
    hipLaunchKernelGGL(reader_loss_rank<false>, dim3(n_rank), dim3(kRankThreads), 0, st, (const _Float16*)o.q, o.para, o.labels,
                       o.qs, x, rank_part);
  }
  PROQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(reader_loss_finish, dim3((unsigned)o.qs.n), dim3(kFinishThreads), 0, st, o.g, o.qs, n_blocks, o.n_answers,
                     o.start_pos, o.end_pos, o.flags, (const _Float16*)logits_out, span_part, (const float*)rank_part,
                     (const float*)x, stats, loss_out);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

int launch_backward(const Operands& o, const void* logits, const float* stats, const float* grad_in, void* d_hidden,
                    float* d_qa_w, float* d_qa_b, void* d_q, void* ws, const Scratch& sc, hipStream_t st) {
  const int n_blocks = ceil_div(o.g.seq_len, kRowsPerBlock);
  const unsigned n_rank = (unsigned)((size_t)o.qs.n * o.qs.rank_blocks);
  float* w = (float*)((char*)ws + sc.w);
  float* omega = (float*)((char*)ws + sc.omega);
  float* slabs = (float*)((char*)ws + sc.slabs);
  float* dq_slabs = (float*)((char*)ws + sc.dq_slabs);
  hipLaunchKernelGGL(reader_loss_pairs, dim3((unsigned)ceil_div(o.qs.batch, 4)), dim3(256), 0, st, o.g, o.qs, o.n_answers,
                     o.start_pos, o.end_pos, (const _Float16*)o.q, o.para, (int)(o.para_dtype == PROQA_F32),
                     (const _Float16*)logits, stats, w, omega);
  PROQA_LAUNCH_CHECK();
  const dim3 row_grid((unsigned)((size_t)n_blocks * o.qs.batch));
  const size_t lds = (size_t)(kRowWaves / 2) * (2 * (size_t)o.hsize + 8) * sizeof(float);
  if (o.drop.thr > 0) {
    hipLaunchKernelGGL(reader_loss_bwd_rows<true>, row_grid, dim3(kRowThreads), lds, st, (const _Float16*)o.hidden, o.g, o.qs, n_blocks,
                       o.hsize, (const _Float16*)o.qa_w, o.n_answers, o.start_pos, o.end_pos, o.flags, o.drop,
                       (const _Float16*)logits, stats, grad_in, (const float*)w, (const float*)omega, (_Float16*)d_hidden, slabs);
  } else {
    hipLaunchKernelGGL(reader_loss_bwd_rows<false>, row_grid, dim3(kRowThreads), lds, st, (const _Float16*)o.hidden, o.g, o.qs, n_blocks,
                       o.hsize, (const _Float16*)o.qa_w, o.n_answers, o.start_pos, o.end_pos, o.flags, o.drop,
                       (const _Float16*)logits, stats, grad_in, (const float*)w, (const float*)omega, (_Float16*)d_hidden, slabs);
  }
  PROQA_LAUNCH_CHECK();
  if (o.para_dtype == PROQA_F32) {
    hipLaunchKernelGGL(reader_loss_bwd_rank<true>, dim3(n_rank), dim3(kRankThreads), 0, st, (const _Float16*)o.q, o.para, o.labels,
                       o.qs, stats, grad_in, (const float*)omega, dq_slabs);
  } else {
    hipLaunchKernelGGL(reader_loss_bwd_rank<false>, dim3(n_rank), dim3(kRankThreads), 0, st, (const _Float16*)o.q, o.para, o.labels,
                       o.qs, stats, grad_in, (const float*)omega, dq_slabs);
  }
  PROQA_LAUNCH_CHECK();
  const int n_out = 2 * o.hsize + 2 + o.qs.n * PROQA_EMBED_DIM;
  hipLaunchKernelGGL(reader_loss_bwd_sum, dim3((unsigned)ceil_div(n_out, 256)), dim3(256), 0, st, (const float*)slabs, o.qs, n_blocks,
                     o.hsize, (const float*)dq_slabs, d_qa_w, d_qa_b, (_Float16*)d_q);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

// the questions of a multi call, as its entry points receive them
struct QuestionArgs {
  const int32_t *seq_dev, *para_dev;
  int n, max_seqs, max_paras;
  const int32_t *seq_host, *para_host;
};

// What all four entry points do before they launch: the checks, in one order and one wording, then the operands and the
// regions of the scratch.  questions == nullptr: one question that owns the whole batch, in either layout; otherwise the
// packed layout (seq_lens_dev is NULL; a NULL cu_seqlens is reported with the other NULLs).  `own`: the entry's own pointers
// that must not be NULL (qa_b and the outputs, or the saved tensors and the gradients).  logits is the forward's output or the
// backward's input; d_hidden is NULL in a forward call.
int prepare(const char* who, const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
            int seq_len, int hsize, const int32_t* para_offset_dev, const void* qa_w, const int32_t* start_pos,
            const int32_t* end_pos, int n_answers, const void* q, const void* para_embed, int para_dtype, const int32_t* labels,
            int n_paras, int dim, const QuestionArgs* questions, int flags, double p, uint64_t seed, int site, uint32_t call,
            std::initializer_list<const void*> own, const void* logits, const void* d_hidden, const void* ws, size_t ws_bytes,
            Operands* o, Scratch* sc) {
  const QuestionArgs* qa = questions;
  int rc = check_sizes(who, batch, seq_len, hsize, n_answers, n_paras, qa ? kMaxPackParas : kMaxParas, dim, para_dtype, flags,
                       seq_lens_dev, qa ? (const void*)&kPackedOnly : cu_seqlens_dev);
  if (rc == PROQA_OK && qa)
    rc = check_questions(who, qa->n, batch, n_paras, qa->max_seqs, qa->max_paras, qa->seq_host, qa->para_host);
  if (rc != PROQA_OK) return rc;
  DropoutParams drop;
  if (!make_dropout_params(p, seed, site, call, &drop))
    return fail(PROQA_EINVAL, "%s: p=%g must be in [0, 1) and site=%d in [0, 255]", who, p, site);
  bool null = !hidden || !para_offset_dev || !qa_w || !start_pos || !end_pos || !q || !para_embed || !labels || !logits || !ws ||
              (qa && (!cu_seqlens_dev || !qa->seq_dev || !qa->para_dev));
  for (const void* ptr : own) null = null || !ptr;
  if (null) return fail(PROQA_EINVAL, "%s: NULL argument", who);
  if (!aligned16(hidden) || !aligned16(qa_w) || !aligned16(q) || !aligned16(para_embed) || !aligned16(ws) ||
      (d_hidden && !aligned16(d_hidden)) || ((uintptr_t)logits & 3))
    return fail(PROQA_EINVAL, "%s: hidden / qa_w / q / para_embed / %sws must be 16-byte aligned, logits 4-byte aligned", who,
                d_hidden ? "d_hidden / " : "");
  const int n_questions = qa ? qa->n : 1;
  const int rank_blocks = ceil_div(qa ? qa->max_paras : n_paras, kRankRows);
  *sc = scratch_of(batch, seq_len, hsize, n_answers, n_paras, (size_t)n_questions * rank_blocks);
  if (ws_bytes < sc->bytes) return fail(PROQA_EINVAL, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, sc->bytes);
  *o = Operands{hidden, Layout{(const int*)seq_lens_dev, (const int*)cu_seqlens_dev, (const int*)para_offset_dev, seq_len},
                Questions{qa ? (const int*)qa->seq_dev : nullptr, qa ? (const int*)qa->para_dev : nullptr, n_questions, batch,
                          n_paras, rank_blocks},
                hsize, qa_w, (const int*)start_pos, (const int*)end_pos, n_answers, q, para_embed, para_dtype,
                (const int*)labels, flags, drop};
  return PROQA_OK;
}

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

size_t proqa_reader_loss_workspace_bytes(int batch, int seq_len, int hidden_size, int n_answers, int n_paras) {
  if (batch < 1 || seq_len < 1 || hidden_size < 1 || n_answers < 1 || n_paras < 1) return 0;
  return scratch_of(batch, seq_len, hidden_size, n_answers, n_paras, (size_t)ceil_div(n_paras, kRankRows)).bytes;
}

int proqa_reader_loss_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                          int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w, const void* qa_b,
                          const int32_t* start_pos, const int32_t* end_pos, int n_answers, const void* q,
                          const void* para_embed, int para_dtype, const int32_t* labels, int n_paras, int dim, int flags,
                          double p, uint64_t seed, int site, uint32_t call, void* logits_out, float* stats, float* loss_out,
                          void* ws, size_t ws_bytes, void* stream) {
  Operands o;
  Scratch sc;
  const int rc = prepare("reader_loss", hidden, seq_lens_dev, cu_seqlens_dev, batch, seq_len, hidden_size, para_offset_dev, qa_w,
                         start_pos, end_pos, n_answers, q, para_embed, para_dtype, labels, n_paras, dim, nullptr, flags, p, seed,
                         site, call, {qa_b, stats, loss_out}, logits_out, nullptr, ws, ws_bytes, &o, &sc);
  if (rc != PROQA_OK) return rc;
  return launch_forward(o, qa_b, logits_out, stats, loss_out, ws, sc, as_stream(stream));
}

int proqa_reader_loss_backward_f16(const void* hidden, const int32_t* seq_lens_dev, const int32_t* cu_seqlens_dev, int batch,
                                   int seq_len, int hidden_size, const int32_t* para_offset_dev, const void* qa_w,
                                   const int32_t* start_pos, const int32_t* end_pos, int n_answers, const void* q,
                                   const void* para_embed, int para_dtype, const int32_t* labels, int n_paras, int dim,
                                   int flags, double p, uint64_t seed, int site, uint32_t call, const void* logits,
                                   const float* stats, const float* grad_in, void* d_hidden, float* d_qa_w, float* d_qa_b,
                                   void* d_q, void* ws, size_t ws_bytes, void* stream) {
  Operands o;
  Scratch sc;
  const int rc = prepare("reader_loss_backward", hidden, seq_lens_dev, cu_seqlens_dev, batch, seq_len, hidden_size,
                         para_offset_dev, qa_w, start_pos, end_pos, n_answers, q, para_embed, para_dtype, labels, n_paras, dim,
                         nullptr, flags, p, seed, site, call, {stats, grad_in, d_hidden, d_qa_w, d_qa_b, d_q}, logits, d_hidden,
                         ws, ws_bytes, &o, &sc);
  if (rc != PROQA_OK) return rc;
  return launch_backward(o, logits, stats, grad_in, d_hidden, d_qa_w, d_qa_b, d_q, ws, sc, as_stream(stream));
}

size_t proqa_reader_loss_multi_workspace_bytes(int n_questions, int batch, int seq_len, int hidden_size, int n_answers,
                                               int n_paras, int max_paras) {
  if (n_questions < 1 || batch < 1 || seq_len < 1 || hidden_size < 1 || n_answers < 1 || n_paras < 1 || max_paras < 1) return 0;
  return scratch_of(batch, seq_len, hidden_size, n_answers, n_paras, (size_t)n_questions * ceil_div(max_paras, kRankRows)).bytes;
}

int proqa_reader_loss_multi_f16(const void* hidden, const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden_size,
                                const int32_t* para_offset_dev, const void* qa_w, const void* qa_b, const int32_t* start_pos,
                                const int32_t* end_pos, int n_answers, const void* q, const void* para_embed, int para_dtype,
                                const int32_t* labels, int n_paras, int dim, const int32_t* question_seq_dev,
                                const int32_t* question_para_dev, int n_questions, int max_seqs, int max_paras,
                                const int32_t* question_seq_host, const int32_t* question_para_host, int flags, double p,
                                uint64_t seed, int site, uint32_t call, void* logits_out, float* stats, float* loss_out,
                                void* ws, size_t ws_bytes, void* stream) {
  const QuestionArgs qa = {question_seq_dev, question_para_dev, n_questions, max_seqs, max_paras, question_seq_host,
                           question_para_host};
  Operands o;
  Scratch sc;
  const int rc = prepare("reader_loss_multi", hidden, nullptr, cu_seqlens_dev, batch, seq_len, hidden_size, para_offset_dev, qa_w,
                         start_pos, end_pos, n_answers, q, para_embed, para_dtype, labels, n_paras, dim, &qa, flags, p, seed, site,
                         call, {qa_b, stats, loss_out}, logits_out, nullptr, ws, ws_bytes, &o, &sc);
  if (rc != PROQA_OK) return rc;
  return launch_forward(o, qa_b, logits_out, stats, loss_out, ws, sc, as_stream(stream));
}

int proqa_reader_loss_multi_backward_f16(const void* hidden, const int32_t* cu_seqlens_dev, int batch, int seq_len,
                                         int hidden_size, const int32_t* para_offset_dev, const void* qa_w,
                                         const int32_t* start_pos, const int32_t* end_pos, int n_answers, const void* q,
                                         const void* para_embed, int para_dtype, const int32_t* labels, int n_paras, int dim,
                                         const int32_t* question_seq_dev, const int32_t* question_para_dev, int n_questions,
                                         int max_seqs, int max_paras, const int32_t* question_seq_host,
                                         const int32_t* question_para_host, int flags, double p, uint64_t seed, int site,
                                         uint32_t call, const void* logits, const float* stats, const float* grad_in,
                                         void* d_hidden, float* d_qa_w, float* d_qa_b, void* d_q, void* ws, size_t ws_bytes,
                                         void* stream) {
  const QuestionArgs qa = {question_seq_dev, question_para_dev, n_questions, max_seqs, max_paras, question_seq_host,
                           question_para_host};
  Operands o;
  Scratch sc;
  const int rc = prepare("reader_loss_multi_backward", hidden, nullptr, cu_seqlens_dev, batch, seq_len, hidden_size,
                         para_offset_dev, qa_w, start_pos, end_pos, n_answers, q, para_embed, para_dtype, labels, n_paras, dim,
                         &qa, flags, p, seed, site, call, {stats, grad_in, d_hidden, d_qa_w, d_qa_b, d_q}, logits, d_hidden, ws,
                         ws_bytes, &o, &sc);
  if (rc != PROQA_OK) return rc;
  return launch_backward(o, logits, stats, grad_in, d_hidden, d_qa_w, d_qa_b, d_q, ws, sc, as_stream(stream));
}

}  // extern "C"
