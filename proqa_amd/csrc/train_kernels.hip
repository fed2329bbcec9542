// Backward operators of the BERT tower and of the in-batch objective (proqa_*_backward_f16, proqa_inbatch_loss_grad_f16,
// proqa_colsum_f16 in proqa_hip.h): what retriever pre-training (README section 3 of the reference,
// retrieval/train_retriever.py:196-214) differentiates through.  The forward kernels (encoder_kernels.hip,
// attention_kernel.hip, inbatch_kernels.hip) save nothing; every operator here recomputes what it needs from the forward's
// own inputs.  Operands are fp16, every sum is fp32, activation gradients leave as fp16, parameter gradients as fp32.
//
// Determinism.  Column sums over rows (bias, gamma, beta gradients) are taken in a fixed order: a workgroup owns a
// contiguous slab of rows, its partial sums go to the caller's workspace ([slab][k][cols] fp32), and reduce_slabs adds the
// slabs in ascending order.  The attention backward has no cross-workgroup sum at all: one kernel owns query rows (softmax
// statistics and dQ), a second owns key rows (dK, dV).  The only atomics are the fp32 adds into the word-embedding gradient
// of the default entry points; the *_det entry points sum it in a fixed order instead (word_grad_* below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "dropout_rng.h"

namespace proqa {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxChunksPerLane = 2;   // row-wise kernels: one wave per row, cols <= 64 * 2 * 8 = 1024 (as the forward)
constexpr int kMaxSlabs = 512;         // row slabs (workgroups) of a column sum
constexpr int kMaxColChunks = 4;       // column-owning kernels: 256 threads x 4 x 8 columns = 8192

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- slabs -> sums ------------------------------------------------------------------------------------------------------
// out_k[c] (+)= sum over the slabs, in ascending order, of ws[slab][k][c], k < n_k <= 4; one thread per (k, column); a null
// out_k is skipped
__global__ __launch_bounds__(256) void reduce_slabs(const float* __restrict__ ws, int n_slabs, int n_k, int cols,
                                                    float* out0, float* out1, float* out2, float* out3, int accumulate) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_k * cols) return;
  const int k = t / cols, c = t - k * cols;
  float* out = k == 0 ? out0 : (k == 1 ? out1 : (k == 2 ? out2 : out3));
  // compensated (Kahan) sum: the slabs of a long batch are many and of one sign more often than not
  float s = 0.f, comp = 0.f;
  for (int b = 0; b < n_slabs; ++b) {
    const float y = ws[((long long)b * n_k + k) * cols + c] - comp;
    const float t = s + y;
    comp = (t - s) - y;
    s = t;
  }
  if (out) out[c] = accumulate ? out[c] + s : s;   // (looked at after the loop: the pointers' loads overlap it)
}

// ---- LayerNorm backward of one register-resident row -------------------------------------------------------------------
// z = the normalised operand (x + bias + residual, or the embedding sum); dz = rstd (a - mean(a) - xhat mean(a xhat)),
// a = dy gamma; dgam += dy xhat, dbet += dy.  Lanes hold chunks lane, lane + 64 of the row (8 columns each).
// Every fused multiply-add is written out and contraction is off: which products the compiler fuses on its own depends on
// how it happens to pack these loops in the kernel they are inlined into, and the kernels that share this row (with and
// without dropout, typed and untyped) must give the same bits.
__device__ __forceinline__ void layernorm_backward_row(const float (&z)[kMaxChunksPerLane][8],
                                                       const float (&dy)[kMaxChunksPerLane][8],
                                                       const float (&gam)[kMaxChunksPerLane][8], int lane, int n_chunks,
                                                       int cols, float eps, float (&dz)[kMaxChunksPerLane][8],
                                                       float (&dgam)[kMaxChunksPerLane][8],
                                                       float (&dbet)[kMaxChunksPerLane][8]) {
#pragma clang fp contract(off)
  const float inv_n = 1.0f / (float)cols;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c)
    if (lane + 64 * c < n_chunks) {
#pragma unroll
      for (int i = 0; i < 8; ++i) s += z[c][i];
    }
  const float mean = wave_sum(s) * inv_n;
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c)
    if (lane + 64 * c < n_chunks) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = z[c][i] - mean;
        v += d * d;
      }
    }
  const float rstd = rsqrtf(__builtin_fmaf(wave_sum(v), inv_n, eps));
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c)
    if (lane + 64 * c < n_chunks) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xhat = (z[c][i] - mean) * rstd;
        const float a = dy[c][i] * gam[c][i];
        s1 += a;
        s2 += a * xhat;
      }
    }
  s1 = wave_sum(s1) * inv_n;
  s2 = wave_sum(s2) * inv_n;
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c)
    if (lane + 64 * c < n_chunks) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xhat = (z[c][i] - mean) * rstd;
        dz[c][i] = rstd * __builtin_fmaf(-s2, xhat, __builtin_fmaf(dy[c][i], gam[c][i], -s1));
        dgam[c][i] = __builtin_fmaf(dy[c][i], xhat, dgam[c][i]);
        dbet[c][i] += dy[c][i];
      }
    }
}

__device__ __forceinline__ void load8(const _Float16* p, float (&dst)[8]) {
  const f16x8 v = *(const f16x8*)p;
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = (float)v[i];
}

// the N per-wave column partials of a 4-wave workgroup -> ws[slab][0..N-1][cols], waves added in ascending order; wave 0
// is left holding the sums
template <int N>
__device__ __forceinline__ void reduce_waves_to_slab(float (*red)[N][64 * kMaxChunksPerLane * 8],
                                                     float (&part)[N][kMaxChunksPerLane][8], int lane, int wave, int n_chunks,
                                                     int cols, float* __restrict__ slab) {
  if (wave > 0) {
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
          for (int k = 0; k < N; ++k) red[wave - 1][k][chunk * 8 + i] = part[k][c][i];
        }
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
          for (int k = 0; k < N; ++k) {
            for (int w = 0; w < 3; ++w) part[k][c][i] += red[w][k][chunk * 8 + i];
            slab[k * cols + chunk * 8 + i] = part[k][c][i];
          }
        }
      }
    }
  }
}

// ---- bias + residual + LayerNorm backward ------------------------------------------------------------------------------
// workgroup = slab of rows_per_slab rows, wave = one row at a time; partials (dgamma, dbeta, dbias) -> ws[slab][3][cols]
// DROP: the forward was LN(dropout(x + bias) + residual).  dz (to dz_out) is the gradient of the residual; the gradient of
// x is dx = dz * keep * factor (to dx_out), and dbias is the column sum of dx before its rounding.
template <bool DROP>
__device__ __forceinline__ void bias_residual_layernorm_bwd_body(
    const _Float16* __restrict__ dy_in, const _Float16* __restrict__ xin, const _Float16* __restrict__ bias,
    const _Float16* __restrict__ residual, const _Float16* __restrict__ gamma, float eps, long long rows, int cols,
    long long rows_per_slab, _Float16* __restrict__ dz_out, _Float16* __restrict__ dx_out, float* __restrict__ ws,
    const DropoutParams& drop) {
  __shared__ float red[3][3][64 * kMaxChunksPerLane * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_chunks = cols >> 3;
  float gam[kMaxChunksPerLane][8], bia[kMaxChunksPerLane][8];
  float part[3][kMaxChunksPerLane][8];                 // dgamma, dbeta, dbias
  auto &dgam = part[0], &dbet = part[1], &dbia = part[2];
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c) {
    const int chunk = lane + 64 * c;
#pragma unroll
    for (int i = 0; i < 8; ++i) gam[c][i] = bia[c][i] = dgam[c][i] = dbet[c][i] = dbia[c][i] = 0.f;
    if (chunk < n_chunks) {
      load8(gamma + chunk * 8, gam[c]);
      load8(bias + chunk * 8, bia[c]);
    }
  }
  const long long row0 = (long long)blockIdx.x * rows_per_slab;
  const long long row1 = row0 + rows_per_slab < rows ? row0 + rows_per_slab : rows;
  for (long long row = row0 + wave; row < row1; row += 4) {
    float z[kMaxChunksPerLane][8], dy[kMaxChunksPerLane][8], dz[kMaxChunksPerLane][8];
    Philox4 bits[kMaxChunksPerLane];                   // (DROP only) the row's decisions: read again for dx
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
        float a[8], r[8];
        load8(xin + row * cols + chunk * 8, a);
        load8(residual + row * cols + chunk * 8, r);
        load8(dy_in + row * cols + chunk * 8, dy[c]);
        if constexpr (DROP) {
          bits[c] = dropout_hidden_call(drop, (uint32_t)row, (uint32_t)chunk);
#pragma unroll
          for (int i = 0; i < 8; ++i)   // the forward's expression
            z[c][i] = (dropout_hidden_keep(drop, bits[c], i) ? (a[i] + bia[c][i]) * drop.factor : 0.f) + r[i];
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) z[c][i] = a[i] + bia[c][i] + r[i];
        }
      }
    }
    layernorm_backward_row(z, dy, gam, lane, n_chunks, cols, eps, dz, dgam, dbet);
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
        f16x8 o;
        if constexpr (DROP) {
          f16x8 ox;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            // a dropped element has no gradient, whatever dz is (0 * inf would be NaN)
            const float dx = dropout_hidden_keep(drop, bits[c], i) ? dz[c][i] * drop.factor : 0.f;
            o[i] = (_Float16)dz[c][i];
            ox[i] = (_Float16)dx;
            dbia[c][i] += dx;
          }
          *(f16x8*)(dx_out + row * cols + chunk * 8) = ox;
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            o[i] = (_Float16)dz[c][i];
            dbia[c][i] += dz[c][i];
          }
        }
        *(f16x8*)(dz_out + row * cols + chunk * 8) = o;
      }
    }
  }
  reduce_waves_to_slab<3>(red, part, lane, wave, n_chunks, cols, ws + (long long)blockIdx.x * 3 * cols);
}

__global__ __launch_bounds__(256) void bias_residual_layernorm_bwd(const _Float16* __restrict__ dy_in,
                                                                   const _Float16* __restrict__ xin,
                                                                   const _Float16* __restrict__ bias,
                                                                   const _Float16* __restrict__ residual,
                                                                   const _Float16* __restrict__ gamma, float eps,
                                                                   long long rows, int cols, long long rows_per_slab,
                                                                   _Float16* __restrict__ dz_out, float* __restrict__ ws) {
  bias_residual_layernorm_bwd_body<false>(dy_in, xin, bias, residual, gamma, eps, rows, cols, rows_per_slab, dz_out, nullptr, ws,
                                          DropoutParams{});
}

__global__ __launch_bounds__(256) void bias_residual_layernorm_dropout_bwd(
    const _Float16* __restrict__ dy_in, const _Float16* __restrict__ xin, const _Float16* __restrict__ bias,
    const _Float16* __restrict__ residual, const _Float16* __restrict__ gamma, float eps, long long rows, int cols,
    long long rows_per_slab, _Float16* __restrict__ dz_out, _Float16* __restrict__ dx_out, float* __restrict__ ws,
    DropoutParams drop) {
  bias_residual_layernorm_bwd_body<true>(dy_in, xin, bias, residual, gamma, eps, rows, cols, rows_per_slab, dz_out, dx_out, ws,
                                         drop);
}

// ---- embedding + LayerNorm backward --------------------------------------------------------------------------------------
// workgroup = position s, its waves take the sequences that are longer than s in turns: dx of token (b, s) goes to the word
// row of its id (fp32 atomics, the one non-deterministic output) and into the position's own sum; d_pos[s] is final when
// the workgroup ends, and (dgamma, dbeta, d_pos[s]) are slab s of the workspace: the type-0 gradient is the sum of the
// position gradients.  ATOMIC false (the *_det entry points) leaves d_word to the word_grad_* kernels below.
// TYPED (the reader's [CLS] q [SEP] p [SEP]): a fourth per-wave accumulator.  The position's sum is kept in two parts, the
// tokens of type 0 and those of type 1 (a type id outside [0, n_types) read row 0 in the forward and counts as type 0 here).
// Slab s of the workspace is (dgamma, dbeta, d_types[0], d_types[1]) of position s; d_pos[s] += part 0 + part 1.  With
// type_ids == nullptr part 1 is +0 and every sum is the sum the untyped kernel takes, in its order.
template <bool TYPED, bool ATOMIC = true>
__device__ __forceinline__ void embed_layernorm_bwd_body(
    const _Float16* __restrict__ dy_in, const long long* __restrict__ ids, const long long* __restrict__ type_ids,
    const int* __restrict__ cu_seqlens, int batch, int seq_len, int hidden, const _Float16* __restrict__ word, long long vocab,
    const _Float16* __restrict__ pos, const _Float16* __restrict__ type_table, int n_types,
    const _Float16* __restrict__ gamma, float eps, long long n_tokens, float* __restrict__ d_word, float* __restrict__ d_pos,
    float* __restrict__ ws) {
  constexpr int N = TYPED ? 4 : 3;
  __shared__ float red[3][N][64 * kMaxChunksPerLane * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_chunks = hidden >> 3;
  const int s = blockIdx.x;
  float gam[kMaxChunksPerLane][8], base[kMaxChunksPerLane][8];   // base = pos[s] (TYPED) or pos[s] + type[0]
  float part[N][kMaxChunksPerLane][8];                           // dgamma, dbeta, the position's sum (TYPED: by type)
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c) {
    const int chunk = lane + 64 * c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      gam[c][i] = base[c][i] = 0.f;
#pragma unroll
      for (int k = 0; k < N; ++k) part[k][c][i] = 0.f;
    }
    if (chunk < n_chunks) {
      load8(gamma + chunk * 8, gam[c]);
      if constexpr (TYPED) {
        load8(pos + (long long)s * hidden + chunk * 8, base[c]);
      } else {
        float p[8], t[8];
        load8(pos + (long long)s * hidden + chunk * 8, p);
        load8(type_table + chunk * 8, t);
#pragma unroll
        for (int i = 0; i < 8; ++i) base[c][i] = p[i] + t[i];
      }
    }
  }
  for (int b = wave; b < batch; b += 4) {
    const int first = cu_seqlens[b];
    const long long row = (long long)first + s;
    if (s >= cu_seqlens[b + 1] - first || row >= n_tokens) continue;   // wave-uniform
    long long id = ids[(long long)b * seq_len + s];
    if (id < 0 || id >= vocab) id = 0;   // the forward read row 0 for such an id
    long long tt = 0;
    if constexpr (TYPED) {
      if (type_ids) tt = type_ids[(long long)b * seq_len + s];
      if (tt < 0 || tt >= n_types) tt = 0;   // and row 0 of the type table
    }
    float z[kMaxChunksPerLane][8], dy[kMaxChunksPerLane][8], dz[kMaxChunksPerLane][8];
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
        float w[8];
        load8(word + id * hidden + chunk * 8, w);
        load8(dy_in + row * hidden + chunk * 8, dy[c]);
        if constexpr (TYPED) {
          float t[8];
          load8(type_table + tt * hidden + chunk * 8, t);
#pragma unroll
          for (int i = 0; i < 8; ++i) z[c][i] = w[i] + (base[c][i] + t[i]);   // the untyped association
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) z[c][i] = w[i] + base[c][i];
        }
      }
    }
    layernorm_backward_row(z, dy, gam, lane, n_chunks, hidden, eps, dz, part[0], part[1]);
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (!TYPED || tt == 0) part[2][c][i] += dz[c][i];   // wave-uniform
          else part[N - 1][c][i] += dz[c][i];
          if constexpr (ATOMIC) atomicAdd(d_word + id * hidden + chunk * 8 + i, dz[c][i]);
        }
      }
    }
  }
  reduce_waves_to_slab<N>(red, part, lane, wave, n_chunks, hidden, ws + (long long)s * N * hidden);
  if (wave == 0) {
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          d_pos[(long long)s * hidden + chunk * 8 + i] += TYPED ? part[2][c][i] + part[N - 1][c][i] : part[2][c][i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void embed_layernorm_bwd(const _Float16* __restrict__ dy_in, const long long* __restrict__ ids,
                                                           const int* __restrict__ cu_seqlens, int batch, int seq_len,
                                                           int hidden, const _Float16* __restrict__ word, long long vocab,
                                                           const _Float16* __restrict__ pos,
                                                           const _Float16* __restrict__ type0,
                                                           const _Float16* __restrict__ gamma, float eps, long long n_tokens,
                                                           float* __restrict__ d_word, float* __restrict__ d_pos,
                                                           float* __restrict__ ws) {
  embed_layernorm_bwd_body<false>(dy_in, ids, nullptr, cu_seqlens, batch, seq_len, hidden, word, vocab, pos, type0, 1, gamma,
                                  eps, n_tokens, d_word, d_pos, ws);
}

__global__ __launch_bounds__(256) void embed_layernorm_typed_bwd(
    const _Float16* __restrict__ dy_in, const long long* __restrict__ ids, const long long* __restrict__ type_ids,
    const int* __restrict__ cu_seqlens, int batch, int seq_len, int hidden, const _Float16* __restrict__ word, long long vocab,
    const _Float16* __restrict__ pos, const _Float16* __restrict__ type_table, int n_types,
    const _Float16* __restrict__ gamma, float eps, long long n_tokens, float* __restrict__ d_word, float* __restrict__ d_pos,
    float* __restrict__ ws) {
  embed_layernorm_bwd_body<true>(dy_in, ids, type_ids, cu_seqlens, batch, seq_len, hidden, word, vocab, pos, type_table,
                                 n_types, gamma, eps, n_tokens, d_word, d_pos, ws);
}

// the same two kernels without the adds into d_word (the *_det entry points: d_word is summed below)
__global__ __launch_bounds__(256) void embed_layernorm_bwd_no_word(
    const _Float16* __restrict__ dy_in, const long long* __restrict__ ids, const int* __restrict__ cu_seqlens, int batch,
    int seq_len, int hidden, const _Float16* __restrict__ word, long long vocab, const _Float16* __restrict__ pos,
    const _Float16* __restrict__ type0, const _Float16* __restrict__ gamma, float eps, long long n_tokens,
    float* __restrict__ d_pos, float* __restrict__ ws) {
  embed_layernorm_bwd_body<false, false>(dy_in, ids, nullptr, cu_seqlens, batch, seq_len, hidden, word, vocab, pos, type0, 1,
                                         gamma, eps, n_tokens, nullptr, d_pos, ws);
}

__global__ __launch_bounds__(256) void embed_layernorm_typed_bwd_no_word(
    const _Float16* __restrict__ dy_in, const long long* __restrict__ ids, const long long* __restrict__ type_ids,
    const int* __restrict__ cu_seqlens, int batch, int seq_len, int hidden, const _Float16* __restrict__ word, long long vocab,
    const _Float16* __restrict__ pos, const _Float16* __restrict__ type_table, int n_types,
    const _Float16* __restrict__ gamma, float eps, long long n_tokens, float* __restrict__ d_pos, float* __restrict__ ws) {
  embed_layernorm_bwd_body<true, false>(dy_in, ids, type_ids, cu_seqlens, batch, seq_len, hidden, word, vocab, pos, type_table,
                                        n_types, gamma, eps, n_tokens, nullptr, d_pos, ws);
}

// ---- the word-embedding gradient in a fixed order (the *_det entry points) ----------------------------------------------------
// The position-owning kernels above run with their atomics compiled out (dgamma, dbeta, d_pos, d_types keep their bits) and
// d_word is summed by a route of its own, launch after launch on the one stream:
//   word_grad_keys      key[r] = (clamped id << 32 | r) of every packed row r < n_tokens; a row that no sequence owns gets
//                       the id `vocab`, which sorts behind every real id
//   word_grad_sort_pass an LSD radix sort of the keys by their id, 8 bits a pass (x3 launches: count, scan, scatter).  A wave
//                       owns kSortKeysPerWave consecutive keys and ranks them 64 at a time with ballots, so a pass is stable
//                       and the rows of one id stay in ascending order
//   word_grad_units     wave = sorted position i.  The occurrences of an id are cut into chunks of kWordGradChunk counted from
//                       the id's first occurrence; a wave whose position does not start a chunk exits.  The others recompute
//                       dz of their chunk's tokens one after the other (the same layernorm_backward_row on the same z, so the
//                       bits the atomic route adds) and sum them in that order.  The only chunk of an id is added straight
//                       into d_word; a chunk of several goes to the workspace
//   word_grad_combine   workgroup = first occurrence of an id with several chunks: its partials in ascending order, then one add
// The sums are written with __fadd_rn: dz ends in a multiply, and `acc += dz` would be contracted into another association.
constexpr int kWordGradChunk = 16;
constexpr int kSortKeysPerWave = 512;   // x 4 waves: a sort workgroup takes 2048 keys
constexpr int kSortScanThreads = 1024;

// the sequence that owns packed row r: the last b with cu_seqlens[b] <= r.  -> false when no valid token lies there
__device__ __forceinline__ bool locate_row(const int* __restrict__ cu_seqlens, int batch, int seq_len, long long r, int* b_out,
                                           int* s_out) {
  int lo = 0, hi = batch;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu_seqlens[mid] <= r) lo = mid;
    else hi = mid;
  }
  const int first = cu_seqlens[lo];
  const long long s = r - first;
  *b_out = lo;
  *s_out = (int)s;
  return s >= 0 && s < cu_seqlens[lo + 1] - first && s < seq_len;
}

__global__ __launch_bounds__(256) void word_grad_keys(const long long* __restrict__ ids, const int* __restrict__ cu_seqlens,
                                                      int batch, int seq_len, long long vocab, int n_tokens,
                                                      unsigned long long* __restrict__ keys) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_tokens) return;
  int b, s;
  long long id = vocab;
  if (locate_row(cu_seqlens, batch, seq_len, r, &b, &s)) {
    id = ids[(long long)b * seq_len + s];
    if (id < 0 || id >= vocab) id = 0;
  }
  keys[r] = ((unsigned long long)id << 32) | (unsigned)r;
}

// SCATTER false: hist[digit][wave] = how many of the wave's keys have that digit.  SCATTER true: hist holds the exclusive
// scan of those counts (digit-major), where the wave's first key of each digit goes; the keys follow in their order.
template <bool SCATTER>
__global__ __launch_bounds__(256) void word_grad_sort_pass(const unsigned long long* __restrict__ in, int n, int shift,
                                                           int n_waves, int* __restrict__ hist,
                                                           unsigned long long* __restrict__ out) {
  __shared__ int cnt[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * 4 + wave;
  if (gw >= n_waves) return;   // wave-uniform; no workgroup barrier below
  int* my = cnt[wave];
#pragma unroll
  for (int k = 0; k < 4; ++k) my[lane + 64 * k] = SCATTER ? hist[(long long)(lane + 64 * k) * n_waves + gw] : 0;
  __builtin_amdgcn_wave_barrier();
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int first = gw * kSortKeysPerWave;
  for (int round = 0; round < kSortKeysPerWave / 64; ++round) {
    const int i = first + round * 64 + lane;
    const bool valid = i < n;
    const unsigned long long key = valid ? in[i] : 0ull;
    const int digit = (int)((key >> shift) & 255u);
    unsigned long long same = __ballot(valid);   // the lanes of this round whose digit is mine
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long has = __ballot(valid && ((digit >> bit) & 1));
      same &= ((digit >> bit) & 1) ? has : ~has;
    }
    const int before = __popcll(same & below);
    int at = 0;
    if (valid) at = my[digit] + before;
    __builtin_amdgcn_wave_barrier();
    if (valid && before == 0) my[digit] = at + __popcll(same);
    __builtin_amdgcn_wave_barrier();
    if constexpr (SCATTER) {
      if (valid) out[at] = key;   // at < n: the scan's total is n
    }
  }
  if constexpr (!SCATTER) {
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[(long long)(lane + 64 * k) * n_waves + gw] = my[lane + 64 * k];
  }
}

// data[0..n) -> its exclusive prefix sums, in place; one workgroup, a thread owns a contiguous piece
__global__ __launch_bounds__(kSortScanThreads) void word_grad_scan(int* __restrict__ data, int n) {
  __shared__ int sums[kSortScanThreads];
  const int t = threadIdx.x;
  const int per = (n + kSortScanThreads - 1) / kSortScanThreads;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += data[i];
  sums[t] = s;
  __syncthreads();
  for (int off = 1; off < kSortScanThreads; off <<= 1) {
    const int v = t >= off ? sums[t - off] : 0;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  int run = sums[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int v = data[i];
    data[i] = run;
    run += v;
  }
}

// the first sorted position whose id is `id` (position i holds it)
__device__ __forceinline__ int word_grad_run_start(const unsigned long long* __restrict__ sorted, int i, unsigned id) {
  int lo = -1, hi = i;   // sorted[lo] has a smaller id (or lo == -1), sorted[hi] has `id`
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)(sorted[mid] >> 32) < id) lo = mid;
    else hi = mid;
  }
  return hi;
}

// where the partial of the chunk at sorted position i of an id with several chunks lies: two chunk starts of such ids can
// share a window of kWordGradChunk positions only as the tail of one id and the first chunk of the next
__device__ __forceinline__ long long word_grad_slot(int i, bool first_of_id) {
  return 2ll * (i / kWordGradChunk) + (first_of_id ? 1 : 0);
}

template <bool TYPED>
__global__ __launch_bounds__(256) void word_grad_units(
    const _Float16* __restrict__ dy_in, const long long* __restrict__ type_ids, const int* __restrict__ cu_seqlens, int batch,
    int seq_len, int hidden, const _Float16* __restrict__ word, long long vocab, const _Float16* __restrict__ pos,
    const _Float16* __restrict__ type_table, int n_types, const _Float16* __restrict__ gamma, float eps, int n_tokens,
    const unsigned long long* __restrict__ sorted, float* __restrict__ d_word, float* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_tokens) return;
  const unsigned id = (unsigned)(sorted[i] >> 32);
  if (id >= vocab) return;   // the rows that no sequence owns
  int start = i;
  if (i > 0 && (unsigned)(sorted[i - 1] >> 32) == id) {
    start = word_grad_run_start(sorted, i, id);
    if ((i - start) % kWordGradChunk) return;
  }
  const int n_chunks = hidden >> 3;
  float gam[kMaxChunksPerLane][8], acc[kMaxChunksPerLane][8], unused[2][kMaxChunksPerLane][8];
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c) {
#pragma unroll
    for (int k = 0; k < 8; ++k) gam[c][k] = acc[c][k] = unused[0][c][k] = unused[1][c][k] = 0.f;
    if (lane + 64 * c < n_chunks) load8(gamma + (lane + 64 * c) * 8, gam[c]);
  }
  int j = 0;
  for (; j < kWordGradChunk && i + j < n_tokens; ++j) {
    const unsigned long long key = sorted[i + j];
    if ((unsigned)(key >> 32) != id) break;
    const long long row = (long long)(unsigned)key;
    int b, s;
    locate_row(cu_seqlens, batch, seq_len, row, &b, &s);   // valid: word_grad_keys gave the row a real id
    long long tt = 0;
    if constexpr (TYPED) {
      if (type_ids) tt = type_ids[(long long)b * seq_len + s];
      if (tt < 0 || tt >= n_types) tt = 0;
    }
    float z[kMaxChunksPerLane][8], dy[kMaxChunksPerLane][8], dz[kMaxChunksPerLane][8];
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      const int chunk = lane + 64 * c;
      if (chunk < n_chunks) {
        float w[8], p[8], t[8];
        load8(word + (long long)id * hidden + chunk * 8, w);
        load8(dy_in + row * hidden + chunk * 8, dy[c]);
        load8(pos + (long long)s * hidden + chunk * 8, p);
        load8(type_table + tt * hidden + chunk * 8, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) z[c][k] = w[k] + (p[k] + t[k]);   // the association of embed_layernorm_bwd_body
      }
    }
    layernorm_backward_row(z, dy, gam, lane, n_chunks, hidden, eps, dz, unused[0], unused[1]);
#pragma unroll
    for (int c = 0; c < kMaxChunksPerLane; ++c) {
      if (lane + 64 * c < n_chunks) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[c][k] = j == 0 ? dz[c][k] : __fadd_rn(acc[c][k], dz[c][k]);
      }
    }
  }
  const bool more = j == kWordGradChunk && i + j < n_tokens && (unsigned)(sorted[i + j] >> 32) == id;
  const bool single = start == i && !more;
  float* dst = single ? d_word + (long long)id * hidden : partials + word_grad_slot(i, start == i) * hidden;
#pragma unroll
  for (int c = 0; c < kMaxChunksPerLane; ++c) {
    const int chunk = lane + 64 * c;
    if (chunk < n_chunks) {
#pragma unroll
      for (int k = 0; k < 8; ++k) dst[chunk * 8 + k] = single ? __fadd_rn(dst[chunk * 8 + k], acc[c][k]) : acc[c][k];
    }
  }
}

// workgroup = sorted position i, thread = 4 columns: the chain of adds is as long as the id has chunks, so the columns are
// spread as thin as the workgroup allows and the partials of the next chunks are loaded ahead of the adds
__global__ __launch_bounds__(256) void word_grad_combine(int hidden, long long vocab, int n_tokens,
                                                         const unsigned long long* __restrict__ sorted,
                                                         const float* __restrict__ partials, float* __restrict__ d_word) {
  const int i = blockIdx.x;   // < n_tokens: the grid
  const unsigned id = (unsigned)(sorted[i] >> 32);
  if (id >= vocab) return;
  if (i > 0 && (unsigned)(sorted[i - 1] >> 32) == id) return;   // not the id's first occurrence
  if (i + kWordGradChunk >= n_tokens || (unsigned)(sorted[i + kWordGradChunk] >> 32) != id) return;   // a single chunk
  int lo = i + kWordGradChunk, hi = n_tokens;   // sorted[lo] has `id`, sorted[hi] (or the end) does not
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)(sorted[mid] >> 32) == id) lo = mid;
    else hi = mid;
  }
  const int col = threadIdx.x * 4;
  if (col >= hidden) return;   // hidden is a multiple of 8, <= 1024
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 sum = *(const f32x4*)(partials + word_grad_slot(i, true) * hidden + col);
#pragma unroll 8
  for (int at = i + kWordGradChunk; at < hi; at += kWordGradChunk) {
    const f32x4 p = *(const f32x4*)(partials + word_grad_slot(at, false) * hidden + col);
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] = __fadd_rn(sum[k], p[k]);
  }
  float* dst = d_word + (long long)id * hidden + col;
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[k] = __fadd_rn(dst[k], sum[k]);
}

// ---- column-owning kernels: column sum, bias + GELU backward --------------------------------------------------------------
// workgroup = slab of rows, thread = up to kMaxColChunks 8-column pieces of every row of the slab, summed in row order:
// no reduction inside the workgroup.  MODE 0: sum of x.  MODE 1: dx = dy gelu'(x_pre + bias), sum of dx.
__device__ __forceinline__ float gelu_erf_grad(float t) {
  // d/dt [t Phi(t)] = Phi(t) + t phi(t); exp(-t^2/2) underflows to 0 long before t^2 overflows
  const float cdf = 0.5f * (1.0f + erff(t * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * t * t);
  return cdf + t * pdf;
}

template <int MODE>
__global__ __launch_bounds__(256) void column_kernel(const _Float16* __restrict__ x, const _Float16* __restrict__ dy_in,
                                                     const _Float16* __restrict__ bias, long long rows, int cols,
                                                     long long rows_per_slab, _Float16* __restrict__ dx_out,
                                                     float* __restrict__ ws) {
  const int n_chunks = cols >> 3;
  float acc[kMaxColChunks][8], bia[kMaxColChunks][8];
#pragma unroll
  for (int c = 0; c < kMaxColChunks; ++c) {
    const int chunk = threadIdx.x + 256 * c;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[c][i] = bia[c][i] = 0.f;
    if (MODE == 1 && chunk < n_chunks) load8(bias + chunk * 8, bia[c]);
  }
  const long long row0 = (long long)blockIdx.x * rows_per_slab;
  const long long row1 = row0 + rows_per_slab < rows ? row0 + rows_per_slab : rows;
  for (long long row = row0; row < row1; ++row) {
#pragma unroll
    for (int c = 0; c < kMaxColChunks; ++c) {
      const int chunk = threadIdx.x + 256 * c;
      if (chunk < n_chunks) {
        float v[8];
        load8(x + row * cols + chunk * 8, v);
        if (MODE == 1) {
          float g[8];
          load8(dy_in + row * cols + chunk * 8, g);
          f16x8 o;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            v[i] = g[i] * gelu_erf_grad(v[i] + bia[c][i]);
            o[i] = (_Float16)v[i];
          }
          *(f16x8*)(dx_out + row * cols + chunk * 8) = o;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[c][i] += v[i];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kMaxColChunks; ++c) {
    const int chunk = threadIdx.x + 256 * c;
    if (chunk < n_chunks) {
#pragma unroll
      for (int i = 0; i < 8; ++i) ws[(long long)blockIdx.x * cols + chunk * 8 + i] = acc[c][i];
    }
  }
}

// out = gelu_erf(x + bias), out of place: the training forward keeps x (the backward's operand)
__global__ __launch_bounds__(256) void bias_gelu_out(const _Float16* __restrict__ x, const _Float16* __restrict__ bias,
                                                     long long n_chunks_total, int chunks_per_row,
                                                     _Float16* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks_total; c += stride) {
    const int col_chunk = (int)(c % chunks_per_row);
    f16x8 v = *(const f16x8*)(x + c * 8);
    const f16x8 b = *(const f16x8*)(bias + col_chunk * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float t = (float)v[i] + (float)b[i];
      v[i] = (_Float16)(0.5f * t * (1.0f + erff(t * 0.70710678118654752440f)));   // the forward kernel's expression
    }
    *(f16x8*)(out + c * 8) = v;
  }
}

// ---- attention backward ---------------------------------------------------------------------------------------------------
// With S = (Q + b_q) K^T / 8, P = softmax(S), ctx = P V (+ b_v):
//   dP = d_ctx V^T,  delta_q = sum_k P dP,  dS = P (dP - delta),  dQ = dS K / 8,  dK = dS^T (Q + b_q) / 8,  dV = P^T d_ctx.
// (b_v shifts dP and delta alike and drops out; the key bias never reached the scores.)
// Both kernels use v_mfma_f32_32x32x16_f16 in the forward's orientation: the accumulator tile of a product has its column
// on the lane and 16 rows in registers, and is the B operand of the next product as it stands (the k-order of a step is
// free as long as both operands agree: A fragments gather rows {0-3, 8-11} + 4*half + 16*step of the transposed LDS copy).
//   attention_bwd_dq   workgroup = 128 queries of a (sequence, head), wave = 32 queries, lane = one query.  Pass 1 over
//                      the keys: S^T = K Q^T and dP^T = V dO^T -> running max, sum and sum of p dP (online softmax);
//                      lse and delta go to the workspace.  Pass 2: the same two products again, dS^T in registers, and
//                      dQ^T += K^T dS^T.  Five products.
//   attention_bwd_dkv  workgroup = 128 keys, wave = 32 keys, lane = one key, queries in chunks of 64 through LDS (rows and
//                      transposed): S = Q K^T, dP = dO V^T, then dV^T += dO^T P and dK^T += Q^T dS.  Four products.
// Nine products where five are the minimum: the price of owning every output row in exactly one place (no atomics, no
// second reduction pass over [T, hidden] partials).
constexpr int kHeadDim = 64;
constexpr int kRowStride = kHeadDim + 8;   // fp16 elements of a row-major LDS row (144 B: conflict-free b128)
constexpr int kChunk = 128;                // rows a workgroup owns; keys per LDS stage of attention_bwd_dq
constexpr int kTPad = 4;                   // transposed copies: rows are n + 4 elements long (as the forward's V^T)
constexpr int kQChunk = 64;                // queries per LDS stage of attention_bwd_dkv
constexpr float kExpScale = 0.125f * 1.4426950408889634f;   // log2(e) / sqrt(head_dim)

// Row r (piece c: 8 of its 64 values) -> dst[d][r], d = 8c .. 8c + 7.  Rows r and r ^ 1 sit in lanes 8 apart (thread ->
// (r, c) = (i >> 3, i & 7), i = tid + 256 * it); the even row's lane writes d = 8c .. 8c+3, the odd row's d = 8c+4 .. 8c+7,
// each as 4-byte stores {row r & ~1, row r | 1} (the forward kernel's V^T staging).
__device__ __forceinline__ void stage_transposed(f16x8 vv, int r, int c, _Float16* __restrict__ dst, int stride) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 w = __builtin_bit_cast(u32x4, vv);
  const bool odd = (r & 1) != 0;
  const unsigned s0 = odd ? w[0] : w[2], s1 = odd ? w[1] : w[3];
  const unsigned g0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s0, 0x128, 0xf, 0xf, false);
  const unsigned g1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s1, 0x128, 0xf, 0xf, false);
  const unsigned lo[2] = {odd ? g0 : w[0], odd ? g1 : w[1]};   // the d values of the EVEN row (low half of the store)
  const unsigned hi[2] = {odd ? w[2] : g0, odd ? w[3] : g1};   // ... of the odd row
  _Float16* p = dst + (c * 8 + (odd ? 4 : 0)) * stride + (r & ~1);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    *(unsigned*)(p + (2 * t) * stride) = __builtin_amdgcn_perm(hi[t], lo[t], 0x05040100u);
    *(unsigned*)(p + (2 * t + 1) * stride) = __builtin_amdgcn_perm(hi[t], lo[t], 0x07060302u);
  }
}

// the A fragment of a step over rows k0 .. of a transposed copy: row `d`, elements {k0 .. k0+3, k0+8 .. k0+11}
__device__ __forceinline__ f16x8 transposed_fragment(const _Float16* __restrict__ t_lds, int stride, int d, int k0) {
  const _Float16* r = t_lds + d * stride + k0;
  const f16x4 a = *(const f16x4*)r, b = *(const f16x4*)(r + 8);
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
  return v;
}

// a wave's [32 rows][64] fp32 tile held transposed in two accumulators (lane = row, registers = columns) -> 16-byte
// pieces of rows row0 .. row0 + 31 of `out` (row stride out_stride), through the wave's own LDS tile
__device__ __forceinline__ void store_tile(const f32x16& o0, const f32x16& o1, float scale, _Float16* __restrict__ tile,
                                           int lane, _Float16* __restrict__ out, long long out_stride, int row0,
                                           int rows_valid) {
  const int li = lane & 31, half = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f16x4 a, c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = (_Float16)(o0[g * 4 + e] * scale);
      c[e] = (_Float16)(o1[g * 4 + e] * scale);
    }
    *(f16x4*)(tile + li * kRowStride + g * 8 + 4 * half) = a;
    *(f16x4*)(tile + li * kRowStride + 32 + g * 8 + 4 * half) = c;
  }
  // same wave writes and reads its tile: LDS ops of a wave complete in order
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + (lane >> 3), piece = lane & 7;
    const f16x8 v = *(const f16x8*)(tile + row * kRowStride + piece * 8);
    if (row0 + row < rows_valid) *(f16x8*)(out + (long long)(row0 + row) * out_stride + piece * 8) = v;
  }
}

// DROP (the backward of proqa_attention_dropout_f16): with D = factor where a probability was kept and 0 elsewhere, the
// forward was ctx = (P D)(V + b_v), so dP = D (dO (V + b_v)^T) -- the value bias does NOT drop out: the rows of P D do not
// sum to 1 -- and delta = sum_k P dP, dS = P (dP - delta) as before; dV = (P D)^T dO.  dO b_v is one scalar per query.
template <bool DROP>
__device__ __forceinline__ void attention_bwd_dq_body(const _Float16* __restrict__ qkv, const _Float16* __restrict__ qkv_bias,
                                                      const _Float16* __restrict__ dctx, const int* __restrict__ cu_seqlens,
                                                      int max_seq_len, int n_heads, int n_qc, long long n_tokens,
                                                      _Float16* __restrict__ dqkv, float* __restrict__ ws_lse,
                                                      float* __restrict__ ws_delta, const DropoutParams& drop) {
  constexpr int t_stride = kChunk + kTPad;
  __shared__ __attribute__((aligned(16))) _Float16 smem[2 * kChunk * kRowStride + kHeadDim * t_stride];
  _Float16* k_lds = smem;                              // [128][72]
  _Float16* v_lds = smem + kChunk * kRowStride;        // [128][72]
  _Float16* kt_lds = smem + 2 * kChunk * kRowStride;   // [64][132]  K transposed
  const int pair = blockIdx.x / n_qc, qc = blockIdx.x - pair * n_qc;
  const int b = pair / n_heads, head = pair - b * n_heads;
  const int hidden = n_heads * kHeadDim;
  const long long row_stride = 3ll * hidden;
  const long long tok0 = cu_seqlens[b];
  int len = cu_seqlens[b + 1] - cu_seqlens[b];
  len = len < 1 ? 1 : (len > max_seq_len ? max_seq_len : len);
  if (tok0 < 0 || tok0 + len > n_tokens) return;       // offsets that do not describe the buffers: touch nothing
  if (qc * kChunk >= len) return;                      // (the whole workgroup: no barrier has been met)
  const _Float16* base = qkv + tok0 * row_stride + head * kHeadDim;
  const int n_ktiles = (len + 31) >> 5;
  const int n_kchunks = (n_ktiles + 3) >> 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
  const int qb = qc * 4 + wave;
  const bool active = qb * 32 < len;                   // wave-uniform: a wave without queries still stages and meets barriers
  const int q = qb * 32 + li;
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f16x8 qf[4], dof[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    qf[j] = dof[j] = zero8;
    if (q < len) {
      qf[j] = *(const f16x8*)(base + q * row_stride + (2 * j + half) * 8);
      if (qkv_bias) qf[j] = qf[j] + *(const f16x8*)(qkv_bias + head * kHeadDim + (2 * j + half) * 8);
      dof[j] = *(const f16x8*)(dctx + (tok0 + q) * hidden + head * kHeadDim + (2 * j + half) * 8);
    }
  }
  float dob = 0.f;                                     // (DROP only) dO_q . b_v
  if constexpr (DROP) {
    if (qkv_bias) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f16x8 bv = *(const f16x8*)(qkv_bias + 2 * hidden + head * kHeadDim + (2 * j + half) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) dob = __builtin_fmaf((float)dof[j][e], (float)bv[e], dob);
      }
      dob += __shfl_xor(dob, 32, 64);
    }
  }
  // DROP: dP^T of key tile kt <- D (dP^T + dO b_v); registers 4g .. 4g+3 are four consecutive keys: one generator call
  auto drop_dp = [&](int kc, int kt, f32x16& dp) {
    const int key_base = (kc * 4 + kt) * 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const Philox4 bits = dropout_prob_call(drop, (uint32_t)pair, (uint32_t)(q >> 1), (uint32_t)((key_base + 8 * g + 4 * half) >> 2));
#pragma unroll
      for (int e = 0; e < 4; ++e) dp[4 * g + e] = dropout_prob_keep(drop, bits, q, e) ? (dp[4 * g + e] + dob) * drop.factor : 0.f;
    }
  };

  auto stage = [&](int kc) {
    constexpr int kIters = kChunk * 8 / 256;
    f16x8 kreg[kIters], vreg[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = tid + it * 256;
      const int row = kc * kChunk + (i >> 3), c = i & 7;
      kreg[it] = vreg[it] = zero8;
      if (row < len) {
        const _Float16* src = base + row * row_stride + c * 8;
        kreg[it] = *(const f16x8*)(src + hidden);
        vreg[it] = *(const f16x8*)(src + 2 * hidden);
      }
    }
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = tid + it * 256;
      const int r = i >> 3, c = i & 7;
      *(f16x8*)(k_lds + r * kRowStride + c * 8) = kreg[it];
      *(f16x8*)(v_lds + r * kRowStride + c * 8) = vreg[it];
      stage_transposed(kreg[it], r, c, kt_lds, t_stride);
    }
  };
  // S^T and dP^T of key tile kt of the staged chunk: lane = query, registers = keys (r & 3) + 8 (r >> 2) + 4 half
  auto products = [&](int kc, int kt, f32x16& st, f32x16& dp) {
    const _Float16* krow = k_lds + (kt * 32 + li) * kRowStride + half * 8;
    const _Float16* vrow = v_lds + (kt * 32 + li) * kRowStride + half * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const f16x8*)(krow + j * 16), qf[j], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const f16x8*)(vrow + j * 16), dof[j], dp, 0, 0, 0);
    }
    const int key_base = (kc * 4 + kt) * 32;
    if (key_base + 32 > len) {                         // wave-uniform: only the last tile of a sequence is masked
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = key_base + (r & 3) + 8 * (r >> 2) + 4 * half;
        st[r] = key < len ? st[r] : -__builtin_inff();
      }
    }
  };

  // pass 1: the softmax statistics and delta = sum_k P dP, online
  float m = -__builtin_inff(), l = 0.f, dsum = 0.f;
  for (int kc = 0; kc < n_kchunks; ++kc) {
    if (kc) __syncthreads();                           // every wave is done with the previous chunk
    stage(kc);
    __syncthreads();
    if (!active) continue;
    const int tiles_here = n_ktiles - kc * 4 < 4 ? n_ktiles - kc * 4 : 4;
    for (int kt = 0; kt < tiles_here; ++kt) {
      f32x16 st = {0}, dp = {0};
      products(kc, kt, st, dp);
      if constexpr (DROP) drop_dp(kc, kt, dp);
      float mt = st[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mt = __builtin_fmaxf(mt, st[r]);
      mt = __builtin_fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float m_new = __builtin_fmaxf(m, mt);
      const float mc = m_new * kExpScale;
      float rs = 0.f, rd = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], kExpScale, -mc));
        rs += p;
        rd = __builtin_fmaf(p, dp[r], rd);
      }
      rs += __shfl_xor(rs, 32, 64);
      rd += __shfl_xor(rd, 32, 64);
      const float alpha = __builtin_amdgcn_exp2f((m - m_new) * kExpScale);   // 0 at the first tile (m = -inf)
      l = l * alpha + rs;
      dsum = dsum * alpha + rd;
      m = m_new;
    }
  }
  const float lse2 = m * kExpScale + __log2f(l);   // log2 of the softmax denominator, scores in log2 units
  const float delta = dsum / l;
  if (active && half == 0 && q < len) {
    ws_lse[(long long)head * n_tokens + tok0 + q] = lse2;
    ws_delta[(long long)head * n_tokens + tok0 + q] = delta;
  }

  // pass 2: dS^T = P^T (dP^T - delta) in registers, dQ^T += K^T dS^T
  f32x16 o0 = {0}, o1 = {0};
  for (int kc = 0; kc < n_kchunks; ++kc) {
    if (n_kchunks > 1) {                               // (a single chunk is still staged)
      __syncthreads();
      stage(kc);
      __syncthreads();
    }
    if (!active) continue;
    const int tiles_here = n_ktiles - kc * 4 < 4 ? n_ktiles - kc * 4 : 4;
    for (int kt = 0; kt < tiles_here; ++kt) {
      f32x16 st = {0}, dp = {0};
      products(kc, kt, st, dp);
      if constexpr (DROP) drop_dp(kc, kt, dp);
      f16x8 dsf[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], kExpScale, -lse2));
        dsf[r >> 3][r & 7] = (_Float16)(p * (dp[r] - delta));
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int key0 = kt * 32 + 16 * jj + 4 * half;
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(transposed_fragment(kt_lds, t_stride, li, key0), dsf[jj], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(transposed_fragment(kt_lds, t_stride, 32 + li, key0), dsf[jj], o1, 0, 0, 0);
      }
    }
  }
  __syncthreads();                                     // the last chunk is dead: its K rows become the output staging tiles
  if (!active) return;
  store_tile(o0, o1, 0.125f, smem + wave * 32 * kRowStride, lane, dqkv + tok0 * row_stride + head * kHeadDim, row_stride,
             qb * 32, len);
}

__global__ __launch_bounds__(256, 2) void attention_bwd_dq(const _Float16* __restrict__ qkv, const _Float16* __restrict__ qkv_bias,
                                                           const _Float16* __restrict__ dctx, const int* __restrict__ cu_seqlens,
                                                           int max_seq_len, int n_heads, int n_qc, long long n_tokens,
                                                           _Float16* __restrict__ dqkv, float* __restrict__ ws_lse,
                                                           float* __restrict__ ws_delta) {
  attention_bwd_dq_body<false>(qkv, qkv_bias, dctx, cu_seqlens, max_seq_len, n_heads, n_qc, n_tokens, dqkv, ws_lse, ws_delta,
                               DropoutParams{});
}

__global__ __launch_bounds__(256, 2) void attention_dropout_bwd_dq(const _Float16* __restrict__ qkv,
                                                                   const _Float16* __restrict__ qkv_bias,
                                                                   const _Float16* __restrict__ dctx,
                                                                   const int* __restrict__ cu_seqlens, int max_seq_len,
                                                                   int n_heads, int n_qc, long long n_tokens,
                                                                   _Float16* __restrict__ dqkv, float* __restrict__ ws_lse,
                                                                   float* __restrict__ ws_delta, DropoutParams drop) {
  attention_bwd_dq_body<true>(qkv, qkv_bias, dctx, cu_seqlens, max_seq_len, n_heads, n_qc, n_tokens, dqkv, ws_lse, ws_delta, drop);
}

// dob_lds (DROP only; [kQChunk] floats of LDS, the kernel's own): dO_q . b_v of the staged queries
template <bool DROP>
__device__ __forceinline__ void attention_bwd_dkv_body(const _Float16* __restrict__ qkv, const _Float16* __restrict__ qkv_bias,
                                                       const _Float16* __restrict__ dctx, const int* __restrict__ cu_seqlens,
                                                       int max_seq_len, int n_heads, int n_kc, long long n_tokens,
                                                       _Float16* __restrict__ dqkv, const float* __restrict__ ws_lse,
                                                       const float* __restrict__ ws_delta, float* dob_lds,
                                                       const DropoutParams& drop) {
  constexpr int t_stride = kQChunk + kTPad;
  __shared__ __attribute__((aligned(16))) _Float16 smem[2 * kQChunk * kRowStride + 2 * kHeadDim * t_stride];
  __shared__ float lse_lds[kQChunk], delta_lds[kQChunk];
  _Float16* q_lds = smem;                                                   // [64][72]  Q + b_q
  _Float16* do_lds = smem + kQChunk * kRowStride;                           // [64][72]  d_ctx
  _Float16* qt_lds = smem + 2 * kQChunk * kRowStride;                       // [64][68]  (Q + b_q)^T
  _Float16* dot_lds = smem + 2 * kQChunk * kRowStride + kHeadDim * t_stride; // [64][68]  d_ctx^T
  const int pair = blockIdx.x / n_kc, kc = blockIdx.x - pair * n_kc;
  const int b = pair / n_heads, head = pair - b * n_heads;
  const int hidden = n_heads * kHeadDim;
  const long long row_stride = 3ll * hidden;
  const long long tok0 = cu_seqlens[b];
  int len = cu_seqlens[b + 1] - cu_seqlens[b];
  len = len < 1 ? 1 : (len > max_seq_len ? max_seq_len : len);
  if (tok0 < 0 || tok0 + len > n_tokens) return;
  if (kc * kChunk >= len) return;                      // (the whole workgroup: no barrier has been met)
  const _Float16* base = qkv + tok0 * row_stride + head * kHeadDim;
  const _Float16* dbase = dctx + tok0 * hidden + head * kHeadDim;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, half = lane >> 5;
  const int kb = kc * 4 + wave;
  const bool active = kb * 32 < len;                   // wave-uniform
  const int key = kb * 32 + li;
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f16x8 kf[4], vf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    kf[j] = vf[j] = zero8;
    if (key < len) {
      const _Float16* src = base + key * row_stride + (2 * j + half) * 8;
      kf[j] = *(const f16x8*)(src + hidden);           // (no key bias: the forward drops it)
      vf[j] = *(const f16x8*)(src + 2 * hidden);
    }
  }
  f32x16 dk0 = {0}, dk1 = {0}, dv0 = {0}, dv1 = {0};
  const int n_qchunks = (len + kQChunk - 1) / kQChunk;
  for (int qc = 0; qc < n_qchunks; ++qc) {
    if (qc) __syncthreads();                           // every wave is done with the previous chunk
    {
      constexpr int kIters = kQChunk * 8 / 256;
      f16x8 qreg[kIters], dreg[kIters];
#pragma unroll
      for (int it = 0; it < kIters; ++it) {
        const int i = tid + it * 256;
        const int row = qc * kQChunk + (i >> 3), c = i & 7;
        qreg[it] = dreg[it] = zero8;
        if (row < len) {
          qreg[it] = *(const f16x8*)(base + row * row_stride + c * 8);
          if (qkv_bias) qreg[it] = qreg[it] + *(const f16x8*)(qkv_bias + head * kHeadDim + c * 8);
          dreg[it] = *(const f16x8*)(dbase + (long long)row * hidden + c * 8);
        }
      }
      if constexpr (DROP) {
        // the eight pieces of a row sit in eight consecutive lanes
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
          const int i = tid + it * 256;
          float part = 0.f;
          if (qkv_bias) {
            const f16x8 bv = *(const f16x8*)(qkv_bias + 2 * hidden + head * kHeadDim + (i & 7) * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) part = __builtin_fmaf((float)dreg[it][e], (float)bv[e], part);
          }
          part += __shfl_xor(part, 1, 64);
          part += __shfl_xor(part, 2, 64);
          part += __shfl_xor(part, 4, 64);
          if ((i & 7) == 0) dob_lds[i >> 3] = part;
        }
      }
#pragma unroll
      for (int it = 0; it < kIters; ++it) {
        const int i = tid + it * 256;
        const int r = i >> 3, c = i & 7;
        *(f16x8*)(q_lds + r * kRowStride + c * 8) = qreg[it];
        *(f16x8*)(do_lds + r * kRowStride + c * 8) = dreg[it];
        stage_transposed(qreg[it], r, c, qt_lds, t_stride);
        stage_transposed(dreg[it], r, c, dot_lds, t_stride);
      }
      if (tid < kQChunk) {
        const int row = qc * kQChunk + tid;
        // a query row that does not exist has P = exp2(s - inf) = 0
        lse_lds[tid] = row < len ? ws_lse[(long long)head * n_tokens + tok0 + row] : __builtin_inff();
        delta_lds[tid] = row < len ? ws_delta[(long long)head * n_tokens + tok0 + row] : 0.f;
      }
    }
    __syncthreads();
    if (!active) continue;
    const int rows_here = len - qc * kQChunk < kQChunk ? len - qc * kQChunk : kQChunk;
    const int tiles_here = (rows_here + 31) >> 5;
    for (int qt = 0; qt < tiles_here; ++qt) {
      // S = Q K^T and dP = dO V^T of query tile qt: lane = key, registers = queries (r & 3) + 8 (r >> 2) + 4 half
      f32x16 st = {0}, dp = {0};
      const _Float16* qrow = q_lds + (qt * 32 + li) * kRowStride + half * 8;
      const _Float16* drow = do_lds + (qt * 32 + li) * kRowStride + half * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const f16x8*)(qrow + j * 16), kf[j], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const f16x8*)(drow + j * 16), vf[j], dp, 0, 0, 0);
      }
      f16x8 pf[2], dsf[2];
      if constexpr (DROP) {
        // registers 4g .. 4g+3 are four consecutive queries of the lane's key: two generator calls (a call covers queries
        // 2n, 2n + 1).  pf holds the kept probabilities; the factor enters dV once, at the store
#pragma unroll
        for (int g2 = 0; g2 < 8; ++g2) {
          const int qi0 = qt * 32 + 8 * (g2 >> 1) + 4 * half + 2 * (g2 & 1);
          const Philox4 bits = dropout_prob_call(drop, (uint32_t)pair, (uint32_t)((qc * kQChunk + qi0) >> 1), (uint32_t)(key >> 2));
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int r = 2 * g2 + e, qi = qi0 + e;
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], kExpScale, -lse_lds[qi]));
            p = key < len ? p : 0.f;
            const bool kept = dropout_prob_keep(drop, bits, e, key);
            const float dpd = kept ? (dp[r] + dob_lds[qi]) * drop.factor : 0.f;
            pf[r >> 3][r & 7] = (_Float16)(kept ? p : 0.f);
            dsf[r >> 3][r & 7] = (_Float16)(p * (dpd - delta_lds[qi]));
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qi = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], kExpScale, -lse_lds[qi]));
          p = key < len ? p : 0.f;                     // a key row that does not exist was masked in the forward
          pf[r >> 3][r & 7] = (_Float16)p;
          dsf[r >> 3][r & 7] = (_Float16)(p * (dp[r] - delta_lds[qi]));
        }
      }
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int q0 = qt * 32 + 16 * jj + 4 * half;
        dv0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(transposed_fragment(dot_lds, t_stride, li, q0), pf[jj], dv0, 0, 0, 0);
        dv1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(transposed_fragment(dot_lds, t_stride, 32 + li, q0), pf[jj], dv1, 0, 0, 0);
        dk0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(transposed_fragment(qt_lds, t_stride, li, q0), dsf[jj], dk0, 0, 0, 0);
        dk1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(transposed_fragment(qt_lds, t_stride, 32 + li, q0), dsf[jj], dk1, 0, 0, 0);
      }
    }
  }
  __syncthreads();                                     // the last chunk is dead: Q and d_ctx rows become the output staging tiles
  if (!active) return;
  _Float16* tile = smem + wave * 32 * kRowStride;      // 4 x 32 x 72 = the two row-major arrays
  _Float16* out = dqkv + tok0 * row_stride + head * kHeadDim;
  store_tile(dk0, dk1, 0.125f, tile, lane, out + hidden, row_stride, kb * 32, len);
  store_tile(dv0, dv1, DROP ? drop.factor : 1.0f, tile, lane, out + 2 * hidden, row_stride, kb * 32, len);
}

__global__ __launch_bounds__(256, 2) void attention_bwd_dkv(const _Float16* __restrict__ qkv, const _Float16* __restrict__ qkv_bias,
                                                            const _Float16* __restrict__ dctx, const int* __restrict__ cu_seqlens,
                                                            int max_seq_len, int n_heads, int n_kc, long long n_tokens,
                                                            _Float16* __restrict__ dqkv, const float* __restrict__ ws_lse,
                                                            const float* __restrict__ ws_delta) {
  attention_bwd_dkv_body<false>(qkv, qkv_bias, dctx, cu_seqlens, max_seq_len, n_heads, n_kc, n_tokens, dqkv, ws_lse, ws_delta,
                                nullptr, DropoutParams{});
}

__global__ __launch_bounds__(256, 2) void attention_dropout_bwd_dkv(const _Float16* __restrict__ qkv,
                                                                    const _Float16* __restrict__ qkv_bias,
                                                                    const _Float16* __restrict__ dctx,
                                                                    const int* __restrict__ cu_seqlens, int max_seq_len,
                                                                    int n_heads, int n_kc, long long n_tokens,
                                                                    _Float16* __restrict__ dqkv, const float* __restrict__ ws_lse,
                                                                    const float* __restrict__ ws_delta, DropoutParams drop) {
  __shared__ float dob_lds[kQChunk];
  attention_bwd_dkv_body<true>(qkv, qkv_bias, dctx, cu_seqlens, max_seq_len, n_heads, n_kc, n_tokens, dqkv, ws_lse, ws_delta,
                               dob_lds, drop);
}

// ---- in-batch loss gradient -------------------------------------------------------------------------------------------------
// loss = mean_i (lse_i - s[i, t_i]), s = q c^T:  d s[i, j] = (g / nq) (exp(s[i, j] - lse_i) - [j == t_i]).
// One wave owns 32 rows of the side it differentiates (X: q when BY_ROW, else c) and walks the other side (Y) in tiles of 32
// through LDS (rows and transposed): G^T = Y X^T on the matrix pipe with lane = x and the 16 y of a step in registers, the
// coefficients in registers as fp16, then dX^T += Y^T coeff.  The score matrix exists one 32 x 32 tile at a time.
constexpr int kEmb = PROQA_EMBED_DIM;
constexpr int kEmbStride = kEmb + 8;
constexpr int kEmbTStride = 32 + kTPad;

template <bool BY_ROW>
__global__ __launch_bounds__(64) void inbatch_loss_grad(const _Float16* __restrict__ xs, int nx, const _Float16* __restrict__ ys,
                                                        int ny, const int* __restrict__ target, const float* __restrict__ lse,
                                                        const float* __restrict__ grad_in, int nq,
                                                        _Float16* __restrict__ dx) {
#include "inbatch_loss_grad_body.h"
}

// The block-diagonal objective: grid (X tiles of the largest block, 1, blocks).  Wave (x, ., m) runs the body on block m's
// slices of q, c, lse and dx with the implicit diagonal target, its own grad_in[m] and n_m rows -- what the single launch
// forms on those slices, so dq and dc carry its bits; nothing outside the block is read.  Waves past a smaller block's
// last tile leave at once.
template <bool BY_ROW>
__global__ __launch_bounds__(64) void inbatch_loss_blocks_grad(const _Float16* __restrict__ xs_all,
                                                               const _Float16* __restrict__ ys_all, BlockOffsets offs,
                                                               const float* __restrict__ lse_all,
                                                               const float* __restrict__ grad_all, _Float16* __restrict__ dx_all) {
  const int block = blockIdx.z;
  const int o = offs.o[block], n = offs.o[block + 1] - o;
  if ((int)blockIdx.x * 32 >= n) return;
  // what the single launch is handed for this rectangle
  const _Float16* __restrict__ xs = xs_all + (long long)o * kEmb;
  const _Float16* __restrict__ ys = ys_all + (long long)o * kEmb;
  const int* __restrict__ target = nullptr;
  const float* __restrict__ lse = lse_all + o;
  const float* __restrict__ grad_in = grad_all + block;
  const int nx = n, ny = n, nq = n;
  _Float16* __restrict__ dx = dx_all + (long long)o * kEmb;
#include "inbatch_loss_grad_body.h"
}

int slabs_for(int64_t rows, int64_t min_rows_per_slab, int64_t* rows_per_slab) {
  int64_t per = std::max<int64_t>(min_rows_per_slab, ceil_div<int64_t>(rows, kMaxSlabs));
  per = round_up<int64_t>(per, 4);
  *rows_per_slab = per;
  return (int)ceil_div<int64_t>(rows, per);
}

int launch_reduce(const float* ws, int n_slabs, int n_k, int cols, float* o0, float* o1, float* o2, float* o3, int accumulate,
                  hipStream_t st) {
  hipLaunchKernelGGL(reduce_slabs, dim3((unsigned)ceil_div<int>(n_k * cols, 256)), dim3(256), 0, st, ws, n_slabs, n_k, cols,
                     o0, o1, o2, o3, accumulate);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

// The launchers of the operator pairs.  An exported function checks its own pointers (and makes its DropoutParams), names
// itself in `op` for the messages and says how much workspace it asks for; sizes, the empty cases and the launches are here.

// drop == nullptr: without dropout (dx unused)
static int launch_bias_residual_layernorm_backward(const char* op, const void* dy, const void* x, const void* bias,
                                                   const void* residual, const void* gamma, float eps, int64_t rows, int cols,
                                                   const DropoutParams* drop, void* dx, void* dz, float* dgamma, float* dbeta,
                                                   float* dbias, void* ws, size_t ws_bytes, size_t ws_need, void* stream) {
  if (rows < 0 || cols <= 0 || cols % 8 || cols > 64 * kMaxChunksPerLane * 8)
    return fail(PROQA_EINVAL, "%s: cols=%d must be a multiple of 8 and <= %d%s", op, cols, 64 * kMaxChunksPerLane * 8,
                drop ? ", rows < 2^32" : "");
  if (ws_bytes < ws_need) return fail(PROQA_EINVAL, "%s: workspace too small", op);
  hipStream_t st = as_stream(stream);
  if (rows == 0) {
    for (float* p : {dgamma, dbeta, dbias}) PROQA_HIP(hipMemsetAsync(p, 0, (size_t)cols * sizeof(float), st));
    return PROQA_OK;
  }
  int64_t per;
  const int n_slabs = slabs_for(rows, 16, &per);
  if (drop)
    hipLaunchKernelGGL(bias_residual_layernorm_dropout_bwd, dim3((unsigned)n_slabs), dim3(256), 0, st, (const _Float16*)dy,
                       (const _Float16*)x, (const _Float16*)bias, (const _Float16*)residual, (const _Float16*)gamma, eps,
                       (long long)rows, cols, (long long)per, (_Float16*)dz, (_Float16*)dx, (float*)ws, *drop);
  else
    hipLaunchKernelGGL(bias_residual_layernorm_bwd, dim3((unsigned)n_slabs), dim3(256), 0, st, (const _Float16*)dy,
                       (const _Float16*)x, (const _Float16*)bias, (const _Float16*)residual, (const _Float16*)gamma, eps,
                       (long long)rows, cols, (long long)per, (_Float16*)dz, (float*)ws);
  PROQA_LAUNCH_CHECK();
  return launch_reduce((const float*)ws, n_slabs, 3, cols, dgamma, dbeta, dbias, nullptr, 0, st);
}

// The workspace of the *_det entry points: the position kernel's slabs, then the plan's pieces (each 256-byte aligned)
struct WordGradPlan {
  size_t keys_a, keys_b, hist, partials, total;   // byte offsets
  int n_waves;
};

WordGradPlan word_grad_plan(size_t slabs_bytes, int64_t n_tokens, int hidden) {
  WordGradPlan p;
  const size_t t = n_tokens > 0 ? (size_t)n_tokens : 0;
  p.n_waves = (int)ceil_div<size_t>(t, kSortKeysPerWave);
  p.keys_a = round_up<size_t>(slabs_bytes, 256);
  p.keys_b = p.keys_a + round_up<size_t>(t * sizeof(unsigned long long), 256);
  p.hist = p.keys_b + round_up<size_t>(t * sizeof(unsigned long long), 256);
  p.partials = p.hist + round_up<size_t>((size_t)256 * p.n_waves * sizeof(int), 256);
  p.total = p.partials + 2 * ceil_div<size_t>(t, kWordGradChunk) * (size_t)(hidden > 0 ? hidden : 0) * sizeof(float);
  return p;
}

// typed: d_types is [n_types][hidden] and type_ids may be null; else d_types is the type-0 row alone (n_types, type_ids unused)
// det: d_word is summed in a fixed order (ws_need then covers word_grad_plan)
static int launch_embed_layernorm_backward(const char* op, bool typed, bool det, const void* dy, const int64_t* ids,
                                           const int64_t* type_ids, const int32_t* cu_seqlens, int batch, int seq_len,
                                           int hidden, int64_t n_tokens, const void* word, int64_t vocab, const void* pos,
                                           const void* type_emb, int n_types, const void* gamma, float eps, float* dgamma,
                                           float* dbeta, float* d_word, float* d_pos, float* d_types, void* ws, size_t ws_bytes,
                                           size_t ws_need, void* stream) {
  if (batch < 0 || seq_len <= 0 || seq_len > kMaxSlabs || vocab <= 0 || n_tokens < 0)
    return fail(PROQA_EINVAL, "%s: bad sizes (seq_len <= %d)", op, kMaxSlabs);
  if (hidden <= 0 || hidden % 8 || hidden > 64 * kMaxChunksPerLane * 8)
    return fail(PROQA_EINVAL, "%s: hidden=%d must be a multiple of 8 and <= %d", op, hidden, 64 * kMaxChunksPerLane * 8);
  if (det && (vocab >= 0x7fffffffll || n_tokens >= 0x7fffffffll))   // the sort key is (id, row) in 32 bits each
    return fail(PROQA_EINVAL, "%s: vocab and n_tokens must be below 2^31 - 1", op);
  if (ws_bytes < ws_need) return fail(PROQA_EINVAL, "%s: workspace too small", op);
  if (batch == 0 || n_tokens == 0) return PROQA_OK;
  hipStream_t st = as_stream(stream);
  if (typed && det)
    hipLaunchKernelGGL(embed_layernorm_typed_bwd_no_word, dim3((unsigned)seq_len), dim3(256), 0, st, (const _Float16*)dy,
                       (const long long*)ids, (const long long*)type_ids, (const int*)cu_seqlens, batch, seq_len, hidden,
                       (const _Float16*)word, (long long)vocab, (const _Float16*)pos, (const _Float16*)type_emb, n_types,
                       (const _Float16*)gamma, eps, (long long)n_tokens, d_pos, (float*)ws);
  else if (det)
    hipLaunchKernelGGL(embed_layernorm_bwd_no_word, dim3((unsigned)seq_len), dim3(256), 0, st, (const _Float16*)dy,
                       (const long long*)ids, (const int*)cu_seqlens, batch, seq_len, hidden, (const _Float16*)word,
                       (long long)vocab, (const _Float16*)pos, (const _Float16*)type_emb, (const _Float16*)gamma, eps,
                       (long long)n_tokens, d_pos, (float*)ws);
  else if (typed)
    hipLaunchKernelGGL(embed_layernorm_typed_bwd, dim3((unsigned)seq_len), dim3(256), 0, st, (const _Float16*)dy,
                       (const long long*)ids, (const long long*)type_ids, (const int*)cu_seqlens, batch, seq_len, hidden,
                       (const _Float16*)word, (long long)vocab, (const _Float16*)pos, (const _Float16*)type_emb, n_types,
                       (const _Float16*)gamma, eps, (long long)n_tokens, d_word, d_pos, (float*)ws);
  else
    hipLaunchKernelGGL(embed_layernorm_bwd, dim3((unsigned)seq_len), dim3(256), 0, st, (const _Float16*)dy,
                       (const long long*)ids, (const int*)cu_seqlens, batch, seq_len, hidden, (const _Float16*)word,
                       (long long)vocab, (const _Float16*)pos, (const _Float16*)type_emb, (const _Float16*)gamma, eps,
                       (long long)n_tokens, d_word, d_pos, (float*)ws);
  PROQA_LAUNCH_CHECK();
  // slab s is (dgamma, dbeta, the position's sum [by type]) of position s: the position sums add up to the type gradients
  if (int rc = launch_reduce((const float*)ws, seq_len, typed ? 4 : 3, hidden, dgamma, dbeta, d_types,
                             typed && n_types == 2 ? d_types + hidden : nullptr, 1, st))
    return rc;
  if (!det) return PROQA_OK;

  const int T = (int)n_tokens;
  const WordGradPlan plan = word_grad_plan((size_t)kMaxSlabs * (typed ? 4 : 3) * (size_t)hidden * sizeof(float), n_tokens, hidden);
  unsigned long long* keys = (unsigned long long*)((char*)ws + plan.keys_a);
  unsigned long long* spare = (unsigned long long*)((char*)ws + plan.keys_b);
  int* hist = (int*)((char*)ws + plan.hist);
  float* partials = (float*)((char*)ws + plan.partials);
  hipLaunchKernelGGL(word_grad_keys, dim3((unsigned)ceil_div<int>(T, 256)), dim3(256), 0, st, (const long long*)ids,
                     (const int*)cu_seqlens, batch, seq_len, (long long)vocab, T, keys);
  PROQA_LAUNCH_CHECK();
  int id_bits = 1;   // of the ids 0 .. vocab (vocab itself marks the rows that no sequence owns)
  while ((vocab >> id_bits) != 0) ++id_bits;
  const unsigned sort_grid = (unsigned)ceil_div<int>(plan.n_waves, 4);
  for (int shift = 32; shift < 32 + id_bits; shift += 8) {
    hipLaunchKernelGGL(word_grad_sort_pass<false>, dim3(sort_grid), dim3(256), 0, st, (const unsigned long long*)keys, T, shift,
                       plan.n_waves, hist, (unsigned long long*)nullptr);
    PROQA_LAUNCH_CHECK();
    hipLaunchKernelGGL(word_grad_scan, dim3(1), dim3(kSortScanThreads), 0, st, hist, 256 * plan.n_waves);
    PROQA_LAUNCH_CHECK();
    hipLaunchKernelGGL(word_grad_sort_pass<true>, dim3(sort_grid), dim3(256), 0, st, (const unsigned long long*)keys, T, shift,
                       plan.n_waves, hist, spare);
    PROQA_LAUNCH_CHECK();
    std::swap(keys, spare);
  }
  const unsigned wave_grid = (unsigned)ceil_div<int>(T, 4);
  if (typed)
    hipLaunchKernelGGL(word_grad_units<true>, dim3(wave_grid), dim3(256), 0, st, (const _Float16*)dy,
                       (const long long*)type_ids, (const int*)cu_seqlens, batch, seq_len, hidden, (const _Float16*)word,
                       (long long)vocab, (const _Float16*)pos, (const _Float16*)type_emb, n_types, (const _Float16*)gamma, eps,
                       T, (const unsigned long long*)keys, d_word, partials);
  else
    hipLaunchKernelGGL(word_grad_units<false>, dim3(wave_grid), dim3(256), 0, st, (const _Float16*)dy,
                       (const long long*)nullptr, (const int*)cu_seqlens, batch, seq_len, hidden, (const _Float16*)word,
                       (long long)vocab, (const _Float16*)pos, (const _Float16*)type_emb, 1, (const _Float16*)gamma, eps, T,
                       (const unsigned long long*)keys, d_word, partials);
  PROQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(word_grad_combine, dim3((unsigned)T), dim3(256), 0, st, hidden, (long long)vocab, T,
                     (const unsigned long long*)keys, (const float*)partials, d_word);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

// drop == nullptr: without dropout
static int launch_attention_backward(const char* op, const void* qkv, const void* qkv_bias, const void* d_ctx,
                                     const int32_t* cu_seqlens, int batch, int max_seq_len, int n_heads, int64_t n_tokens,
                                     const DropoutParams* drop, void* d_qkv, void* ws, size_t ws_bytes, size_t ws_need,
                                     void* stream) {
  if (batch < 0 || max_seq_len <= 0 || max_seq_len > 512 || n_heads <= 0 || n_tokens < 0)
    return fail(PROQA_EINVAL, "%s: bad sizes (max_seq_len <= 512)", op);
  if (ws_bytes < ws_need) return fail(PROQA_EINVAL, "%s: workspace too small", op);
  if (batch == 0 || n_tokens == 0) return PROQA_OK;
  hipStream_t st = as_stream(stream);
  const int n_c = (max_seq_len + kChunk - 1) / kChunk;
  const unsigned grid = (unsigned)batch * (unsigned)n_heads * (unsigned)n_c;
  float* ws_lse = (float*)ws;
  float* ws_delta = ws_lse + n_tokens * n_heads;
  if (drop)
    hipLaunchKernelGGL(attention_dropout_bwd_dq, dim3(grid), dim3(256), 0, st, (const _Float16*)qkv, (const _Float16*)qkv_bias,
                       (const _Float16*)d_ctx, (const int*)cu_seqlens, max_seq_len, n_heads, n_c, (long long)n_tokens,
                       (_Float16*)d_qkv, ws_lse, ws_delta, *drop);
  else
    hipLaunchKernelGGL(attention_bwd_dq, dim3(grid), dim3(256), 0, st, (const _Float16*)qkv, (const _Float16*)qkv_bias,
                       (const _Float16*)d_ctx, (const int*)cu_seqlens, max_seq_len, n_heads, n_c, (long long)n_tokens,
                       (_Float16*)d_qkv, ws_lse, ws_delta);
  PROQA_LAUNCH_CHECK();
  if (drop)
    hipLaunchKernelGGL(attention_dropout_bwd_dkv, dim3(grid), dim3(256), 0, st, (const _Float16*)qkv, (const _Float16*)qkv_bias,
                       (const _Float16*)d_ctx, (const int*)cu_seqlens, max_seq_len, n_heads, n_c, (long long)n_tokens,
                       (_Float16*)d_qkv, (const float*)ws_lse, (const float*)ws_delta, *drop);
  else
    hipLaunchKernelGGL(attention_bwd_dkv, dim3(grid), dim3(256), 0, st, (const _Float16*)qkv, (const _Float16*)qkv_bias,
                       (const _Float16*)d_ctx, (const int*)cu_seqlens, max_seq_len, n_heads, n_c, (long long)n_tokens,
                       (_Float16*)d_qkv, (const float*)ws_lse, (const float*)ws_delta);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // namespace
}  // namespace proqa

using namespace proqa;

extern "C" {

size_t proqa_backward_workspace_bytes(int cols) {
  return cols > 0 ? (size_t)kMaxSlabs * 3 * (size_t)cols * sizeof(float) : 0;
}

size_t proqa_attention_backward_workspace_bytes(int64_t n_tokens, int n_heads) {
  return n_tokens > 0 && n_heads > 0 ? (size_t)2 * (size_t)n_tokens * (size_t)n_heads * sizeof(float) : 0;
}

int proqa_colsum_f16(const void* x, int64_t rows, int cols, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !out || !ws) return fail(PROQA_EINVAL, "colsum: NULL argument");
  if (rows < 0 || cols <= 0 || cols % 8 || cols > 256 * kMaxColChunks * 8)
    return fail(PROQA_EINVAL, "colsum: cols=%d must be a multiple of 8 and <= %d", cols, 256 * kMaxColChunks * 8);
  if (ws_bytes < proqa_backward_workspace_bytes(cols)) return fail(PROQA_EINVAL, "colsum: workspace too small");
  hipStream_t st = as_stream(stream);
  if (rows == 0) return hipMemsetAsync(out, 0, (size_t)cols * sizeof(float), st) == hipSuccess ? PROQA_OK : fail(PROQA_EHIP, "colsum: memset");
  int64_t per;
  const int n_slabs = slabs_for(rows, 16, &per);
  hipLaunchKernelGGL(column_kernel<0>, dim3((unsigned)n_slabs), dim3(256), 0, st, (const _Float16*)x, (const _Float16*)nullptr,
                     (const _Float16*)nullptr, (long long)rows, cols, (long long)per, (_Float16*)nullptr, (float*)ws);
  PROQA_LAUNCH_CHECK();
  return launch_reduce((const float*)ws, n_slabs, 1, cols, out, nullptr, nullptr, nullptr, 0, st);
}

int proqa_bias_gelu_out_f16(const void* x, const void* bias, int64_t rows, int cols, void* out, void* stream) {
  if (!x || !bias || !out) return fail(PROQA_EINVAL, "bias_gelu_out: NULL argument");
  if (rows < 0 || cols <= 0 || cols % 8) return fail(PROQA_EINVAL, "bias_gelu_out: cols=%d must be a multiple of 8", cols);
  if (rows == 0) return PROQA_OK;
  const long long n_chunks = rows * (long long)(cols / 8);
  const unsigned grid = (unsigned)std::min<long long>(ceil_div<long long>(n_chunks, 256), (long long)device_cu_count() * 8);
  hipLaunchKernelGGL(bias_gelu_out, dim3(grid), dim3(256), 0, as_stream(stream), (const _Float16*)x, (const _Float16*)bias,
                     n_chunks, cols / 8, (_Float16*)out);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

int proqa_bias_gelu_backward_f16(const void* dy, const void* x_pre, const void* bias, int64_t rows, int cols, void* dx,
                                 float* dbias, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !x_pre || !bias || !dx || !dbias || !ws) return fail(PROQA_EINVAL, "bias_gelu_backward: NULL argument");
  if (rows < 0 || cols <= 0 || cols % 8 || cols > 256 * kMaxColChunks * 8)
    return fail(PROQA_EINVAL, "bias_gelu_backward: cols=%d must be a multiple of 8 and <= %d", cols, 256 * kMaxColChunks * 8);
  if (ws_bytes < proqa_backward_workspace_bytes(cols)) return fail(PROQA_EINVAL, "bias_gelu_backward: workspace too small");
  hipStream_t st = as_stream(stream);
  if (rows == 0)
    return hipMemsetAsync(dbias, 0, (size_t)cols * sizeof(float), st) == hipSuccess ? PROQA_OK : fail(PROQA_EHIP, "bias_gelu_backward: memset");
  int64_t per;
  const int n_slabs = slabs_for(rows, 16, &per);
  hipLaunchKernelGGL(column_kernel<1>, dim3((unsigned)n_slabs), dim3(256), 0, st, (const _Float16*)x_pre, (const _Float16*)dy,
                     (const _Float16*)bias, (long long)rows, cols, (long long)per, (_Float16*)dx, (float*)ws);
  PROQA_LAUNCH_CHECK();
  return launch_reduce((const float*)ws, n_slabs, 1, cols, dbias, nullptr, nullptr, nullptr, 0, st);
}

int proqa_bias_residual_layernorm_backward_f16(const void* dy, const void* x, const void* bias, const void* residual,
                                               const void* gamma, float eps, int64_t rows, int cols, void* dz, float* dgamma,
                                               float* dbeta, float* dbias, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !x || !bias || !residual || !gamma || !dz || !dgamma || !dbeta || !dbias || !ws)
    return fail(PROQA_EINVAL, "bias_residual_layernorm_backward: NULL argument");
  return launch_bias_residual_layernorm_backward("bias_residual_layernorm_backward", dy, x, bias, residual, gamma, eps, rows, cols,
                                                 nullptr, nullptr, dz, dgamma, dbeta, dbias, ws, ws_bytes,
                                                 proqa_backward_workspace_bytes(cols), stream);
}

int proqa_bias_residual_layernorm_dropout_backward_f16(const void* dy, const void* x, const void* bias, const void* residual,
                                                       const void* gamma, float eps, int64_t rows, int cols, double p,
                                                       uint64_t seed, int site, uint32_t call, void* dx, void* dresidual,
                                                       float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes,
                                                       void* stream) {
  if (!dy || !x || !bias || !residual || !gamma || !dx || !dresidual || !dgamma || !dbeta || !dbias || !ws)
    return fail(PROQA_EINVAL, "bias_residual_layernorm_dropout_backward: NULL argument");
  if (rows > 0xffffffffll)   // the generator's row counter is 32 bits
    return fail(PROQA_EINVAL, "bias_residual_layernorm_dropout_backward: cols=%d must be a multiple of 8 and <= %d, rows < 2^32",
                cols, 64 * kMaxChunksPerLane * 8);
  DropoutParams drop;
  if (!make_dropout_params(p, seed, site, call, &drop))
    return fail(PROQA_EINVAL, "bias_residual_layernorm_dropout_backward: p=%g must be in [0, 1) and site=%d in [0, 255]", p, site);
  return launch_bias_residual_layernorm_backward("bias_residual_layernorm_dropout_backward", dy, x, bias, residual, gamma, eps,
                                                 rows, cols, &drop, dx, dresidual, dgamma, dbeta, dbias, ws, ws_bytes,
                                                 proqa_backward_workspace_bytes(cols), stream);
}

int proqa_embed_layernorm_varlen_backward_f16(const void* dy, const int64_t* ids_dev, const int32_t* cu_seqlens_dev,
                                              int batch, int seq_len, int hidden, int64_t n_tokens, const void* word_emb,
                                              int64_t vocab, const void* pos_emb, const void* type_emb, const void* ln_gamma,
                                              float eps, float* dgamma, float* dbeta, float* d_word, float* d_pos,
                                              float* d_type0, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !ids_dev || !cu_seqlens_dev || !word_emb || !pos_emb || !type_emb || !ln_gamma || !dgamma || !dbeta || !d_word ||
      !d_pos || !d_type0 || !ws)
    return fail(PROQA_EINVAL, "embed_layernorm_backward: NULL argument");
  return launch_embed_layernorm_backward("embed_layernorm_backward", false, false, dy, ids_dev, nullptr, cu_seqlens_dev, batch, seq_len,
                                         hidden, n_tokens, word_emb, vocab, pos_emb, type_emb, 1, ln_gamma, eps, dgamma, dbeta,
                                         d_word, d_pos, d_type0, ws, ws_bytes, proqa_backward_workspace_bytes(hidden), stream);
}

size_t proqa_embed_layernorm_typed_backward_workspace_bytes(int hidden) {
  return hidden > 0 ? (size_t)kMaxSlabs * 4 * (size_t)hidden * sizeof(float) : 0;
}

int proqa_embed_layernorm_typed_varlen_backward_f16(const void* dy, const int64_t* ids_dev, const int64_t* type_ids_dev,
                                                    const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden,
                                                    int64_t n_tokens, const void* word_emb, int64_t vocab,
                                                    const void* pos_emb, const void* type_emb_table, int n_types,
                                                    const void* ln_gamma, float eps, float* dgamma, float* dbeta,
                                                    float* d_word, float* d_pos, float* d_types, void* ws, size_t ws_bytes,
                                                    void* stream) {
  if (!dy || !ids_dev || !cu_seqlens_dev || !word_emb || !pos_emb || !type_emb_table || !ln_gamma || !dgamma || !dbeta ||
      !d_word || !d_pos || !d_types || !ws)
    return fail(PROQA_EINVAL, "embed_layernorm_typed_backward: NULL argument");
  if (n_types != 1 && n_types != 2)
    return fail(PROQA_EINVAL, "embed_layernorm_typed_backward: n_types=%d must be 1 or 2", n_types);
  return launch_embed_layernorm_backward("embed_layernorm_typed_backward", true, false, dy, ids_dev, type_ids_dev, cu_seqlens_dev, batch,
                                         seq_len, hidden, n_tokens, word_emb, vocab, pos_emb, type_emb_table, n_types, ln_gamma,
                                         eps, dgamma, dbeta, d_word, d_pos, d_types, ws, ws_bytes,
                                         proqa_embed_layernorm_typed_backward_workspace_bytes(hidden), stream);
}

int proqa_embed_word_grad_chunk(void) { return kWordGradChunk; }

size_t proqa_embed_layernorm_backward_det_workspace_bytes(int64_t n_tokens, int hidden, int typed) {
  if (hidden <= 0) return 0;
  return word_grad_plan(typed ? proqa_embed_layernorm_typed_backward_workspace_bytes(hidden) : proqa_backward_workspace_bytes(hidden),
                        n_tokens, hidden).total;
}

int proqa_embed_layernorm_varlen_backward_det_f16(const void* dy, const int64_t* ids_dev, const int32_t* cu_seqlens_dev,
                                                  int batch, int seq_len, int hidden, int64_t n_tokens, const void* word_emb,
                                                  int64_t vocab, const void* pos_emb, const void* type_emb,
                                                  const void* ln_gamma, float eps, float* dgamma, float* dbeta, float* d_word,
                                                  float* d_pos, float* d_type0, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !ids_dev || !cu_seqlens_dev || !word_emb || !pos_emb || !type_emb || !ln_gamma || !dgamma || !dbeta || !d_word ||
      !d_pos || !d_type0 || !ws)
    return fail(PROQA_EINVAL, "embed_layernorm_backward_det: NULL argument");
  return launch_embed_layernorm_backward("embed_layernorm_backward_det", false, true, dy, ids_dev, nullptr, cu_seqlens_dev, batch,
                                         seq_len, hidden, n_tokens, word_emb, vocab, pos_emb, type_emb, 1, ln_gamma, eps, dgamma,
                                         dbeta, d_word, d_pos, d_type0, ws, ws_bytes,
                                         proqa_embed_layernorm_backward_det_workspace_bytes(n_tokens, hidden, 0), stream);
}

int proqa_embed_layernorm_typed_varlen_backward_det_f16(const void* dy, const int64_t* ids_dev, const int64_t* type_ids_dev,
                                                        const int32_t* cu_seqlens_dev, int batch, int seq_len, int hidden,
                                                        int64_t n_tokens, const void* word_emb, int64_t vocab,
                                                        const void* pos_emb, const void* type_emb_table, int n_types,
                                                        const void* ln_gamma, float eps, float* dgamma, float* dbeta,
                                                        float* d_word, float* d_pos, float* d_types, void* ws,
                                                        size_t ws_bytes, void* stream) {
  if (!dy || !ids_dev || !cu_seqlens_dev || !word_emb || !pos_emb || !type_emb_table || !ln_gamma || !dgamma || !dbeta ||
      !d_word || !d_pos || !d_types || !ws)
    return fail(PROQA_EINVAL, "embed_layernorm_typed_backward_det: NULL argument");
  if (n_types != 1 && n_types != 2)
    return fail(PROQA_EINVAL, "embed_layernorm_typed_backward_det: n_types=%d must be 1 or 2", n_types);
  return launch_embed_layernorm_backward("embed_layernorm_typed_backward_det", true, true, dy, ids_dev, type_ids_dev,
                                         cu_seqlens_dev, batch, seq_len, hidden, n_tokens, word_emb, vocab, pos_emb,
                                         type_emb_table, n_types, ln_gamma, eps, dgamma, dbeta, d_word, d_pos, d_types, ws,
                                         ws_bytes, proqa_embed_layernorm_backward_det_workspace_bytes(n_tokens, hidden, 1), stream);
}

int proqa_attention_backward_f16(const void* qkv, const void* qkv_bias, const void* d_ctx, const int32_t* cu_seqlens_dev,
                                 int batch, int max_seq_len, int n_heads, int64_t n_tokens, void* d_qkv, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!qkv || !d_ctx || !cu_seqlens_dev || !d_qkv || !ws) return fail(PROQA_EINVAL, "attention_backward: NULL argument");
  return launch_attention_backward("attention_backward", qkv, qkv_bias, d_ctx, cu_seqlens_dev, batch, max_seq_len, n_heads,
                                   n_tokens, nullptr, d_qkv, ws, ws_bytes,
                                   proqa_attention_backward_workspace_bytes(n_tokens, n_heads), stream);
}

int proqa_attention_dropout_backward_f16(const void* qkv, const void* qkv_bias, const void* d_ctx,
                                         const int32_t* cu_seqlens_dev, int batch, int max_seq_len, int n_heads,
                                         int64_t n_tokens, double p, uint64_t seed, int site, uint32_t call, void* d_qkv,
                                         void* ws, size_t ws_bytes, void* stream) {
  if (!qkv || !d_ctx || !cu_seqlens_dev || !d_qkv || !ws) return fail(PROQA_EINVAL, "attention_dropout_backward: NULL argument");
  DropoutParams drop;
  if (!make_dropout_params(p, seed, site, call, &drop))
    return fail(PROQA_EINVAL, "attention_dropout_backward: p=%g must be in [0, 1) and site=%d in [0, 255]", p, site);
  return launch_attention_backward("attention_dropout_backward", qkv, qkv_bias, d_ctx, cu_seqlens_dev, batch, max_seq_len, n_heads,
                                   n_tokens, &drop, d_qkv, ws, ws_bytes,
                                   proqa_attention_backward_workspace_bytes(n_tokens, n_heads), stream);
}

int proqa_inbatch_loss_grad_f16(const void* q, const void* c, const int32_t* target, const float* lse, const float* grad_in,
                                int nq, int nc, int dim, void* dq, void* dc, void* stream) {
  if (nq < 0 || nc < 0) return fail(PROQA_EINVAL, "inbatch_loss_grad: negative size");
  if (dim != kEmb) return fail(PROQA_EINVAL, "inbatch_loss_grad: dim=%d must be %d", dim, kEmb);
  if (nq == 0) {
    if (nc > 0 && dc) PROQA_HIP(hipMemsetAsync(dc, 0, (size_t)nc * kEmb * sizeof(_Float16), as_stream(stream)));
    return PROQA_OK;
  }
  if (nc == 0) return fail(PROQA_EINVAL, "inbatch_loss_grad: nc == 0 with nq > 0");
  if (!q || !c || !lse || !grad_in || !dq || !dc) return fail(PROQA_EINVAL, "inbatch_loss_grad: NULL argument");
  if (!target && nq > nc) return fail(PROQA_EINVAL, "inbatch_loss_grad: the implicit target i needs nq <= nc");
  if (nq > (1 << 24) || nc > (1 << 24)) return fail(PROQA_EINVAL, "inbatch_loss_grad: more than 2^24 rows");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(inbatch_loss_grad<true>, dim3((unsigned)ceil_div<int>(nq, 32)), dim3(64), 0, st, (const _Float16*)q, nq,
                     (const _Float16*)c, nc, (const int*)target, lse, grad_in, nq, (_Float16*)dq);
  PROQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(inbatch_loss_grad<false>, dim3((unsigned)ceil_div<int>(nc, 32)), dim3(64), 0, st, (const _Float16*)c, nc,
                     (const _Float16*)q, nq, (const int*)target, lse, grad_in, nq, (_Float16*)dc);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

int proqa_inbatch_loss_blocks_grad_f16(const void* q, const void* c, const int32_t* block_offsets, int n_blocks, int n, int dim,
                                       const float* lse, const float* grad_in, void* dq, void* dc, void* stream) {
  BlockOffsets offs;
  int widest = 0;
  const int rc = check_inbatch_blocks("inbatch_loss_blocks_grad", block_offsets, n_blocks, n, dim, &offs, &widest);
  if (rc != PROQA_OK) return rc;
  if (!q || !c || !lse || !grad_in || !dq || !dc) return fail(PROQA_EINVAL, "inbatch_loss_blocks_grad: NULL argument");
  if ((((uintptr_t)q | (uintptr_t)c | (uintptr_t)dq | (uintptr_t)dc) & 15) != 0)
    return fail(PROQA_EINVAL, "inbatch_loss_blocks_grad: q / c / dq / dc must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)ceil_div<int>(widest, 32), 1u, (unsigned)n_blocks);
  hipLaunchKernelGGL(inbatch_loss_blocks_grad<true>, grid, dim3(64), 0, st, (const _Float16*)q, (const _Float16*)c, offs, lse,
                     grad_in, (_Float16*)dq);
  PROQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(inbatch_loss_blocks_grad<false>, grid, dim3(64), 0, st, (const _Float16*)c, (const _Float16*)q, offs, lse,
                     grad_in, (_Float16*)dc);
  PROQA_LAUNCH_CHECK();
  return PROQA_OK;
}

}  // extern "C"
