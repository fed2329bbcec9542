// The arithmetic of the reader head, qa_outputs = Linear(hidden, 2) in half precision, shared by the span search
// (reader_kernels.hip) and the training objective (reader_loss_kernels.hip) so that both produce the same bits:
//   logit_k[t] = fp16(fp32(hidden[t] . qa_w[k]) + qa_b[k]), k = 0 start / 1 end
// One wave owns a row; lane l holds chunks l and l + 64 of it (8 columns each, hidden <= 1024); the products are added in
// column order within a lane and the lanes by the xor butterfly below.  With dropout (training, qa_drop) the hidden element
// is x * keep * factor in fp32 before it meets the weight; without, the row is used as it is.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dropout_rng.h"

namespace proqa {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kHeadMaxChunks = 2;   // hidden <= 64 lanes * 2 chunks * 8 = 1024

__device__ __forceinline__ float head_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// element i of chunk `chunk` of packed row `row` as the head sees it
template <bool kDrop>
__device__ __forceinline__ float head_element(_Float16 x, const DropoutParams& d, const Philox4& bits, int i) {
  if (kDrop) return dropout_hidden_keep(d, bits, i) ? (float)x * d.factor : 0.f;
  return (float)x;
}

// this lane's share of the two dot products of one row; `row` is the packed row (the dropout coordinate)
template <bool kDrop>
__device__ __forceinline__ void head_row_dots(const f16x8 (&x)[kHeadMaxChunks], const f16x8 (&w0)[kHeadMaxChunks],
                                              const f16x8 (&w1)[kHeadMaxChunks], int lane, int n_chunks,
                                              const DropoutParams& d, uint32_t row, float& s, float& e) {
  s = 0.f;
  e = 0.f;
#pragma unroll
  for (int c = 0; c < kHeadMaxChunks; ++c) {
    const int chunk = lane + 64 * c;
    if (chunk < n_chunks) {
      Philox4 bits = {};
      if (kDrop) bits = dropout_hidden_call(d, row, (uint32_t)chunk);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = head_element<kDrop>(x[c][i], d, bits, i);
        s += v * (float)w0[c][i];
        e += v * (float)w1[c][i];
      }
    }
  }
}

// the wave's sum + bias, rounded as a half-precision nn.Linear rounds it
__device__ __forceinline__ _Float16 head_logit(float lane_sum, float bias) { return (_Float16)(head_wave_sum(lane_sum) + bias); }

}  // namespace proqa
